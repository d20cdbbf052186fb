cd "$(dirname "$0")/.." && O=${OUT:-bench_out} && mkdir -p "$O"
for c in 4 5 6 8; do
  timeout -k 10 200 python3 bench.py --full --workload cfg3 --steps 2 --warmup 1 --no-cpu --no-also --concurrent $c --no-classes > "$O/conc_$c.json" 2> "$O/conc_err.txt" || { tail "$O/conc_err.txt"; exit 1; }
  python3 -c "
import json;d=json.loads(open('$O/conc_$c.json').read().strip().splitlines()[-1]);print($c, [(x['streams'],x['symbolic_phases_kept'],round(x['circuits_per_sec'],1)) for x in d['concurrent']['all']])"
done
