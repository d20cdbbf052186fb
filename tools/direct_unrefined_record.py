"""profiles/direct_unrefined.json from the output of

    python -m pytest tests/test_gpu_direct_unrefined.py -m gpu -s > out.txt
    python tools/direct_unrefined_record.py out.txt profiles/direct_unrefined.json

Per setting, table and matrix (G or G^T): the largest scaled(device) / max(scaled(SuperLU), 2^-53) over the case's
columns (three single right-hand sides, sixteen interleaved ones), the column it belongs to and the largest normwise
difference from SuperLU's solution; and the worst ratio of all."""
import json
import re
import sys

LINE = re.compile(r"RATIO \| (.+?) \| (.+?) \| (G\^T|G) \| (\S+) \| device (\S+) \| SuperLU (\S+) \| ratio (\S+) \| normwise (\S+)$")


def main():
    cases = {}
    for line in open(sys.argv[1]):
        m = LINE.search(line.strip())  # (pytest -s puts its progress dots in front of a test's first line)
        if not m:
            continue
        setting, table, matrix, column = m.group(1, 2, 3, 4)
        device, superlu, ratio, err = (float(v) for v in m.group(5, 6, 7, 8))
        c = cases.setdefault((setting, table, matrix), {"setting": setting, "table": table, "matrix": matrix, "columns": 0,
                                                        "worst_ratio": -1.0, "worst_normwise": 0.0})
        c["columns"] += 1
        c["worst_normwise"] = max(c["worst_normwise"], err)
        if ratio > c["worst_ratio"]:
            c.update(worst_ratio=ratio, worst_column=column, device=device, superlu=superlu)
    rows = list(cases.values())
    worst = max(rows, key=lambda c: c["worst_ratio"])
    record = {"measure": "scaled(device) / max(scaled(SuperLU), 2**-53), scaled(x) = |Mx-b|_inf / (|M|_inf |x|_inf + |b|_inf) in "
                         "np.longdouble; unrefined on both sides; the suite's bound is 16",
              "worst_ratio": worst["worst_ratio"], "worst_case": [worst["setting"], worst["table"], worst["matrix"]],
              "cases": rows}
    with open(sys.argv[2], "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(f"{len(rows)} cases, worst ratio {worst['worst_ratio']} ({worst['setting']}, {worst['table']}, {worst['matrix']})")


if __name__ == "__main__":
    main()
