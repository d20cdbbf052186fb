#!/usr/bin/env python3
"""A rocprofv3 kernel trace (CSV) split by kernel and grid size: kernel, grid threads, calls, total and mean us, longest
total first; last line: the multigrid setup's span, from the start of `row_stats` to the start of the next `f_init`, over
the solves of the trace.  Usage: kernel_by_grid.py KERNEL_TRACE.csv > BY_GRID.csv"""
import csv
import statistics
import sys


def short(name):
    name = name.replace("(anonymous namespace)::", "")
    name = name[5:] if name.startswith("void ") else name
    depth = 0
    for k, ch in enumerate(name):  # cut the argument list, keep the template arguments
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return name[:k]
    return name


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    by = {}
    for r in rows:
        grid = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])
        key = (short(r["Kernel_Name"]), grid)
        e = by.setdefault(key, [0, 0.0])
        e[0] += 1
        e[1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    print("kernel,grid_threads,calls,total_us,avg_us")
    for (name, grid), (calls, total) in sorted(by.items(), key=lambda kv: -kv[1][1]):
        print(f'"{name}",{grid},{calls},{total:.1f},{total / calls:.2f}')
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    spans, start = [], None
    for r in rows:
        name = short(r["Kernel_Name"])
        if name == "row_stats" and start is None:
            start = int(r["Start_Timestamp"])
        elif name == "f_init" and start is not None:
            spans.append((int(r["Start_Timestamp"]) - start) / 1e3)
            start = None
    if spans:
        print(f'"# setup span row_stats -> f_init: {len(spans)} solves, median {statistics.median(spans):.1f} us, '
              f'mean {statistics.mean(spans):.1f} us, min {min(spans):.1f} us"')


if __name__ == "__main__":
    main()
