#!/usr/bin/env python3
"""As tools/rocprof_region.py, but one row per (kernel, grid): launches of one kernel on different layers are told apart by
their grid size (x3s_conv_kernel<8,1,1,2,608,...> runs layer1 with 1470 x 1 workgroups and layer4 with 184 x 8).

    python tools/rocprof_region_grids.py <dir>/<prefix>_kernel_trace.csv [steps] [name filter] > profiles/...csv
"""
import csv
import sys
from collections import defaultdict


def main():
    path = sys.argv[1]
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    only = sys.argv[3] if len(sys.argv) > 3 else ""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            grid = "x".join(str(int(r["Grid_Size_" + d]) // max(1, int(r["Workgroup_Size_" + d]))) for d in "XYZ")
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], grid,
                         r.get("VGPR_Count", ""), r.get("Accum_VGPR_Count", ""), r.get("LDS_Block_Size", ""), r.get("Scratch_Size", "")))
    rows.sort()
    marks = [i for i, r in enumerate(rows) if "dmc_profile_mark_kernel" in r[2]]
    if len(marks) < 2:
        raise SystemExit("need two dmc_profile_mark_kernel launches, found %d" % len(marks))
    agg = defaultdict(list)
    for s, e, name, grid, *res in rows[marks[0] + 1:marks[-1]]:
        if only in name:
            agg[(name, grid) + tuple(res)].append(e - s)
    w = csv.writer(sys.stdout)
    w.writerow(["Name", "Workgroups", "VGPR", "AGPR", "LDS", "Scratch", "Calls", "CallsPerStep", "AverageNs", "MsPerStep", "MinNs", "MaxNs"])
    for key, v in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
        w.writerow([key[0][:160]] + list(key[1:]) + [len(v), "%.2f" % (len(v) / steps), "%.1f" % (sum(v) / len(v)),
                                                      "%.4f" % (sum(v) / steps / 1e6), min(v), max(v)])


if __name__ == "__main__":
    main()
