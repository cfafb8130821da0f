#!/usr/bin/env python3
"""Per-launch kernel time by launch parity, from a rocprofv3 --kernel-trace
CSV: the launches of the kernels whose name contains --kernel-substr, in start
order, the last --last of them split into even and odd positions.  With the
alternating block sweep (hspmv_set_sweep) the two are the two directions.

    python heterogeneous-spmv_amd/tools/trace_parity.py bench_kernel_trace.csv [--last 200] [-o F.json]
"""
import argparse
import csv
import json

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--kernel-substr", default="hspmv_")
    ap.add_argument("--last", type=int, default=200)
    ap.add_argument("-o", "--out", default="")
    a = ap.parse_args()
    rows = []
    with open(a.trace, newline="") as fp:
        for r in csv.DictReader(fp):
            if a.kernel_substr in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    n0 = max(0, len(rows) - a.last)
    n0 += n0 % 2  # keep the parity of the handle's call count
    us = np.array([(e - s) * 1e-3 for s, e, _ in rows])
    gap = np.array([(rows[i][0] - rows[i - 1][1]) * 1e-3 for i in range(n0 + 1, len(rows))])
    sel = us[n0:]
    rec = {"trace": a.trace, "kernel": rows[-1][2].split("(")[0][:80] if rows else None,
           "launches": len(rows), "counted": int(sel.size),
           "all_us": {"mean": round(float(sel.mean()), 3), "median": round(float(np.median(sel)), 3)},
           "even_us": {"mean": round(float(sel[0::2].mean()), 3), "median": round(float(np.median(sel[0::2])), 3)},
           "odd_us": {"mean": round(float(sel[1::2].mean()), 3), "median": round(float(np.median(sel[1::2])), 3)},
           "gap_between_launches_us": round(float(np.median(gap)), 3) if gap.size else None}
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as fp:
            fp.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
