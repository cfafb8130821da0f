#!/usr/bin/env python3
"""The mixed handle (fp32 values, fp64 vectors) against the fp64 and the fp32
handle of the same library, in ONE process per shape.

    python heterogeneous-spmv_amd/tools/mixed_ab.py --shape c3 [--rounds 3] [--iters 20]
           [--out profiles/mixed/ab_c3.jsonl] [--only mixed|f64|f32]

Shapes: c3 (the bench's 125^3 27-point stencil with its maps) and c2, built as
bench.py builds them (hspmv.dist.build_shard, one rank); the values are rounded
to fp32 once, and the fp64 handle runs their exact widening.  Three handles
live in the process: fp64 on the widened values -- the baseline, the unchanged
path of this library, never the mixed operator's own number -- mixed, and fp32.
The rounds alternate the three hspmv_run calls after a warm-up.  The record
holds each handle's minimum and its spread across the rounds (max - min of the
rounds' minima), t_mixed / t_f64, each handle's format_bytes, the byte ratio
format_bytes_mixed / format_bytes_f64, format_bytes / t as a share of the
8 TB/s HBM peak, and whether y_mixed equals y_f64 bit for bit on the rows of at
most 40 nonzeros.

--only NAME: create that handle alone and run it (the profiler's target:
rocprofv3 --kernel-trace --stats -- python ... --only mixed).
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import torch  # noqa: E402,F401  (load order: torch's HIP runtime first)

import hspmv  # noqa: E402
from hspmv import dist as hdist  # noqa: E402
from hspmv import gen  # noqa: E402

PEAK_BPS = 8.0e12


def handles(A32, maps, which):
    A64 = A32.astype(np.float64)
    make = {"f64": lambda: hspmv.SpMV(A64, maps, device=0),
            "mixed": lambda: hspmv.SpMV(A32, maps, device=0, vector_dtype=np.float64),
            "f32": lambda: hspmv.SpMV(A32, maps, device=0)}
    return {k: make[k]() for k in which}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", required=True, choices=["c2", "c3"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default="", choices=["", "mixed", "f64", "f32"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if hspmv.device_count() < 1:
        sys.exit("mixed_ab: no HIP device visible")
    if a.rounds < 3 or a.iters < 20:
        sys.exit("mixed_ab: at least 3 rounds of 20 iterations")
    sh = hdist.build_shard(a.shape, 0, 1, dtype=np.float64)
    A32, maps = sh.A.astype(np.float32), sh.maps  # rounded once; every handle sees these values
    x = gen.rand_x(A32.n, 100)
    names = [a.only] if a.only else ["f64", "mixed", "f32"]
    ops = handles(A32, maps, names)
    y = {k: op(x.astype(op.dtype)) for k, op in ops.items()}
    if a.only:
        t = ops[a.only].run(5, a.iters)
        print(json.dumps({"shape": a.shape, "handle": a.only, "t_us": round(t["t_min"] * 1e6, 3),
                          "kernel": ops[a.only].info["kernel_name"]}))
        return
    short = np.diff(A32.row_ptr) <= 40
    same = bool(y["mixed"][short].tobytes() == y["f64"][short].tobytes())
    for op in ops.values():
        op.run(5, a.iters)  # warm-up
    ts = {k: [] for k in names}
    for _ in range(a.rounds):
        for k in names:
            ts[k].append(ops[k].run(3, a.iters)["t_min"])
    info = {k: ops[k].info for k in names}
    rec = {"shape": a.shape, "m": A32.m, "nnz": A32.nnz, "rounds": a.rounds, "iters": a.iters}
    for k in names:
        tmin = min(ts[k])
        rec[f"t_{k}_us"] = round(tmin * 1e6, 3)
        rec[f"spread_{k}_us"] = round((max(ts[k]) - tmin) * 1e6, 3)
        rec[f"t_{k}_rounds_us"] = [round(v * 1e6, 3) for v in ts[k]]
        rec[f"format_bytes_{k}"] = info[k]["format_bytes"]
        rec[f"alg_bytes_{k}"] = info[k]["alg_bytes"]
        rec[f"frac_of_8TBps_{k}"] = round(info[k]["format_bytes"] / tmin / PEAK_BPS, 4)
        rec[f"kernel_{k}"] = info[k]["kernel_name"]
        rec[f"row_slices_{k}"] = info[k]["row_slices"]
        rec[f"slice_pos_bits_{k}"] = info[k]["slice_pos_bits"]
        rec[f"sweep_{k}"] = info[k]["sweep"]
    rec["ratio_t_mixed_over_f64"] = round(min(ts["mixed"]) / min(ts["f64"]), 4)
    rec["ratio_bytes_mixed_over_f64"] = round(info["mixed"]["format_bytes"] / info["f64"]["format_bytes"], 4)
    rec["mixed_faster_than_f64_by_more_than_spread"] = bool(
        min(ts["f64"]) - min(ts["mixed"]) > max(rec["spread_mixed_us"], rec["spread_f64_us"]) * 1e-6)
    rec["y_mixed_bits_equal_f64_short_rows"] = same
    rec["short_rows"] = int(short.sum())
    print(json.dumps(rec), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
