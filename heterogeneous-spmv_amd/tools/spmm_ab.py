#!/usr/bin/env python3
"""SpMM against k SpMVs of the same library, in ONE process per shape.

    python heterogeneous-spmv_amd/tools/spmm_ab.py --shape c3_f64 [--ks 2,4,8,16,32]
           [--rounds 3] [--iters 20] [--out profiles/spmm/ab_c3_f64.jsonl] [--only-mm K]

Shapes: c3_f64 / c3_f32 (the 125^3 27-point stencil) and c5_f32 (the power-law
matrix), built as bench.py builds them (hspmv.dist.build_shard, one rank).
The baseline is k * t_spmv of the handle bench.py times -- SpMV(A, maps), the
unchanged single-vector path of this same library -- never the SpMM's own
number.  Per k the rounds alternate (a) hspmv_mm_run and (b) hspmv_run; the
record holds the minima, the ratio t_mm / (k * t_spmv) and alg_bytes / t_mm as
a fraction of the 8 TB/s HBM peak.  Column 0 of Y is compared with the
single-vector y on the rows both sum serially (the same bits).

--only-mm K: create the operator for that k alone and run it (the profiler's
target: rocprofv3 --kernel-trace --stats -- python ... --only-mm 8).
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
SHAPES = {"c3_f64": ("c3", np.float64), "c3_f32": ("c3", np.float32), "c5_f32": ("c5", np.float32)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", required=True, choices=sorted(SHAPES))
    ap.add_argument("--ks", default="2,4,8,16,32")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--nt", action="store_true", help="nontemporal col/val loads in the SpMM")
    ap.add_argument("--only-mm", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if hspmv.device_count() < 1:
        sys.exit("spmm_ab: no HIP device visible")
    cfg, dtype = SHAPES[a.shape]
    sh = hdist.build_shard(cfg, 0, 1, dtype=dtype)
    A, maps = sh.A, sh.maps
    short = np.diff(A.row_ptr) <= (40 if dtype == np.float64 else 56)
    ks = [a.only_mm] if a.only_mm else [int(v) for v in a.ks.split(",")]
    out = []
    sv = None
    if not a.only_mm:
        sv = hspmv.SpMV(A, maps, device=0)
        x0 = gen.rand_x(A.n, 100).astype(dtype)
        y0 = sv(x0)
    for k in ks:
        X = np.stack([gen.rand_x(A.n, 100 + c) for c in range(k)], axis=1).astype(dtype)
        with hspmv.SpMM(A, k, nontemporal=a.nt) as mm:
            Y = mm(X)
            info = mm.info
            if a.only_mm:
                t = mm.run(3, a.iters)
                print(json.dumps({"shape": a.shape, "k": k, "t_mm_us": round(t["t_min"] * 1e6, 3)}))
                return
            same = bool(np.array_equal(Y[short, 0], y0[short]))
            t_mm, t_sv = [], []
            for _ in range(a.rounds):
                t_mm.append(mm.run(3, a.iters)["t_min"])
                t_sv.append(sv.run(3, a.iters)["t_min"])
        tm, ts = min(t_mm), min(t_sv)
        rec = {"shape": a.shape, "dtype": np.dtype(dtype).name, "m": A.m, "nnz": A.nnz, "k": k,
               "nontemporal": a.nt, "lanes_per_row": info["lanes_per_row"], "long_rows": info["long_rows"],
               "t_mm_us": round(tm * 1e6, 3), "t_spmv_us": round(ts * 1e6, 3),
               "k_t_spmv_us": round(k * ts * 1e6, 3), "ratio_mm_over_k_spmv": round(tm / (k * ts), 4),
               "alg_bytes": info["alg_bytes"], "frac_of_8TBps": round(info["alg_bytes"] / tm / PEAK_BPS, 4),
               "gflops_mm": round(info["flops"] / tm * 1e-9, 1),
               "t_mm_rounds_us": [round(v * 1e6, 3) for v in t_mm],
               "t_spmv_rounds_us": [round(v * 1e6, 3) for v in t_sv],
               "spmv_kernel": sv.info["kernel_name"], "col0_bits_equal_spmv_short_rows": same}
        out.append(rec)
        print(json.dumps(rec), flush=True)
        if a.out:  # rewritten after every k: a cut-short run keeps what it measured
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in out))


if __name__ == "__main__":
    main()
