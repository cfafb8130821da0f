#!/usr/bin/env python3
"""y = alpha A x + beta y on a handle (hspmv_spmv_axpby) against what a caller
ran before it existed, in ONE process per shape.

    python heterogeneous-spmv_amd/tools/axpby_ab.py --shape c3 [--mixed] [--rounds 5] [--iters 20]
           [--out profiles/axpby/ab_c3_f64.jsonl]

Shapes: c3 (the bench's 125^3 27-point stencil with its maps) and c2, built as
bench.py builds them (hspmv.dist.build_shard, one rank); --mixed: the values
rounded to fp32 under fp64 vectors.  One handle on a torch stream, four legs:

  a  spmv       hspmv_spmv alone: the unchanged SpMV (the floor)
  b  unfused    hspmv_spmv into a spare tensor t, then ONE torch kernel
                y.add_(t, alpha=-1) on the same stream: what a caller of the
                library ran for a residual before hspmv_spmv_axpby.  This is
                the baseline.  (beta = 1 is the only beta torch updates in one
                kernel; any other costs the caller a second pass over y.)
  c  two_pass   hspmv_spmv_axpby(-1, 0.5) forced through the two-pass path
  d  fused      hspmv_spmv_axpby(-1, 0.5) on the fused path (row-slice handles)

Every leg is timed the same way: a HIP event pair around each call on the
handle's stream, synchronised per call, the minimum of --iters calls; the
rounds alternate the legs after a warm-up.  The record holds each leg's
minimum over the rounds and its spread (max - min of the rounds' minima).
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import torch  # noqa: E402  (load order: torch's HIP runtime first)

import hspmv  # noqa: E402
from hspmv import dist as hdist  # noqa: E402
from hspmv import gen  # noqa: E402


def timed_min(stream, iters, call):
    """Minimum HIP-event time (seconds) of `iters` calls, each synchronised."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(iters):
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e-3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", required=True, choices=["c2", "c3"])
    ap.add_argument("--mixed", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if hspmv.device_count() < 1:
        sys.exit("axpby_ab: no HIP device visible")
    if a.rounds < 3 or a.iters < 20:
        sys.exit("axpby_ab: at least 3 rounds of 20 iterations")
    sh = hdist.build_shard(a.shape, 0, 1, dtype=np.float64)
    A, maps = sh.A, sh.maps
    kw = {}
    if a.mixed:
        A, kw = A.astype(np.float32), {"vector_dtype": np.float64}
    st = torch.cuda.Stream()
    alpha, beta = -1.0, 0.5
    with torch.cuda.stream(st):
        op = hspmv.SpMV(A, maps, device=0, stream=st.cuda_stream, **kw)
        tdt = torch.float64 if np.dtype(op.dtype) == np.float64 else torch.float32
        op.set_x(gen.rand_x(A.n, 100).astype(op.dtype))
        y0 = torch.from_numpy(gen.rand_x(A.m, 101).astype(op.dtype)).to("cuda")
        y = y0.clone()
        t = torch.empty(A.m, dtype=tdt, device="cuda")
        st.synchronize()
        fusable = op.axpby_path == "fused"

        def reset(target):
            y.copy_(y0)
            op.bind_y_device(target.data_ptr())
            st.synchronize()

        def unfused():
            op.spmv()
            y.add_(t, alpha=alpha)

        def leg(name):
            if name == "spmv":
                reset(y)
                return timed_min(st, a.iters, op.spmv)
            if name == "unfused":
                reset(t)
                return timed_min(st, a.iters, unfused)
            op.set_axpby_path("two_pass" if name == "two_pass" else "auto")
            assert op.axpby_path == name
            reset(y)
            return timed_min(st, a.iters, lambda: op.spmv_axpby(alpha, beta))

        names = ["spmv", "unfused", "two_pass"] + (["fused"] if fusable else [])
        for k in names:
            leg(k)  # warm-up (the two-pass scratch is allocated here)
        ts = {k: [] for k in names}
        for _ in range(a.rounds):
            for k in names:
                ts[k].append(leg(k))
        info = op.info
    sv = np.dtype(op.dtype).itemsize
    rec = {"shape": a.shape, "mixed": bool(a.mixed), "m": A.m, "nnz": A.nnz, "rounds": a.rounds, "iters": a.iters,
           "alpha": alpha, "beta": beta, "baseline": "unfused", "kernel": info["kernel_name"],
           "row_slices": info["row_slices"], "sweep": info["sweep"], "format_bytes": info["format_bytes"],
           "vector_pass_bytes": A.m * sv}
    for k in names:
        tmin = min(ts[k])
        rec[f"t_{k}_us"] = round(tmin * 1e6, 3)
        rec[f"spread_{k}_us"] = round((max(ts[k]) - tmin) * 1e6, 3)
        rec[f"t_{k}_rounds_us"] = [round(v * 1e6, 3) for v in ts[k]]
    spread = max(rec[f"spread_{k}_us"] for k in names if k != "spmv")
    rec["largest_spread_us"] = spread
    if fusable:
        rec["fused_below_unfused_and_two_pass_by_more_than_spread"] = bool(
            rec["t_fused_us"] + spread < min(rec["t_unfused_us"], rec["t_two_pass_us"]))
    rec["two_pass_slower_than_unfused_by_more_than_spread"] = bool(
        rec["t_two_pass_us"] > rec["t_unfused_us"] + spread)
    print(json.dumps(rec), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
