#!/usr/bin/env python3
"""w . y and y . y from the pass that writes y (hspmv_spmv_axpby_dot) against
what a caller runs without it, in ONE process per shape.

    python heterogeneous-spmv_amd/tools/dot_ab.py --shape c3 [--mixed] [--rounds 5] [--iters 20]
           [--out profiles/dot/ab_c3_f64.jsonl]

Shapes and protocol are tools/axpby_ab.py's: c3 / c2 built as bench.py builds
them, --mixed the values rounded to fp32 under fp64 vectors; one handle on a
torch stream, x, y, w and the two results bound torch tensors.  Four legs:

  a  axpby      hspmv_spmv_axpby(-1, 0.5) alone (the floor)
  b  unfused    leg a, then torch.dot(w, y) and torch.dot(y, y) on the same
                stream into a 2-element tensor: what a caller runs today.
                This is the baseline.
  c  two_pass   hspmv_spmv_axpby_dot(-1, 0.5, both dots) forced two-pass
  d  fused      the same on the fused path (row-slice handles)

Every leg is timed the same way: a HIP event pair around each call on the
handle's stream, synchronised per call, the minimum of --iters calls; the
rounds alternate the legs after a warm-up.  The record holds each leg's
minimum over the rounds and its spread (max - min of the rounds' minima), and
the byte model of the dots: + m sizeof(T) for w, + 16 bytes per partial pair
written and read again.
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
        sys.exit("dot_ab: no HIP device visible")
    if a.rounds < 3 or a.iters < 20:
        sys.exit("dot_ab: at least 3 rounds of 20 iterations")
    sh = hdist.build_shard(a.shape, 0, 1, dtype=np.float64)
    A, maps = sh.A, sh.maps
    kw = {}
    if a.mixed:
        A, kw = A.astype(np.float32), {"vector_dtype": np.float64}
    st = torch.cuda.Stream()
    alpha, beta = -1.0, 0.5
    with torch.cuda.stream(st):
        op = hspmv.SpMV(A, maps, device=0, stream=st.cuda_stream, **kw)
        op.set_x(gen.rand_x(A.n, 100).astype(op.dtype))
        y0 = torch.from_numpy(gen.rand_x(A.m, 101).astype(op.dtype)).to("cuda")
        w = torch.from_numpy(gen.rand_x(A.m, 102).astype(op.dtype)).to("cuda")
        y = y0.clone()
        res = torch.zeros(2, dtype=y.dtype, device="cuda")    # torch.dot's results: the vectors' dtype
        dots = torch.zeros(2, dtype=torch.float64, device="cuda")
        op.bind_y_device(y.data_ptr())
        op.bind_w_device(w.data_ptr())
        op.bind_dots_device(dots.data_ptr())
        st.synchronize()
        fusable = op.axpby_path == "fused"

        def unfused():
            op.spmv_axpby(alpha, beta)
            torch.dot(w, y, out=res[0])
            torch.dot(y, y, out=res[1])

        def leg(name):
            op.set_axpby_path("two_pass" if name == "two_pass" else "auto")
            y.copy_(y0)
            st.synchronize()
            if name == "axpby":
                return timed_min(st, a.iters, lambda: op.spmv_axpby(alpha, beta))
            if name == "unfused":
                return timed_min(st, a.iters, unfused)
            assert op.axpby_path == name
            return timed_min(st, a.iters, lambda: op.spmv_axpby_dot(alpha, beta, wy=True, yy=True))

        names = ["axpby", "unfused", "two_pass"] + (["fused"] if fusable else [])
        for k in names:
            leg(k)  # warm-up (scratch, partials: allocated here)
        ts = {k: [] for k in names}
        for _ in range(a.rounds):
            for k in names:
                ts[k].append(leg(k))
        # the two paths' dots and torch's, from the same y0 (one call each)
        seen = {}
        for k in names[1:]:
            op.set_axpby_path("two_pass" if k == "two_pass" else "auto")
            y.copy_(y0)
            if k == "unfused":
                unfused()
                st.synchronize()
                seen[k] = [float(v) for v in res.cpu()]
            else:
                op.spmv_axpby_dot(alpha, beta, wy=True, yy=True)
                st.synchronize()
                seen[k] = [float(v) for v in dots.cpu()]
        info = op.info
    sv = np.dtype(op.dtype).itemsize
    n_fused = (A.m + 63) // 64 if fusable else 0   # at least: one pair per wave task
    rec = {"shape": a.shape, "mixed": bool(a.mixed), "m": A.m, "nnz": A.nnz, "rounds": a.rounds, "iters": a.iters,
           "alpha": alpha, "beta": beta, "baseline": "unfused", "kernel": info["kernel_name"],
           "row_slices": info["row_slices"], "sweep": info["sweep"], "format_bytes": info["format_bytes"],
           "w_pass_bytes": A.m * sv, "partials_bytes_two_pass": 2 * 16 * ((A.m + 255) // 256),
           "partials_bytes_fused_at_least": 2 * 16 * n_fused, "blocks": info["blocks"], "dots": seen}
    for k in names:
        tmin = min(ts[k])
        rec[f"t_{k}_us"] = round(tmin * 1e6, 3)
        rec[f"spread_{k}_us"] = round((max(ts[k]) - tmin) * 1e6, 3)
        rec[f"t_{k}_rounds_us"] = [round(v * 1e6, 3) for v in ts[k]]
    spread = max(rec[f"spread_{k}_us"] for k in names if k != "axpby")
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
