#!/usr/bin/env python3
"""Forward against alternating block sweep (hspmv_set_sweep) on ONE handle:
the same device arrays, the same placement, only the mode switched between
rounds -- none of the handle-to-handle HBM placement scatter of a two-handle
A/B.

    python heterogeneous-spmv_amd/tools/sweep_ab.py --configs c3,c3:f32,c2,c4,c5
           [--rounds 7] [--iters 20] [--options deterministic=1] [--out F.jsonl]

Per config one record: t_med_us of each mode (the median over the rounds of
hspmv_run's mean kernel time), the spread of the forward rounds (max - min,
as a fraction of their median: the bar a difference has to clear, with 2 %),
what AUTO picked (info.sweep), and in alternate mode the median time of the
even and of the odd calls, one call per hspmv_run, so both directions show.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE))

import torch  # noqa: E402,F401  (load order: torch's HIP runtime first)

import hspmv  # noqa: E402
from hspmv import gen  # noqa: E402
from auto_regret import build  # noqa: E402  (sweep.build + the planner zoo)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3")
    ap.add_argument("--kernel", default="auto")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--options", default="", help="hspmv_options fields, name=value[,name=value]")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    options = {k: int(v) for k, v in (kv.split("=") for kv in a.options.split(",") if kv)} or None
    out = []
    for cfg in a.configs.split(","):
        A, maps, desc = build(cfg)
        x = gen.rand_x(A.n, 42).astype(A.val.dtype)
        with hspmv.SpMV(A, maps, device=0, kernel=a.kernel, options=options) as op:
            info = op.info
            op.set_sweep("forward")
            y0 = op(x)
            times = {"forward": [], "alternate": []}
            same = True
            for _ in range(a.rounds):
                for mode in ("forward", "alternate"):
                    op.set_sweep(mode)
                    times[mode].append(op.run(warmup=4, iters=a.iters)["t_avg"] * 1e6)
                    same = same and op.get_y().tobytes() == y0.tobytes()
            op.set_sweep("alternate")
            op.run(warmup=4, iters=1)
            calls = [op.run(warmup=0, iters=1)["t_min"] * 1e6 for _ in range(2 * a.iters)]
            fwd, alt = np.array(times["forward"]), np.array(times["alternate"])
            rec = {"config": cfg, "desc": desc, "kernel": info["kernel_name"], "row_slices": info["row_slices"],
                   "x_slabs": info["x_slabs"], "auto_sweep": info["sweep"], "options": options,
                   "format_mb": round(info["format_bytes"] * 1e-6, 1),
                   "forward_t_med_us": round(float(np.median(fwd)), 3),
                   "alternate_t_med_us": round(float(np.median(alt)), 3),
                   "gain": round(1.0 - float(np.median(alt) / np.median(fwd)), 4),
                   "forward_spread": round(float((fwd.max() - fwd.min()) / np.median(fwd)), 4),
                   "forward_rounds_us": [round(float(t), 3) for t in fwd],
                   "alternate_rounds_us": [round(float(t), 3) for t in alt],
                   "alternate_even_calls_us": round(float(np.median(calls[0::2])), 3),
                   "alternate_odd_calls_us": round(float(np.median(calls[1::2])), 3),
                   "y_equal_to_first": same}
        out.append(rec)
        print(json.dumps(rec), flush=True)
        if a.out:
            Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in out))


if __name__ == "__main__":
    main()
