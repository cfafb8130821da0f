#!/usr/bin/env python3
"""The alternating block sweep (hspmv_set_sweep) in a solver-shaped loop: one
SpMV, two dot products and three axpys over m-length torch vectors per
iteration, all on one stream, the SpMV alone timed with events.  The vector
kernels make 12 passes over 4 vectors between two SpMVs, which pushes part of
the matrix's tail out of the Infinity Cache: this measures how much of the
back-to-back gain (the same handle with nothing in between) survives.

    python heterogeneous-spmv_amd/tools/sweep_cg.py [--config c3] [--rounds 5] [--iters 40] [--out F.json]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE))

import torch  # noqa: E402

import hspmv  # noqa: E402
from hspmv import gen  # noqa: E402
from auto_regret import build  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    A, maps, desc = build(a.config)
    assert A.m == A.n, "the loop feeds y back into x: square matrices"
    tdt = torch.float64 if A.val.dtype == np.float64 else torch.float32
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    op = hspmv.SpMV(A, maps, device=0, stream=stream.cuda_stream)
    p = torch.from_numpy(gen.rand_x(A.n, 42, dtype=A.val.dtype)).cuda()
    r = p.clone()
    xk = torch.zeros_like(p)
    Ap = torch.empty(A.m, dtype=tdt, device="cuda")
    op.bind_x_device(p.data_ptr())
    op.bind_y_device(Ap.data_ptr())

    def loop(vectors: bool):
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
               for _ in range(a.iters)]
        for e0, e1 in evs:
            e0.record(stream)
            op.spmv()
            e1.record(stream)
            if vectors:  # CG's shape; the scalars stay on the device and keep the vectors bounded
                pAp = torch.dot(p, Ap)
                rr = torch.dot(r, r)
                alpha = torch.tanh(rr / (pAp.abs() + 1.0)) * 1e-3
                xk.addcmul_(p, alpha)
                r.addcmul_(Ap, -alpha)
                torch.addcmul(r, p, torch.full_like(alpha, 0.5), out=p)
        torch.cuda.synchronize()
        return float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in evs[4:]]))

    res = {m: {"back_to_back": [], "cg_loop": []} for m in ("forward", "alternate")}
    for _ in range(a.rounds):
        for mode in ("forward", "alternate"):
            op.set_sweep(mode)
            res[mode]["back_to_back"].append(loop(False))
            res[mode]["cg_loop"].append(loop(True))
    med = {m: {k: round(float(np.median(v)), 3) for k, v in d.items()} for m, d in res.items()}
    gain_b = 1.0 - med["alternate"]["back_to_back"] / med["forward"]["back_to_back"]
    gain_c = 1.0 - med["alternate"]["cg_loop"] / med["forward"]["cg_loop"]
    rec = {"config": a.config, "desc": desc, "m": A.m, "iters": a.iters, "rounds": a.rounds,
           # between two SpMVs: 12 vector passes (9 reads, 3 writes) over 4 distinct vectors
           "vector_traffic_between_spmvs_mb": round(12 * A.m * A.val.dtype.itemsize * 1e-6, 1),
           "vector_footprint_mb": round(4 * A.m * A.val.dtype.itemsize * 1e-6, 1),
           "spmv_us": med, "gain_back_to_back": round(gain_b, 4), "gain_cg_loop": round(gain_c, 4),
           "share_of_gain_left": round(gain_c / gain_b, 3) if gain_b > 0 else None,
           "rounds_us": {m: {k: [round(t, 3) for t in v] for k, v in d.items()} for m, d in res.items()},
           "finite": bool(torch.isfinite(p).all().item() and torch.isfinite(xk).all().item())}
    op.close()
    print(json.dumps(rec), flush=True)
    if a.out:
        Path(a.out).write_text(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
