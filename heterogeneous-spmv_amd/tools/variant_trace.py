#!/usr/bin/env python3
"""One SpMV (or SpMM) on a fixed list of small handles that walks every
branch of the launch dispatch (row_launch.cuh, spmv_kernels.hip, csort.hip,
spmm.hip), for a kernel trace:

    rocprofv3 --kernel-trace -d OUT -- python tools/variant_trace.py --lib L [--out F.jsonl]

Run once per library, one process each; the ordered kernel names of two
libraries' traces are equal when both dispatch every plan to the same
instantiation -- which equal results cannot show, since every variant of a
kernel computes the same bits.  Prints (and writes to --out) one JSON line
per case: its name and the plan the handle reports, so that a case that no
longer reaches its branch shows up.

The split rows' serial sums always run on the forked stream (the handle
creates it whenever the order is serial), so the list has no unforked case.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import info_ab  # noqa: E402  (sets the import paths; torch first)
import hspmv  # noqa: E402
from hspmv import _lib, gen  # noqa: E402
from ab import load  # noqa: E402
from info_ab import spmm_case, spmv_case as S  # noqa: E402
from test_serial import long_rows  # noqa: E402
from test_slice_pos12 import OFF, ON, block_run  # noqa: E402
from test_spmm import long_matrix  # noqa: E402

PLAN = ("kernel", "lanes", "waves_per_block", "chunk_u", "blocks", "x_windows", "x_dict", "row_slices",
        "slice_pos_bits", "lds_pad", "col16", "x_slabs", "n_split_rows", "serial_order", "csr3_plan",
        "groups_per_wave", "col16_group", "wave_tasks", "deterministic")


def blocks32(dtype, m=4 * 64 * 3 + 37, b=32):
    """Dense b x b diagonal blocks: rows of 32 nonzeros, which STREAM pads for."""
    n = (m + b - 1) // b * b
    rows = np.arange(m, dtype=np.int64)
    ci = ((rows // b) * b)[:, None] + np.arange(b, dtype=np.int64)[None, :]
    rp = np.arange(0, m * b + 1, b, dtype=np.int64).astype(np.int32)
    val = np.random.default_rng(11).uniform(-1, 1, m * b).astype(dtype)
    return hspmv.CsrMatrix(m, n, rp, ci.reshape(-1).astype(np.int32), val)


def cases():
    U = lambda u: u << _lib.U_SHIFT  # noqa: E731
    band = gen.banded(5000, per_row=10, half=32, seed=5)
    band32 = band.astype(np.float32)
    st21, lap = gen.stencil27(21), gen.laplace2d(200, 150)
    tasks = hspmv.build_csr3_maps(band, 7, 8)
    plain = {"x_dict": -1, "x_windows": -1}
    for u in (2, 3, 4, 5, 6, 8, 16):
        for pf in (0, _lib.FLAG_PREFETCH):
            for nt in (0, _lib.FLAG_NONTEMPORAL):
                tag = f"u{u}{'_pf' if pf else ''}{'_nt' if nt else ''}"
                yield f"stream_{tag}", lambda L, f=U(u) | pf | nt: S(L, band, kernel="stream", flags=f, options=plain)
                yield f"csr3_{tag}", lambda L, f=U(u) | pf | nt: S(L, band, tasks, flags=f, options=plain)
    # column formats: 32-bit, 16-bit offsets per 256-nonzero block, per 64-row group
    for name, A in (("f64", band), ("f32", band32)):
        for kern, maps in (("stream", None), ("csr3", tasks)):
            yield f"{kern}_{name}_col32", lambda L, A=A, m=maps, k=kern: S(
                L, A, m, kernel=k, flags=_lib.FLAG_NO_COL16, options=plain)
            yield f"{kern}_{name}_col16_blocks", lambda L, A=A, m=maps, k=kern: S(
                L, A, m, kernel=k, flags=_lib.FLAG_COL16, options={**plain, "col16_group": -1})
            yield f"{kern}_{name}_col16_groups", lambda L, A=A, m=maps, k=kern: S(
                L, A, m, kernel=k, options={**plain, "col16_group": 1})
            yield f"{kern}_{name}_xwin", lambda L, A=A, m=maps, k=kern: S(L, A, m, kernel=k, options={"x_dict": -1})
    # STREAM workgroup shapes, unpadded and padded, x windows on and off
    for w in (1, 2, 4):
        for name, A in (("band", band), ("pad_f64", blocks32(np.float64)), ("pad_f32", blocks32(np.float32))):
            for xw in (0, -1):
                yield f"stream_{name}_w{w}{'_xwin' if xw == 0 else ''}", lambda L, A=A, w=w, xw=xw: S(
                    L, A, kernel="stream", options={"x_dict": -1, "stream_waves": w, "x_windows": xw})
    # CSR3 with 1, 2, 4 and 8 waves (a workgroup per super-super-row), and its
    # dictionaries of 4 and 8 tasks
    for ssrs, srs in ((7, 8), (12, 10), (20, 10), (40, 10), (400, 2)):
        maps = hspmv.build_csr3_maps(st21, ssrs, srs)
        yield f"csr3_ssr_{ssrs}x{srs}", lambda L, m=maps: S(L, st21, m, options={"csr3_plan": "ssr", "x_dict": -1})
        yield f"csr3_ssr_{ssrs}x{srs}_dict", lambda L, m=maps: S(L, st21, m, options={"csr3_plan": "ssr", "x_dict": 1,
                                                                                     "row_slices": -1})
    maps21 = hspmv.build_csr3_maps(st21, 20, 10)
    yield "stream_dict", lambda L: S(L, st21, kernel="stream", options=OFF)
    yield "csr3_dict", lambda L: S(L, st21, maps21, options=OFF)
    yield "stream_dict_f32", lambda L: S(L, st21.astype(np.float32), kernel="stream", options=OFF)
    yield "slices_pos16", lambda L: S(L, block_run(20), kernel="stream", options=ON)
    yield "slices_pos12", lambda L: S(L, st21, kernel="stream", options=ON)
    yield "slices_pos12_csr3_nt", lambda L: S(L, st21, maps21, flags=_lib.FLAG_NONTEMPORAL, options=ON)
    st32 = gen.stencil27(21, dtype=np.float32)
    yield "mixed_stream", lambda L: S(L, st32, kernel="stream", options=plain, vector_dtype=np.float64)
    yield "mixed_dict", lambda L: S(L, st32, kernel="stream", options=OFF, vector_dtype=np.float64)
    yield "mixed_slices", lambda L: S(L, st32, kernel="stream", options=ON, vector_dtype=np.float64)
    yield "x_slabs3", lambda L: S(L, st21, kernel="stream", options={"x_slabs": 3})
    lr = long_rows()
    yield "long_rows_chunks", lambda L: S(L, lr)
    yield "long_rows_chunks_nt", lambda L: S(L, lr, flags=_lib.FLAG_NONTEMPORAL)
    yield "long_rows_serial_forked", lambda L: S(L, lr, options={"deterministic": 3})
    for lanes in (1, 2, 4, 8, 16, 32, 64):
        yield f"vector_l{lanes}", lambda L, f=_lib.lanes_flag(lanes): S(L, lap, kernel="vector", flags=f)
    pl = gen.powerlaw(60_000, seed=5, dtype=np.float64)
    pl32 = pl.astype(np.float32)
    for u in (4, 8, 16):
        yield f"csort_u{u}", lambda L, u=u: S(L, pl, kernel="csort", options={"csort_chunk_u": u})
        yield f"csort_u{u}_f32", lambda L, u=u: S(L, pl32, kernel="csort", options={"csort_chunk_u": u})
    yield "csort_reproducible", lambda L: S(L, pl, kernel="csort", options={"deterministic": 2})
    lm = long_matrix(np.float64)
    for k in (1, 2, 3, 5, 9, 17):
        yield f"spmm_k{k}", lambda L, k=k: spmm_case(L, lm, k, False)
    yield "spmm_k3_f32", lambda L: spmm_case(L, long_matrix(np.float32), 3, False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = load(a.lib)
    out = []
    for name, make in cases():
        info, _ = make(L)
        rec = {"case": name, "plan": {k: info[k] for k in PLAN if k in info} if "kernel" in info else info}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in out))
    print(f"{len(out)} cases")
    return 0


if __name__ == "__main__":
    sys.exit(main())
