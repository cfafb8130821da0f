#!/usr/bin/env python3
"""The handle reports of two libhspmv builds side by side, in ONE process.

    python heterogeneous-spmv_amd/tools/info_ab.py --libs A.so,B.so [--out F.jsonl]

One small handle per device-table family (the matrices tests/ builds for
them), created by each library (loaded as tools/ab.py loads them):
hspmv_get_info_sized / hspmv_mm_get_info field by field, and y after one
SpMV byte by byte.  One JSON line per family: the first library's report, and
under "diff" every field in which the second differs (placement_us is not
compared).  Exit status 1 when any family differs.
"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(REPO / "tests"))

import torch  # noqa: E402  (load order: torch's HIP runtime first)

import hspmv  # noqa: E402
from hspmv import _lib, gen  # noqa: E402
from hspmv.api import _KERNELS, dtype_code  # noqa: E402
from ab import load  # noqa: E402
from test_csort import _hub_rows as csort_hub_rows, _long_rows as csort_long_rows  # noqa: E402
from test_gpu_parity import _band_random  # noqa: E402
from test_serial import long_rows  # noqa: E402
from test_slice_pos12 import OFF, ON, block_run, ragged_all_widths  # noqa: E402
from test_spmm import long_matrix  # noqa: E402

SKIP = {"placement_us", "reserved0"}


def fields(st):
    out = {}
    for k, _ in st._fields_:
        v = getattr(st, k)
        out[k] = list(v) if hasattr(v, "__len__") else v
    return out


def spmv_case(L, A, maps=None, kernel="auto", flags=0, options=None, devices=None, vector_dtype=None,
              borrowed=False, updatable=False, update=False):
    """(info, y) of one handle of library L.  updatable: created by
    hspmv_create_updatable; update: one hspmv_update_values (host memory, other
    values) before the SpMV, so y and the report are those after the refresh."""
    vdt = np.dtype(A.val.dtype if vector_dtype is None else vector_dtype)
    keep = []
    if borrowed:  # the matrix arrays stay the caller's (HSPMV_FLAG_DEVICE_PTRS)
        keep = [torch.from_numpy(a).cuda() for a in (A.row_ptr, A.col_idx, A.val)]
        torch.cuda.synchronize()
        cs = _lib.Csr(A.m, A.n, A.nnz, *(t.data_ptr() for t in keep), dtype_code(A.val.dtype))
        flags |= _lib.FLAG_DEVICE_PTRS
    else:
        cs = A.c_struct()
    ms = maps.c_struct() if maps is not None else None
    opt = _lib.make_options(_KERNELS[kernel] | flags, options, devices=devices)
    h = C.c_void_p()
    if updatable:
        rc = L.hspmv_create_updatable(C.byref(h), C.byref(cs), C.byref(ms) if ms else None, C.byref(opt),
                                      dtype_code(vdt))
    elif vdt != A.val.dtype:
        rc = L.hspmv_create_mixed(C.byref(h), C.byref(cs), C.byref(ms) if ms else None, C.byref(opt),
                                  dtype_code(vdt))
    else:
        rc = L.hspmv_create_ex(C.byref(h), C.byref(cs), C.byref(ms) if ms else None, C.byref(opt))
    assert rc == 0, L.hspmv_last_error()
    if update:
        v2 = np.ascontiguousarray(A.val * A.val.dtype.type(0.75) - A.val.dtype.type(0.5))
        assert L.hspmv_update_values(h, v2.ctypes.data, 0) == 0, L.hspmv_last_error()
    inf = _lib.Info()
    assert L.hspmv_get_info_sized(h, C.byref(inf), C.sizeof(inf)) == 0
    x = gen.rand_x(A.n, 42).astype(vdt)
    y = np.empty(A.m, dtype=vdt)
    assert L.hspmv_set_x(h, x.ctypes.data) == 0 and L.hspmv_spmv(h) == 0
    assert L.hspmv_get_y(h, y.ctypes.data) == 0
    L.hspmv_destroy(h)
    del keep
    return fields(inf), y


def spmm_case(L, A, k, borrowed):
    keep = []
    flags = 0
    if borrowed:
        keep = [torch.from_numpy(a).cuda() for a in (A.row_ptr, A.col_idx, A.val)]
        torch.cuda.synchronize()
        cs = _lib.Csr(A.m, A.n, A.nnz, *(t.data_ptr() for t in keep), dtype_code(A.val.dtype))
        flags = _lib.FLAG_DEVICE_PTRS
    else:
        cs = A.c_struct()
    opt = _lib.make_options(flags, None)
    h = C.c_void_p()
    assert L.hspmv_mm_create(C.byref(h), C.byref(cs), k, C.byref(opt)) == 0, L.hspmv_last_error()
    inf = _lib.MmInfo()
    assert L.hspmv_mm_get_info(h, C.byref(inf), C.sizeof(inf)) == 0
    X = np.ascontiguousarray(gen.rand_x(A.n * k, 42).reshape(A.n, k).astype(A.val.dtype))
    Y = np.empty((A.m, k), dtype=A.val.dtype)
    assert L.hspmv_mm_set_x(h, X.ctypes.data, k) == 0 and L.hspmv_mm_spmm(h) == 0
    assert L.hspmv_mm_get_y(h, Y.ctypes.data, k) == 0
    L.hspmv_mm_destroy(h)
    del keep
    return fields(inf), Y


def families():
    lap, st20, st21 = gen.laplace2d(200, 150), gen.stencil27(20), gen.stencil27(21)
    band = gen.banded(5000, per_row=10, half=32).astype(np.float32)
    pl = gen.powerlaw(60_000, seed=5, dtype=np.float64)
    lr = long_rows()
    no_dict = {"x_dict": -1}
    S = spmv_case
    yield "stream", lambda L: S(L, lap, kernel="stream")
    yield "csr3_maps", lambda L: S(L, st20, hspmv.build_csr3_maps(st20, 20, 10))
    yield "vector", lambda L: S(L, st21, kernel="vector")
    yield "col16_blocks", lambda L: S(L, band, kernel="stream", flags=_lib.FLAG_COL16,
                                      options={"x_dict": -1, "col16_group": -1})
    yield "col16_groups", lambda L: S(L, band, kernel="stream", options={"col16_group": 1, "x_dict": -1})
    # block bases with one high-bit plane (random columns within +-50 000 of
    # the diagonal), and group bases over the packed CSR3 tasks
    yield "col16_blocks_plane", lambda L: S(L, _band_random(150000, 10, 50000, 6), kernel="stream",
                                            flags=_lib.FLAG_COL16, options={"x_dict": -1, "col16_group": -1})
    yield "col16_groups_csr3", lambda L: S(L, st20, hspmv.build_csr3_maps(st20, 20, 10), kernel="csr3",
                                           options={"col16_group": 1, "x_dict": -1})
    band64 = gen.banded(5000, per_row=10, half=32, seed=5)
    yield "x_windows", lambda L: S(L, band64, kernel="stream", options=no_dict)
    yield "x_dict_stream", lambda L: S(L, st21, kernel="stream", options=OFF)
    yield "x_dict_csr3", lambda L: S(L, st21, hspmv.build_csr3_maps(st21, 20, 10), options=OFF)
    yield "slices_pos16", lambda L: S(L, block_run(20), kernel="stream", options=ON)
    yield "slices_pos12", lambda L: S(L, st21, kernel="stream", options=ON)
    yield "slices_pos12_csr3", lambda L: S(L, st21, hspmv.build_csr3_maps(st21, 20, 10), options=ON)
    yield "slices_pos12_ragged_f32", lambda L: S(L, ragged_all_widths(np.float32), kernel="stream", options=ON)
    yield "x_slabs3", lambda L: S(L, st21, kernel="stream", options={"x_slabs": 3})
    yield "csort", lambda L: S(L, pl, kernel="csort")
    yield "csort_reproducible", lambda L: S(L, pl, kernel="csort", options={"deterministic": 2})
    # every branch of the csort tables: fp32, one and four column parts,
    # sliced long rows, segmented hub-row chunks; each also reproducible
    # (fixed-point: y byte for byte)
    csort_mats = [("f32", pl.astype(np.float32), {}), ("parts1", pl, {"csort_parts": 1}),
                  ("parts4", pl, {"csort_parts": 4}), ("long_rows", csort_long_rows(), {}),
                  ("hub_rows", csort_hub_rows(), {})]
    for tag, A, o in csort_mats:
        yield f"csort_{tag}", lambda L, A=A, o=o: S(L, A, kernel="csort", options=o)
        yield (f"csort_{tag}_reproducible",
               lambda L, A=A, o=o: S(L, A, kernel="csort", options={**o, "deterministic": 2}))
    # new values before the SpMV (hspmv_update_values): the refresh of the
    # column-sorted entry stream of an updatable handle, and of the row slices
    yield "csort_updatable_update", lambda L: S(L, pl, kernel="csort", updatable=True, update=True)
    yield "slices_pos12_update", lambda L: S(L, st21, kernel="stream", options=ON, update=True)
    yield "long_rows", lambda L: S(L, lr)
    yield "long_rows_serial", lambda L: S(L, lr, options={"deterministic": 3})
    yield "devices_0_0", lambda L: S(L, lap, devices=[0, 0])
    yield "mixed", lambda L: S(L, gen.stencil27(21, dtype=np.float32), vector_dtype=np.float64)
    yield "borrowed_stream", lambda L: S(L, lap, kernel="stream", borrowed=True)
    lm = long_matrix(np.float64)
    yield "spmm_k4", lambda L: spmm_case(L, lm, 4, False)
    yield "spmm_k4_borrowed", lambda L: spmm_case(L, lm, 4, True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", required=True, help="two library paths, comma-separated")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    paths = a.libs.split(",")
    assert len(paths) == 2
    libs = [load(p) for p in paths]
    out, bad = [], 0
    for name, make in families():
        (i0, y0), (i1, y1) = make(libs[0]), make(libs[1])
        diff = {k: [i0[k], i1[k]] for k in i0 if k not in SKIP and i0[k] != i1[k]}
        # (the default csort sums with atomics in any order: deterministic = 0)
        same = y0.tobytes() == y1.tobytes() if i0.get("deterministic", 1) else np.allclose(y0, y1, rtol=1e-12)
        rec = {"family": name, "libs": paths, "y_equal": bool(same),
               "diff": diff, "info": {k: v for k, v in i0.items() if k not in SKIP}}
        bad += bool(diff) or not rec["y_equal"]
        out.append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in out))
    print(f"{len(out)} families, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
