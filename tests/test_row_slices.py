"""Row slices: the lane-per-row kernel of dictionary handles whose rows are
all summed serially (hspmv_slices.cpp, slice_kernel.cuh hspmv_slices).

Host: hspmv_slices_plan's arrays hold exactly the input CSR (values, and the
columns through the dictionary run records), its counts match the CPU model
of the flagship matrix, and the eligibility rules answer as documented.

GPU: y of a handle with ``row_slices = 1`` equals, byte for byte, y of the
same options with ``row_slices = -1`` (the chunked dictionary kernel): both
multiply and add each row's products left to right from 0.
"""
import numpy as np
import pytest

import hspmv
from hspmv import gen
from hspmv.api import CsrMatrix

F64_SERIAL, F32_SERIAL = 40, 56  # hspmv_internal.h kSerialMax / kSerialMaxF32


# ------------------------------------------------------------------ matrices

def fixed_rows(L, m=200, dtype=np.float64, seed=3):
    """m rows of exactly L nonzeros, columns r .. r + L - 1 (3 full slices and
    one of 8 rows)."""
    rng = np.random.default_rng(seed + L)
    rp = (np.arange(m + 1, dtype=np.int64) * L).astype(np.int32)
    col = (np.arange(m)[:, None] + np.arange(L)[None, :]).astype(np.int32).ravel()
    val = rng.uniform(-1.0, 1.0, m * L).astype(dtype)
    return CsrMatrix(m, m + L, rp, col, val)


def ragged(lens, dtype=np.float64, seed=5, n=None):
    """Row r has lens[r] nonzeros in columns r, r + 2, r + 4, ..."""
    lens = np.asarray(lens, np.int64)
    m = len(lens)
    rng = np.random.default_rng(seed)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([r + 2 * np.arange(k) for r, k in enumerate(lens)] + [np.zeros(0, np.int64)])
    n = n or int(m + 2 * lens.max() + 1)
    val = rng.uniform(-1.0, 1.0, int(lens.sum())).astype(dtype)
    return CsrMatrix(m, n, rp, col.astype(np.int32), val)


def with_empty_rows(dtype=np.float64):
    """320 rows of 3 nonzeros, two rows of every slice empty and rows 64..127
    (one whole slice, w = 0) empty: few enough empty rows for the padding rule."""
    lens = np.full(320, 3)
    lens[5::32] = 0
    lens[64:128] = 0
    return ragged(lens, dtype)


def one_long_row_per_slice(dtype=np.float64):
    """Short rows with one 40-nonzero row in each slice: padding every row to
    40 slots would move far more bytes than the CSR order."""
    lens = np.full(256, 2)
    lens[::64] = 40
    return ragged(lens, dtype)


def paths(A):
    """(maps, kernel) of the two dictionary shapes: CSR3 tasks and STREAM."""
    return [("csr3", hspmv.build_csr3_maps(A, 20, 10), "auto"), ("stream", None, "stream")]


ON = {"x_dict": 1, "row_slices": 1}
OFF = {"x_dict": 1, "row_slices": -1}


# ------------------------------------------------------------------ host

def rebuild_and_compare(A, maps, kernel, options=ON):
    """The slice arrays hold A: every nonzero sits at its slot with its value
    and the position whose run record gives back its column; everything else
    is 0; the lengths are the rows' lengths."""
    S = hspmv.slices_plan(A, maps, kernel=kernel, options=options)
    assert S["why"] == "ok", S["why"]
    blk, runs, _ = hspmv.xdict_plan(A, maps, kernel=kernel, options=options)
    desc, G = S["desc"].astype(np.int64), 16 // A.val.dtype.itemsize
    assert desc.shape[0] == S["n_desc"] + 1
    assert desc[-1, 1] == A.m and 64 * desc[-1, 0] == S["padded_entries"] == len(S["val"])
    rows = np.diff(desc[:, 1])
    assert rows.min() >= 0 and rows.max() <= 64 and int((rows > 0).sum()) == S["n_slices"]
    assert len(blk) - 1 == (S["n_desc"] + 3) // 4  # four tasks per dictionary block
    lens = np.diff(A.row_ptr).astype(np.int64)
    assert np.array_equal(S["len"], lens.astype(np.uint8))
    # each row's slice: the last task starting at or before it (empty tasks share a start)
    r = np.repeat(np.arange(A.m, dtype=np.int64), lens)
    k = np.arange(A.nnz, dtype=np.int64) - np.repeat(A.row_ptr[:-1].astype(np.int64), lens)
    s = np.searchsorted(desc[:-1, 1], np.arange(A.m), side="right") - 1
    width = np.diff(desc[:, 0])
    # the slice width is the longest of its rows: no alignment padding
    longest = np.zeros(len(width), np.int64)
    np.maximum.at(longest, s, lens)
    assert np.array_equal(width, longest)
    sn, i, w = s[r], r - desc[s[r], 1], width[s[r]]
    base = 64 * desc[sn, 0]

    def at(g):
        wg = w // g * g
        return np.where(k < wg, base + (k // g) * 64 * g + i * g + k % g, base + k * 64 + i)

    ev, ep = at(G), at(4)
    assert np.array_equal(S["val"][ev].view(np.uint8), A.val.view(np.uint8))
    hit = np.zeros(len(S["val"]), bool)
    hit[ev] = True
    assert not S["val"][~hit].any()
    hit[:] = False
    hit[ep] = True
    assert not S["pos"][~hit].any()
    # columns through the run records of the nonzero's dictionary block
    pos = S["pos"][ep].astype(np.int64)
    nb = len(blk) - 1
    is_rec = np.ones(len(runs), bool)
    is_rec[blk[1:] - 1] = False  # the sentinels
    rec_blk = np.repeat(np.arange(nb), np.diff(blk))[is_rec]
    key = rec_blk * (1 << 17) + runs[is_rec, 1]
    j = np.searchsorted(key, (sn // 4) * (1 << 17) + pos, side="right") - 1
    assert np.array_equal(rec_blk[j], sn // 4)
    col = runs[is_rec, 0][j] + pos - runs[is_rec, 1][j]
    assert np.array_equal(col, A.col_idx)
    return S


SMALL = {
    "stencil21": lambda dt: gen.stencil27(21, dtype=dt),
    "laplace": lambda dt: gen.laplace2d(300, 200).astype(dt),
    "banded": lambda dt: gen.banded(30000, per_row=10, half=32).astype(dt),
    "empty_rows": with_empty_rows,
}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", sorted(SMALL))
def test_slices_plan_holds_the_matrix(name, dtype):
    A = SMALL[name](dtype)
    for _, maps, kernel in paths(A):
        rebuild_and_compare(A, maps, kernel)
    if name == "stencil21":
        assert A.m == 9261 and sorted(set(np.diff(A.row_ptr))) == [8, 12, 18, 27]
        S = hspmv.slices_plan(A, None, kernel="stream", options=ON)
        assert S["n_slices"] == 145 and S["desc"][-1, 1] - S["desc"][-2, 1] == 45


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_slices_plan_every_width_remainder(dtype):
    """Fixed row lengths 1..8 and the serial bound: every w mod 4 and w mod 2
    (value groups of 2 fp64 / 4 fp32, position groups of 4)."""
    bound = F64_SERIAL if dtype == np.float64 else F32_SERIAL
    for L in list(range(1, 9)) + [bound - 1, bound]:
        A = fixed_rows(L, dtype=dtype)
        for _, maps, kernel in paths(A):
            S = rebuild_and_compare(A, maps, kernel)
            assert S["padded_entries"] == 64 * L * S["n_slices"]


def test_slices_plan_flagship_model():
    """C3 (27-point 125^3 RCM stencil): 30,518 slices, 52,315,008 padded
    entries = 1.0081 x nnz, and the arrays give the matrix back."""
    A = gen.stencil27(125)
    assert A.m == 1953125 and A.nnz == 51895117
    lens, cnt = np.unique(np.diff(A.row_ptr), return_counts=True)
    assert dict(zip(lens.tolist(), cnt.tolist())) == {8: 8, 12: 1476, 18: 90774, 27: 1860867}
    maps = hspmv.build_csr3_maps(A, *hspmv.csr3_params(A.nnz / A.m, "volta"))
    S = rebuild_and_compare(A, maps, "auto", options=None)  # auto: it streams from HBM
    assert S["n_slices"] == 30518 and S["padded_entries"] == 52315008
    assert S["n_desc"] == 30518  # no occupancy cuts: the LDS of a workgroup is its dictionary


def test_slices_eligibility_answers():
    A = gen.stencil27(21)
    maps = hspmv.build_csr3_maps(A, 20, 10)
    def why(M, mp=None, kernel="auto", **o):
        return hspmv.slices_plan(M, mp, kernel=kernel, options=o or None, fill=False)["why"]

    assert why(A, maps, x_dict=1, row_slices=1) == "ok"
    assert why(A, None, kernel="stream", x_dict=1, row_slices=1) == "ok"
    # auto: only matrices that stream from HBM (the dictionaries' own rule)
    assert why(A, maps, x_dict=1, row_slices=-1) == "off"
    assert why(A, maps, x_dict=-1, row_slices=1) == "no_dict"
    # the packed and SSR CSR-3 plans keep the chunked kernel
    assert why(A, maps, x_dict=1, row_slices=1, csr3_plan="packed") == "shape"
    assert why(A, maps, x_dict=1, row_slices=1, csr3_plan="ssr") == "shape"
    assert why(A, None, kernel="vector", row_slices=1) == "shape"
    assert why(A, maps, row_slices=1, deterministic="serial") == "chunked"
    # a row past the dtype's serial bound
    for dt, bound in ((np.float64, F64_SERIAL), (np.float32, F32_SERIAL)):
        lens = np.full(130, 3)
        lens[70] = bound
        assert why(ragged(lens, dt), None, kernel="stream", row_slices=1) == "ok"
        lens[70] = bound + 1
        assert why(ragged(lens, dt), None, kernel="stream", row_slices=1) == "long_row"
    lens = np.full(130, 3)
    lens[70] = 5000
    assert why(ragged(lens), None, kernel="stream", row_slices=1) == "split_rows"
    # padding to one 40-nonzero row per slice would move more bytes than the
    # CSR order: refused before the residence rule is asked, whatever the size
    B = one_long_row_per_slice()
    S = hspmv.slices_plan(B, None, kernel="stream", options={"x_dict": 1})
    assert S["why"] == "bytes" and S["padded_entries"] == 4 * 64 * 40 and "val" not in S
    assert why(B, hspmv.build_csr3_maps(B, 20, 10), x_dict=1) == "bytes"
    assert B.nnz == 4 * (40 + 63 * 2)
    # (row_slices = 1 asks for the kernel wherever it can run: the byte and
    # residence rules are auto's -- stencil27(21) itself pads 10 %)
    assert why(B, None, kernel="stream", row_slices=1) == "ok"
    assert why(A, maps, x_dict=1) == "bytes"
    L = gen.laplace2d(300, 200)
    assert why(L, None, kernel="stream", x_dict=1) == "resident"


def test_slices_abi_fields_are_appended():
    from hspmv import _lib
    assert _lib.Options._fields_[-1][0] == "row_slices" and "row_slices" in _lib.Options.TUNABLE
    assert _lib.Info.row_slices.offset > _lib.Info.csort_part_begin.offset
    assert _lib.Info.row_slices.offset >= _lib.Info.heavy_group_frac.offset + 8  # hspmv_get_info_sized only
    assert _lib.make_options(0, {"row_slices": -1}).row_slices == -1


# ------------------------------------------------------------------ GPU

def run_pair(A, maps, kernel, x, want=1):
    """y with row slices and y of the chunked kernel, same options otherwise."""
    with hspmv.SpMV(A, maps, kernel=kernel, device=0, options=ON) as op:
        y1, i1 = op(x), op.info
    with hspmv.SpMV(A, maps, kernel=kernel, device=0, options=OFF) as op:
        y0, i0 = op(x), op.info
    assert i1["row_slices"] == want and i0["row_slices"] == 0
    assert i1["x_dict"] == 1 and i0["x_dict"] == 1
    assert i1["kernel_name"] == i0["kernel_name"] and i1["blocks"] > 0
    if want:
        # one copy of the values and positions on the device: the slice streams,
        # lengths and descriptors in place of the CSR-order values and positions
        S = hspmv.slices_plan(A, maps, kernel=kernel, options=ON, fill=False)
        sv = A.val.dtype.itemsize
        assert (i1["device_bytes"] - i0["device_bytes"] <=
                (S["padded_entries"] - A.nnz) * (sv + 2) + A.m + 8 * (S["n_desc"] + 1) + 1024)
    assert y1.tobytes() == y0.tobytes()
    return y1


@pytest.fixture(scope="module")
def need_gpu():
    assert hspmv.device_count() >= 1, "no HIP device visible: the gpu tests must run on the MI355X box"


DTYPES = [np.float64, np.float32]
PATHS = ["csr3", "stream"]


def path_of(A, which):
    return [p for p in paths(A) if p[0] == which][0][1:]


@pytest.mark.gpu
@pytest.mark.parametrize("which", PATHS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["stencil21", "laplace", "banded", "empty_rows"])
def test_gpu_slices_bitwise_equal_to_chunked(need_gpu, name, dtype, which):
    A = SMALL[name](dtype)
    maps, kernel = path_of(A, which)
    x = gen.rand_x(A.n, 42).astype(dtype)
    y = run_pair(A, maps, kernel, x)
    if name == "empty_rows":
        assert not y[np.diff(A.row_ptr) == 0].any()  # empty rows (and the empty slice) store 0
    if name == "stencil21" and dtype == np.float64:
        from test_gpu_parity import check_fp64
        check_fp64(A, x, y, exact_rows=slice(None))


@pytest.mark.gpu
@pytest.mark.parametrize("which", PATHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_slices_every_width_remainder(need_gpu, dtype, which):
    Ls = list(range(1, 9)) + [39, 40] + ([55, 56] if dtype == np.float32 else [])
    for L in Ls:
        A = fixed_rows(L, dtype=dtype)
        maps, kernel = path_of(A, which)
        run_pair(A, maps, kernel, gen.rand_x(A.n, 7).astype(dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("which", PATHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_slices_refused_for_a_row_past_the_serial_bound(need_gpu, dtype, which):
    lens = np.full(300, 4)
    lens[131] = (F64_SERIAL if dtype == np.float64 else F32_SERIAL) + 1
    A = ragged(lens, dtype)
    maps, kernel = path_of(A, which)
    run_pair(A, maps, kernel, gen.rand_x(A.n, 9).astype(dtype), want=0)


@pytest.mark.gpu
@pytest.mark.parametrize("which", PATHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_slices_inf_and_nan_in_x(need_gpu, dtype, which):
    """inf and NaN in x -- also at dictionary position 0 of some blocks,
    where every padded slot points -- reach exactly the rows that reference
    them: the padding is masked, never multiplied in."""
    A = gen.stencil27(21, dtype=dtype)
    maps, kernel = path_of(A, which)
    blk, runs, _ = hspmv.xdict_plan(A, maps, kernel=kernel, options=ON)
    x = gen.rand_x(A.n, 11).astype(dtype)
    first = runs[blk[:-1], 0]  # x entry staged at position 0 of each block
    assert np.all(runs[blk[:-1], 1] == 0)
    x[first[1]] = np.inf
    x[first[len(first) // 2]] = np.nan
    x[first[-1]] = -np.inf
    x[A.n // 3] = np.nan
    x[A.n // 3 + 5] = np.inf
    y = run_pair(A, maps, kernel, x)
    # rows that reference no non-finite x stay finite
    bad = ~np.isfinite(x)
    touched = np.add.reduceat(bad[A.col_idx].astype(np.int64), A.row_ptr[:-1]) > 0
    assert np.isfinite(y[~touched]).all() and not np.isfinite(y[touched]).any()
