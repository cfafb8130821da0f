"""hspmv_create_updatable / hspmv_can_update_values: hspmv_update_values on
column-sorted handles.

An updatable handle keeps, per stored entry of the column-sorted stream, the
CSR index it came from, so new values can be put in place on the device
(refresh.hip: hspmv_refresh_csort, and under fixed-point slots
hspmv_refresh_row_scales before it).  The yardstick is test_update_values.py's:
a handle newly created from the new values.  The default column-sorted slots
add in atomic order, so y is bit-stable only where the arithmetic is exact
(small integers) or under deterministic = 2 (fixed-point slots); both are used.

One small matrix reaches every branch of the planner and the refresh: chunks
closed early on the 65535-column span, empty rows, a sliced row of contiguous
columns (segmented chunks, several slices in one column part), a sliced row of
random columns, and a crowded short row.
"""
import ctypes as C
import re
from functools import lru_cache

import numpy as np
import pytest

import hspmv
import oracle
from conftest import GOLDEN
from hspmv import _lib, gen
from test_update_values import (BUILD, E_INVALID, assert_oracle, bits, cli, cuda, need_gpu,  # noqa: F401
                                new_values, run, with_values)

gpu = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
M, N = 6000, 300_000
EMPTY = tuple(range(100, 6000, 500))  # a dozen empty rows
ROW_HUB, ROW_SPREAD, ROW_CROWDED, ROW_ZERO, ROW_SPAN = 41, 2500, 4000, 77, 1234


# ------------------------------------------------------------------ CPU

def test_symbols_declared_and_bound():
    text = _lib.HEADER.read_text()
    assert re.search(r"int hspmv_create_updatable\(hspmv_handle \*\*h, const hspmv_csr \*A, "
                     r"const hspmv_csr3_maps \*maps,\s+const hspmv_options \*opt, int vector_dtype\);", text)
    assert re.search(r"int hspmv_can_update_values\(const hspmv_handle \*h\);", text)
    res, args = _lib.SIGNATURES["hspmv_create_updatable"]
    assert res is C.c_int and args == _lib.SIGNATURES["hspmv_create_mixed"][1]
    assert _lib.SIGNATURES["hspmv_can_update_values"] == (C.c_int, [C.c_void_p])


def test_header_names_the_calls_under_1_1():
    text = _lib.HEADER.read_text()
    assert "#define HSPMV_VERSION_MINOR 1\n" in text and text.count("Also in 1.1") == 1
    para = text.split("Also in 1.1")[1].split("*/")[0]
    assert para.index("HSPMV_VALUES_DEVICE") < para.index("hspmv_create_updatable") < \
        para.index("hspmv_can_update_values")


def test_null_arguments_without_a_device():
    L = _lib.lib()
    assert L.hspmv_can_update_values(None) == 0
    A = gen.laplace2d(4, 3)
    cs = A.c_struct()
    opt = _lib.make_options(0, None)
    assert L.hspmv_create_updatable(None, C.byref(cs), None, C.byref(opt), _lib.F64) == E_INVALID
    assert _lib.last_error()
    h = C.c_void_p()
    assert L.hspmv_create_updatable(C.byref(h), None, None, C.byref(opt), _lib.F64) == E_INVALID and not h
    # the dtype pair is hspmv_create_mixed's rule (fp32 vectors over fp64 values)
    assert L.hspmv_create_updatable(C.byref(h), C.byref(cs), None, C.byref(opt), _lib.F32) == E_INVALID and not h


# ------------------------------------------------------------------ the matrix

@lru_cache(maxsize=None)
def pattern():
    rng = np.random.default_rng(7)
    lens = rng.integers(6, 15, M)
    lens[list(EMPTY)] = 0
    rows = {}
    c0 = 120_000
    rows[ROW_HUB] = np.arange(c0, c0 + 9000)  # sliced (> 4096), contiguous: segmented chunks
    rows[ROW_SPREAD] = np.sort(rng.choice(N, 9000, replace=False))  # sliced, both column parts
    rows[ROW_CROWDED] = np.arange(200_000, 203_000)  # a crowded short row
    for r, c in rows.items():
        lens[r] = len(c)
    cols = []
    for r in range(M):
        cols.append(rows[r] if r in rows else np.sort(rng.choice(N, lens[r], replace=False)))
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return rp, np.concatenate(cols).astype(np.int32)


def matrix(val):
    rp, ci = pattern()
    return hspmv.CsrMatrix(M, N, rp, ci, val)


def row_slice(r):
    rp, _ = pattern()
    return slice(int(rp[r]), int(rp[r + 1]))


@lru_cache(maxsize=None)
def int_values(seed, dtype):
    """Integers in [-4, 4], a few of them 0: every product and partial sum is
    exact (|sum| <= 9000 * 16 < 2^24), so y does not depend on the order."""
    rng = np.random.default_rng(seed)
    return rng.integers(-4, 5, pattern()[0][-1]).astype(dtype)


@lru_cache(maxsize=None)
def int_x(dtype):
    return np.random.default_rng(99).integers(-4, 5, N).astype(dtype)


@lru_cache(maxsize=None)
def rand_values(seed, dtype):
    """U(-1, 1) with one all-zero row (ROW_ZERO)."""
    v = np.random.default_rng(seed).uniform(-1.0, 1.0, pattern()[0][-1]).astype(dtype)
    v[row_slice(ROW_ZERO)] = 0
    return v


def fresh_y(val, x, **kw):
    """y of a handle newly created (not updatable) over val, held against the oracle."""
    A = matrix(val)
    with hspmv.SpMV(A, kernel="csort", **kw) as f:
        assert f.info["kernel_name"] == "csort" and not f.can_update
        y = f(x)
    assert_oracle(A, x, y)
    return y


def exact_oracle(val, x):
    rp, ci = pattern()
    return oracle.spmv(rp, ci, val, x)


# ------------------------------------------------------------------ GPU

@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_matrix_reaches_every_branch(need_gpu, dtype):
    with hspmv.SpMV(matrix(rand_values(1, dtype)), kernel="csort") as op:
        info = op.info
    assert info["kernel_name"] == "csort" and info["csort_parts"] >= 2
    assert info["csort_seg_chunks"] > 0 and info["n_split_rows"] == 2  # the two sliced rows
    # chunks closed early on the 65535-column span: more chunks than the entries fill
    per_chunk = 64 * info["chunk_u"]
    assert info["csort_chunks"] * per_chunk > pattern()[0][-1] + per_chunk * info["blocks"]


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_default_mode_is_exact(need_gpu, dtype):
    v0, v1, x = int_values(1, dtype), int_values(2, dtype), int_x(dtype)
    assert np.count_nonzero(v1 == 0) > 3 and np.any(v0 != v1)
    want = {0: fresh_y(v0, x), 1: fresh_y(v1, x)}
    for k, v in ((0, v0), (1, v1)):
        assert np.array_equal(want[k], exact_oracle(v, x))
    assert not np.array_equal(bits(want[0]), bits(want[1]))
    with hspmv.SpMV(matrix(v0), kernel="csort", updatable=True) as op:
        assert op.can_update and op.info["kernel_name"] == "csort"
        info = op.info
        op.set_x(x)
        assert np.array_equal(bits(run(op)), bits(want[0]))
        op.update_values(v1)
        assert np.array_equal(bits(run(op)), bits(want[1])) and np.array_equal(op.A.val, v1)
        op.update_values(v0)
        assert np.array_equal(bits(run(op)), bits(want[0]))
        t = cuda(v1)
        op.update_values_device(t.data_ptr())
        assert np.array_equal(bits(run(op)), bits(want[1]))  # (get_y synchronises: t outlives the work)
        assert op.info == info


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_default_mode_random_values(need_gpu, dtype):
    v0, v1 = rand_values(1, dtype), rand_values(2, dtype)
    x = gen.rand_x(N, 5).astype(dtype)
    with hspmv.SpMV(matrix(v0), kernel="csort", updatable=True) as op:
        op.set_x(x)
        assert_oracle(matrix(v0), x, run(op))
        op.update_values(v1)
        y = run(op)
    assert_oracle(matrix(v1), x, y)
    with pytest.raises(AssertionError):  # ... and is no longer the old values' y
        assert_oracle(matrix(v0), x, y)


def det2_steps(dtype):
    """The value sets of the deterministic = 2 test, from rand_values(1)."""
    rp, _ = pattern()
    v0 = rand_values(1, dtype)
    v1 = rand_values(2, dtype)
    rows = np.repeat(np.arange(M), np.diff(rp))
    scaled = (v1 * np.where(rows % 3 == 0, 2.0 ** 40, np.where(rows % 3 == 1, 2.0 ** -40, 1.0))).astype(dtype)
    swapped = v1.copy()
    swapped[row_slice(ROW_SPAN + 1)] = 0  # a row set to zero
    swapped[row_slice(ROW_ZERO)] = 0.375  # the zero row filled
    span = v1.copy()  # values over 2^140 in one short row and in the crowded one
    for r in (ROW_SPAN, ROW_CROWDED):
        s = row_slice(r)
        k = np.arange(s.stop - s.start)
        span[s] = (span[s] * np.where(k % 2 == 0, 2.0 ** 60, 2.0 ** -80)).astype(dtype)
    assert np.all(np.isfinite(scaled)) and np.all(np.isfinite(span))
    return v0, [("v1", v1), ("rescaled", scaled), ("zeroed and filled", swapped), ("span", span)]


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_reproducible_mode(need_gpu, dtype):
    opts = {"deterministic": 2}
    x = gen.rand_x(N, 5).astype(dtype)
    v0, steps = det2_steps(dtype)
    with hspmv.SpMV(matrix(v0), kernel="csort", options=opts) as plain:
        info0 = plain.info
        y0 = plain(x)
        assert info0["csort_fixed_point"] == 1 and not plain.can_update
    assert_oracle(matrix(v0), x, y0)
    with hspmv.SpMV(matrix(v0), kernel="csort", options=opts, updatable=True) as op:
        info = op.info
        assert op.can_update
        # the same plan and tables; one more allocation, the source-index
        # table: 4 bytes per stored entry (chunks x 64 lanes x chunk_u)
        grow = 4 * info0["csort_chunks"] * 64 * info0["chunk_u"]
        assert {**info, "device_bytes": 0} == {**info0, "device_bytes": 0}
        assert info["device_bytes"] - info0["device_bytes"] == grow > 0
        op.set_x(x)
        assert np.array_equal(bits(run(op)), bits(y0))
        for name, v in steps:
            op.update_values(v)
            y = run(op)
            with hspmv.SpMV(matrix(v), kernel="csort", options=opts) as f:
                assert f.info == info0, name
                y_fresh = f(x)
            assert_oracle(matrix(v), x, y_fresh)
            assert not np.array_equal(bits(y_fresh), bits(y0))
            assert np.array_equal(bits(y), bits(y_fresh)), (name, int((y != y_fresh).sum()))
            assert op.info == info
        # three more updates that end at v0: the first y again
        t = cuda(steps[1][1])
        op.update_values_device(t.data_ptr())
        op.update_values(steps[0][1])
        op.update_values(v0)
        assert np.array_equal(bits(run(op)), bits(y0))


@gpu
def test_gpu_refusals_leave_the_handle_intact(need_gpu):
    dtype = np.float32
    v0, v1 = rand_values(1, dtype), rand_values(2, dtype)
    x = gen.rand_x(N, 5).astype(dtype)
    opts = {"deterministic": 2}
    # not created updatable: refused as before, the way out named
    with hspmv.SpMV(matrix(v0), kernel="csort", options=opts) as op:
        assert not op.can_update
        y_old = op(x)
        with pytest.raises(hspmv.HspmvError, match="E_INVALID") as e:
            op.update_values(v1)
        assert "csort = -1" in str(e.value) and "hspmv_create_updatable" in str(e.value)
        assert np.array_equal(bits(run(op)), bits(y_old))
    # fixed-point slots: a NaN from host memory is refused before anything is written
    with hspmv.SpMV(matrix(v0), kernel="csort", options=opts, updatable=True) as op:
        assert op.can_update and op.info["csort_fixed_point"] == 1
        y_old = op(x)
        bad = v1.copy()
        bad[len(bad) // 2] = np.nan
        with pytest.raises(hspmv.HspmvError, match="E_INVALID") as e:
            op.update_values(bad)
        assert "NaN" in str(e.value) and op.A.val is not bad
        assert np.array_equal(bits(run(op)), bits(y_old))
    # device pointers on a sharded handle
    with hspmv.SpMV(matrix(v0), kernel="csort", options=opts, updatable=True, devices=[0, 0]) as op:
        assert op.can_update and op.info["num_gpus"] == 2
        y_old = op(x)
        t = cuda(v1)
        with pytest.raises(hspmv.HspmvError, match="E_INVALID"):
            op.update_values_device(t.data_ptr())
        assert np.array_equal(bits(run(op)), bits(y_old))


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_sharded(need_gpu, dtype):
    kw = dict(devices=[0, 0])
    # exact arithmetic in the default mode
    v0, v1, x = int_values(1, dtype), int_values(2, dtype), int_x(dtype)
    y_new = fresh_y(v1, x, **kw)
    assert np.array_equal(y_new, exact_oracle(v1, x))
    with hspmv.SpMV(matrix(v0), kernel="csort", updatable=True, **kw) as op:
        assert op.can_update and op.info["num_gpus"] == 2 and op.info["kernel_name"] == "csort"
        y_old = op(x)
        op.update_values(v1)
        assert np.array_equal(bits(run(op)), bits(y_new))
        op.update_values(v0)
        assert np.array_equal(bits(run(op)), bits(y_old))
    # fixed-point slots, random values
    opts = {"deterministic": 2}
    x = gen.rand_x(N, 5).astype(dtype)
    v0, steps = det2_steps(dtype)
    with hspmv.SpMV(matrix(v0), kernel="csort", options=opts, updatable=True, **kw) as op:
        info = op.info
        y_old = op(x)
        for name, v in (steps[0], steps[3]):
            op.update_values(v)
            assert np.array_equal(bits(run(op)), bits(fresh_y(v, x, options=opts, **kw))), name
        assert op.info == info
        op.update_values(v0)
        assert np.array_equal(bits(run(op)), bits(y_old))


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_borrowed(need_gpu, dtype):
    import torch
    v0, v1, v2, x = int_values(1, dtype), int_values(2, dtype), int_values(3, dtype), int_x(dtype)
    want = [fresh_y(v, x) for v in (v0, v1, v2)]
    rp, ci = pattern()
    d_rp, d_ci, val, val2 = cuda(rp), cuda(ci), cuda(v0), cuda(v2)
    cs = _lib.Csr(M, N, len(ci), d_rp.data_ptr(), d_ci.data_ptr(), val.data_ptr(), hspmv.api.dtype_code(dtype))
    A = matrix(v0)
    with hspmv.SpMV.from_device(cs, None, A, device=0, kernel="csort", updatable=True) as op:
        info = op.info
        assert info["kernel_name"] == "csort" and op.can_update
        op.set_x(x)
        assert np.array_equal(bits(run(op)), bits(want[0]))
        val.copy_(torch.from_numpy(v1))
        torch.cuda.synchronize()
        op.update_values_device(None)
        assert np.array_equal(bits(run(op)), bits(want[1]))
        op.update_values_device(val2.data_ptr())
        assert np.array_equal(bits(run(op)), bits(want[2]))
        assert op.info == info and op.A is A
        with pytest.raises(hspmv.HspmvError, match="E_INVALID"):  # host memory: refused as before
            op.update_values(v1)
        assert np.array_equal(bits(run(op)), bits(want[2]))
    # a borrowed handle not created updatable still refuses
    with hspmv.SpMV.from_device(cs, None, A, device=0, kernel="csort") as op:
        assert not op.can_update
        with pytest.raises(hspmv.HspmvError, match="E_INVALID"):
            op.update_values_device(None)


@gpu
def test_gpu_row_kernel_handles_are_unchanged(need_gpu):
    A = gen.laplace2d(90, 70)
    x = gen.rand_x(A.n, 3)
    v1 = new_values(A, 5)
    with hspmv.SpMV(A) as plain:
        info0, y0 = plain.info, plain(x)
        assert plain.can_update and info0["kernel_name"] != "csort"
    with hspmv.SpMV(with_values(A, v1)) as f:
        y1 = f(x)
    assert_oracle(with_values(A, v1), x, y1)
    with hspmv.SpMV(A, updatable=True) as op:
        assert op.can_update and op.info == info0
        assert np.array_equal(bits(op(x)), bits(y0))
        op.update_values(v1)
        assert np.array_equal(bits(run(op)), bits(y1))
        t = cuda(A.val)
        op.update_values_device(t.data_ptr())
        assert np.array_equal(bits(run(op)), bits(y0))
        assert op.info == info0


@gpu
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_gpu_cli_update_values_csort(need_gpu, dtype):
    out = cli(BUILD / "spmv-csr", GOLDEN / "powerlaw1500.csr", 3, "--kernel", "csort", "--update-values", 2,
              "--dtype", dtype, "--x", "rand:3")
    assert re.search(r"^UpdateCheck: PASS maxrel=\S+ wrong=0$", out, re.M), out
    assert re.search(r"^Check: PASS", out, re.M)
