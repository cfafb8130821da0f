"""hspmv_update_values / hspmv_mm_update_values: new matrix values for a
planned handle, in place.

The yardstick is a fresh handle: after an update, y must be bit for bit what a
handle newly created with the same arguments from the new values gives, on
every row.  Once per matrix and value set the fresh y is also held against the
oracle (the fp64 bar of conftest.fp64_tol_ok, or the fp32 bar of
test_gpu_parity's x-slab test), so that two wrong results cannot agree.

Pre-existing behaviour this file documents rather than changes: a handle over
borrowed device arrays whose plan reads a derived copy of the values (row
slices, x slabs) keeps computing with the OLD values after the caller
overwrites its array, until hspmv_update_values(h, NULL, HSPMV_VALUES_DEVICE).
"""
import ctypes as C
import re
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import hspmv
import lattice_cases as lc
import oracle
from conftest import GOLDEN, REPO, fp64_tol_ok
from hspmv import _lib, gen

gpu = pytest.mark.gpu
BUILD = REPO / "heterogeneous-spmv_amd" / "build"
E_INVALID = -1


# ------------------------------------------------------------------ CPU

def test_symbols_declared_and_bound():
    text = _lib.HEADER.read_text()
    assert re.search(r"#define HSPMV_VALUES_DEVICE 1u\b", text)
    assert re.search(r"int hspmv_update_values\(hspmv_handle \*h, const void \*val, unsigned flags\);", text)
    assert re.search(r"int hspmv_mm_update_values\(hspmv_mm \*mm, const void \*val, unsigned flags\);", text)
    for name in ("hspmv_update_values", "hspmv_mm_update_values"):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_uint]
    assert _lib.VALUES_DEVICE == 1


def test_null_handle_is_refused_without_a_device():
    L = _lib.lib()
    buf = np.zeros(4)
    for fn in (L.hspmv_update_values, L.hspmv_mm_update_values):
        for flags in (0, _lib.VALUES_DEVICE, 6):
            assert fn(None, buf.ctypes.data, flags) == E_INVALID
            assert _lib.last_error()


def test_version_minor_stays_1():
    text = _lib.HEADER.read_text()
    assert "#define HSPMV_VERSION_MINOR 1\n" in text
    assert "hspmv_update_values" in text.split("Also in 1.1")[1][:1100]
    assert text.count("Also in 1.1") == 1


def test_python_shape_and_dtype_errors_come_before_the_library():
    """On stubs without a handle behind them a call into the library is an
    HspmvError (NULL handle), so a ValueError proves the check came first."""
    A = gen.laplace2d(6, 5)
    sv = hspmv.SpMV.__new__(hspmv.SpMV)
    sv._h, sv.A, sv.maps, sv.value_dtype, sv.dtype = None, A, None, A.val.dtype, A.val.dtype
    mm = hspmv.SpMM.__new__(hspmv.SpMM)
    mm._init_meta(A, 3)
    for op in (sv, mm):
        for bad in (np.zeros(A.nnz + 1), np.zeros(A.nnz - 1), np.zeros((A.nnz, 1)), np.zeros(()),
                    np.zeros(A.nnz, np.complex128), np.full(A.nnz, "a")):
            with pytest.raises(ValueError):
                op.update_values(bad)
        with pytest.raises(hspmv.HspmvError, match="E_INVALID"):  # a good array does reach the library
            op.update_values(np.ones(A.nnz, np.float32))
        with pytest.raises(hspmv.HspmvError, match="E_INVALID"):
            op.update_values_device(None)
        assert op.A is A  # a refused update leaves op.A alone
    # a mixed handle stores float32: float64 input casts (same_kind), integers do too, complex not
    sv.value_dtype = np.dtype(np.float32)
    with pytest.raises(ValueError):
        sv.update_values(np.zeros(A.nnz, np.complex64))


# ------------------------------------------------------------------ GPU helpers

@pytest.fixture(scope="module")
def need_gpu():
    assert hspmv.device_count() >= 1, "no HIP device visible: the gpu tests must run on the MI355X box"


def bits(y):
    return np.ascontiguousarray(y).view(np.uint8)


def new_values(A, seed):
    """An independent draw in A's value dtype with a few exact zeros; every
    entry differs from A's."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1.0, 1.0, A.nnz).astype(A.val.dtype)
    nz = np.flatnonzero(A.val != 0)
    v[nz[:: max(1, len(nz) // 7)]] = 0.0
    same = v == A.val
    v[same] = np.where(A.val[same] == 0, 0.5, -A.val[same]).astype(A.val.dtype)
    assert np.all(v != A.val) and np.count_nonzero(v == 0) >= 3
    return v


def with_values(A, v):
    return hspmv.CsrMatrix(A.m, A.n, A.row_ptr, A.col_idx, v)


def assert_oracle(A, x, y):
    """y (of x's dtype) against omp_spmv on A's values: the fp64 bar for fp64
    vectors (a mixed handle: over the widened values), else the fp32 bar."""
    absrow = oracle.abs_rowsum(A.row_ptr, A.col_idx, A.val, x.astype(np.float64))
    if x.dtype == np.float64:
        y64 = oracle.spmv(A.row_ptr, A.col_idx, A.val.astype(np.float64), x)
        assert fp64_tol_ok(y, y64, absrow), np.abs(y - y64).max()
    else:
        ref = oracle.spmv(A.row_ptr, A.col_idx, A.val, x)
        err = np.abs(y.astype(np.float64) - ref.astype(np.float64))
        assert np.all(err <= (np.diff(A.row_ptr) + 2) * 2.0 ** -23 * absrow + 1e-30)


def run(op):
    op.spmv()
    return op.get_y()


def cuda(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def roundtrip(A, x, maps=None, expect=None, **kw):
    """Creates a handle over A, updates it from host memory to new values,
    from a device array to a third set, and from host memory back: after each
    step y is the bits of a fresh handle over those values (the first handle's
    own y for the way back), and info never moves."""
    v1, v2 = new_values(A, 11), new_values(A, 12)
    with hspmv.SpMV(A, maps, **kw) as op:
        info = op.info
        for k, want in (expect or {}).items():
            assert info[k] == want, (k, info[k], want)
        op.set_x(x)
        y0 = run(op)
        assert_oracle(A, x, y0)
        for step, v in (("host", v1), ("device", v2), ("host", A.val)):
            if step == "host":
                op.update_values(v)
                assert op.A.row_ptr is A.row_ptr and op.A.col_idx is A.col_idx
                assert np.array_equal(op.A.val, v)
            else:
                t = cuda(v)
                op.update_values_device(t.data_ptr())
            y = run(op)  # (get_y synchronises: t outlives the stream work)
            assert op.info == info, step
            if v is A.val:
                assert np.array_equal(bits(y), bits(y0)), "there and back"
                continue
            Av = with_values(A, v)
            with hspmv.SpMV(Av, maps, **kw) as fresh:
                assert fresh.info == info
                y_fresh = fresh(x)
            if step == "host":
                assert_oracle(Av, x, y_fresh)
            assert not np.array_equal(bits(y_fresh), bits(y0))
            assert np.array_equal(bits(y), bits(y_fresh)), (step, int((y != y_fresh).sum()))
    return info


SLICE_OPTS = dict(x_dict=1, row_slices=1, x_dict_cap=lc.SLICE_CAP)


def unit_kw(unit):
    _, xdt = lc.unit_dtypes(unit)
    return dict(vector_dtype=xdt) if unit == "mixed" else {}


# ------------------------------------------------------------------ row slices

@gpu
@pytest.mark.parametrize("path", ["stream", "csr3"])
@pytest.mark.parametrize("bits_", [12, 16])
@pytest.mark.parametrize("unit", lc.UNITS)
def test_gpu_row_slices(need_gpu, unit, bits_, path):
    A = lc.g_slices(unit, bits_)
    _, xdt = lc.unit_dtypes(unit)
    x = gen.rand_x(A.n, 31).astype(xdt)
    maps = lc.ssr_maps(A.m, 3) if path == "csr3" else None
    info = roundtrip(A, x, maps, expect=dict(row_slices=1, x_dict=1), kernel=path, options=SLICE_OPTS,
                     **unit_kw(unit))
    if path == "stream":
        assert info["slice_pos_bits"] == bits_


# ------------------------------------------------------------------ x slabs

@lru_cache(maxsize=None)
def slab_matrix(name):
    rng = np.random.default_rng(4)
    if name == "wide":  # test_gpu_parity._wide_random(3000, 1 << 20, 40, 4)
        m, n, per_row = 3000, 1 << 20, 40
        cols = np.sort(rng.choice(n, size=(m, per_row), replace=True), axis=1)
        rp = np.arange(0, m * per_row + 1, per_row, dtype=np.int32)
        return hspmv.CsrMatrix(m, n, rp, cols.reshape(-1).astype(np.int32), rng.uniform(-1, 1, m * per_row))
    if name == "split":  # test_gpu_parity._split_row_matrix: split rows first, last, adjacent, at group edges
        rng = np.random.default_rng(3)
        m, n = 700, 150_000
        lens = rng.integers(0, 40, m)
        lens[rng.integers(0, m, 40)] = rng.integers(33, 4000, 40)
        for r, ln in [(0, 120_000), (1, 4097), (63, 5000), (64, 9000), (65, 4096), (300, 30_000),
                      (301, 70_000), (699, 8193)]:
            lens[r] = ln
        rp = np.concatenate([[0], np.cumsum(lens)])
        ci = np.concatenate([np.sort(rng.choice(n, ln, replace=False)) for ln in lens])
        return hspmv.CsrMatrix(m, n, rp, ci, rng.uniform(-1, 1, rp[-1]))
    return gen.laplace2d(300, 200)


@gpu
@pytest.mark.parametrize("kernel", ["stream", "csr3"])
@pytest.mark.parametrize("slabs", [2, 5])
@pytest.mark.parametrize("unit", lc.UNITS)
@pytest.mark.parametrize("name", ["wide", "split", "laplace"])
def test_gpu_x_slabs(need_gpu, name, unit, slabs, kernel):
    vdt, xdt = lc.unit_dtypes(unit)
    A = slab_matrix(name).astype(vdt)
    x = gen.rand_x(A.n, 9).astype(xdt)
    maps = hspmv.build_csr3_maps(A, 20, 10) if kernel == "csr3" else None
    expect = dict(x_slabs=slabs, row_slices=0)
    if name == "split":
        expect["n_split_rows"] = int((np.diff(A.row_ptr) > 4096).sum())
    roundtrip(A, x, maps, expect=expect, kernel=kernel, options={"x_slabs": slabs}, **unit_kw(unit))


# ------------------------------------------------------------------ plans that read only the CSR-order values

VALUE_PLANS = {
    "col32": (dict(kernel="stream", col16=False), dict(col16=0, x_dict=0)),
    "default": (dict(kernel="stream"), dict(x_slabs=0)),
    "dict": (dict(kernel="stream", options=dict(x_dict=1, row_slices=-1, x_dict_cap=lc.DICT_CAP)),
             dict(x_dict=1, row_slices=0)),
    "vector": (dict(kernel="vector"), dict(kernel=1)),
    "serial": (dict(kernel="stream", options=dict(deterministic="serial")), dict(serial_order=1)),
}


@gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("plan", sorted(VALUE_PLANS))
def test_gpu_values_only_plans(need_gpu, plan, dtype):
    """The gauntlet's base matrix: split rows (the split-row kernels, or the
    forked long-row kernel of the serial order) beside cooperative rows."""
    A = lc.gauntlet(dtype=dtype).A
    x = gen.rand_x(A.n, 42).astype(dtype)
    kw, expect = VALUE_PLANS[plan]
    if plan != "vector":
        expect = dict(expect, n_split_rows=len(lc.SPLIT_ROWS))
    roundtrip(A, x, expect=expect, **kw)


# ------------------------------------------------------------------ borrowed device arrays

@gpu
@pytest.mark.parametrize("which", ["stream", "slices", "slabs"])
def test_gpu_borrowed(need_gpu, which):
    """In-place change + update_values_device(None), then another array.  The
    slice and slab handles read their own copies: before the call they still
    give the old y (documented, not changed); the STREAM handle reads the
    array itself."""
    import torch
    if which == "slices":
        A, kw = lc.g_slices("f64", 16), dict(kernel="stream", options=SLICE_OPTS)
        key, want = "row_slices", 1
    elif which == "slabs":
        A, kw = gen.stencil27(30), dict(kernel="stream", options={"x_slabs": 3})
        key, want = "x_slabs", 3
    else:
        A, kw = gen.stencil27(30), dict(kernel="stream")
        key, want = "row_slices", 0
    x = gen.rand_x(A.n, 13)
    v1, v2 = new_values(A, 21), new_values(A, 22)
    fresh = {}
    for name, v in (("v0", A.val), ("v1", v1), ("v2", v2)):
        with hspmv.SpMV(with_values(A, v), **kw) as f:
            fresh[name] = f(x)
        assert_oracle(with_values(A, v), x, fresh[name])
    rp, ci, val, val2 = cuda(A.row_ptr), cuda(A.col_idx), cuda(A.val), cuda(v2)
    cs = _lib.Csr(A.m, A.n, A.nnz, rp.data_ptr(), ci.data_ptr(), val.data_ptr(), 1)
    with hspmv.SpMV.from_device(cs, None, A, device=0, **kw) as op:
        info = op.info
        assert info[key] == want
        op.set_x(x)
        assert np.array_equal(bits(run(op)), bits(fresh["v0"]))
        val.copy_(torch.from_numpy(v1))
        torch.cuda.synchronize()
        y_stale = run(op)
        if which == "stream":
            assert np.array_equal(bits(y_stale), bits(fresh["v1"]))
        else:
            assert np.array_equal(bits(y_stale), bits(fresh["v0"]))
        op.update_values_device(None)
        assert np.array_equal(bits(run(op)), bits(fresh["v1"]))
        op.update_values_device(val2.data_ptr())
        assert np.array_equal(bits(run(op)), bits(fresh["v2"]))
        val.zero_()  # the first array is no longer read
        torch.cuda.synchronize()
        assert np.array_equal(bits(run(op)), bits(fresh["v2"]))
        assert op.info == info and op.A is A
        # host memory is refused, the handle intact
        with pytest.raises(hspmv.HspmvError, match="E_INVALID"):
            op.update_values(v1)
        assert np.array_equal(bits(run(op)), bits(fresh["v2"]))


# ------------------------------------------------------------------ stream order

@gpu
def test_gpu_device_update_is_ordered_on_the_stream(need_gpu):
    """SpMV into y1, device update, SpMV into y2, one synchronise at the end."""
    import torch
    A = lc.g_slices("f64", 12)
    x = gen.rand_x(A.n, 31)
    v1 = new_values(A, 31)
    kw = dict(kernel="stream", options=SLICE_OPTS)
    with hspmv.SpMV(with_values(A, v1), **kw) as f:
        y_new = f(x)
    y1 = torch.zeros(A.m, dtype=torch.float64, device="cuda")
    y2 = torch.zeros(A.m, dtype=torch.float64, device="cuda")
    t = cuda(v1)
    with hspmv.SpMV(A, **kw) as op:
        assert op.info["row_slices"] == 1
        y_old = op(x)
        op.bind_y_device(y1.data_ptr())
        op.spmv()
        op.bind_y_device(y2.data_ptr())
        op.update_values_device(t.data_ptr())
        op.spmv()
        op.synchronize()
        assert np.array_equal(bits(y1.cpu().numpy()), bits(y_old))
        assert np.array_equal(bits(y2.cpu().numpy()), bits(y_new))


# ------------------------------------------------------------------ sharded

@gpu
@pytest.mark.parametrize("kernel", ["stream", "csr3", "slices"])
def test_gpu_sharded(need_gpu, kernel):
    """Three shards on one device: each takes its range of the global values
    (the gauntlet's split rows make the row ranges uneven; the slice shards
    stage their range and rebuild their own value streams); device pointers
    are refused."""
    A = lc.g_slices("f64", 12) if kernel == "slices" else lc.gauntlet().A
    x = gen.rand_x(A.n, 42)
    maps = None
    if kernel == "csr3":  # uneven super-super-rows over 16-row super-rows
        inner = np.append(np.arange(0, A.m, 16), A.m).astype(np.int32)
        n_sr = len(inner) - 1
        maps = hspmv.Csr3Maps(np.array([0, 3, 10, 11, 30, n_sr], np.int32), inner)
    v1 = new_values(A, 41)
    kw = dict(devices=[0, 0, 0], kernel=kernel)
    if kernel == "slices":
        kw = dict(devices=[0, 0, 0], kernel="stream", options=SLICE_OPTS)
    with hspmv.SpMV(with_values(A, v1), maps, **kw) as f:
        y_new = f(x)
    assert_oracle(with_values(A, v1), x, y_new)
    with hspmv.SpMV(A, maps, **kw) as op:
        info = op.info
        assert info["num_gpus"] == 3 and info["row_slices"] == int(kernel == "slices")
        y_old = op(x)
        t = cuda(v1)
        with pytest.raises(hspmv.HspmvError, match="E_INVALID"):
            op.update_values_device(t.data_ptr())
        assert np.array_equal(bits(run(op)), bits(y_old))
        op.update_values(v1)
        assert np.array_equal(bits(run(op)), bits(y_new))
        assert op.info == info
        op.update_values(A.val)
        assert np.array_equal(bits(run(op)), bits(y_old))


# ------------------------------------------------------------------ refusals

@gpu
def test_gpu_csort_handles_are_refused(need_gpu):
    A = gen.powerlaw(20000, dtype=np.float32)
    x = gen.rand_x(A.n, 5).astype(np.float32)
    v1 = new_values(A, 51)
    with hspmv.SpMV(A, kernel="csort") as op:
        assert op.info["kernel_name"] == "csort"
        op.set_x(x)
        assert_oracle(A, x, run(op))
        with pytest.raises(hspmv.HspmvError, match="E_INVALID") as e:
            op.update_values(v1)
        assert "csort = -1" in str(e.value) and "deterministic = 1" in str(e.value)
        t = cuda(v1)
        with pytest.raises(hspmv.HspmvError, match="E_INVALID"):
            op.update_values_device(t.data_ptr())
        assert op.A is A
        # (csort's fp64 slot sums add in LDS-atomic order: the old values' y within the fp32 bar)
        assert_oracle(A, x, run(op))
    # the way to a handle that can be updated
    with hspmv.SpMV(A, options={"csort": -1}) as op:
        assert op.info["kernel_name"] != "csort"
        op.set_x(x)
        op.update_values(v1)
        assert_oracle(with_values(A, v1), x, run(op))


@gpu
def test_gpu_refusals_leave_the_handle_intact(need_gpu):
    A = lc.g_slices("f64", 16)
    x = gen.rand_x(A.n, 31)
    v1 = new_values(A, 61)
    L = _lib.lib()
    with hspmv.SpMV(A, kernel="stream", options=SLICE_OPTS) as op:
        info = op.info
        y_old = op(x)
        t = cuda(v1)
        for val, flags in ((None, 0), (None, _lib.VALUES_DEVICE), (v1.ctypes.data, 2),
                           (t.data_ptr(), _lib.VALUES_DEVICE | 0x80000000), (v1.ctypes.data, 0x10)):
            assert L.hspmv_update_values(op._h, val, flags) == E_INVALID, (val, flags)
            assert _lib.last_error()
            assert np.array_equal(bits(run(op)), bits(y_old))
        assert op.info == info


# ------------------------------------------------------------------ SpMM

@gpu
@pytest.mark.parametrize("borrowed", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("k", [1, 5, 32])
def test_gpu_spmm(need_gpu, k, dtype, borrowed):
    import torch
    A = gen.powerlaw(3000, seed=2, dtype=dtype)
    X = np.stack([gen.rand_x(A.n, 70 + c) for c in range(k)], axis=1).astype(dtype)
    v1, v2 = new_values(A, 71), new_values(A, 72)
    fresh = {}
    for name, v in (("v0", A.val), ("v1", v1), ("v2", v2)):
        with hspmv.SpMM(with_values(A, v), k) as f:
            fresh[name] = f(X)
    assert_oracle(with_values(A, v1), np.ascontiguousarray(X[:, 0]), np.ascontiguousarray(fresh["v1"][:, 0]))

    def go(op):
        op.spmm()
        return op.get_y()

    if not borrowed:
        with hspmv.SpMM(A, k) as op:
            info = op.info
            assert np.array_equal(bits(op(X)), bits(fresh["v0"]))
            op.update_values(v1)
            assert op.A.col_idx is A.col_idx and np.array_equal(op.A.val, v1)
            assert np.array_equal(bits(go(op)), bits(fresh["v1"]))
            t = cuda(v2)
            op.update_values_device(t.data_ptr())
            assert np.array_equal(bits(go(op)), bits(fresh["v2"]))
            assert op.info == info
            for val, flags in ((None, 0), (None, _lib.VALUES_DEVICE), (v1.ctypes.data, 2)):
                assert _lib.lib().hspmv_mm_update_values(op._h, val, flags) == E_INVALID
            assert np.array_equal(bits(go(op)), bits(fresh["v2"]))
        return
    rp, ci, val, val2 = cuda(A.row_ptr), cuda(A.col_idx), cuda(A.val), cuda(v2)
    cs = _lib.Csr(A.m, A.n, A.nnz, rp.data_ptr(), ci.data_ptr(), val.data_ptr(),
                  _lib.F64 if dtype == np.float64 else _lib.F32)
    with hspmv.SpMM.from_device(cs, A, k) as op:
        assert np.array_equal(bits(op(X)), bits(fresh["v0"]))
        val.copy_(torch.from_numpy(v1))
        torch.cuda.synchronize()
        op.update_values_device(None)  # nothing derived: accepted, nothing to do
        assert np.array_equal(bits(go(op)), bits(fresh["v1"]))
        op.update_values_device(val2.data_ptr())
        assert np.array_equal(bits(go(op)), bits(fresh["v2"]))
        with pytest.raises(hspmv.HspmvError, match="E_INVALID"):
            op.update_values(v1)
        assert np.array_equal(bits(go(op)), bits(fresh["v2"]))


# ------------------------------------------------------------------ CLI

def cli(*args):
    p = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, f"{args} -> {p.returncode}\n{p.stdout}\n{p.stderr}"
    return p.stdout


@gpu
@pytest.mark.parametrize("tool,ext", [("spmv-csr", "csr"), ("spmv-csrk", "csr3")])
def test_gpu_cli_update_values(need_gpu, tool, ext):
    f = GOLDEN / f"powerlaw1500.{ext}"
    for dtype in ("f64", "f32"):
        out = cli(BUILD / tool, f, 3, "--update-values", 2, "--dtype", dtype, "--x", "rand:3")
        umin = float(re.search(r"^UpdateMin: (\S+)$", out, re.M).group(1))
        uavg = float(re.search(r"^UpdateAvg: (\S+)$", out, re.M).group(1))
        assert 0 < umin <= uavg
        assert re.search(r"^UpdateCheck: PASS maxrel=\S+ wrong=0$", out, re.M), out
        assert re.search(r"^Check: PASS", out, re.M)
        plain = cli(BUILD / tool, f, 3, "--dtype", dtype, "--x", "rand:3")
        assert "Update" not in plain
        # the report before the update lines is today's, line for line
        strip = re.compile(r"^(Time|Kernel|GFLOPs|GBps|KernelGFLOPs|KernelGBps)\w*:.*$|reordered in", re.M)
        head = [ln for ln in out.splitlines() if not ln.startswith("Update") and not strip.search(ln)]
        assert head == [ln for ln in plain.splitlines() if not strip.search(ln)]
