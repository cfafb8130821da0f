"""Multi-vector SpMM (hspmv_mm_* / hspmv.SpMM): Y = A X for k right-hand
sides, X row-major (n, k).

CPU part: the refusals of hspmv_mm_create before any device is touched, the
hspmv_mm_info layout, the Python layer's shape / dtype checks.

GPU part, against ``oracle.spmv`` per column (the restatement pinned to the
reference's omp_spmv): rows of at most the dtype's serial bound (40 nonzeros
in fp64, 56 in fp32) are checked BITWISE, longer rows within the project's
bars -- ``fp64_tol_ok`` in fp64, (len + 2) * 2^-23 * sum|a x| in fp32.
"""
import ctypes
import subprocess

import numpy as np
import pytest

import hspmv
import oracle
from conftest import GOLDEN, REPO, fp64_tol_ok, load_golden
from hspmv import _lib, gen

BUILD = REPO / "heterogeneous-spmv_amd" / "build"
SERIAL_MAX = {np.dtype(np.float64): 40, np.dtype(np.float32): 56}
gpu = pytest.mark.gpu


# ------------------------------------------------------------------ CPU part

def _create(mm_ref, cs_ref, k, opt):
    return hspmv.lib().hspmv_mm_create(mm_ref, cs_ref, k, ctypes.byref(opt) if opt is not None else None)


def test_create_refusals_name_the_argument():
    """Each bad argument is HSPMV_E_INVALID (-1) with a message that names it;
    none of these reaches a device (this test runs without one)."""
    L = hspmv.lib()
    A = gen.laplace2d(8, 8)
    cs = A.c_struct()
    h = ctypes.c_void_p()
    ok = _lib.make_options(0, None)
    assert _create(None, ctypes.byref(cs), 4, ok) == -1
    assert b"mm" in L.hspmv_last_error()
    assert _create(ctypes.byref(h), None, 4, ok) == -1
    assert b"A " in L.hspmv_last_error() and not h.value
    for k in (0, 33):
        assert _create(ctypes.byref(h), ctypes.byref(cs), k, ok) == -1
        assert b"k = %d" % k in L.hspmv_last_error() and not h.value
    stream = _lib.make_options(_lib.KERNEL_STREAM, None)
    assert _create(ctypes.byref(h), ctypes.byref(cs), 4, stream) == -1
    assert b"flags" in L.hspmv_last_error() and b"kernel" in L.hspmv_last_error()
    two = _lib.make_options(0, None, devices=[0, 1])
    assert two.n_devices == 2
    assert _create(ctypes.byref(h), ctypes.byref(cs), 4, two) == -1
    assert b"n_devices" in L.hspmv_last_error() and not h.value


def test_null_operator_is_an_error_not_a_crash():
    L = hspmv.lib()
    assert L.hspmv_mm_spmm(None) == -1
    assert L.hspmv_mm_synchronize(None) == -1
    assert L.hspmv_mm_get_info(None, None, 8) == -1
    L.hspmv_mm_destroy(None)


def test_mm_info_layout_matches_the_header(tmp_path):
    """_lib.MmInfo has the header's size and field offsets (the gcc offsetof
    program of test_abi.test_struct_layouts_match_the_header, for
    hspmv_mm_info)."""
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "hspmv.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(hspmv_mm_info));']
    for f, _ in _lib.MmInfo._fields_:
        lines.append(f'  printf("{f} %zu\\n", offsetof(hspmv_mm_info, {f}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(_lib.HEADER.parent), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in
               subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(_lib.MmInfo)
    for f, _ in _lib.MmInfo._fields_:
        assert int(got[f]) == getattr(_lib.MmInfo, f).offset, f


def test_python_shape_and_dtype_errors_come_before_the_library():
    """SpMM.set_x / __call__ raise ValueError for a 1-D X, an (n, k + 1) X and a
    dtype that does not cast: on a stub without an operator behind it, so a
    call into the library would be an HspmvError (NULL mm), not a ValueError."""
    A = gen.laplace2d(6, 5)
    op = hspmv.SpMM.__new__(hspmv.SpMM)
    op._init_meta(A, 3)
    for bad in (np.zeros(A.n), np.zeros((A.n, 4)), np.zeros((A.n + 1, 3)),
                np.zeros((A.n, 3), np.complex128), np.full((A.n, 3), "a")):
        with pytest.raises(ValueError):
            op.set_x(bad)
        with pytest.raises(ValueError):
            op(bad)
    with pytest.raises(hspmv.HspmvError):  # a good X does reach the library
        op.set_x(np.zeros((A.n, 3), np.float32))
    for k in (0, 33):
        with pytest.raises(ValueError):
            hspmv.SpMM(A, k)


# ------------------------------------------------------------------ GPU part

@pytest.fixture(scope="module")
def need_gpu():
    assert hspmv.device_count() >= 1, "no HIP device visible: the gpu tests must run on the MI355X box"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def rand_X(n, k, dtype, seed0=100):
    return np.stack([gen.rand_x(n, seed0 + c) for c in range(k)], axis=1).astype(dtype)


_REF = {}


def reference(key, A, X):
    """oracle.spmv per column and the abs row sums, computed once per key."""
    if key not in _REF:
        Y = np.stack([oracle.spmv(A.row_ptr, A.col_idx, A.val, X[:, c]) for c in range(X.shape[1])], axis=1)
        absrow = np.stack([oracle.abs_rowsum(A.row_ptr, A.col_idx, A.val, X[:, c])
                           for c in range(X.shape[1])], axis=1)
        _REF[key] = (Y, absrow)
    return _REF[key]


def check_against_oracle(A, X, Y, key):
    """Short rows bitwise, long rows within the dtype's bar; every column."""
    Yref, absrow = reference(key, A, X)
    lens = np.diff(A.row_ptr)
    short = lens <= SERIAL_MAX[A.val.dtype]
    assert Y.shape == Yref.shape and Y.dtype == A.val.dtype
    assert np.array_equal(bits(Y[short]), bits(Yref[short])), key
    if (~short).any():
        if A.val.dtype == np.float64:
            assert fp64_tol_ok(Y[~short], Yref[~short], absrow[~short]), key
        else:
            err = np.abs(Y[~short].astype(np.float64) - Yref[~short])
            assert np.all(err <= (lens[~short, None] + 2) * 2.0 ** -23 * absrow[~short] + 1e-30), key


_STENCIL = {}


def stencil(dtype):
    dt = np.dtype(dtype)
    if dt not in _STENCIL:
        _STENCIL[dt] = gen.stencil27(12, dtype=dtype)
    return _STENCIL[dt]


@gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 16, 17, 32])
def test_order_contract_stencil(need_gpu, dtype, k):
    """Every row of the 27-point stencil is short: every column of Y is
    omp_spmv's bits, for every lane mapping (k = 17 runs 32 lanes per row)."""
    A = stencil(dtype)
    assert np.diff(A.row_ptr).max() <= 27
    X = rand_X(A.n, 32, dtype)[:, :k]
    with hspmv.SpMM(A, k) as op:
        Y = op(X)
        info = op.info
    Yref, _ = reference(("stencil", np.dtype(dtype).name), A, rand_X(A.n, 32, dtype))
    assert np.array_equal(bits(Y), bits(Yref[:, :k]))
    kp = 1 << (k - 1).bit_length()
    assert (info["k"], info["lanes_per_row"], info["rows_per_wave"]) == (k, kp, 64 // kp)
    assert info["long_rows"] == 0 and info["serial_max"] == SERIAL_MAX[np.dtype(dtype)]
    assert info["blocks"] == -(-A.m // (4 * (64 // kp))) and info["flops"] == 2.0 * A.nnz * k


@gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_k4_matches_the_single_vector_handle(need_gpu, dtype):
    A = stencil(dtype)
    X = rand_X(A.n, 4, dtype)
    with hspmv.SpMM(A, 4) as op:
        Y = op(X)
    with hspmv.SpMV(A, device=0) as sv:
        for c in range(4):
            assert np.array_equal(bits(Y[:, c]), bits(sv(np.ascontiguousarray(X[:, c])))), c


@gpu
def test_golden_fp32(need_gpu, golden_names):
    """k = 3 over the golden fixtures in fp32: columns 0 and 1 carry the
    reference binary's own bits on rows of <= 56 nonzeros."""
    for name in golden_names:
        A = hspmv.read_csr(GOLDEN / f"{name}.csr", np.float32)
        g = load_golden(name)
        X = np.stack([gen.rand_x(A.n, 42), np.ones(A.n), gen.rand_x(A.n, 7)], axis=1).astype(np.float32)
        with hspmv.SpMM(A, 3) as op:
            Y = op(X)
        short = np.diff(A.row_ptr) <= 56
        assert np.array_equal(bits(Y[short, 0]), bits(g["y_ref_f32_rand"][short])), name
        if "y_ref_f32_ones" in g:
            assert np.array_equal(bits(Y[short, 1]), bits(g["y_ref_f32_ones"][short])), name
        check_against_oracle(A, X, Y, ("golden", name))


LONG_LENS = (0, 1, 39, 40, 41, 56, 57, 63, 64, 65, 300, 4096, 4500)
_LONG = {}


def long_matrix(dtype):
    """m = 300, n = 5000, row lengths from LONG_LENS in shuffled order (each
    at least 23 times), sorted random columns."""
    dt = np.dtype(dtype)
    if dt not in _LONG:
        rng = np.random.default_rng(2024)
        m, n = 300, 5000
        lens = np.resize(np.array(LONG_LENS), m)
        rng.shuffle(lens)
        rp = np.concatenate([[0], np.cumsum(lens)])
        ci = np.concatenate([np.sort(rng.choice(n, int(ln), replace=False)) for ln in lens])
        val = rng.uniform(-1, 1, int(rp[-1])).astype(dtype)
        _LONG[dt] = hspmv.CsrMatrix(m, n, rp, ci.astype(np.int32), val)
    return _LONG[dt]


@gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("k", [1, 4, 7])
def test_long_rows_and_the_serial_boundary(need_gpu, dtype, k):
    A = long_matrix(dtype)
    assert set(np.diff(A.row_ptr)) == set(LONG_LENS)
    X = rand_X(A.n, 7, dtype)[:, :k]
    with hspmv.SpMM(A, k) as op:
        Y1 = op(X)
        Y2 = op(X)
        info = op.info
    assert info["long_rows"] == int((np.diff(A.row_ptr) > SERIAL_MAX[np.dtype(dtype)]).sum())
    assert Y1.tobytes() == Y2.tobytes()
    check_against_oracle(A, X, Y1, ("long", np.dtype(dtype).name, k))


def _edge_matrices():
    rng = np.random.default_rng(5)

    def rows(lens, n):
        lens = np.asarray(lens)
        rp = np.concatenate([[0], np.cumsum(lens)])
        ci = np.concatenate([np.sort(rng.choice(n, int(ln), replace=False)) for ln in lens] +
                            [np.zeros(0, np.int64)])
        return hspmv.CsrMatrix(len(lens), n, rp, ci.astype(np.int32), rng.uniform(-1, 1, int(rp[-1])))

    yield "m1", rows([5], 9)
    for m in (63, 64, 65):
        yield f"m{m}", rows(rng.integers(0, 12, m), 70)
    yield "nnz0", rows(np.zeros(10, np.int64), 6)
    yield "empty_tail", rows(np.concatenate([rng.integers(1, 9, 130), np.zeros(70, np.int64)]), 50)


@gpu
def test_edges(need_gpu):
    """m = 1; m = 63, 64, 65 at R = 2, 64 and the odd k = 3; nnz = 0; empty
    last rows (an empty row stores +0.0: the oracle's bits)."""
    for name, A in _edge_matrices():
        for k in (32, 1, 3):
            X = rand_X(A.n, k, np.float64, seed0=9)
            with hspmv.SpMM(A, k) as op:
                Y = op(X)
            check_against_oracle(A, X, Y, ("edge", name, k))
            if A.nnz == 0:
                assert not bits(Y).any()


@gpu
def test_leading_dimensions_and_padding(need_gpu):
    """k = 5 in device buffers with ldx = 8 (NaN padding) and ldy = 7 (canary
    padding): the k columns are right, no padding element of Y is written and
    no NaN is read into Y."""
    import torch
    A = long_matrix(np.float64)
    k, ldx, ldy, canary = 5, 8, 7, -12345.5
    X = rand_X(A.n, k, np.float64)
    Xp = np.full((A.n, ldx), np.nan)
    Xp[:, :k] = X
    xd = torch.from_numpy(Xp).cuda()
    yd = torch.full((A.m, ldy), canary, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with hspmv.SpMM(A, k) as op:
        op.bind_x_device(xd.data_ptr(), ldx)
        op.bind_y_device(yd.data_ptr(), ldy)
        op.spmm()
        op.synchronize()
        Yp = yd.cpu().numpy()
        Yh = op.get_y()  # the bound Y, compacted to (m, k)
    assert np.all(Yp[:, k:] == canary)
    assert not np.isnan(Yp).any()
    check_against_oracle(A, X, np.ascontiguousarray(Yp[:, :k]), ("ld", k))
    assert np.array_equal(bits(Yh), bits(np.ascontiguousarray(Yp[:, :k])))


@gpu
def test_leading_dimension_past_2_31_elements(need_gpu):
    """n * ldx and m * ldy beyond 2^31 elements (byte offsets beyond 2^33):
    the index arithmetic into X and Y is 64-bit in both kernels.  fp32, ld =
    2^20: X in columns [0, k) and Y in columns [k, 2k) of the rows of ONE
    9.2 GB device buffer (allocated, never filled), rows past 2048 lie beyond
    element 2^31; a 32-bit product would wrap into other rows."""
    import torch
    rng = np.random.default_rng(31)
    m = n = 2200
    k, ld = 4, 1 << 20
    lens = rng.integers(0, 9, m)
    lens[[5, 2100, 2199]] = (100, 64, 57)  # the wave-per-row kernel, below and past 2^31
    rp = np.concatenate([[0], np.cumsum(lens)])
    ci = np.concatenate([np.sort(rng.choice(n, int(ln), replace=False)) for ln in lens])
    A = hspmv.CsrMatrix(m, n, rp, ci.astype(np.int32), rng.uniform(-1, 1, int(rp[-1])).astype(np.float32))
    assert (n - 1) * ld > 2 ** 31 and (ci >= 2048).any()
    X = rand_X(n, k, np.float32)
    buf = torch.empty(n * ld, dtype=torch.float32, device="cuda").view(n, ld)
    buf[:, :k] = torch.from_numpy(X).cuda()
    buf[:, k:2 * k] = 7.0
    torch.cuda.synchronize()
    with hspmv.SpMM(A, k) as op:
        assert op.info["long_rows"] == 3
        op.bind_x_device(buf.data_ptr(), ld)
        op.bind_y_device(buf.data_ptr() + k * 4, ld)
        op.spmm()
        op.synchronize()
    Y = buf[:, k:2 * k].cpu().numpy()
    assert np.array_equal(buf[:, :k].cpu().numpy(), X)  # X untouched
    del buf
    check_against_oracle(A, X, np.ascontiguousarray(Y), ("ld2_31",))


@gpu
def test_get_info_fills_the_callers_size(need_gpu):
    """hspmv_mm_get_info writes min(out_size, sizeof) bytes: a canary after a
    16-byte prefix survives, and the prefix agrees with the full report."""
    L = hspmv.lib()
    with hspmv.SpMM(stencil(np.float64), 5) as op:
        full = _lib.MmInfo()
        assert L.hspmv_mm_get_info(op._h, ctypes.byref(full), ctypes.sizeof(full)) == 0
        assert (full.k, full.lanes_per_row, full.rows_per_wave, full.waves_per_block) == (5, 8, 8, 4)
        buf = (ctypes.c_ubyte * (ctypes.sizeof(_lib.MmInfo) + 32))(*([0xA5] * (ctypes.sizeof(_lib.MmInfo) + 32)))
        assert L.hspmv_mm_get_info(op._h, ctypes.cast(buf, ctypes.POINTER(_lib.MmInfo)), 16) == 0
        assert all(b == 0xA5 for b in buf[16:])
        assert bytes(buf[:16]) == bytes(memoryview(full).cast("B")[:16])
        assert L.hspmv_mm_get_info(op._h, ctypes.cast(buf, ctypes.POINTER(_lib.MmInfo)), 4096) == 0
        assert all(b == 0xA5 for b in buf[ctypes.sizeof(_lib.MmInfo):])
        assert L.hspmv_mm_get_info(op._h, None, 16) == -1


@gpu
def test_bound_torch_tensors_on_torch_stream(need_gpu):
    import torch
    A = stencil(np.float64)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        xd = torch.rand(A.n, 8, dtype=torch.float64, device="cuda")
        yd = torch.empty(A.m, 8, dtype=torch.float64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        assert stream == st.cuda_stream and stream
        with hspmv.SpMM(A, 8, stream=stream) as op:
            op.bind_x_device(xd.data_ptr(), 8)
            op.bind_y_device(yd.data_ptr(), 8)
            op.spmm()
            st.synchronize()
            Y = yd.cpu().numpy()
    with hspmv.SpMM(A, 8) as op:
        Yh = op(xd.cpu().numpy())
    assert np.array_equal(bits(Y), bits(Yh))


@gpu
def test_device_pointer_matrix(need_gpu):
    import torch
    A = long_matrix(np.float64)
    X = rand_X(A.n, 4, np.float64)
    rp, ci, val = (torch.from_numpy(a).cuda() for a in (A.row_ptr, A.col_idx, A.val))
    torch.cuda.synchronize()
    cs = _lib.Csr(A.m, A.n, A.nnz, rp.data_ptr(), ci.data_ptr(), val.data_ptr(), 1)
    with hspmv.SpMM.from_device(cs, A, 4) as op:
        Yd = op(X)
        assert op.info["long_rows"] > 0
    with hspmv.SpMM(A, 4) as op:
        Yo = op(X)
    assert np.array_equal(bits(Yd), bits(Yo))


@gpu
def test_state_errors(need_gpu):
    A = stencil(np.float64)
    with hspmv.SpMM(A, 4) as op:
        for call in (op.spmm, op.run, op.get_y):
            with pytest.raises(hspmv.HspmvError) as e:
                call()
            assert e.value.code == -7
        ptr = 256  # never dereferenced: the leading dimension is refused first
        with pytest.raises(hspmv.HspmvError) as e:
            op.bind_x_device(ptr, 3)
        assert e.value.code == -1 and "ldx" in str(e.value)
        with pytest.raises(hspmv.HspmvError) as e:
            op.bind_y_device(ptr, 3)
        assert e.value.code == -1 and "ldy" in str(e.value)
        with pytest.raises(hspmv.HspmvError):  # still no X: the refused bind set nothing
            op.spmm()


@gpu
def test_run_reports_and_leaves_y(need_gpu):
    A = stencil(np.float64)
    k = 8
    X = rand_X(A.n, k, np.float64)
    with hspmv.SpMM(A, k, nontemporal=True) as op:
        Y1 = op(X)
        t = op.run(warmup=2, iters=6)
        Y2 = op.get_y()
        info = op.info
    assert t["iters"] == 6 and t["num_gpus"] == 1
    assert 0 < t["t_min"] <= t["t_avg"] <= t["t_max"]
    assert t["gflops"] == pytest.approx(2.0 * A.nnz * k / t["t_min"] * 1e-9, rel=1e-9)
    assert t["gbps_alg"] == pytest.approx(info["alg_bytes"] / t["t_min"] * 1e-9, rel=1e-9)
    assert info["alg_bytes"] == A.nnz * 12 + (A.m + 1) * 4 + (A.n + A.m) * k * 8
    assert np.array_equal(bits(Y1), bits(Y2))
    Yref, _ = reference(("stencil", "float64"), A, rand_X(A.n, 32, np.float64))
    assert np.array_equal(bits(Y1), bits(Yref[:, :k]))  # the nontemporal loads: same bits


def _cli(*args):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)


@gpu
def test_cli_rhs(need_gpu, tmp_path):
    exe, mat = BUILD / "spmv-csr", GOLDEN / "lap32.mtx.rcm.csr"
    out4, out1 = tmp_path / "y4.bin", tmp_path / "y1.bin"
    p = _cli(exe, mat, 3, "--rhs", 4, "--x", "rand:42", "--dump-y", out4)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Rhs: 4" in p.stdout and "Check: PASS" in p.stdout and "Number Wrong: 0" in p.stdout
    p1 = _cli(exe, mat, 3, "--x", "rand:42", "--dump-y", out1)
    assert p1.returncode == 0 and "Rhs:" not in p1.stdout
    y1 = np.fromfile(out1, np.float64)
    Y = np.fromfile(out4, np.float64).reshape(y1.shape[0], 4)
    assert np.array_equal(bits(Y[:, 0]), bits(y1))
    A = hspmv.read_csr(mat, np.float64)
    for c in range(4):  # column c: the generator with seed 42 + c
        assert np.array_equal(bits(Y[:, c]), bits(oracle.spmv(A.row_ptr, A.col_idx, A.val, gen.rand_x(A.n, 42 + c))))
    bad = _cli(exe, mat, 3, "--rhs", 4, "--gpus", 2)
    assert bad.returncode != 0 and "--rhs" in bad.stderr
    bad = _cli(exe, mat, 3, "--rhs", 4, "--kernel", "stream")
    assert bad.returncode != 0 and "--rhs" in bad.stderr
