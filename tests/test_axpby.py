"""y = alpha A x + beta y on a handle (hspmv_spmv_axpby).

The model, for every case: s = op(x) comes from the GPU (the bits hspmv_spmv
writes for this handle and plan); ``T(alpha) * s`` and ``T(beta) * y0`` are
formed as separate numpy arrays in the vectors' dtype T and added -- three
roundings, no fma -- and with beta == 0 the first array alone is the answer.
The comparison is of bytes (``.view(np.uint32 / np.uint64)``), not of values.

CPU: the NULL-handle refusals, the struct sizes (no field was added) and the
Python argument errors.  GPU: every plan through the two-pass path, the row
slices through the fused kernel and again forced through the two passes, the
alternating sweep, bound torch arrays, the order of calls, and the sharded
handle's refusal.
"""
import ctypes as C

import numpy as np
import pytest

import hspmv
from hspmv import _lib, gen
from hspmv.api import CsrMatrix

F64_SERIAL, F32_SERIAL = 40, 56  # hspmv_internal.h kSerialMax / kSerialMaxF32
E_INVALID = -1

# (alpha, beta); the last one runs over a y0 that is all NaN
PAIRS = [(1.0, 0.0), (-1.0, 1.0), (0.5, -0.25), (0.0, 1.0), (2.0, 0.0)]
NAN_PAIR = (2.0, 0.0)


def uint_of(dtype):
    return np.uint64 if np.dtype(dtype) == np.float64 else np.uint32


def model(s, y0, alpha, beta):
    """fl(fl(alpha_T s) + fl(beta_T y0)) in s's dtype; beta == 0: fl(alpha_T s)."""
    T = s.dtype.type
    first = T(alpha) * s
    assert first.dtype == s.dtype
    if beta == 0:
        return first
    second = T(beta) * y0
    assert second.dtype == s.dtype
    return first + second


def same_bytes(got, want):
    u = uint_of(want.dtype)
    return got.dtype == want.dtype and np.array_equal(got.view(u), want.view(u))


def check_pairs(op, x, s=None):
    """Every scalar pair on op against the model; returns s."""
    m, dt = op.A.m, np.dtype(op.dtype)
    if s is None:
        s = op(x)
    y0 = gen.rand_x(m, 99).astype(dt)
    for alpha, beta in PAIRS:
        yold = np.full(m, np.nan, dt) if (alpha, beta) == NAN_PAIR else y0
        op.set_y(yold)
        op.spmv_axpby(alpha, beta)
        got = op.get_y()
        assert same_bytes(got, model(s, yold, alpha, beta)), (alpha, beta, op.axpby_path)
    return s


# ------------------------------------------------------------------ CPU

def test_null_handle_is_invalid_and_touches_no_device():
    L = hspmv.lib()
    t = _lib.Timing()
    assert L.hspmv_spmv_axpby(None, 1.0, 0.0) == E_INVALID
    assert L.hspmv_set_y(None, None) == E_INVALID
    assert L.hspmv_run_axpby(None, 1.0, 0.0, 1, 1, C.byref(t)) == E_INVALID
    assert L.hspmv_set_axpby_path(None, 0) == E_INVALID
    assert L.hspmv_axpby_path(None) == E_INVALID
    assert "invalid handle" in _lib.last_error()


def test_no_struct_grew():
    """Everything new is a function: hspmv_options and hspmv_info keep the
    sizes of the commit before this feature."""
    assert C.sizeof(_lib.Options) == 88
    assert C.sizeof(_lib.Info) == 304
    assert _lib.Options._fields_[-1][0] == "row_slices" and _lib.Info._fields_[-1][0] == "reserved1"


def test_python_argument_errors_come_before_any_library_call():
    op = hspmv.SpMV.__new__(hspmv.SpMV)  # no handle: a library call would fail on _h
    op.A = CsrMatrix(5, 7, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    op.dtype = np.dtype(np.float32)
    with pytest.raises(ValueError):
        op.set_y(np.zeros(4, np.float32))  # not (m,)
    with pytest.raises(ValueError):
        op.set_y(np.zeros((5, 1), np.float32))
    with pytest.raises(ValueError):
        op.set_y(np.zeros(5, np.complex64))  # does not cast same_kind
    with pytest.raises(ValueError):
        op.set_axpby_path("fused")
    with pytest.raises(ValueError):
        op.set_axpby_path(1)


def test_model_rounds_three_times():
    """The model itself: two products and a sum, each rounded to T (a fused
    multiply-add of the same operands gives another last bit here)."""
    s = np.array([1.0 + 2.0 ** -23], np.float32)
    alpha = 1.0 + 2.0 ** -23  # alpha s = 1 + 2^-22 + 2^-46: rounds to 1 + 2^-22
    y0 = np.array([1.0 + 2.0 ** -22], np.float32)
    fused = np.float32(np.float64(np.float32(alpha)) * np.float64(s[0]) - np.float64(y0[0]))
    assert model(s, y0, alpha, -1.0)[0] == 0.0 and fused == np.float32(2.0 ** -46)


# ------------------------------------------------------------------ matrices (tests/test_row_slices.py's shapes)

def fixed_rows(L, m=200, dtype=np.float64, seed=3):
    rng = np.random.default_rng(seed + L)
    rp = (np.arange(m + 1, dtype=np.int64) * L).astype(np.int32)
    col = (np.arange(m)[:, None] + np.arange(L)[None, :]).astype(np.int32).ravel()
    val = rng.uniform(-1.0, 1.0, m * L).astype(dtype)
    return CsrMatrix(m, m + L, rp, col, val)


def ragged(lens, dtype=np.float64, seed=5):
    lens = np.asarray(lens, np.int64)
    m = len(lens)
    rng = np.random.default_rng(seed)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([r + 2 * np.arange(k) for r, k in enumerate(lens)] + [np.zeros(0, np.int64)])
    val = rng.uniform(-1.0, 1.0, int(lens.sum())).astype(dtype)
    return CsrMatrix(m, int(m + 2 * lens.max() + 1), rp, col.astype(np.int32), val)


def with_empty_rows(dtype=np.float64):
    lens = np.full(320, 3)
    lens[5::32] = 0
    lens[64:128] = 0
    return ragged(lens, dtype)


def ragged_lengths(m, dtype, seed=17):
    rng = np.random.default_rng(seed)
    return ragged(rng.integers(1, 20, m), dtype, seed=seed)


def slice_matrices(dtype):
    """(name, matrix): fixed rows of 1..17 nonzeros (m = 200: 16-bit
    positions below 8 slots, the 12-bit groups from 8 on, every batch
    remainder), ragged lengths, empty rows, m = 1, m = 65 and m = 257 (a last
    slice of one row, a last block of one slice)."""
    out = [(f"fixed{L}", fixed_rows(L, dtype=dtype)) for L in range(1, 18)]
    out.append(("ragged", ragged_lengths(300, dtype)))
    out.append(("empty_rows", with_empty_rows(dtype)))
    for m in (1, 65, 257):
        out.append((f"m{m}", ragged_lengths(m, dtype, seed=m)))
    return out


ON = {"x_dict": 1, "row_slices": 1}


def slice_handle(A, which, dtype_name):
    """The handle of group 2: STREAM, or CSR3 over maps, with forced row
    slices; "mixed": fp32 values under fp64 vectors."""
    maps = hspmv.build_csr3_maps(A, 20, 10) if which == "csr3" else None
    kw = {"vector_dtype": np.float64} if dtype_name == "mixed" else {}
    return hspmv.SpMV(A, maps, kernel=which, device=0, options=ON, **kw)


VALUE_DTYPE = {"f64": np.float64, "f32": np.float32, "mixed": np.float32}
VECTOR_DTYPE = {"f64": np.float64, "f32": np.float32, "mixed": np.float64}


def test_slice_matrices_take_the_slice_format():
    """Host: every matrix of group 2 is eligible for the row slices in both
    shapes (so the GPU cases below can ask for the fused path)."""
    for dtype in (np.float64, np.float32):
        for name, A in slice_matrices(dtype):
            for which in ("stream", "csr3"):
                maps = hspmv.build_csr3_maps(A, 20, 10) if which == "csr3" else None
                S = hspmv.slices_plan(A, maps, kernel=which, options=ON, fill=False)
                assert S["why"] == "ok", (name, which, S["why"])


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def need_gpu():
    assert hspmv.device_count() >= 1, "no HIP device visible: the gpu tests must run on the MI355X box"


def split_row_matrix(dtype=np.float64):
    """130 short rows and one of 5000 nonzeros (> 4096: the split-row kernels)."""
    lens = np.full(130, 3)
    lens[70] = 5000
    return ragged(lens, dtype)


def two_pass_cases():
    """(id, dtype name, matrix maker, SpMV keywords, info the plan must report)."""
    lap = lambda dt: gen.laplace2d(64, 48).astype(dt)  # noqa: E731
    plaw = lambda dt: gen.powerlaw(5000, seed=3, dtype=dt)  # noqa: E731
    cases = []
    for dn in ("f64", "f32", "mixed"):
        cases.append((f"stream-{dn}", dn, lap, {"kernel": "stream"}, {"kernel_name": "stream"}))
        cases.append((f"csr3-{dn}", dn, lap, {"kernel": "csr3", "maps": (7, 8)}, {"kernel_name": "csr3"}))
    for dn in ("f64", "f32"):
        cases.append((f"csort-{dn}", dn, plaw, {"kernel": "csort"}, {"kernel_name": "csort"}))
    cases += [
        ("vector-f64", "f64", lap, {"kernel": "vector"}, {"kernel_name": "vector"}),
        ("csort-reproducible-f64", "f64", plaw, {"kernel": "csort", "options": {"deterministic": "reproducible"}},
         {"kernel_name": "csort", "csort_fixed_point": 1}),
        ("serial-f64", "f64", plaw, {"options": {"deterministic": "serial"}}, {"serial_order": 1}),
        # x_slabs = 1 asks for one slab, which is no slab at any size
        # (plan_xslabs keeps B >= 2): the handle runs its plain plan.  The slab
        # passes themselves are the next case, with the smallest count that
        # reports them.
        ("xslabs1-f64", "f64", plaw, {"options": {"x_slabs": 1}}, {"x_slabs": 0}),
        ("xslabs2-f64", "f64", plaw, {"options": {"x_slabs": 2}}, {"x_slabs": 2}),
        ("split-row-f64", "f64", split_row_matrix, {}, {"n_split_rows": 1}),
    ]
    return cases


TWO_PASS = two_pass_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("case", TWO_PASS, ids=[c[0] for c in TWO_PASS])
def test_gpu_every_plan_two_pass(need_gpu, case):
    _, dn, make, kw, want_info = case
    A = make(VALUE_DTYPE[dn])
    kw = dict(kw)
    maps = hspmv.build_csr3_maps(A, *kw.pop("maps")) if "maps" in kw else None
    if dn == "mixed":
        kw["vector_dtype"] = np.float64
    x = gen.rand_x(A.n, 42).astype(VECTOR_DTYPE[dn])
    with hspmv.SpMV(A, maps, device=0, **kw) as op:
        info = op.info
        for k, v in want_info.items():
            assert info[k] == v, (k, info[k])
        assert info["row_slices"] == 0 and op.axpby_path == "two_pass"
        before = info["device_bytes"]
        check_pairs(op, x)
        # the scratch vector: m elements from the first call on, nothing later
        grown = op.info["device_bytes"] - before
        assert grown == A.m * np.dtype(op.dtype).itemsize
        op.spmv_axpby(0.5, 0.5)
        assert op.info["device_bytes"] - before == grown


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["stream", "csr3"])
@pytest.mark.parametrize("dn", ["f64", "f32", "mixed"])
def test_gpu_fused_equals_model_and_two_pass(need_gpu, dn, which):
    bits = set()
    for name, A in slice_matrices(VALUE_DTYPE[dn]):
        x = gen.rand_x(A.n, 7).astype(VECTOR_DTYPE[dn])
        with slice_handle(A, which, dn) as op:
            info = op.info
            assert info["row_slices"] == 1, name
            bits.add(info["slice_pos_bits"])
            assert op.axpby_path == "fused", name
            before = info["device_bytes"]
            s = check_pairs(op, x)
            assert op.info["device_bytes"] == before  # the fused path owns no scratch
            op.set_axpby_path("two_pass")
            assert op.axpby_path == "two_pass", name
            check_pairs(op, x, s)
            op.set_axpby_path("auto")
            assert op.axpby_path == "fused", name
    assert bits == {12, 16}


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["stream", "csr3"])
@pytest.mark.parametrize("dn", ["f64", "f32", "mixed"])
def test_gpu_row_past_the_serial_bound_takes_two_passes(need_gpu, dn, which):
    lens = np.full(300, 4)
    lens[131] = (F32_SERIAL if dn == "f32" else F64_SERIAL) + 1
    A = ragged(lens, VALUE_DTYPE[dn])
    with slice_handle(A, which, dn) as op:
        assert op.info["row_slices"] == 0 and op.axpby_path == "two_pass"
        check_pairs(op, gen.rand_x(A.n, 9).astype(VECTOR_DTYPE[dn]))


@pytest.mark.gpu
@pytest.mark.parametrize("dn", ["f64", "f32", "mixed"])
def test_gpu_fused_alternating_sweep(need_gpu, dn):
    """Four calls on a handle that alternates its sweep: y after each is the
    model iterated on the host (the direction never changes a row's bits), and
    a plain spmv in between keeps the alternation going."""
    A = ragged_lengths(1500, VALUE_DTYPE[dn], seed=23)  # 24 slices, 6 blocks
    dt = np.dtype(VECTOR_DTYPE[dn])
    x = gen.rand_x(A.n, 5).astype(dt)
    with slice_handle(A, "stream", dn) as op:
        op.set_sweep("alternate")
        assert op.info["sweep"] == 1 and op.axpby_path == "fused"
        s = op(x)  # one spmv: the phase is odd from here on
        y = gen.rand_x(A.m, 77).astype(dt)
        op.set_y(y)
        for k in range(4):
            op.spmv_axpby(0.5, 0.5)
            y = model(s, y, 0.5, 0.5)
            assert same_bytes(op.get_y(), y), k
            if k == 1:  # a plain spmv between the calls, then y put back
                assert same_bytes(op(x), s)
                op.set_y(y)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False])
def test_gpu_bound_arrays_residual_in_place(need_gpu, fused):
    """b - A x in place in the torch tensor that holds b."""
    import torch
    A = ragged_lengths(777, np.float64, seed=31)
    x = gen.rand_x(A.n, 3)
    b = gen.rand_x(A.m, 4)
    opts = ON if fused else None
    with hspmv.SpMV(A, kernel="stream", device=0, options=opts) as op:
        s = op(x)
        xd = torch.from_numpy(x).to("cuda")
        # an 8-byte offset into the allocation: a bound y that is not 16-byte aligned
        buf = torch.full((A.m + 3,), 7.0, dtype=torch.float64, device="cuda")
        buf[1:1 + A.m] = torch.from_numpy(b).to("cuda")
        torch.cuda.synchronize()
        op.bind_x_device(xd.data_ptr())
        op.bind_y_device(buf.data_ptr() + 8)
        assert op.axpby_path == ("fused" if fused else "two_pass")
        op.spmv_axpby(-1.0, 1.0)
        op.synchronize()
        h = buf.cpu().numpy()
        assert h[0] == 7.0 and np.all(h[1 + A.m:] == 7.0)
        assert same_bytes(h[1:1 + A.m].copy(), model(s, b, -1.0, 1.0))
        # set_y writes the bound array
        op.set_y(b)
        assert same_bytes(buf.cpu().numpy()[1:1 + A.m].copy(), b)
        # x and y the same pointer
        op.bind_y_device(xd.data_ptr())
        with pytest.raises(hspmv.HspmvError) as e:
            op.spmv_axpby(-1.0, 1.0)
        assert e.value.code == E_INVALID
        op.synchronize()
        assert np.array_equal(xd.cpu().numpy(), x)  # refused before any launch
        op.bind_x_device(None)
        op.bind_y_device(None)


@pytest.mark.gpu
def test_gpu_order_of_calls(need_gpu):
    A = ragged_lengths(500, np.float64, seed=41)
    x = gen.rand_x(A.n, 8)
    with slice_handle(A, "stream", "f64") as op:
        assert op.axpby_path == "fused"
        s = op(x)
        y0 = gen.rand_x(A.m, 12)
        op.set_y(y0)
        op.spmv_axpby(0.5, -0.25)
        assert not same_bytes(op.get_y(), s)
        op.spmv()  # spmv after spmv_axpby: s's bytes again
        assert same_bytes(op.get_y(), s)
        # new values on the planned handle: the fused kernel reads them
        v2 = A.val * 0.75 - 0.5
        op.update_values(v2)
        s2 = op(x)
        assert not same_bytes(s2, s)
        with hspmv.SpMV(CsrMatrix(A.m, A.n, A.row_ptr, A.col_idx, v2), kernel="stream", device=0,
                        options=ON) as fresh:
            assert same_bytes(fresh(x), s2)
        op.set_y(y0)
        op.spmv_axpby(0.5, -0.25)
        assert same_bytes(op.get_y(), model(s2, y0, 0.5, -0.25))


@pytest.mark.gpu
def test_gpu_run_axpby_times_and_evolves_y(need_gpu):
    """hspmv_run_axpby: warmup + iters calls in a row, y evolving."""
    A = ragged_lengths(500, np.float64, seed=43)
    x = gen.rand_x(A.n, 8)
    for opts in (ON, None):
        with hspmv.SpMV(A, kernel="stream", device=0, options=opts) as op:
            s = op(x)
            y = gen.rand_x(A.m, 13)
            op.set_y(y)
            t = op.run_axpby(-1.0, 0.5, warmup=1, iters=2)
            assert t["iters"] == 2 and 0 < t["t_min"] <= t["t_max"] and t["num_gpus"] == 1
            for _ in range(3):
                y = model(s, y, -1.0, 0.5)
            assert same_bytes(op.get_y(), y)


@pytest.mark.gpu
def test_gpu_sharded_handle_refuses(need_gpu):
    import oracle
    A = gen.laplace2d(64, 48)
    x = gen.rand_x(A.n, 42)
    with hspmv.SpMV(A, devices=[0, 0]) as op:
        assert op.info["num_gpus"] == 2
        y = op(x)
        for call in (lambda: op.spmv_axpby(-1.0, 1.0), lambda: op.set_y(np.zeros(A.m)),
                     lambda: op.run_axpby(-1.0, 0.5, 1, 1), lambda: op.axpby_path):
            with pytest.raises(hspmv.HspmvError) as e:
                call()
            assert e.value.code == E_INVALID
        assert same_bytes(op.get_y(), y)  # y untouched
        assert np.array_equal(op(x), oracle.spmv(A.row_ptr, A.col_idx, A.val, x))
