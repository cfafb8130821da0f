"""w . y and y . y from the pass that writes y (hspmv_spmv_axpby_dot).

y, for every case, is compared byte for byte with tests/test_axpby.py's model
over the GPU's own s = A x, so no dot check depends on the SpMV's rounding.
The dots are compared with math.fsum over the double products of the y that
get_y() returned, within the derived bound of tests/dot_cases.py:
(m + 4) 2^-53 sum|t_i|.

CPU: the refusals that need no device, the struct sizes, the Python argument
errors, and the bound itself (legitimate orders stay inside it, a dropped
slice falls far outside).  GPU: the fused path over the row-slice shapes and
the same forced through the two passes, every other plan through the two-pass
path, block and group boundaries, a misaligned bound y, reproducibility across
the alternating sweep, bound results and w, the order of calls, the timing
call and the sharded handle's refusals.
"""
import ctypes as C

import numpy as np
import pytest

import hspmv
from dot_cases import (DOT_WY, DOT_YY, E_INVALID, E_STATE, NAN_PAIR, PAIRS, VALUE_DTYPE, VECTOR_DTYPE, WHICH,
                       assert_dots, dot_bound, dot_ref, model, ragged_lengths, same_bytes, slice_handle,
                       slice_matrices, square_ragged, terms_of, two_pass_cases)
from hspmv import _lib, gen
from hspmv.api import CsrMatrix


# ------------------------------------------------------------------ CPU

def test_null_handle_is_invalid_and_touches_no_device():
    L = hspmv.lib()
    t = _lib.Timing()
    d = (C.c_double * 2)()
    for rc in (L.hspmv_spmv_axpby_dot(None, 1.0, 0.0, DOT_YY),
               L.hspmv_run_axpby_dot(None, 1.0, 0.0, DOT_WY | DOT_YY, 1, 1, C.byref(t)),
               L.hspmv_set_w(None, None), L.hspmv_bind_w_device(None, None),
               L.hspmv_bind_dots_device(None, None), L.hspmv_get_dots(None, d)):
        assert rc == E_INVALID
        assert "invalid handle" in _lib.last_error()


def test_bad_which_is_refused_without_a_handle():
    L = hspmv.lib()
    t = _lib.Timing()
    for which in (0, 4, 7, 1 << 31):
        assert L.hspmv_spmv_axpby_dot(None, 1.0, 0.0, which) == E_INVALID
        assert "which" in _lib.last_error()
        assert L.hspmv_run_axpby_dot(None, 1.0, 0.0, which, 1, 1, C.byref(t)) == E_INVALID
        assert "which" in _lib.last_error()


def test_no_struct_grew():
    assert C.sizeof(_lib.Options) == 88
    assert C.sizeof(_lib.Info) == 304
    assert _lib.Options._fields_[-1][0] == "row_slices" and _lib.Info._fields_[-1][0] == "reserved1"
    text = _lib.HEADER.read_text()
    assert "#define HSPMV_DOT_WY 1u" in text and "#define HSPMV_DOT_YY 2u" in text
    assert (_lib.DOT_WY, _lib.DOT_YY) == (1, 2)
    assert "#define HSPMV_VERSION_MINOR 1\n" in text


def test_python_argument_errors_come_before_any_library_call():
    op = hspmv.SpMV.__new__(hspmv.SpMV)  # no handle: a library call would fail on _h
    op.A = CsrMatrix(5, 7, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    op.dtype = np.dtype(np.float32)
    with pytest.raises(ValueError):
        op.set_w(np.zeros(4, np.float32))  # not (m,)
    with pytest.raises(ValueError):
        op.set_w(np.zeros((5, 1), np.float32))
    with pytest.raises(ValueError):
        op.set_w(np.zeros(5, np.complex64))  # does not cast same_kind
    with pytest.raises(ValueError):
        op.spmv_axpby_dot(1.0, 0.0, wy=False, yy=False)
    with pytest.raises(ValueError):
        op.run_axpby_dot(1.0, 0.0, wy=False, yy=False)


def test_bound_holds_for_legitimate_orders_and_catches_a_dropped_slice():
    """The bound is neither vacuous nor violated by another order of the same
    double additions: numpy's pairwise dot and a cumulative sum from the last
    term down stay inside it; leaving out one 64-row slice's terms is outside
    it by orders of magnitude."""
    for dt, m in ((np.float64, 1500), (np.float32, 1500), (np.float64, 257), (np.float32, 65)):
        w = gen.rand_x(m, 5).astype(dt)
        y = gen.rand_x(m, 6).astype(dt)
        for a in (w, y):
            t = terms_of(a, y)
            ref, bound = dot_ref(t), dot_bound(t)
            assert 0 < bound < 1e-10 * np.abs(t).sum()
            assert abs(float(np.dot(a.astype(np.float64), y.astype(np.float64))) - ref) <= bound
            assert abs(float(np.cumsum(t[::-1])[-1]) - ref) <= bound
            dropped = np.concatenate([t[:m - 1 if m < 128 else 64], t[128:]])  # one slice (or one term) missing
            assert abs(float(dropped.sum()) - ref) > 1e6 * bound


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def need_gpu():
    assert hspmv.device_count() >= 1, "no HIP device visible: the gpu tests must run on the MI355X box"


def check_all(op, x, w, s=None, what=""):
    """Every scalar pair and every `which` on op: y against the model's bytes,
    the dots against fsum over that y.  Returns s."""
    m, dt = op.A.m, np.dtype(op.dtype)
    if s is None:
        s = op(x)
    y0 = gen.rand_x(m, 99).astype(dt)
    for alpha, beta in PAIRS:
        yold = np.full(m, np.nan, dt) if (alpha, beta) == NAN_PAIR else y0
        for wy, yy in WHICH:
            op.set_y(yold)
            op.spmv_axpby_dot(alpha, beta, wy=wy, yy=yy)
            got = op.get_y()
            assert same_bytes(got, model(s, yold, alpha, beta)), (what, alpha, beta, op.axpby_path)
            assert_dots(op.get_dots(), w, got, wy, yy, f"{what} {alpha},{beta} {op.axpby_path}")
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["stream", "csr3"])
@pytest.mark.parametrize("dn", ["f64", "f32", "mixed"])
def test_gpu_fused_dots_and_the_same_two_pass(need_gpu, dn, which):
    bits = set()
    for name, A in slice_matrices(VALUE_DTYPE[dn]):
        dt = np.dtype(VECTOR_DTYPE[dn])
        x = gen.rand_x(A.n, 7).astype(dt)
        w = gen.rand_x(A.m, 8).astype(dt)
        with slice_handle(A, which, dn) as op:
            info = op.info
            assert info["row_slices"] == 1, name
            bits.add(info["slice_pos_bits"])
            assert op.axpby_path == "fused", name
            s = op(x)
            before = op.info["device_bytes"]
            op.set_w(w)
            op.set_y(np.zeros(A.m, dt))
            op.spmv_axpby_dot(1.0, 0.0, wy=True, yy=True)
            grown = op.info["device_bytes"] - before
            # own w, the partial pairs (one per wave task, one per 256 rows) and the result pair
            n_slices = info["wave_tasks"] if which == "csr3" else (A.m + 63) // 64
            assert info["blocks"] == (n_slices + 3) // 4, name
            assert grown == A.m * dt.itemsize + 16 * (n_slices + (A.m + 255) // 256) + 16, name
            check_all(op, x, w, s, name)
            assert op.info["device_bytes"] - before == grown, name  # the first call only
            op.set_axpby_path("two_pass")
            assert op.axpby_path == "two_pass", name
            check_all(op, x, w, s, name)
            # the two-pass path's scratch vector and nothing else
            assert op.info["device_bytes"] - before == grown + A.m * dt.itemsize, name
            op.set_axpby_path("auto")
            assert op.axpby_path == "fused", name
    assert bits == {12, 16}


TWO_PASS = two_pass_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("case", TWO_PASS, ids=[c[0] for c in TWO_PASS])
def test_gpu_every_plan_two_pass(need_gpu, case):
    cid, dn, make, kw, want_info = case
    A = make(VALUE_DTYPE[dn])
    kw = dict(kw)
    maps = hspmv.build_csr3_maps(A, *kw.pop("maps")) if "maps" in kw else None
    if dn == "mixed":
        kw["vector_dtype"] = np.float64
    dt = np.dtype(VECTOR_DTYPE[dn])
    x = gen.rand_x(A.n, 42).astype(dt)
    w = gen.rand_x(A.m, 43).astype(dt)
    with hspmv.SpMV(A, maps, device=0, **kw) as op:
        info = op.info
        for k, v in want_info.items():
            assert info[k] == v, (k, info[k])
        assert info["row_slices"] == 0 and op.axpby_path == "two_pass"
        op.set_w(w)
        before = op.info["device_bytes"]
        check_all(op, x, w, what=cid)
        # scratch vector, one pair per 256 rows, the result pair: from the first call on
        grown = op.info["device_bytes"] - before
        assert grown == A.m * dt.itemsize + 16 * ((A.m + 255) // 256) + 16
        op.spmv_axpby_dot(0.5, 0.5, wy=True, yy=True)
        assert op.info["device_bytes"] - before == grown


@pytest.mark.gpu
@pytest.mark.parametrize("dn", ["f64", "f32"])
@pytest.mark.parametrize("m", [1, 255, 256, 257, 513])
def test_gpu_two_pass_block_and_group_boundaries(need_gpu, dn, m):
    A = ragged_lengths(m, VALUE_DTYPE[dn], seed=100 + m)
    dt = np.dtype(VECTOR_DTYPE[dn])
    with hspmv.SpMV(A, kernel="stream", device=0) as op:
        assert op.axpby_path == "two_pass"
        w = gen.rand_x(A.m, 11).astype(dt)
        op.set_w(w)
        check_all(op, gen.rand_x(A.n, 10).astype(dt), w, what=f"m{m}")


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False])
def test_gpu_bound_y_at_an_8_byte_offset(need_gpu, fused):
    """A bound y that is not 16-byte aligned: the two-pass kernel's per-element
    threads (and the slice kernel, which never groups y)."""
    import torch
    A = ragged_lengths(777, np.float64, seed=31)
    x, b, w = gen.rand_x(A.n, 3), gen.rand_x(A.m, 4), gen.rand_x(A.m, 5)
    with hspmv.SpMV(A, kernel="stream", device=0, options=ON_OR_NONE[fused]) as op:
        assert op.axpby_path == ("fused" if fused else "two_pass")
        s = op(x)
        xd = torch.from_numpy(x).to("cuda")
        buf = torch.full((A.m + 3,), 7.0, dtype=torch.float64, device="cuda")
        buf[1:1 + A.m] = torch.from_numpy(b).to("cuda")
        torch.cuda.synchronize()
        op.bind_x_device(xd.data_ptr())
        op.bind_y_device(buf.data_ptr() + 8)
        op.set_w(w)
        op.spmv_axpby_dot(-1.0, 1.0, wy=True, yy=True)
        dots = op.get_dots()
        h = buf.cpu().numpy()
        assert h[0] == 7.0 and np.all(h[1 + A.m:] == 7.0)
        got = h[1:1 + A.m].copy()
        assert same_bytes(got, model(s, b, -1.0, 1.0))
        assert_dots(dots, w, got, True, True, "offset y")
        op.bind_x_device(None)
        op.bind_y_device(None)


ON_OR_NONE = {True: {"x_dict": 1, "row_slices": 1}, False: None}


@pytest.mark.gpu
@pytest.mark.parametrize("dn", ["f64", "f32", "mixed"])
def test_gpu_same_16_bytes_on_every_call_and_sweep_direction(need_gpu, dn):
    A = ragged_lengths(1500, VALUE_DTYPE[dn], seed=23)  # 24 slices, 6 blocks
    dt = np.dtype(VECTOR_DTYPE[dn])
    x = gen.rand_x(A.n, 5).astype(dt)
    w = gen.rand_x(A.m, 6).astype(dt)
    with slice_handle(A, "stream", dn) as op:
        op.set_sweep("alternate")
        assert op.info["sweep"] == 1 and op.axpby_path == "fused"
        op.set_x(x)
        op.set_w(w)
        seen = []
        for _ in range(4):  # two calls in each direction
            op.spmv_axpby_dot(0.5, 0.0, wy=True, yy=True)
            seen.append(np.array(op.get_dots()).tobytes())
        assert len(set(seen)) == 1 and len(seen[0]) == 16
        assert_dots(tuple(np.frombuffer(seen[0])), w, op.get_y(), True, True, "alternate")


@pytest.mark.gpu
def test_gpu_csort_handle_same_16_bytes_twice(need_gpu):
    A = gen.powerlaw(5000, seed=3, dtype=np.float64)
    with hspmv.SpMV(A, kernel="csort", device=0, options={"deterministic": "reproducible"}) as op:
        assert op.info["kernel_name"] == "csort" and op.axpby_path == "two_pass"
        op.set_x(gen.rand_x(A.n, 7))
        w = gen.rand_x(A.m, 8)
        op.set_w(w)
        seen = []
        for _ in range(2):
            op.spmv_axpby_dot(2.0, 0.0, wy=True, yy=True)
            seen.append(np.array(op.get_dots()).tobytes())
        assert seen[0] == seen[1]
        assert_dots(tuple(np.frombuffer(seen[0])), w, op.get_y(), True, True, "csort")


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False])
def test_gpu_bound_dots_and_w(need_gpu, fused):
    import torch
    A = square_ragged(900)
    x = gen.rand_x(A.n, 3)
    with hspmv.SpMV(A, kernel="stream", device=0, options=ON_OR_NONE[fused]) as op:
        assert op.axpby_path == ("fused" if fused else "two_pass")
        # a fresh handle has no dots; WY needs a w
        with pytest.raises(hspmv.HspmvError) as e:
            op.get_dots()
        assert e.value.code == E_STATE
        s = op(x)
        with pytest.raises(hspmv.HspmvError) as e:
            op.spmv_axpby_dot(1.0, 0.0, wy=True, yy=False)
        assert e.value.code == E_STATE
        assert same_bytes(op.get_y(), s)  # nothing ran
        # results into elements 1..2 of a 4-element tensor: the sentinels survive
        res = torch.tensor([-3.0, 11.0, 12.0, -4.0], dtype=torch.float64, device="cuda")
        xd = torch.from_numpy(x).to("cuda")
        torch.cuda.synchronize()
        op.bind_dots_device(res.data_ptr() + 8)
        op.bind_x_device(xd.data_ptr())
        op.bind_w_device(xd.data_ptr())  # w = x: x . A x
        op.spmv_axpby_dot(1.0, 0.0, wy=True, yy=False)
        op.synchronize()
        r = res.cpu().numpy()
        assert r[0] == -3.0 and r[3] == -4.0 and r[2] == 0.0
        y = op.get_y()
        assert same_bytes(y, s)
        assert_dots((r[1], r[2]), x, y, True, False, "x.Ax")
        assert op.get_dots() == (r[1], r[2])
        # w = y's pointer: refused, nothing launched, the results as they were
        op.bind_w_device(op.y_device())
        with pytest.raises(hspmv.HspmvError) as e:
            op.spmv_axpby_dot(3.0, 0.0, wy=True, yy=True)
        assert e.value.code == E_INVALID
        op.synchronize()
        assert same_bytes(op.get_y(), s) and np.array_equal(res.cpu().numpy(), r)
        # YY alone never looks at w
        op.spmv_axpby_dot(1.0, 0.0, wy=False, yy=True)
        op.synchronize()
        r2 = res.cpu().numpy()
        assert r2[0] == -3.0 and r2[3] == -4.0 and r2[1] == 0.0
        assert_dots((r2[1], r2[2]), x, op.get_y(), False, True, "yy alone")
        # back to the handle's own pair
        op.bind_dots_device(None)
        op.bind_w_device(None)
        op.set_w(x)
        op.spmv_axpby_dot(1.0, 0.0, wy=True, yy=True)
        assert_dots(op.get_dots(), x, op.get_y(), True, True, "own pair")
        assert np.array_equal(res.cpu().numpy(), r2)
        op.bind_x_device(None)


@pytest.mark.gpu
def test_gpu_order_of_calls(need_gpu):
    A = ragged_lengths(500, np.float64, seed=41)
    x = gen.rand_x(A.n, 8)
    w = gen.rand_x(A.m, 9)
    with slice_handle(A, "stream", "f64") as op:
        assert op.axpby_path == "fused"
        s = op(x)
        y0 = gen.rand_x(A.m, 12)
        op.set_w(w)
        op.set_y(y0)
        op.spmv_axpby_dot(0.5, -0.25, wy=True, yy=True)
        d1 = op.get_dots()
        assert same_bytes(op.get_y(), model(s, y0, 0.5, -0.25))
        op.spmv()  # spmv after the dot call: s's bytes again
        assert same_bytes(op.get_y(), s)
        # spmv_axpby and spmv_axpby_dot write the same y
        op.set_y(y0)
        op.spmv_axpby(0.5, -0.25)
        assert same_bytes(op.get_y(), model(s, y0, 0.5, -0.25))
        # new values on the planned handle: the dots follow them
        v2 = A.val * 0.75 - 0.5
        op.update_values(v2)
        s2 = op(x)
        assert not same_bytes(s2, s)
        op.set_y(y0)
        op.spmv_axpby_dot(0.5, -0.25, wy=True, yy=True)
        got = op.get_y()
        assert same_bytes(got, model(s2, y0, 0.5, -0.25))
        d2 = op.get_dots()
        assert_dots(d2, w, got, True, True, "after update_values")
        assert d2 != d1


@pytest.mark.gpu
def test_gpu_run_axpby_dot_times_and_evolves_y(need_gpu):
    A = ragged_lengths(500, np.float64, seed=43)
    x = gen.rand_x(A.n, 8)
    w = gen.rand_x(A.m, 9)
    for opts in (ON_OR_NONE[True], None):
        with hspmv.SpMV(A, kernel="stream", device=0, options=opts) as op:
            s = op(x)
            y = gen.rand_x(A.m, 13)
            op.set_y(y)
            op.set_w(w)
            t = op.run_axpby_dot(-1.0, 0.5, wy=True, yy=True, warmup=1, iters=2)
            assert t["iters"] == 2 and 0 < t["t_min"] <= t["t_max"] and t["num_gpus"] == 1
            assert t["gbps_alg"] > 0
            for _ in range(3):
                y = model(s, y, -1.0, 0.5)
            got = op.get_y()
            assert same_bytes(got, y)
            assert_dots(op.get_dots(), w, got, True, True, "run")


@pytest.mark.gpu
def test_gpu_sharded_handle_refuses(need_gpu):
    A = gen.laplace2d(64, 48)
    x = gen.rand_x(A.n, 42)
    with hspmv.SpMV(A, devices=[0, 0]) as op:
        assert op.info["num_gpus"] == 2
        y = op(x)
        for call in (lambda: op.spmv_axpby_dot(-1.0, 1.0, wy=False, yy=True), lambda: op.set_w(np.zeros(A.m)),
                     lambda: op.bind_w_device(None), lambda: op.bind_dots_device(None), lambda: op.get_dots(),
                     lambda: op.run_axpby_dot(-1.0, 0.5, warmup=1, iters=1)):
            with pytest.raises(hspmv.HspmvError) as e:
                call()
            assert e.value.code == E_INVALID
        assert same_bytes(op.get_y(), y)  # y untouched
