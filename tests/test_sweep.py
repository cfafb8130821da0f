"""Alternating block sweep (hspmv_set_sweep): every other SpMV of a handle
runs the row kernel's workgroups last block to first, so that it starts on
the bytes the Infinity Cache still holds from the call before.

CPU: the block order the kernels and the host share (hspmv_block_order:
xcd_chunk_remap, then the mirror) is a bijection on [0, nb) for every chunk,
and the reversed order is nb - 1 - forward pointwise; the entry point's
argument checks; the ABI mirrors.

GPU: a handle that alternates writes, on each of four consecutive calls, the
bytes a forward-only handle of the same options writes -- y poisoned with NaN
before every call, so a block the mirrored order skipped (or ran twice in
place of another) shows.  A row's sum never leaves its workgroup, so the
bar is equality of bytes, for every kernel shape that takes the block order.
"""
import ctypes

import numpy as np
import pytest

import hspmv
from hspmv import _lib, gen
from hspmv.api import CsrMatrix


# ------------------------------------------------------------------ CPU

def block_order(nb, chunk, reverse):
    out = np.full(nb, -1, np.int32)
    rc = hspmv.lib().hspmv_block_order(nb, chunk, int(reverse), out.ctypes.data if nb else None)
    assert rc == 0, _lib.last_error()
    return out


def chunks_for(nb):
    return sorted({1, 2, 4, 8, 64, max(nb // 8, 1)})


@pytest.mark.parametrize("nb", list(range(1, 301)) + [3907, 7633, 40001, 1 << 20, (1 << 20) + 37])
def test_block_order_is_a_bijection_and_reverse_is_its_mirror(nb):
    ident = np.arange(nb, dtype=np.int32)
    for chunk in chunks_for(nb):
        fwd = block_order(nb, chunk, False)
        rev = block_order(nb, chunk, True)
        assert np.array_equal(np.sort(fwd), ident), (nb, chunk)
        assert np.array_equal(np.sort(rev), ident), (nb, chunk)
        assert np.array_equal(rev, nb - 1 - fwd), (nb, chunk)


def test_block_order_forward_is_the_xcd_chunk_remap():
    """The forward order is the documented one: test_block_order.py's numpy
    restatement of xcd_chunk_remap."""
    from test_block_order import xcd_chunk_remap
    for nb in (1, 9, 37, 64, 65, 1000, 7633):
        for chunk in chunks_for(nb):
            assert np.array_equal(block_order(nb, chunk, False), xcd_chunk_remap(np.arange(nb), nb, chunk))
    # chunk 0 (unset) and 1 are the dispatch order; its mirror counts down
    assert np.array_equal(block_order(10, 0, False), np.arange(10))
    assert np.array_equal(block_order(10, 1, True), np.arange(9, -1, -1))
    # the largest chunk the flags can ask for (2^30): no full span, and no overflow of 8 * chunk
    assert np.array_equal(block_order(1000, 1 << 30, False), np.arange(1000))
    assert np.array_equal(block_order(1000, 1 << 30, True), np.arange(999, -1, -1))


def test_block_order_keeps_xcd_turns_together_when_reversed():
    """The mirror comes after the remap: the s blocks of one XCD turn are still
    s consecutive logical blocks (the dictionary halo stays in that L2)."""
    nb, s = 8 * 16 * 5, 16
    rev = block_order(nb, s, True)
    for x in range(8):
        mine = rev[x::8]  # the blocks XCD x is dispatched, in dispatch order
        for t in range(0, len(mine), s):
            turn = np.sort(mine[t:t + s])
            assert np.array_equal(turn, np.arange(turn[0], turn[0] + s))


def test_block_order_and_set_sweep_reject_bad_arguments():
    L = hspmv.lib()
    assert L.hspmv_set_sweep(None, 0) == -1 and L.hspmv_last_error()
    assert L.hspmv_set_sweep(None, 2) == -1
    assert L.hspmv_block_order(-1, 1, 0, None) == -1
    assert L.hspmv_block_order(4, 1, 0, None) == -1
    assert L.hspmv_block_order(4, -2, 0, None) == -1
    assert L.hspmv_block_order(1 << 31, 1, 0, None) == -1
    assert L.hspmv_block_order(0, 1, 0, None) == 0


def test_sweep_abi_fields_are_appended():
    assert _lib.Info.sweep.offset > _lib.Info.slice_pos_bits.offset
    assert _lib.Info.reserved1.offset == _lib.Info.sweep.offset + 4
    assert ctypes.sizeof(_lib.Info) == _lib.Info.reserved1.offset + 4  # no hidden padding
    assert _lib.SWEEP == {"auto": 0, "forward": 1, "alternate": 2}
    text = _lib.HEADER.read_text()
    for name, v in _lib.SWEEP.items():
        assert f"#define HSPMV_SWEEP_{name.upper()} {v}\n" in text


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def need_gpu():
    assert hspmv.device_count() >= 1, "no HIP device visible: the gpu tests must run on the MI355X box"


_HIP = None


def hip_runtime():
    """The HIP runtime this process already runs on (the one libhspmv's and
    torch's SONAME resolved to), for hipMemset on the handles' own y."""
    global _HIP
    if _HIP is None:
        hspmv.device_count()
        path = None
        with open("/proc/self/maps") as fp:
            for line in fp:
                if "libamdhip64.so" in line:
                    path = line.split()[-1]
                    break
        assert path, "no HIP runtime mapped"
        _HIP = ctypes.CDLL(path)
        _HIP.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
        _HIP.hipMemset.restype = ctypes.c_int
        _HIP.hipDeviceSynchronize.restype = ctypes.c_int
    return _HIP


def poison_y(op, A, splits):
    """Every byte of every shard's y to 0xFF (a NaN in fp32 and fp64)."""
    H = hip_runtime()
    op.synchronize()
    sv = A.val.dtype.itemsize
    for g in range(len(splits) - 1):
        rows = int(splits[g + 1] - splits[g])
        if rows:
            assert H.hipMemset(op.y_device(g), 0xFF, rows * sv) == 0
    assert H.hipDeviceSynchronize() == 0


def four_calls(A, maps, x, mode, devices=None, **kw):
    """y after each of four consecutive SpMVs of one handle, and its info."""
    kw = dict(kw)
    if devices is None:
        kw["device"] = 0
        splits = [0, A.m]
    else:
        kw["devices"] = devices
        splits = hspmv.partition_rows(A.row_ptr, len(devices), maps)
    with hspmv.SpMV(A, maps, **kw) as op:
        if mode is not None:
            op.set_sweep(mode)
        op.set_x(x)
        ys = []
        for _ in range(4):
            poison_y(op, A, splits)
            op.spmv()
            ys.append(op.get_y().tobytes())
        return ys, op.info


def check_case(A, maps, want_sweep=(0, 1), **kw):
    x = gen.rand_x(A.n, 42).astype(A.val.dtype)
    fwd, i0 = four_calls(A, maps, x, "forward", **kw)
    alt, i1 = four_calls(A, maps, x, "alternate", **kw)
    assert (i0["sweep"], i1["sweep"]) == want_sweep
    for k in ("kernel", "blocks", "xcd_remap", "row_slices", "x_dict", "x_windows", "x_slabs", "csr3_plan"):
        assert i0[k] == i1[k], k
    for call in range(4):
        assert alt[call] == fwd[call], call
        y = np.frombuffer(fwd[call], A.val.dtype)
        assert not np.isnan(y).any(), call  # every row was written
    assert fwd[0] == fwd[1] == fwd[2] == fwd[3]
    return i1


def ragged_rows(m, dtype=np.float64, seed=2, n=500, hi=30):
    """m rows of 0 .. hi - 1 nonzeros at random columns."""
    rng = np.random.default_rng(seed + m)
    lens = rng.integers(0, hi, m)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.sort(rng.integers(0, n, (m, hi)), axis=1)
    col = np.concatenate([ci[r, :lens[r]] for r in range(m)] + [np.zeros(0, np.int64)]).astype(np.int32)
    return CsrMatrix(m, n, rp, col, rng.uniform(-1, 1, int(rp[-1])).astype(dtype))


def short_banded(m, dtype=np.float64):
    """m rows of 5 nonzeros on a band: eligible for the row slices."""
    rp = (np.arange(m + 1, dtype=np.int64) * 5).astype(np.int32)
    col = (np.arange(m)[:, None] + np.arange(5)[None, :]).astype(np.int32).ravel()
    val = np.random.default_rng(m).uniform(-1, 1, 5 * m).astype(dtype)
    return CsrMatrix(m, m + 5, rp, col, val)


SLICES = {"x_dict": 1, "row_slices": 1}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_gpu_row_slices_stencil(need_gpu, dtype):
    """9261 rows = 37 dictionary blocks: not a multiple of 8 * chunk, so the
    remap's tail rule and the mirror meet."""
    A = gen.stencil27(21, dtype=dtype)
    for maps, kernel in ((hspmv.build_csr3_maps(A, 20, 10), "auto"), (None, "stream")):
        info = check_case(A, maps, kernel=kernel, options=SLICES)
        assert info["row_slices"] == 1
        if maps is None:
            assert info["blocks"] == 37


@pytest.mark.gpu
@pytest.mark.parametrize("m", [65, 256 * 3 + 1])
def test_gpu_row_slices_one_block_and_a_one_row_tail(need_gpu, m):
    """65 rows: one block, two wave tasks; 256 k + 1 rows: a last block of one row."""
    A = short_banded(m)
    info = check_case(A, None, kernel="stream", options=SLICES)
    assert info["row_slices"] == 1 and info["blocks"] == (m + 255) // 256


@pytest.mark.gpu
def test_gpu_stream_x_windows_and_forced_dictionaries(need_gpu):
    B = gen.banded(5000, per_row=10, half=32, seed=5)
    info = check_case(B, None, kernel="stream", options={"x_dict": -1})
    assert info["x_windows"] == 1 and info["x_dict"] == 0
    A = gen.stencil27(21)
    info = check_case(A, None, kernel="stream", options={"x_dict": 1, "row_slices": -1})
    assert info["x_dict"] == 1 and info["row_slices"] == 0
    for chunk in (2, 4):  # an explicit XCD chunk: full spans remapped, the tail kept, all mirrored
        info = check_case(A, None, kernel="stream", xcd_chunk=chunk, options={"x_dict": 1, "row_slices": -1})
        assert info["xcd_remap"] == chunk


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["aligned", "packed", "ssr"])
def test_gpu_csr3_plans(need_gpu, plan):
    A = gen.stencil27(21)
    maps = hspmv.build_csr3_maps(A, 20, 10)
    info = check_case(A, maps, kernel="csr3", options={"csr3_plan": plan, "row_slices": -1})
    assert info["kernel_name"] == "csr3" and info["csr3_plan"] == _lib.CSR3_PLANS[plan]


@pytest.mark.gpu
def test_gpu_two_shards_on_one_device(need_gpu):
    A = gen.stencil27(21)
    info = check_case(A, None, devices=[0, 0], kernel="stream")
    assert info["num_gpus"] == 2


@pytest.mark.gpu
def test_gpu_x_slab_passes(need_gpu):
    """Forced alternate mirrors each pass's blocks; the passes keep their order
    (each continues the rows from y), so the bits stay."""
    A = gen.powerlaw(20_000, seed=3, dtype=np.float64)
    info = check_case(A, None, kernel="stream", options={"x_slabs": 3})
    assert info["x_slabs"] > 1


@pytest.mark.gpu
def test_gpu_small_row_counts_and_other_kernels(need_gpu):
    for m in (63, 64, 65):
        A = ragged_rows(m)
        check_case(A, None, kernel="stream")
        check_case(A, hspmv.build_csr3_maps(A, 3, 2), kernel="csr3")
    # m = 0: nothing launches, nothing alternates
    E = CsrMatrix(0, 7, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64))
    check_case(E, None, want_sweep=(0, 0))
    # the vector and column-sorted kernels stay forward whatever the mode
    A = ragged_rows(300)
    check_case(A, None, want_sweep=(0, 0), kernel="vector")


@pytest.mark.gpu
def test_gpu_auto_stays_forward_on_resident_matrices_and_modes_switch(need_gpu):
    A = gen.stencil27(21)
    x = gen.rand_x(A.n, 42)
    _, info = four_calls(A, None, x, None, kernel="stream")
    assert info["sweep"] == 0  # fits the Infinity Cache: served from it in either direction
    with hspmv.SpMV(A, device=0, kernel="stream") as op:
        y0 = op(x)
        for mode, want in (("alternate", 1), ("forward", 0), ("auto", 0), ("alternate", 1)):
            op.set_sweep(mode)
            assert op.info["sweep"] == want
            op.spmv()
            assert np.array_equal(op.get_y(), y0)
        with pytest.raises(ValueError):
            op.set_sweep("backward")
        assert hspmv.lib().hspmv_set_sweep(op._h, 3) == -1 and b"sweep" in hspmv.lib().hspmv_last_error()
        assert op.info["sweep"] == 1  # a refused mode changes nothing


@pytest.mark.gpu
def test_gpu_run_leaves_the_same_y_after_odd_and_even_counts(need_gpu):
    A = gen.stencil27(21)
    x = gen.rand_x(A.n, 42)
    with hspmv.SpMV(A, device=0, kernel="stream", options=SLICES) as op:
        op.set_sweep("alternate")
        y0 = op(x)
        for warmup, iters in ((0, 3), (1, 4), (2, 2), (0, 1)):
            poison_y(op, A, [0, A.m])
            t = op.run(warmup=warmup, iters=iters)
            assert t["iters"] == iters
            assert op.get_y().tobytes() == y0.tobytes(), (warmup, iters)


# ------------------------------------------------------------------ CLIs

def run_cli(*args):
    import subprocess
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_cli_rejects_an_unknown_sweep_before_reading_anything():
    build = _lib.PKG_ROOT / "build"
    for exe in ("spmv-csr", "spmv-csrk"):
        p = run_cli(build / exe, "/does/not/exist.csr", 3, "--sweep", "sideways")
        assert p.returncode == 1 and "bad --sweep sideways" in p.stderr and "Before Read" not in p.stdout
        p = run_cli(build / exe, "/does/not/exist.csr", 3, "--sweep")
        assert p.returncode == 1 and "missing value for --sweep" in p.stderr


@pytest.mark.gpu
def test_gpu_cli_sweep_option_keeps_the_report_and_y(need_gpu, tmp_path):
    from conftest import GOLDEN
    build = _lib.PKG_ROOT / "build"
    keys = None
    ys = []
    for extra in ([], ["--sweep", "forward"], ["--sweep", "alternate"]):
        out = tmp_path / f"y{len(ys)}.bin"
        p = run_cli(build / "spmv-csr", GOLDEN / "banded3000.csr", 4, "--x", "rand:42", "--kernel", "stream",
                    "--dump-y", out, *extra)
        assert p.returncode == 0 and "Check: PASS" in p.stdout and "Number Wrong: 0" in p.stdout, p.stdout + p.stderr
        k = [line.split(":")[0] for line in p.stdout.splitlines() if ":" in line]
        keys = keys or k
        assert k == keys  # the stdout contract: the same lines whatever the sweep
        ys.append(out.read_bytes())
    assert ys[0] == ys[1] == ys[2]
    p = run_cli(build / "spmv-csrk", GOLDEN / "banded3000.csr3", 3, "--x", "rand:42", "--sweep", "alternate")
    assert p.returncode == 0 and "Check: PASS" in p.stdout, p.stdout + p.stderr
