"""Row slices with 12-bit dictionary positions (hspmv_slices_pack,
slice_kernel.cuh hspmv_slices<.., PB = 12>).

Host: the packed stream unpacks, in numpy, to hspmv_slices_plan's 16-bit
positions for every slice width; the bit width follows the largest
dictionary; the flagship model's byte count.

GPU: y of a handle that runs the packed stream equals, byte for byte, y of
the same options with ``row_slices = -1`` (the chunked dictionary kernel).
"""
import numpy as np
import pytest

import hspmv
from hspmv import gen
from hspmv.api import CsrMatrix

F64_SERIAL, F32_SERIAL = 40, 56  # hspmv_internal.h kSerialMax / kSerialMaxF32
ON = {"x_dict": 1, "row_slices": 1}
OFF = {"x_dict": 1, "row_slices": -1}
DTYPES = [np.float64, np.float32]


def bound_of(dtype):
    return F64_SERIAL if dtype == np.float64 else F32_SERIAL


# ------------------------------------------------------------------ the format in numpy

def units(w, bits):
    """128-byte units of a slice of width w in the position stream."""
    w = np.asarray(w, np.int64)
    return 6 * (w // 8) + w % 8 if bits == 12 else w


def slot16(w, k, i):
    """Element of slot k, lane i in the 16-bit layout of a slice of width w
    (hspmv_slices_plan: groups of 4 slots per lane, then single columns)."""
    return (k // 4) * 256 + i * 4 + k % 4 if k < w // 4 * 4 else k * 64 + i


def unpack(desc, P):
    """hspmv_slices_plan's ``pos`` (slot order, 16-bit) from slices_pack's
    output, by the documented layout."""
    desc = np.asarray(desc, np.int64)
    packed, prefix = P["packed"], P["pos_prefix"].astype(np.int64)
    if P["bits"] == 16:
        return packed.view("<u2").copy()
    assert P["bits"] == 12
    out = np.zeros(64 * desc[-1, 0], np.uint16)
    lane = np.arange(64)
    for s in range(len(desc) - 1):
        w, base, o = int(desc[s + 1, 0] - desc[s, 0]), 64 * int(desc[s, 0]), 128 * int(prefix[s])
        for g in range(w // 8):
            d = packed[o + 768 * g:o + 768 * (g + 1)].view("<u4").reshape(64, 3).astype(np.uint64)
            for e in range(8):
                word, sh = divmod(12 * e, 32)
                v = d[:, word] >> np.uint64(sh)
                if sh > 20:
                    v = v | (d[:, word + 1] << np.uint64(32 - sh))
                out[base + slot16(w, 8 * g + e, lane)] = (v & np.uint64(0xFFF)).astype(np.uint16)
        w8, t = w // 8 * 8, w % 8
        tail = packed[o + 96 * w8:o + 96 * w8 + 128 * t].view("<u2")
        for k in range(t):
            out[base + slot16(w, w8 + k, lane)] = tail[slot16(t, k, lane)]
    return out


def check_pack(desc, pos):
    """slices_pack's prefix table and stream against the formula and the
    plan's positions; returns the pack."""
    P = hspmv.slices_pack(desc, pos)
    w = np.diff(np.asarray(desc, np.int64)[:, 0])
    want = np.concatenate([[0], np.cumsum(units(w, P["bits"]))])
    assert np.array_equal(P["pos_prefix"], want)
    assert len(P["packed"]) == 128 * want[-1]
    assert np.array_equal(unpack(desc, P), np.asarray(pos)[:64 * int(np.asarray(desc)[-1, 0])])
    return P


# ------------------------------------------------------------------ matrices

def ragged_all_widths(dtype, seed=13):
    """64-row groups whose longest rows are 1 .. the dtype's serial bound (in
    a shuffled order), one whole group empty, some empty rows in every group,
    and a last group of 23 rows.  Row r holds columns r, r + 3, r + 6, ..."""
    rng = np.random.default_rng(seed)
    bound = bound_of(dtype)
    widths = list(rng.permutation(np.arange(1, bound + 1))) + [0, 11]
    lens = []
    for g, w in enumerate(widths):
        rows = 23 if g == len(widths) - 1 else 64
        l = rng.integers(0, w + 1, rows)
        l[rng.integers(0, rows)] = w
        lens.append(l)
    lens = np.concatenate(lens)
    lens[np.flatnonzero(lens)[5::37]] = 0
    for g, w in enumerate(widths):  # the group's longest row is still w
        lens[64 * g + (g % 20)] = w
    m = len(lens)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([r + 3 * np.arange(k) for r, k in enumerate(lens)]).astype(np.int32)
    val = rng.uniform(-1.0, 1.0, int(lens.sum())).astype(dtype)
    return CsrMatrix(m, int(m + 3 * bound + 1), rp, col, val)


def block_run(c, dtype=np.float32, extra_row=None):
    """512 rows, row r holds columns [c r, c r + c): each 256-row STREAM block
    stages one run of 256 c entries.  extra_row: that row holds c + 1 columns
    (one more entry in its block's dictionary)."""
    m = 512
    lens = np.full(m, c, np.int64)
    if extra_row is not None:
        lens[extra_row] += 1
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([c * r + np.arange(k) for r, k in enumerate(lens)]).astype(np.int32)
    val = np.random.default_rng(17 + c).uniform(-1.0, 1.0, int(lens.sum())).astype(dtype)
    return CsrMatrix(m, c * m + 1, rp, col, val)


# (matrix, options beside ON, largest position, bits): the three width-choice
# matrices, and fp64 dictionaries that only a raised cap allows
WIDTH_CASES = {
    "f32_4096": (lambda: block_run(16), {}, 4095, 12),
    "f32_4097": (lambda: block_run(16, extra_row=255), {}, 4096, 16),
    "f32_5120": (lambda: block_run(20), {}, 5119, 16),
    "f64_cap_4096": (lambda: block_run(16, np.float64), {"x_dict_cap": 40960}, 4095, 12),
    "f64_cap_4352": (lambda: block_run(17, np.float64), {"x_dict_cap": 40960}, 4351, 16),
}


def plan_of(name):
    make, extra, top, bits = WIDTH_CASES[name]
    A = make()
    S = hspmv.slices_plan(A, None, kernel="stream", options={**ON, **extra})
    # the matrix really produces that dictionary
    assert S["why"] == "ok" and int(S["pos"].max()) == top
    return A, S, extra, bits


# ------------------------------------------------------------------ host

@pytest.mark.parametrize("bound", [F64_SERIAL, F32_SERIAL])
def test_pack_unpack_every_width(bound):
    """Descriptors of every width 0 .. bound (an empty slice among them) and
    random positions below 4096, 0 and 4095 included; lanes past a slice's
    rows and slots past a row's end hold 0 as in a plan."""
    rng = np.random.default_rng(bound)
    widths = np.concatenate([rng.permutation(np.arange(0, bound + 1)), [8, 16, 27]])
    desc = np.zeros((len(widths) + 1, 2), np.int32)
    desc[1:, 0] = np.cumsum(widths)
    desc[1:, 1] = np.cumsum(np.where(np.arange(len(widths)) % 3 == 0, 40, 64))  # some short slices
    pos = rng.integers(0, 4096, 64 * int(desc[-1, 0])).astype(np.uint16)
    pos[rng.random(len(pos)) < 0.2] = 0
    pos[::7] = 4095
    for s, w in enumerate(widths):  # padding lanes of the short slices
        if s % 3 == 0:
            for k in range(w):
                pos[64 * int(desc[s, 0]) + slot16(int(w), k, np.arange(40, 64))] = 0
    P = check_pack(desc, pos)
    assert P["bits"] == 12 and pos.max() == 4095 and pos.min() == 0
    # one position past 12 bits: the 16-bit stream, the plan's bytes
    pos[5] = 4096
    P = check_pack(desc, pos)
    assert P["bits"] == 16 and P["packed"].tobytes() == pos.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_pack_unpack_ragged_plan(dtype):
    """A plan whose slices take every width 1 .. the serial bound, with
    empty rows, an empty slice and a short last slice."""
    A = ragged_all_widths(dtype)
    S = hspmv.slices_plan(A, None, kernel="stream", options=ON)
    assert S["why"] == "ok"
    w = np.diff(S["desc"][:, 0].astype(np.int64))
    assert set(range(0, bound_of(dtype) + 1)) <= set(w.tolist())
    assert S["desc"][-1, 1] - S["desc"][-2, 1] == 23 and (np.diff(A.row_ptr) == 0).sum() > 64
    assert check_pack(S["desc"], S["pos"])["bits"] == 12
    maps = hspmv.build_csr3_maps(A, 20, 10)
    S3 = hspmv.slices_plan(A, maps, options=ON)
    assert S3["why"] == "ok"
    assert check_pack(S3["desc"], S3["pos"])["bits"] == 12


def test_pack_keeps_16_bits_when_nothing_shrinks():
    """Slices under 8 slots wide hold no 12-bit group: the packed stream
    would be the plan's bytes plus a table, so the handle keeps 16 bits."""
    A = gen.laplace2d(60, 40)
    S = hspmv.slices_plan(A, None, kernel="stream", options=ON)
    assert S["why"] == "ok" and np.diff(S["desc"][:, 0]).max() == 5
    assert check_pack(S["desc"], S["pos"])["bits"] == 16


@pytest.mark.parametrize("name", sorted(WIDTH_CASES))
def test_width_choice(name):
    """12 bits up to 4096 dictionary entries (largest position 4095), 16 from
    4097 on; fp32's default cap (5120 entries) and a raised fp64 cap reach both."""
    A, S, _, bits = plan_of(name)
    assert check_pack(S["desc"], S["pos"])["bits"] == bits


def test_flagship_model_bytes():
    """C3 (27-point 125^3 RCM stencil): 12 bits, and the packed positions
    take 81,379,328 bytes against 104,630,016 at 16 bits (-22.2 %)."""
    A = gen.stencil27(125)
    maps = hspmv.build_csr3_maps(A, *hspmv.csr3_params(A.nnz / A.m, "volta"))
    S = hspmv.slices_plan(A, maps)
    assert S["why"] == "ok" and S["padded_entries"] == 52315008
    P = hspmv.slices_pack(S["desc"], S["pos"])
    assert P["bits"] == 12
    w = np.diff(S["desc"][:, 0].astype(np.int64))
    assert len(P["packed"]) == 128 * int(units(w, 12).sum()) == 128 * int(P["pos_prefix"][-1])
    assert len(P["packed"]) <= 0.8 * 2 * S["padded_entries"]
    assert len(P["packed"]) == 81379328


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def need_gpu():
    assert hspmv.device_count() >= 1, "no HIP device visible: the gpu tests must run on the MI355X box"


def run_pair(A, maps, kernel, x, bits, extra=None):
    """y with row slices (``bits``-bit positions) and y of the chunked
    kernel, same options otherwise: the same bytes."""
    with hspmv.SpMV(A, maps, kernel=kernel, device=0, options={**ON, **(extra or {})}) as op:
        y1, i1 = op(x), op.info
    with hspmv.SpMV(A, maps, kernel=kernel, device=0, options={**OFF, **(extra or {})}) as op:
        y0, i0 = op(x), op.info
    assert i1["row_slices"] == 1 and i0["row_slices"] == 0
    assert i1["slice_pos_bits"] == bits and i0["slice_pos_bits"] == 0
    assert i1["x_dict"] == 1 and i0["x_dict"] == 1 and i1["kernel_name"] == i0["kernel_name"]
    assert y1.tobytes() == y0.tobytes()
    return y1, i1


def paths(A):
    return {"csr3": (hspmv.build_csr3_maps(A, 20, 10), "auto"), "stream": (None, "stream")}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(WIDTH_CASES))
def test_gpu_width_choice(need_gpu, name):
    """Positions up to 4095 in 12 bits (every bit of a field in use), and the
    16-bit stream from 4097 entries on, the raised fp64 cap included."""
    A, S, extra, bits = plan_of(name)
    x = gen.rand_x(A.n, 21).astype(A.val.dtype)
    run_pair(A, None, "stream", x, bits, extra)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["csr3", "stream"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_every_width(need_gpu, dtype, which):
    """Every slice width 1 .. the serial bound, a short last slice, empty
    rows and an empty slice; x is rand_x, so every staged entry is distinct."""
    A = ragged_all_widths(dtype)
    maps, kernel = paths(A)[which]
    y, _ = run_pair(A, maps, kernel, gen.rand_x(A.n, 23).astype(dtype), 12)
    assert not y[np.diff(A.row_ptr) == 0].any()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["csr3", "stream"])
def test_gpu_stencil21_format_bytes(need_gpu, which):
    """stencil27(21) fp64: 12 bits, and format_bytes below the 16-bit
    format's (the parent's formula: 2 bytes per padded position)."""
    A = gen.stencil27(21)
    maps, kernel = paths(A)[which]
    _, info = run_pair(A, maps, kernel, gen.rand_x(A.n, 42), 12)
    S = hspmv.slices_plan(A, maps, kernel=kernel, options=ON)
    P = hspmv.slices_pack(S["desc"], S["pos"])
    nd = S["n_desc"]
    saved = 2 * S["padded_entries"] - (len(P["packed"]) + 4 * (nd + 1))
    assert saved > 0
    # the 16-bit format: alg_bytes less the CSR-order streams and row pointers,
    # plus the slices' values and 2-byte positions, lengths and descriptors,
    # the dictionaries' tables and the x entries staged more than once
    _, runs, _ = hspmv.xdict_plan(A, maps, kernel=kernel, options=ON)
    parent = (info["alg_bytes"] - (A.nnz * 12 + 4 * (A.m + 1)) +
              (S["padded_entries"] * 10 + A.m + 8 * (nd + 1)) + 8 * len(runs) + 4 * info["blocks"] +
              8 * (info["x_dict_entries"] - info["x_entries"]))
    assert info["format_bytes"] == pytest.approx(parent - saved, abs=1.0)
    assert info["format_bytes"] < parent
