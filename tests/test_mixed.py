"""Mixed-precision handles: the matrix values stored and streamed as fp32, x, y,
the products and the sums fp64 (hspmv_create_mixed, include/hspmv.h).

Throughout A32 is a float32 matrix and A64 = A32.astype(float64), its exact
widening.  Host: hspmv_values_fit_f32, the refusals hspmv_create_mixed makes
before any device call, the row-slice plan of a mixed handle (hspmv_slices_plan_vec:
descriptors, lengths and positions of the fp64 plan, fp32 values in groups of
four slots) and the ABI.  GPU: y of the mixed handle equals, byte for byte, y
of the fp64 handle on A64 with the same options on every row of at most 40
nonzeros -- a wrong stride, group width or widening shows as wrong bits -- and
is within the fp64 bar of the oracle on the longer ones.
"""
import ctypes
import subprocess

import numpy as np
import pytest

import hspmv
from hspmv import _lib, gen
from hspmv.api import CsrMatrix

F64_SERIAL = 40  # hspmv_internal.h kSerialMax: a mixed handle's serial bound too
E_INVALID = -1
ON = {"x_dict": 1, "row_slices": 1}
OFF = {"x_dict": 1, "row_slices": -1}
NODICT = {"x_dict": -1}


# ------------------------------------------------------------------ matrices
# (the builders of tests/test_row_slices.py, float32 by default)

def fixed_rows(L, m=200, dtype=np.float32, seed=3):
    """m rows of exactly L nonzeros, columns r .. r + L - 1 (3 full slices and
    one of 8 rows)."""
    rng = np.random.default_rng(seed + L)
    rp = (np.arange(m + 1, dtype=np.int64) * L).astype(np.int32)
    col = (np.arange(m)[:, None] + np.arange(L)[None, :]).astype(np.int32).ravel()
    val = rng.uniform(-1.0, 1.0, m * L).astype(dtype)
    return CsrMatrix(m, m + L, rp, col, val)


def ragged(lens, dtype=np.float32, seed=5, n=None):
    """Row r has lens[r] nonzeros in columns r, r + 2, r + 4, ..."""
    lens = np.asarray(lens, np.int64)
    m = len(lens)
    rng = np.random.default_rng(seed)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([r + 2 * np.arange(k) for r, k in enumerate(lens)] + [np.zeros(0, np.int64)])
    n = n or int(m + 2 * lens.max() + 1)
    val = rng.uniform(-1.0, 1.0, int(lens.sum())).astype(dtype)
    return CsrMatrix(m, n, rp, col.astype(np.int32), val)


def with_empty_rows(dtype=np.float32):
    """320 rows of 3 nonzeros, two rows of every slice empty and rows 64..127
    (one whole slice, w = 0) empty."""
    lens = np.full(320, 3)
    lens[5::32] = 0
    lens[64:128] = 0
    return ragged(lens, dtype)


def one_long_row_per_slice(dtype=np.float32):
    """Short rows with one 40-nonzero row in each slice."""
    lens = np.full(256, 2)
    lens[::64] = 40
    return ragged(lens, dtype)


def block_run(c, dtype=np.float32):
    """512 rows, row r holds columns [c r, c r + c): each 256-row STREAM block
    stages one run of 256 c entries (tests/test_slice_pos12.py)."""
    m = 512
    rp = (np.arange(m + 1, dtype=np.int64) * c).astype(np.int32)
    col = (c * np.arange(m)[:, None] + np.arange(c)[None, :]).astype(np.int32).ravel()
    val = np.random.default_rng(17 + c).uniform(-1.0, 1.0, m * c).astype(dtype)
    return CsrMatrix(m, c * m + 1, rp, col, val)


def wide_random(m, n, per_row, seed):
    rng = np.random.default_rng(seed)
    cols = np.sort(rng.choice(n, size=(m, per_row), replace=True), axis=1)
    rp = np.arange(0, m * per_row + 1, per_row, dtype=np.int32)
    val = rng.uniform(-1, 1, m * per_row).astype(np.float32)
    return CsrMatrix(m, n, rp, cols.reshape(-1).astype(np.int32), val)


def paths(A):
    """(maps, kernel) of the two dictionary shapes: CSR3 tasks and STREAM."""
    return {"csr3": (hspmv.build_csr3_maps(A, 20, 10), "auto"), "stream": (None, "stream")}


SMALL = {
    "stencil21": lambda: gen.stencil27(21, dtype=np.float32),
    "laplace": lambda: gen.laplace2d(300, 200).astype(np.float32),
    "banded": lambda: gen.banded(30000, per_row=10, half=32).astype(np.float32),
    "empty_rows": with_empty_rows,
}
WIDTHS = list(range(1, 9)) + [39, 40]


# ------------------------------------------------------------------ host: values_fit_f32

def fit(a, dtype_code=None):
    a = np.ascontiguousarray(a)
    bad = ctypes.c_int64(-5)
    code = hspmv.api.dtype_code(a.dtype) if dtype_code is None else dtype_code
    rc = hspmv.lib().hspmv_values_fit_f32(a.ctypes.data, len(a), code, ctypes.byref(bad))
    return rc, bad.value


def test_values_fit_f32_accepts_what_round_trips():
    rng = np.random.default_rng(1)
    f = rng.uniform(-1, 1, 1000).astype(np.float32)
    assert fit(f) == (1, -5)  # an fp32 array fits trivially; first_bad untouched
    assert fit(f.astype(np.float64)) == (1, -5)
    edge = np.array([0.0, -0.0, np.inf, -np.inf, np.finfo(np.float32).max, np.finfo(np.float32).tiny,
                     2.0 ** -149, -(2.0 ** -149), np.nan], np.float64)
    assert np.array_equal(edge.astype(np.float32).astype(np.float64).view(np.uint64), edge.view(np.uint64))
    assert fit(edge) == (1, -5)
    assert fit(np.zeros(0, np.float64)) == (1, -5)
    assert hspmv.lib().hspmv_values_fit_f32(None, 0, _lib.F64, None) == 1
    assert CsrMatrix(2, 2, [0, 1, 2], [0, 1], np.array([0.5, -3.0])).fits_float32()
    assert hspmv.values_fit_float32(f) == (True, None)


@pytest.mark.parametrize("name, value", [
    ("rounds", 0.1),
    ("above_flt_max", 2.0 * float(np.finfo(np.float32).max)),
    ("double_subnormal_flushes", 1e-310),
    ("f32_subnormal_loses_bits", float(np.ldexp(1.0 + 2.0 ** -20, -140))),
    ("nan_payload", float(np.array([0x7FF8000000000001], np.uint64).view(np.float64)[0])),
])
def test_values_fit_f32_first_bad(name, value):
    good = np.array([1.0, -2.5, 0.0, 2.0 ** -130, np.inf, 3.0], np.float64)
    for at in (0, 3, len(good)):
        v = np.insert(good, at, value)
        assert v[at].tobytes() == np.float64(value).tobytes()
        assert fit(v) == (0, at), (name, at)
        assert hspmv.lib().hspmv_values_fit_f32(v.ctypes.data, len(v), _lib.F64, None) == 0
        assert hspmv.values_fit_float32(v) == (False, at)
    two = np.insert(np.insert(good, 4, value), 2, value)
    assert fit(two) == (0, 2)  # the first one
    assert not CsrMatrix(1, 7, [0, 7], np.arange(7), np.insert(good, 1, value)).fits_float32()


def test_values_fit_f32_bad_arguments():
    L = hspmv.lib()
    d = np.ones(4)
    bad = ctypes.c_int64()
    assert L.hspmv_values_fit_f32(None, 4, _lib.F64, ctypes.byref(bad)) == E_INVALID
    assert L.hspmv_values_fit_f32(d.ctypes.data, -1, _lib.F64, ctypes.byref(bad)) == E_INVALID
    assert L.hspmv_values_fit_f32(d.ctypes.data, 4, 7, ctypes.byref(bad)) == E_INVALID
    assert _lib.last_error()


# ------------------------------------------------------------------ host: refusals before any device call

def test_create_mixed_refusals_need_no_device():
    L = hspmv.lib()
    A32 = fixed_rows(3, m=10)
    A64 = A32.astype(np.float64)
    c32, c64 = A32.c_struct(), A64.c_struct()
    h = ctypes.c_void_p()

    def refused(cs, opt, vdt, hp=h):
        rc = L.hspmv_create_mixed(ctypes.byref(hp) if hp is not None else None,
                                  ctypes.byref(cs) if cs is not None else None, None,
                                  ctypes.byref(opt) if opt is not None else None, vdt)
        return rc == E_INVALID and _lib.last_error() != "" and not h.value

    plain = _lib.make_options(0, None)
    assert refused(c32, plain, _lib.F64, hp=None)  # NULL handle pointer
    assert refused(None, plain, _lib.F64)          # NULL matrix
    assert refused(c64, plain, _lib.F32)           # fp64 values with fp32 vectors
    assert "fp64 values with fp32 vectors" in _lib.last_error()
    assert refused(c32, plain, 7)
    assert refused(c32, None, 7)
    two = _lib.make_options(0, None, devices=[0, 0])
    assert two.n_devices == 2 and refused(c32, two, _lib.F64)
    n2 = _lib.make_options(0, None)
    n2.n_devices = 2
    assert refused(c32, n2, _lib.F64)
    assert refused(c32, _lib.make_options(_lib.KERNEL_CSORT, None), _lib.F64)
    assert "column-sorted" in _lib.last_error()
    assert refused(c32, _lib.make_options(0, {"csort": 1}), _lib.F64)
    assert L.hspmv_get_dtypes(None, None, None) == E_INVALID
    with pytest.raises(hspmv.HspmvError, match="E_INVALID"):
        hspmv.SpMV(A64, vector_dtype=np.float32)
    with pytest.raises(hspmv.HspmvError, match="E_INVALID"):
        hspmv.SpMV(A32, vector_dtype=np.float64, devices=[0, 0])
    with pytest.raises(hspmv.HspmvError, match="E_INVALID"):
        hspmv.SpMV(A32, vector_dtype=np.float64, kernel="csort")


# ------------------------------------------------------------------ host: the slice plan

def check_mixed_plan(A32, maps, kernel, options=ON):
    """desc / len / pos of the widened fp64 plan; val float32, every nonzero's
    fp32 bits at its slot in value groups of 4 (the index formula of
    tests/test_row_slices.py rebuild_and_compare with G = 4), zero elsewhere."""
    S = hspmv.slices_plan(A32, maps, kernel=kernel, options=options, vector_dtype=np.float64)
    D = hspmv.slices_plan(A32.astype(np.float64), maps, kernel=kernel, options=options)
    assert S["why"] == "ok" and D["why"] == "ok"
    for k in ("n_desc", "n_slices", "padded_entries"):
        assert S[k] == D[k], k
    for k in ("desc", "len", "pos"):
        assert np.array_equal(S[k], D[k]), k
    assert S["val"].dtype == np.float32 and len(S["val"]) == S["padded_entries"]
    desc, G = S["desc"].astype(np.int64), 4
    lens = np.diff(A32.row_ptr).astype(np.int64)
    r = np.repeat(np.arange(A32.m, dtype=np.int64), lens)
    k = np.arange(A32.nnz, dtype=np.int64) - np.repeat(A32.row_ptr[:-1].astype(np.int64), lens)
    s = np.searchsorted(desc[:-1, 1], np.arange(A32.m), side="right") - 1
    width = np.diff(desc[:, 0])
    sn, i, w = s[r], r - desc[s[r], 1], width[s[r]]
    base = 64 * desc[sn, 0]
    wg = w // G * G
    ev = np.where(k < wg, base + (k // G) * 64 * G + i * G + k % G, base + k * 64 + i)
    assert np.array_equal(S["val"][ev].view(np.uint32), A32.val.view(np.uint32))
    hit = np.zeros(len(S["val"]), bool)
    hit[ev] = True
    assert not S["val"][~hit].view(np.uint32).any()
    return S


@pytest.mark.parametrize("name", sorted(SMALL))
def test_mixed_slices_plan_holds_the_matrix(name):
    A = SMALL[name]()
    for maps, kernel in paths(A).values():
        check_mixed_plan(A, maps, kernel)


def test_mixed_slices_plan_every_width_remainder():
    for L in WIDTHS:
        A = fixed_rows(L)
        for maps, kernel in paths(A).values():
            S = check_mixed_plan(A, maps, kernel)
            assert S["padded_entries"] == 64 * L * S["n_slices"]


def test_mixed_slices_eligibility():
    def why(M, mp=None, kernel="auto", vdt=np.float64, **o):
        return hspmv.slices_plan(M, mp, kernel=kernel, options=o or None, fill=False, vector_dtype=vdt)["why"]

    # fp64's serial bound, although fp32 alone allows 56
    lens = np.full(130, 3)
    lens[70] = F64_SERIAL
    assert why(ragged(lens), None, kernel="stream", row_slices=1) == "ok"
    lens[70] = F64_SERIAL + 1
    assert why(ragged(lens), None, kernel="stream", row_slices=1) == "long_row"
    assert why(ragged(lens), None, kernel="stream", vdt=None, row_slices=1) == "ok"  # the fp32 handle: 56
    # the byte rule with 4-byte values, the residence rule with the mixed footprint
    B = one_long_row_per_slice()
    assert why(B, None, kernel="stream", x_dict=1) == "bytes"
    assert why(B, hspmv.build_csr3_maps(B, 20, 10), x_dict=1) == "bytes"
    assert why(B, None, kernel="stream", row_slices=1) == "ok"
    assert why(gen.laplace2d(300, 200).astype(np.float32), None, kernel="stream", x_dict=1) == "resident"
    # equal dtypes: hspmv_slices_plan's own answer, arrays included
    for M in (B, B.astype(np.float64), gen.stencil27(21, dtype=np.float32)):
        for o in (ON, {"x_dict": 1}, None):
            a = hspmv.slices_plan(M, None, kernel="stream", options=o, vector_dtype=M.val.dtype)
            b = hspmv.slices_plan(M, None, kernel="stream", options=o)
            assert a.keys() == b.keys()
            for k in a:
                assert np.array_equal(a[k], b[k]), k
    with pytest.raises(hspmv.HspmvError, match="E_INVALID"):
        hspmv.slices_plan(B.astype(np.float64), None, kernel="stream", vector_dtype=np.float32)


# ------------------------------------------------------------------ host: ABI

def test_mixed_abi_functions_only(tmp_path):
    """The four entry points are declared, bound and exported; hspmv_options
    and hspmv_info are what they were (the feature enters through functions)."""
    names = {"hspmv_create_mixed", "hspmv_get_dtypes", "hspmv_values_fit_f32", "hspmv_slices_plan_vec"}
    assert names <= set(_lib.SIGNATURES)
    L = hspmv.lib()
    for n in names:
        assert getattr(L, n) is not None
    assert ctypes.sizeof(_lib.Options) == 88 and ctypes.sizeof(_lib.Info) == 304
    assert _lib.Options._fields_[-1][0] == "row_slices" and _lib.Info._fields_[-1][0] == "reserved1"
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "hspmv.h"\nint main(void) {\n'
                   '  printf("%zu %zu\\n", sizeof(hspmv_options), sizeof(hspmv_info));\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", str(_lib.HEADER.parent), str(src), "-o", str(exe)], check=True)
    so, si = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert (int(so), int(si)) == (ctypes.sizeof(_lib.Options), ctypes.sizeof(_lib.Info))
    text = _lib.HEADER.read_text()
    assert "#define HSPMV_VERSION_MINOR 1" in text and "hspmv_create_mixed" in text.split("Also in 1.1")[1][:900]


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def need_gpu():
    assert hspmv.device_count() >= 1, "no HIP device visible: the gpu tests must run on the MI355X box"


SAME_INFO = ("kernel_name", "x_dict", "row_slices", "slice_pos_bits", "col16", "col16_group", "x_slabs",
             "n_split_rows", "chunk_u", "waves_per_block", "blocks", "x_windows", "groups_per_wave", "lds_pad",
             "wave_tasks", "csr3_plan", "serial_order", "x_entries", "x_dict_entries")


def run_both(A32, maps, x, exact="short", **kw):
    """y and info of the mixed handle, checked against the fp64 handle on the
    widened matrix (same options: the same plan, and the same bytes on rows of
    at most 40 nonzeros) and against the oracle (check_fp64)."""
    from test_gpu_parity import check_fp64
    A64 = A32.astype(np.float64)
    with hspmv.SpMV(A32, maps, vector_dtype=np.float64, **kw) as op:
        assert op.value_dtype == np.float32 and op.dtype == np.float64
        assert op.dtypes() == (np.dtype(np.float32), np.dtype(np.float64))
        ym, im = op(x), op.info
    with hspmv.SpMV(A64, maps, **kw) as op:
        assert op.dtypes() == (np.dtype(np.float64), np.dtype(np.float64))
        yd, idd = op(x), op.info
    assert ym.dtype == np.float64 and ym.shape == (A32.m,)
    for k in SAME_INFO:
        assert im[k] == idd[k], (k, im[k], idd[k])
    short = np.diff(A32.row_ptr) <= F64_SERIAL
    if exact == "short":
        assert ym[short].tobytes() == yd[short].tobytes()
        check_fp64(A32, x, ym, exact_rows=short)
    elif exact == "all":
        assert ym.tobytes() == yd.tobytes()
        check_fp64(A32, x, ym, exact_rows=slice(None))
    else:  # tolerance only (VECTOR: fma, lanes stride the row)
        check_fp64(A32, x, ym)
    # the byte model: 4 bytes less per stored value than the fp64 handle
    assert im["alg_bytes"] == idd["alg_bytes"] - 4.0 * A32.nnz
    want = A32.nnz * 8 + (A32.m + 1) * 4 + (im["x_entries"] + A32.m) * 8
    if maps is not None:
        want += (maps.n_ssr + 1 + maps.n_sr + 1) * 4
    assert im["alg_bytes"] == want
    return ym, im, idd


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["csr3", "stream"])
@pytest.mark.parametrize("name", ["stencil21", "banded", "empty_rows"])
def test_gpu_mixed_slices(need_gpu, name, which):
    A = SMALL[name]()
    maps, kernel = paths(A)[which]
    y, im, idd = run_both(A, maps, gen.rand_x(A.n, 42), kernel=kernel, device=0, options=ON)
    assert im["row_slices"] == 1 and im["x_dict"] == 1 and im["kernel_name"] == which
    # format and device bytes count 4-byte values: padded slots here, every slot 4 bytes less
    S = hspmv.slices_plan(A, maps, kernel=kernel, options=ON, fill=False, vector_dtype=np.float64)
    assert im["format_bytes"] == idd["format_bytes"] - 4.0 * S["padded_entries"]
    assert im["device_bytes"] == idd["device_bytes"] - 4 * max(S["padded_entries"], 1)
    if name == "empty_rows":
        assert not y[np.diff(A.row_ptr) == 0].any()
    if name == "stencil21":
        assert im["slice_pos_bits"] == 12


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["csr3", "stream"])
def test_gpu_mixed_slices_every_width_remainder(need_gpu, which):
    """Row lengths 1..8, 39, 40: every remainder of the 4-slot value groups and
    of the 4- and 8-slot position groups."""
    for L in WIDTHS:
        A = fixed_rows(L)
        maps, kernel = paths(A)[which]
        _, im, _ = run_both(A, maps, gen.rand_x(A.n, 7), exact="all", kernel=kernel, device=0, options=ON)
        assert im["row_slices"] == 1, L


@pytest.mark.gpu
def test_gpu_mixed_slices_16_bit_positions(need_gpu):
    """A dictionary of 4352 entries (a raised cap, counted in 8-byte x entries):
    16-bit positions; stencil27(21) above packs to 12."""
    A = block_run(17)
    opts = {**ON, "x_dict_cap": 40960}
    S = hspmv.slices_plan(A, None, kernel="stream", options=opts, vector_dtype=np.float64)
    assert S["why"] == "ok" and int(S["pos"].max()) == 4351
    _, im, _ = run_both(A, None, gen.rand_x(A.n, 21), exact="all", kernel="stream", device=0, options=opts)
    assert im["row_slices"] == 1 and im["slice_pos_bits"] == 16
    # fp32's own cap (20 KiB of 4-byte entries) would take 5120 entries; the mixed handle's is fp64's 2560
    assert hspmv.slices_plan(A, None, kernel="stream", options=ON, vector_dtype=np.float64)["why"] == "no_dict"
    assert hspmv.slices_plan(A, None, kernel="stream", options=ON)["why"] == "ok"


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["csr3", "stream"])
@pytest.mark.parametrize("opts", [OFF, NODICT], ids=["chunked_dict", "no_dict"])
def test_gpu_mixed_chunked_kernels(need_gpu, which, opts):
    for A in (SMALL["stencil21"](), fixed_rows(5), fixed_rows(40)):
        maps, kernel = paths(A)[which]
        _, im, _ = run_both(A, maps, gen.rand_x(A.n, 3), kernel=kernel, device=0, options=opts)
        assert im["row_slices"] == 0 and im["x_dict"] == (1 if opts is OFF else 0)
        assert im["kernel_name"] == which


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["aligned", "packed", "ssr"])
def test_gpu_mixed_csr3_plans(need_gpu, plan):
    A = SMALL["stencil21"]()
    maps = hspmv.build_csr3_maps(A, 20, 10)
    for extra in ({}, {"x_dict": 1}, {"x_dict": -1}):
        _, im, _ = run_both(A, maps, gen.rand_x(A.n, 5), kernel="csr3", device=0,
                            options={"csr3_plan": plan, **extra})
        assert im["kernel_name"] == "csr3" and hspmv.api._lib.CSR3_PLAN_NAMES[im["csr3_plan"]] == plan


STREAM_VARIANTS = {
    "waves1": dict(options={"stream_waves": 1}), "waves2": dict(options={"stream_waves": 2}),
    "waves4": dict(options={"stream_waves": 4}),
    "groups2": dict(groups_per_wave=2),
    **{f"u{u}": dict(chunk_u=u) for u in (2, 3, 4, 5, 6, 8, 16)},
    "prefetch": dict(prefetch=True), "prefetch_u3": dict(prefetch=True, chunk_u=3),
    "nontemporal": dict(nontemporal=True),
    "col16_forced": dict(col16=True, options={"x_dict": -1, "col16_group": -1}), "col16_off": dict(col16=False),
    "col16_group": dict(options={"col16_group": 1, "x_dict": -1}),
    "xwin_off": dict(options={"x_windows": -1, "x_dict": -1}), "xwin_on": dict(options=NODICT),
}


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(STREAM_VARIANTS))
def test_gpu_mixed_stream_variants(need_gpu, variant):
    kw = STREAM_VARIANTS[variant]
    for A in (SMALL["stencil21"](), gen.banded(5000, per_row=10, half=32).astype(np.float32)):
        _, im, _ = run_both(A, None, gen.rand_x(A.n, 9), kernel="stream", device=0, **kw)
        assert im["kernel_name"] == "stream"
        if variant.startswith("waves"):
            assert im["waves_per_block"] == int(variant[-1])
        if variant == "groups2":
            assert im["groups_per_wave"] == 2
        if variant.startswith("u"):
            assert im["chunk_u"] == int(variant[1:])
        if variant == "col16_forced":
            assert im["col16"] >= 1 and im["col16_group"] == 0
        if variant == "col16_off":
            assert im["col16"] == 0 and im["x_dict"] == 0
        if variant == "col16_group":
            assert im["col16_group"] == 1
        if variant == "xwin_off":
            assert im["x_windows"] == 0
    if variant == "xwin_on":
        assert im["x_windows"] == 1  # the banded matrix


def cooperative_matrix():
    lens = np.full(300, 7)
    lens[[3, 64, 65, 130, 299]] = [41, 64, 100, 700, 41]
    lens[200:210] = [0, 1, 40, 39, 2, 33, 40, 0, 5, 12]
    return ragged(lens)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["csr3", "stream"])
def test_gpu_mixed_cooperative_rows(need_gpu, which):
    """Rows of 41, 64, 100 and 700 nonzeros among short ones: the long rows by
    tolerance (fixed trees), the short rows bitwise."""
    A = cooperative_matrix()
    maps, kernel = paths(A)[which]
    for opts in (None, NODICT, {"x_dict": 1}):
        run_both(A, maps, gen.rand_x(A.n, 15), kernel=kernel, device=0, options=opts)


def split_matrix():
    lens = np.full(302, 6)
    lens[100], lens[257] = 5000, 9000
    return ragged(lens, seed=8)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["csr3", "stream"])
def test_gpu_mixed_split_rows(need_gpu, which):
    from test_gpu_parity import check_fp64
    A = split_matrix()
    maps, kernel = paths(A)[which]
    x = gen.rand_x(A.n, 17)
    _, im, _ = run_both(A, maps, x, kernel=kernel, device=0)
    assert im["n_split_rows"] == 2
    _, im, _ = run_both(A, maps, x, kernel=kernel, device=0, split_rows=False)
    assert im["n_split_rows"] == 0
    # serial order: every row in omp_spmv's order, the split rows by hspmv_long_serial
    y, im, _ = run_both(A, maps, x, exact="all", kernel=kernel, device=0, options={"deterministic": 3})
    assert im["serial_order"] == 1 and im["n_split_rows"] == 2
    check_fp64(A, x, y, exact_rows=slice(None))
    y, im, _ = run_both(A, maps, x, exact="all", kernel=kernel, device=0, split_rows=False,
                        options={"deterministic": 3})
    assert im["serial_order"] == 1 and im["n_split_rows"] == 0
    # deterministic = 2 is accepted and runs the (reproducible) row kernels
    with hspmv.SpMV(A, maps, vector_dtype=np.float64, kernel=kernel, device=0,
                    options={"deterministic": 2}) as op:
        assert op.info["kernel_name"] == which and op.info["deterministic"] == 1
        check_fp64(A, x, op(x), exact_rows=np.diff(A.row_ptr) <= F64_SERIAL)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 2, 4, 8, 16, 32, 64])
def test_gpu_mixed_vector(need_gpu, lanes):
    for A in (cooperative_matrix(), split_matrix()):
        _, im, _ = run_both(A, None, gen.rand_x(A.n, 19), exact="tol", kernel="vector", lanes=lanes, device=0)
        assert im["kernel_name"] == "vector" and im["lanes"] == lanes


def slab_exact_rows(A, slabs):
    """tests/test_gpu_parity.py _slab_exact_rows: rows whose every x-slab
    segment has <= 40 nonzeros."""
    w = -(-A.n // slabs)
    rows = np.repeat(np.arange(A.m), np.diff(A.row_ptr))
    seg = np.zeros((A.m, slabs), np.int64)
    np.add.at(seg, (rows, A.col_idx.astype(np.int64) // w), 1)
    return (seg.max(axis=1, initial=0) <= F64_SERIAL) & (np.diff(A.row_ptr) <= 4096)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["csr3", "stream"])
def test_gpu_mixed_x_slabs(need_gpu, which):
    from test_gpu_parity import check_fp64
    A = wide_random(2000, 200_000, 12, 4)
    maps, kernel = paths(A)[which]
    x = gen.rand_x(A.n, 2)
    exact = slab_exact_rows(A, 3)
    assert exact.all()
    for kw in ({}, {"prefetch": True}, {"chunk_u": 2, "nontemporal": True}):
        with hspmv.SpMV(A, maps, vector_dtype=np.float64, kernel=kernel, device=0, options={"x_slabs": 3},
                        **kw) as op:
            y, im = op(x), op.info
        with hspmv.SpMV(A.astype(np.float64), maps, kernel=kernel, device=0, options={"x_slabs": 3}, **kw) as op:
            yd, idd = op(x), op.info
        assert im["x_slabs"] == 3 and idd["x_slabs"] == 3 and im["kernel_name"] == idd["kernel_name"]
        assert y[exact].tobytes() == yd[exact].tobytes()
        check_fp64(A, x, y, exact_rows=exact)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["csr3", "stream"])
@pytest.mark.parametrize("opts", [ON, OFF, NODICT], ids=["slices", "chunked_dict", "no_dict"])
def test_gpu_mixed_inf_and_nan(need_gpu, which, opts):
    """inf and NaN in x (placed as in test_gpu_slices_inf_and_nan_in_x: also at
    dictionary position 0, where every padded slot points) and an inf and a NaN
    among the fp32 values reach exactly the rows that reference them."""
    A = gen.stencil27(21, dtype=np.float32)
    maps, kernel = paths(A)[which]
    blk, runs, _ = hspmv.xdict_plan(A.astype(np.float64), maps, kernel=kernel, options=ON)
    x = gen.rand_x(A.n, 11)
    first = runs[blk[:-1], 0]
    assert np.all(runs[blk[:-1], 1] == 0)
    x[first[1]] = np.inf
    x[first[len(first) // 2]] = np.nan
    x[first[-1]] = -np.inf
    x[A.n // 3] = np.nan
    x[A.n // 3 + 5] = np.inf
    val = A.val.copy()
    kinf, knan = int(A.row_ptr[100]) + 2, int(A.row_ptr[5000]) + 7
    val[kinf], val[knan] = np.inf, np.nan
    B = CsrMatrix(A.m, A.n, A.row_ptr, A.col_idx, val)
    with hspmv.SpMV(B, maps, vector_dtype=np.float64, kernel=kernel, device=0, options=opts) as op:
        y, im = op(x), op.info
    with hspmv.SpMV(B.astype(np.float64), maps, kernel=kernel, device=0, options=opts) as op:
        yd = op(x)
    assert im["row_slices"] == (1 if opts is ON else 0)
    assert y.tobytes() == yd.tobytes()  # every row <= 27 nonzeros: the same bits, NaN payloads included
    bad = ~np.isfinite(x)
    touched = np.add.reduceat(bad[A.col_idx].astype(np.int64), A.row_ptr[:-1]) > 0
    touched[[100, 5000]] = True
    assert np.isfinite(y[~touched]).all() and not np.isfinite(y[touched]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("opts", [ON, NODICT], ids=["slices", "no_dict"])
def test_gpu_mixed_sweep_alternate(need_gpu, opts):
    A = gen.stencil27(21, dtype=np.float32)
    maps = hspmv.build_csr3_maps(A, 20, 10)
    x = gen.rand_x(A.n, 31)
    with hspmv.SpMV(A, maps, vector_dtype=np.float64, device=0, options=opts) as op:
        assert op.info["sweep"] == 0  # auto: resident
        y0 = op(x)
        op.set_sweep("alternate")
        assert op.info["sweep"] == 1
        ys = []
        for _ in range(4):
            op.spmv()
            ys.append(op.get_y())
    assert all(y.tobytes() == y0.tobytes() for y in ys)


@pytest.mark.gpu
def test_gpu_mixed_borrowed_device_arrays(need_gpu):
    """HSPMV_FLAG_DEVICE_PTRS: the borrowed val is float32, the bound x and y
    float64 (torch tensors here)."""
    import torch
    from test_gpu_parity import check_fp64
    A = gen.stencil27(21, dtype=np.float32)
    maps = hspmv.build_csr3_maps(A, 20, 10)
    x = gen.rand_x(A.n, 13)
    rp, ci, val = (torch.from_numpy(a).cuda() for a in (A.row_ptr, A.col_idx, A.val))
    assert val.dtype == torch.float32
    xd = torch.from_numpy(x).cuda()
    yd = torch.zeros(A.m, dtype=torch.float64, device="cuda")
    o, i = torch.from_numpy(maps.outer).cuda(), torch.from_numpy(maps.inner).cuda()
    cs = _lib.Csr(A.m, A.n, A.nnz, rp.data_ptr(), ci.data_ptr(), val.data_ptr(), _lib.F32)
    ms = _lib.Csr3Maps(maps.n_ssr, maps.n_sr, o.data_ptr(), i.data_ptr())
    short = np.diff(A.row_ptr) <= F64_SERIAL
    with hspmv.SpMV(A.astype(np.float64), maps, device=0, options=ON) as op:
        y64 = op(x)
    for mdev, kernel, opts in ((None, "stream", None), (ms, "csr3", None), (ms, "csr3", ON), (None, "stream", ON),
                               (None, "stream", {"x_slabs": 3}), (None, "vector", None)):
        yd.zero_()
        op = hspmv.SpMV.from_device(cs, mdev, A, device=0, kernel=kernel, options=opts, vector_dtype=np.float64)
        assert op.value_dtype == np.float32 and op.dtype == np.float64
        assert op.dtypes() == (np.dtype(np.float32), np.dtype(np.float64))
        info = op.info
        assert info["kernel_name"] == kernel
        if opts:
            assert all(info[k] == v for k, v in opts.items())
        op.bind_x_device(xd.data_ptr())
        op.bind_y_device(yd.data_ptr())
        op.spmv()
        op.synchronize()
        y = yd.cpu().numpy()
        op.close()
        check_fp64(A, x, y, exact_rows=short if kernel != "vector" else None)
        if kernel != "vector":
            assert y.tobytes() == y64.tobytes()


@pytest.mark.gpu
def test_gpu_mixed_refusals(need_gpu):
    A = fixed_rows(4)
    with pytest.raises(hspmv.HspmvError, match="E_INVALID"):
        hspmv.SpMV(A, vector_dtype=np.float64, devices=[0, 0])
    with pytest.raises(hspmv.HspmvError, match="E_INVALID"):
        hspmv.SpMV(A, vector_dtype=np.float64, kernel="csort")
    with pytest.raises(hspmv.HspmvError, match="E_INVALID"):
        hspmv.SpMV(A, vector_dtype=np.float64, options={"csort": 1})
    with hspmv.SpMV(A, vector_dtype=np.float64, devices=[0]) as op:  # one device is a mixed handle
        assert op.dtypes() == (np.dtype(np.float32), np.dtype(np.float64))
    with hspmv.SpMV(A, vector_dtype=np.float32) as op:  # equal dtypes: hspmv_create_ex
        assert op.dtypes() == (np.dtype(np.float32), np.dtype(np.float32))
        assert op(gen.rand_x(A.n, 1)).dtype == np.float32


@pytest.mark.gpu
def test_gpu_mixed_irregular_matrix_runs_row_kernels(need_gpu):
    """A matrix AUTO gives the column-sorted kernel in fp32: the mixed handle
    plans as under deterministic = 1, row kernels only."""
    from test_gpu_parity import check_fp64
    # (AUTO asks for a matrix that streams from HBM before it builds the
    # column-sorted blocks, so gen.powerlaw(20000) would stay on the row
    # kernels in fp32 too: 1.5 M rows of 16 random columns, 210 MB in fp32, is
    # about the smallest matrix that meets the precondition)
    A = wide_random(1_500_000, 1_500_000, 16, 12)
    assert A.val.dtype == np.float32
    x = gen.rand_x(A.n, 6)
    with hspmv.SpMV(A, device=0) as op:
        assert op.info["kernel_name"] == "csort"  # the precondition
    with hspmv.SpMV(A, vector_dtype=np.float64, device=0) as op:
        y, im = op(x), op.info
    with hspmv.SpMV(A.astype(np.float64), device=0, options={"deterministic": 1}) as op:
        yd, idd = op(x), op.info
    assert im["kernel_name"] in ("stream", "csr3") and im["csort_parts"] == 0 and im["deterministic"] == 1
    for k in SAME_INFO:
        assert im[k] == idd[k], k
    short = np.diff(A.row_ptr) <= F64_SERIAL
    assert y[short].tobytes() == yd[short].tobytes()
    check_fp64(A, x, y, exact_rows=short if im["x_slabs"] == 0 else None)
