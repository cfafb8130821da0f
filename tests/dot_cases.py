"""Matrices, the y model and the derived bound of tests/test_dot.py and
tests/test_dot_cli.py (hspmv_spmv_axpby_dot).

The generators, the scalar pairs and the byte model of y are those of
tests/test_axpby.py (copied: that file stays as it is).  The bound on a dot:
with t_i the double products of the stored y (each rounded once) and
ref = math.fsum(t), any order of double additions over the m terms lies within
gamma_m sum|t_i| of the exact sum, gamma_m <= (m + 2) 2^-53 for the m here,
and fsum's own result is the exact sum rounded once; (m + 4) 2^-53 sum|t_i|
covers both sides.  Nothing in it comes from what the GPU returns.
"""
import math

import numpy as np

import hspmv
from hspmv import gen
from hspmv.api import CsrMatrix

F64_SERIAL, F32_SERIAL = 40, 56  # hspmv_internal.h kSerialMax / kSerialMaxF32
E_INVALID, E_STATE = -1, -7
DOT_WY, DOT_YY = 1, 2

# (alpha, beta); the last one runs over a y0 that is all NaN
PAIRS = [(1.0, 0.0), (-1.0, 1.0), (0.5, -0.25), (0.0, 1.0), (2.0, 0.0)]
NAN_PAIR = (2.0, 0.0)
# (wy, yy)
WHICH = [(True, False), (False, True), (True, True)]

VALUE_DTYPE = {"f64": np.float64, "f32": np.float32, "mixed": np.float32}
VECTOR_DTYPE = {"f64": np.float64, "f32": np.float32, "mixed": np.float64}
ON = {"x_dict": 1, "row_slices": 1}


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


# ------------------------------------------------------------------ the bound

def terms_of(w, y):
    """The double products w_i y_i, each rounded once (exact for float32 inputs)."""
    return np.asarray(w, np.float64) * np.asarray(y, np.float64)


def dot_ref(t):
    return math.fsum(t.tolist())


def dot_bound(t):
    return (len(t) + 4) * 2.0 ** -53 * math.fsum(np.abs(t).tolist())


def assert_dots(got, w, y, wy, yy, what=""):
    """got = (wy, yy) of the GPU against fsum over the y that get_y returned."""
    for k, (asked, a) in enumerate(((wy, w), (yy, y))):
        if not asked:
            assert got[k] == 0.0 and not np.signbit(got[k]), (what, k, got)
            continue
        t = terms_of(a, y)
        ref, bound = dot_ref(t), dot_bound(t)
        print(f"dot[{k}] {what}: got {got[k]!r} ref {ref!r} |diff| {abs(got[k] - ref):.3e} bound {bound:.3e}")
        assert abs(got[k] - ref) <= bound, (what, k, got[k], ref, bound)


# ------------------------------------------------------------------ matrices (tests/test_axpby.py's)

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


def square_ragged(m, dtype=np.float64, seed=29):
    """m x m, 1..9 nonzeros per row on wrapped diagonals (x . A x needs n = m)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 10, m)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([np.sort((r + 3 * np.arange(k)) % m) for r, k in enumerate(lens)])
    val = rng.uniform(-1.0, 1.0, int(lens.sum())).astype(dtype)
    return CsrMatrix(m, m, rp, col.astype(np.int32), val)


def slice_matrices(dtype):
    """(name, matrix): fixed rows of 1..17 nonzeros (m = 200), ragged lengths,
    empty rows, m = 1, m = 65 and m = 257: a last slice with idle lanes, a last
    block with empty slices."""
    out = [(f"fixed{L}", fixed_rows(L, dtype=dtype)) for L in range(1, 18)]
    out.append(("ragged", ragged_lengths(300, dtype)))
    out.append(("empty_rows", with_empty_rows(dtype)))
    for m in (1, 65, 257):
        out.append((f"m{m}", ragged_lengths(m, dtype, seed=m)))
    return out


def slice_handle(A, which, dtype_name):
    """STREAM, or CSR3 over maps, with forced row slices; "mixed": fp32 values
    under fp64 vectors."""
    maps = hspmv.build_csr3_maps(A, 20, 10) if which == "csr3" else None
    kw = {"vector_dtype": np.float64} if dtype_name == "mixed" else {}
    return hspmv.SpMV(A, maps, kernel=which, device=0, options=ON, **kw)


def split_row_matrix(dtype=np.float64):
    """130 short rows and one of 5000 nonzeros (> 4096: the split-row kernels)."""
    lens = np.full(130, 3)
    lens[70] = 5000
    return ragged(lens, dtype)


def two_pass_cases():
    """(id, dtype name, matrix maker, SpMV keywords, info the plan must report):
    tests/test_axpby.py's two_pass_cases()."""
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
        ("xslabs1-f64", "f64", plaw, {"options": {"x_slabs": 1}}, {"x_slabs": 0}),
        ("xslabs2-f64", "f64", plaw, {"options": {"x_slabs": 2}}, {"x_slabs": 2}),
        ("split-row-f64", "f64", split_row_matrix, {}, {"n_split_rows": 1}),
    ]
    return cases
