"""Python host mirror of the reference's CSR / CSR-3 SpMV interface, on top of
the libhspmv C ABI (include/hspmv.h).

Reference interface it mirrors:

* ``CSRk_Graph(nRows, nCols, nnz, rVec, cVec, val, ..., k, supRowSizes)`` +
  ``putInCSRkFormat()`` / ``setX()`` / ``setY()`` / ``getY()``
  (cuda-spmv-csrk/hip/csrk.cuh:321-353)  ->  :class:`SpMV` (+ :func:`build_csr3_maps`)
* ``my_read_csr`` (spmv-csr/spmv.c:11-57), ``my_read_csr3``
  (reformat-csr-to-csr3/stats.c:10-79)  ->  :func:`read_csr`, :func:`read_csr3`
* the timed loop + ``TimeMin/TimeMax/TimeAvg`` (spmv-csr/spmv.c:164-185)
  ->  :meth:`SpMV.run`

Every call goes to the GPU through libhspmv; errors raise :class:`HspmvError`.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import _lib
from ._lib import (F32, F64, KERNEL_AUTO, KERNEL_CSORT, KERNEL_CSR3, KERNEL_STREAM, KERNEL_VECTOR,
                   FLAG_DEVICE_PTRS, FLAG_NONTEMPORAL, HspmvError, check, lanes_flag, lib,
                   remap_flag)

_KERNELS = {"auto": KERNEL_AUTO, "vector": KERNEL_VECTOR, "stream": KERNEL_STREAM,
            "csr3": KERNEL_CSR3, "csort": KERNEL_CSORT}
KERNEL_NAMES = {v: k for k, v in _KERNELS.items()}


def dtype_code(dtype) -> int:
    dt = np.dtype(dtype)
    if dt == np.float64:
        return F64
    if dt == np.float32:
        return F32
    raise ValueError(f"unsupported dtype {dt} (float32 / float64)")


def np_dtype(code: int):
    return np.float64 if code == F64 else np.float32


def _ptr(a: Optional[np.ndarray]) -> Optional[int]:
    return None if a is None else a.ctypes.data


@dataclass
class CsrMatrix:
    """Host CSR matrix (0-based int32 indices, float32/float64 values)."""
    m: int
    n: int
    row_ptr: np.ndarray
    col_idx: np.ndarray
    val: np.ndarray
    index_base: int = 0

    def __post_init__(self):
        self.row_ptr = np.ascontiguousarray(self.row_ptr, dtype=np.int32)
        self.col_idx = np.ascontiguousarray(self.col_idx, dtype=np.int32)
        self.val = np.ascontiguousarray(self.val)
        if self.val.dtype not in (np.float32, np.float64):
            self.val = self.val.astype(np.float64)

    @property
    def nnz(self) -> int:
        return int(self.col_idx.shape[0])

    @property
    def dtype(self):
        return self.val.dtype

    def astype(self, dtype) -> "CsrMatrix":
        return CsrMatrix(self.m, self.n, self.row_ptr, self.col_idx,
                         self.val.astype(dtype), self.index_base)

    def c_struct(self) -> _lib.Csr:
        return _lib.Csr(self.m, self.n, self.nnz, _ptr(self.row_ptr), _ptr(self.col_idx),
                        _ptr(self.val), dtype_code(self.val.dtype))

    def fits_float32(self) -> bool:
        """True when every value converts to float32 and back to the same bits
        (hspmv_values_fit_f32), so ``SpMV(A.astype(np.float32),
        vector_dtype=np.float64)`` gives the float64 operator's y bit for bit."""
        return values_fit_float32(self.val)[0]

    @classmethod
    def from_scipy(cls, S, dtype=np.float64) -> "CsrMatrix":
        S = S.tocsr()
        S.sort_indices()
        return cls(S.shape[0], S.shape[1], S.indptr, S.indices, S.data.astype(dtype))

    def to_scipy(self):
        import scipy.sparse as sp
        return sp.csr_matrix((self.val, self.col_idx, self.row_ptr), shape=(self.m, self.n))

    def rows(self, r0: int, r1: int) -> "CsrMatrix":
        """Rows [r0, r1) with row_ptr rebased to 0 (global columns kept)."""
        k0, k1 = int(self.row_ptr[r0]), int(self.row_ptr[r1])
        return CsrMatrix(r1 - r0, self.n, self.row_ptr[r0:r1 + 1] - k0,
                         self.col_idx[k0:k1], self.val[k0:k1])


@dataclass
class Csr3Maps:
    """CSR-3 multilevel maps: outer (n_ssr+1) -> super-rows, inner (n_sr+1) -> rows."""
    outer: np.ndarray
    inner: np.ndarray

    def __post_init__(self):
        self.outer = np.ascontiguousarray(self.outer, dtype=np.int32)
        self.inner = np.ascontiguousarray(self.inner, dtype=np.int32)

    @property
    def n_ssr(self) -> int:
        return int(self.outer.shape[0] - 1)

    @property
    def n_sr(self) -> int:
        return int(self.inner.shape[0] - 1)

    def c_struct(self) -> _lib.Csr3Maps:
        return _lib.Csr3Maps(self.n_ssr, self.n_sr, _ptr(self.outer), _ptr(self.inner))


# ------------------------------------------------------------------ formats

def _take_csr(buf: _lib.CsrBuf) -> CsrMatrix:
    m, nnz = int(buf.m), int(buf.nnz)
    dt = np_dtype(buf.dtype)
    rp = np.ctypeslib.as_array(C.cast(buf.row_ptr, C.POINTER(C.c_int32)), (m + 1,)).copy()
    if nnz:
        ci = np.ctypeslib.as_array(C.cast(buf.col_idx, C.POINTER(C.c_int32)), (nnz,)).copy()
        ctype = C.c_double if dt == np.float64 else C.c_float
        val = np.ctypeslib.as_array(C.cast(buf.val, C.POINTER(ctype)), (nnz,)).copy()
    else:
        ci = np.zeros(0, np.int32)
        val = np.zeros(0, dt)
    A = CsrMatrix(m, int(buf.n), rp, ci, val, int(buf.index_base))
    lib().hspmv_free_csr(C.byref(buf))
    return A


def _take_maps(buf: _lib.Csr3Buf) -> Optional[Csr3Maps]:
    if buf.n_ssr <= 0:
        lib().hspmv_free_csr3(C.byref(buf))
        return None
    o = np.ctypeslib.as_array(C.cast(buf.outer, C.POINTER(C.c_int32)), (int(buf.n_ssr) + 1,)).copy()
    i = np.ctypeslib.as_array(C.cast(buf.inner, C.POINTER(C.c_int32)), (int(buf.n_sr) + 1,)).copy()
    lib().hspmv_free_csr3(C.byref(buf))
    return Csr3Maps(o, i)


def read_csr(path: str, dtype=np.float64) -> CsrMatrix:
    buf = _lib.CsrBuf()
    check(lib().hspmv_read_csr(str(path).encode(), dtype_code(dtype), C.byref(buf)), "read_csr")
    return _take_csr(buf)


def read_mtx(path: str, dtype=np.float64) -> CsrMatrix:
    """Matrix Market coordinate file as mmread.m + sparse2csr.m read it
    (hspmv_read_mtx: symmetric files expanded, duplicates summed, zeros
    dropped, columns sorted)."""
    buf = _lib.CsrBuf()
    check(lib().hspmv_read_mtx(str(path).encode(), dtype_code(dtype), C.byref(buf)), "read_mtx")
    return _take_csr(buf)


def rcm_reorder(A: CsrMatrix):
    """Reverse Cuthill-McKee of A's symmetrised pattern (hspmv_rcm_reorder):
    (A_perm, perm) with row i of A_perm = row perm[i] of A."""
    cs, buf = A.c_struct(), _lib.CsrBuf()
    perm = np.empty(A.m, np.int32)
    check(lib().hspmv_rcm_reorder(C.byref(cs), C.byref(buf), _ptr(perm)), "rcm_reorder")
    return _take_csr(buf), perm


def read_csr3(path: str, dtype=np.float64):
    buf, mbuf = _lib.CsrBuf(), _lib.Csr3Buf()
    check(lib().hspmv_read_csr3(str(path).encode(), dtype_code(dtype), C.byref(buf),
                                C.byref(mbuf)), "read_csr3")
    return _take_csr(buf), _take_maps(mbuf)


def write_csr(path: str, A: CsrMatrix) -> None:
    cs = A.c_struct()
    check(lib().hspmv_write_csr(str(path).encode(), C.byref(cs)), "write_csr")


def write_csr3(path: str, A: CsrMatrix, maps: Csr3Maps) -> None:
    cs, ms = A.c_struct(), maps.c_struct()
    check(lib().hspmv_write_csr3(str(path).encode(), C.byref(cs), C.byref(ms)), "write_csr3")


def save_bin(path: str, A: CsrMatrix, maps: Optional[Csr3Maps] = None) -> None:
    cs = A.c_struct()
    ms = maps.c_struct() if maps is not None else None
    check(lib().hspmv_save_bin(str(path).encode(), C.byref(cs),
                               C.byref(ms) if ms is not None else None), "save_bin")


def load_bin(path: str):
    buf, mbuf = _lib.CsrBuf(), _lib.Csr3Buf()
    check(lib().hspmv_load_bin(str(path).encode(), C.byref(buf), C.byref(mbuf)), "load_bin")
    return _take_csr(buf), _take_maps(mbuf)


def build_csr3_maps(A: CsrMatrix, ssrs: int, srs: int) -> Csr3Maps:
    cs, mbuf = A.c_struct(), _lib.Csr3Buf()
    check(lib().hspmv_build_csr3_maps(C.byref(cs), int(ssrs), int(srs), C.byref(mbuf)),
          "build_csr3_maps")
    maps = _take_maps(mbuf)
    if maps is None:  # empty matrix: one empty super-super-row is not needed
        maps = Csr3Maps(np.zeros(1, np.int32), np.zeros(1, np.int32))
    return maps


def build_csr3_bandk(A: CsrMatrix, ssrs: int, srs: int):
    """The reference's band-k CSR-3 build (hspmv_build_csr3_bandk): returns
    (A_perm, maps, perm) with A_perm = P A P^T, row i of A_perm = row perm[i]
    of A; so A_perm @ x[perm] = (A @ x)[perm]."""
    cs, buf, mbuf = A.c_struct(), _lib.CsrBuf(), _lib.Csr3Buf()
    perm = np.empty(A.m, np.int32)
    check(lib().hspmv_build_csr3_bandk(C.byref(cs), int(ssrs), int(srs), C.byref(buf),
                                       C.byref(mbuf), _ptr(perm)), "build_csr3_bandk")
    Ap = _take_csr(buf)
    maps = _take_maps(mbuf)
    if maps is None:
        maps = Csr3Maps(np.zeros(1, np.int32), np.zeros(1, np.int32))
    return Ap, maps, perm


def build_csr2_maps(A: CsrMatrix, super_row_size: int) -> Csr3Maps:
    """CSR-2 maps (one level; outer = identity): hspmv_build_csr2_maps."""
    cs, mbuf = A.c_struct(), _lib.Csr3Buf()
    check(lib().hspmv_build_csr2_maps(C.byref(cs), int(super_row_size), C.byref(mbuf)),
          "build_csr2_maps")
    maps = _take_maps(mbuf)
    if maps is None:
        maps = Csr3Maps(np.zeros(1, np.int32), np.zeros(1, np.int32))
    return maps


def build_csr2_bandk(A: CsrMatrix, super_row_size: int):
    """The k = 2 band-k build (hspmv_build_csr2_bandk): (A_perm, maps, perm)
    as build_csr3_bandk, maps with one super-row per super-super-row."""
    cs, buf, mbuf = A.c_struct(), _lib.CsrBuf(), _lib.Csr3Buf()
    perm = np.empty(A.m, np.int32)
    check(lib().hspmv_build_csr2_bandk(C.byref(cs), int(super_row_size), C.byref(buf),
                                       C.byref(mbuf), _ptr(perm)), "build_csr2_bandk")
    Ap = _take_csr(buf)
    maps = _take_maps(mbuf)
    if maps is None:
        maps = Csr3Maps(np.zeros(1, np.int32), np.zeros(1, np.int32))
    return Ap, maps, perm


_FLAVOURS = {"volta": 0, "csr3-writer": 0, "mi100": 1, "mi355x": 2}


def csr3_params(nnz_per_row: float, flavour: str = "mi355x"):
    a, b = C.c_int(), C.c_int()
    check(lib().hspmv_csr3_params(float(nnz_per_row), _FLAVOURS[flavour], C.byref(a), C.byref(b)),
          "csr3_params")
    return a.value, b.value


def partition_rows(row_ptr: np.ndarray, parts: int, maps: Optional[Csr3Maps] = None) -> np.ndarray:
    rp = np.ascontiguousarray(row_ptr, dtype=np.int32)
    out = np.zeros(parts + 1, np.int64)
    ms = maps.c_struct() if maps is not None else None
    check(lib().hspmv_partition_rows(rp.shape[0] - 1, _ptr(rp),
                                     C.byref(ms) if ms is not None else None, int(parts),
                                     _ptr(out)), "partition_rows")
    return out


def xdict_plan(A: CsrMatrix, maps: Optional[Csr3Maps] = None, *, kernel: str = "auto",
               cap_entries: int = 0, split: bool = True, options: Optional[dict] = None):
    """Block x dictionaries the library would build for A (hspmv_xdict_plan_ex):
    (blk, runs, pos) with runs as an (n_records, 2) array of {x_start,
    lds_off}, or None when some workgroup exceeds cap_entries (0 = the
    library's LDS cap for A's dtype)."""
    cs = A.c_struct()
    ms = maps.c_struct() if maps is not None else None
    flags = _KERNELS[kernel] | (0 if split else _lib.FLAG_NO_SPLIT)
    opt = _lib.make_options(flags, options)
    nb, nr = C.c_int64(), C.c_int64()
    L = lib()
    args = (C.byref(cs), C.byref(ms) if ms is not None else None, C.byref(opt), int(cap_entries))
    check(L.hspmv_xdict_plan_ex(*args, C.byref(nb), C.byref(nr), None, None, None), "xdict_plan")
    if nb.value == 0:
        return None
    blk = np.empty(nb.value + 1, np.int32)
    runs = np.empty((nr.value, 2), np.int32)
    pos = np.zeros(max(A.nnz, 1), np.uint16)
    check(L.hspmv_xdict_plan_ex(*args, C.byref(nb), C.byref(nr), _ptr(blk), _ptr(runs), _ptr(pos)),
          "xdict_plan")
    return blk, runs, pos[:A.nnz]


def values_fit_float32(val: np.ndarray):
    """(fits, first_bad) of hspmv_values_fit_f32 for a float32 / float64 array:
    first_bad is the first index whose float32 round trip changes its bits, or
    None when every value fits."""
    val = np.ascontiguousarray(val)
    bad = C.c_int64(-1)
    rc = lib().hspmv_values_fit_f32(_ptr(val), int(val.shape[0]), dtype_code(val.dtype), C.byref(bad))
    if rc < 0:
        check(rc, "hspmv_values_fit_f32")
    return (True, None) if rc == 1 else (False, int(bad.value))


def slices_plan(A: CsrMatrix, maps: Optional[Csr3Maps] = None, *, kernel: str = "auto",
                split: bool = True, options: Optional[dict] = None, fill: bool = True,
                vector_dtype=None) -> dict:
    """Row slices the library would build for A (hspmv_slices_plan): a dict
    with ``why`` (a _lib.SLICES_WHY name; "ok" = eligible), ``n_desc``,
    ``n_slices``, ``padded_entries`` and -- when eligible and ``fill`` --
    ``desc`` ((n_desc + 1, 2) {prefix, first row}), ``len``, ``pos``, ``val``.
    ``vector_dtype`` (None: A's dtype): the plan of a handle whose x and y are
    of that type (hspmv_slices_plan_vec; float64 over a float32 A: the mixed
    handle's, ``val`` stays float32)."""
    cs = A.c_struct()
    ms = maps.c_struct() if maps is not None else None
    flags = _KERNELS[kernel] | (0 if split else _lib.FLAG_NO_SPLIT)
    opt = _lib.make_options(flags, options)
    nd, ns, pe, why = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
    L = lib()
    args = (C.byref(cs), C.byref(ms) if ms is not None else None, C.byref(opt),
            C.byref(nd), C.byref(ns), C.byref(pe), C.byref(why))
    if vector_dtype is not None:
        vdt = dtype_code(vector_dtype)
        args = args[:3] + (vdt,) + args[3:]

        def plan_fn(*a):
            return L.hspmv_slices_plan_vec(*a)
    else:
        plan_fn = L.hspmv_slices_plan
    check(plan_fn(*args, None, None, None, None), "slices_plan")
    out = {"why": _lib.SLICES_WHY[why.value], "n_desc": nd.value, "n_slices": ns.value,
           "padded_entries": pe.value}
    if why.value != 0 or not fill:
        return out
    desc = np.empty((nd.value + 1, 2), np.int32)
    rl = np.zeros(max(A.m, 1), np.uint8)
    pos = np.zeros(max(pe.value, 1), np.uint16)
    val = np.zeros(max(pe.value, 1), A.val.dtype)
    check(plan_fn(*args, _ptr(desc), _ptr(rl), _ptr(pos), _ptr(val)), "slices_plan")
    out.update(desc=desc, len=rl[:A.m], pos=pos[:pe.value], val=val[:pe.value],
               n_desc=nd.value)
    return out


def slices_pack(desc: np.ndarray, pos: np.ndarray) -> dict:
    """The position stream a handle uploads for slices_plan's ``desc`` and
    ``pos`` (hspmv_slices_pack): ``bits`` (12 or 16), ``pos_prefix`` (each
    slice's start in 128-byte units, n_desc + 1 entries) and ``packed`` (the
    stream's bytes)."""
    desc = np.ascontiguousarray(desc, dtype=np.int32).reshape(-1, 2)
    pos = np.ascontiguousarray(pos, dtype=np.uint16)
    nd = desc.shape[0] - 1
    if nd < 0 or pos.shape[0] < 64 * int(desc[nd, 0]):
        raise ValueError("slices_pack: pos is shorter than desc's 64 * total width")
    bits, nbytes = C.c_int32(), C.c_int64()
    L = lib()
    args = (nd, _ptr(desc), _ptr(pos), C.byref(bits), C.byref(nbytes))
    check(L.hspmv_slices_pack(*args, None, None), "slices_pack")
    prefix = np.empty(nd + 1, np.int32)
    packed = np.zeros(max(nbytes.value, 1), np.uint8)
    check(L.hspmv_slices_pack(*args, _ptr(prefix), _ptr(packed)), "slices_pack")
    return {"bits": bits.value, "pos_prefix": prefix, "packed": packed[:nbytes.value]}


def alg_bytes(m: int, n: int, nnz: int, dtype, n_ssr: int = 0, n_sr: int = 0) -> float:
    return float(lib().hspmv_alg_bytes(m, n, nnz, dtype_code(dtype), n_ssr, n_sr))


def device_count() -> int:
    c = C.c_int()
    rc = lib().hspmv_device_count(C.byref(c))
    return c.value if rc == 0 else 0


def version() -> str:
    return lib().hspmv_version().decode()


# ------------------------------------------------------------------ handle

def _check_values(val, nnz: int, dtype) -> np.ndarray:
    """val as a contiguous (nnz,) array of dtype; ValueError for another shape
    or a dtype that does not cast ``same_kind`` to it."""
    val = np.asarray(val)
    if val.shape != (nnz,):
        raise ValueError(f"val has shape {val.shape}, expected (nnz,) = ({nnz},)")
    if not np.can_cast(val.dtype, dtype, casting="same_kind"):
        raise ValueError(f"val has dtype {val.dtype}, which does not cast to {np.dtype(dtype)}")
    return np.ascontiguousarray(val, dtype=dtype)


class SpMV:
    """One SpMV operator y = A x on one or more GPUs (a libhspmv handle).

    ``kernel``: "auto" | "stream" | "vector" | "csr3" | "csort";  ``lanes``: lanes per row
    for "vector" (0 = auto).  ``device``/``stream``: single-device handle on that
    HIP device / hipStream_t (as an int); ``devices``: row-range shards on that
    device list (hspmv_create_sharded; devices may repeat); otherwise
    ``num_gpus`` GPUs with the row-range partition.  ``options``: explicit
    planner choices (hspmv_options fields by name, e.g. ``{"csr3_plan": "ssr",
    "deterministic": "ordered"}`` -- deterministic 1 / "ordered": the ordered
    row kernels; 2 / "reproducible": bit-identical run to run, csort with
    fixed-point row sums allowed; 3 / "serial": every row summed in
    omp_spmv's order, y bit-identical to it; handle created with
    hspmv_create_ex).  ``vector_dtype``: the type of x, y, the products and the
    sums (None: A's dtype).  ``np.float64`` over a float32 ``A`` is the mixed
    handle (hspmv_create_mixed): the values are stored and streamed as float32,
    y is what the float64 operator gives for the widened matrix; one device
    only.  ``op.dtype`` is the vectors' type, ``op.value_dtype`` the stored
    values'.  ``updatable=True``: the handle takes :meth:`update_values` in
    every plan, the column-sorted one included (hspmv_create_updatable: such
    shards keep a source index per stored entry, 4 bytes each, on the device);
    the plan, ``info`` but for ``device_bytes``, and y are those of the plain
    handle.  ``op.can_update`` tells whether ``update_values`` would be taken.
    The general form y = alpha A x + beta y: :meth:`spmv_axpby` (with
    :meth:`set_y` or a bound y for the old y; :meth:`run_axpby` times it) on
    single-device handles, fused into the row-slice kernel where the plan is
    the row slices and in two passes otherwise -- ``op.axpby_path`` tells
    which, :meth:`set_axpby_path` forces the two passes; the same bytes.
    :meth:`spmv_axpby_dot` is that call with w . y and y . y of the y it
    writes, from the same pass (:meth:`set_w`, :meth:`bind_w_device`,
    :meth:`bind_dots_device`, :meth:`get_dots`, :meth:`run_axpby_dot`).
    """

    def __init__(self, A: CsrMatrix, maps: Optional[Csr3Maps] = None, *, num_gpus: int = 1,
                 kernel: str = "auto", lanes: int = 0, nontemporal: bool = False,
                 device: Optional[int] = None, stream: Optional[int] = None,
                 xcd_remap: Optional[bool] = None, split_rows: bool = True, chunk_u: int = 0,
                 prefetch: Optional[bool] = None, xcd_chunk: int = 0, groups_per_wave: int = 0,
                 col16: Optional[bool] = None, devices: Optional[list] = None,
                 options: Optional[dict] = None, vector_dtype=None, updatable: bool = False):
        self.A = A
        self.maps = maps
        self.value_dtype = A.val.dtype
        self.dtype = A.val.dtype if vector_dtype is None else np.dtype(vector_dtype)
        flags = _KERNELS[kernel] | lanes_flag(lanes) | (FLAG_NONTEMPORAL if nontemporal else 0)
        flags |= remap_flag(xcd_remap, xcd_chunk) | _lib.groups_flag(groups_per_wave)
        flags |= _lib.col16_flag(col16)
        flags |= (0 if split_rows else _lib.FLAG_NO_SPLIT)
        if chunk_u:
            if chunk_u not in (2, 3, 4, 5, 6, 8, 16):
                raise ValueError("chunk_u must be one of 2, 3, 4, 5, 6, 8, 16")
            flags |= chunk_u << _lib.U_SHIFT
        if prefetch:
            flags |= _lib.FLAG_PREFETCH
        cs = A.c_struct()
        ms = maps.c_struct() if maps is not None else None
        h = C.c_void_p()
        if updatable:  # every argument as an option: hspmv_create_updatable
            if num_gpus != 1 and devices is None:
                n = num_gpus if num_gpus > 0 else device_count()
                if n < 1:
                    raise HspmvError("hspmv_create_updatable", -6, "no HIP device visible")
                devices = list(range(n))
            opt = _lib.make_options(flags, options, device=0 if device is None else device,
                                    stream=stream, devices=devices)
            check(lib().hspmv_create_updatable(C.byref(h), C.byref(cs),
                                               C.byref(ms) if ms is not None else None, C.byref(opt),
                                               dtype_code(self.dtype)), "hspmv_create_updatable")
            self._h = h
            return
        if self.dtype != self.value_dtype:  # the mixed handle (any other pair: the library refuses)
            if num_gpus != 1 and devices is None:
                n = num_gpus if num_gpus > 0 else device_count()
                devices = list(range(max(n, 1)))
            opt = _lib.make_options(flags, options, device=0 if device is None else device,
                                    stream=stream, devices=devices)
            check(lib().hspmv_create_mixed(C.byref(h), C.byref(cs),
                                           C.byref(ms) if ms is not None else None, C.byref(opt),
                                           dtype_code(self.dtype)), "hspmv_create_mixed")
            self._h = h
            return
        if options:  # explicit planner choices: hspmv_create_ex
            if num_gpus != 1 and devices is None:
                # num_gpus <= 0 means every visible GPU, as in hspmv_create
                n = num_gpus if num_gpus > 0 else device_count()
                if n < 1:
                    raise HspmvError("hspmv_create_ex", -6, "no HIP device visible")
                devices = list(range(n))
            opt = _lib.make_options(flags, options, device=0 if device is None else device,
                                    stream=stream, devices=devices)
            rc = lib().hspmv_create_ex(C.byref(h), C.byref(cs),
                                       C.byref(ms) if ms is not None else None, C.byref(opt))
        elif devices is not None:  # row-range shards on an explicit device list
            dl = (C.c_int * len(devices))(*[int(d) for d in devices])
            rc = lib().hspmv_create_sharded(C.byref(h), C.byref(cs),
                                            C.byref(ms) if ms is not None else None, dl,
                                            len(devices), flags)
        elif device is not None:
            rc = lib().hspmv_create_on_device(C.byref(h), C.byref(cs),
                                              C.byref(ms) if ms is not None else None,
                                              int(device), stream, flags)
        else:
            rc = lib().hspmv_create(C.byref(h), C.byref(cs),
                                    C.byref(ms) if ms is not None else None, int(num_gpus), flags)
        check(rc, "hspmv_create")
        self._h = h

    @classmethod
    def from_device(cls, csr_dev: "_lib.Csr", maps_dev: "Optional[_lib.Csr3Maps]", A_meta: CsrMatrix,
                    *, device: int = 0, stream: Optional[int] = None, kernel: str = "auto",
                    lanes: int = 0, nontemporal: bool = False, xcd_remap: Optional[bool] = None,
                    split_rows: bool = True, chunk_u: int = 0,
                    prefetch: Optional[bool] = None, xcd_chunk: int = 0,
                    groups_per_wave: int = 0, col16: Optional[bool] = None,
                    options: Optional[dict] = None, vector_dtype=None, updatable: bool = False) -> "SpMV":
        """Handle over caller-owned DEVICE arrays (HSPMV_FLAG_DEVICE_PTRS):
        csr_dev/maps_dev hold device pointers; A_meta supplies m, n, dtype.
        ``vector_dtype=np.float64`` over float32 values: the mixed handle (the
        borrowed val is float32, bound x and y are float64).  ``updatable``:
        as in the constructor."""
        self = cls.__new__(cls)
        self.A = A_meta
        self.maps = None
        self.value_dtype = A_meta.val.dtype
        self.dtype = A_meta.val.dtype if vector_dtype is None else np.dtype(vector_dtype)
        flags = (_KERNELS[kernel] | lanes_flag(lanes) | (FLAG_NONTEMPORAL if nontemporal else 0)
                 | FLAG_DEVICE_PTRS | remap_flag(xcd_remap, xcd_chunk)
                 | _lib.groups_flag(groups_per_wave) | _lib.col16_flag(col16)
                 | (0 if split_rows else _lib.FLAG_NO_SPLIT) | (chunk_u << _lib.U_SHIFT)
                 | (_lib.FLAG_PREFETCH if prefetch else 0))
        h = C.c_void_p()
        opt = _lib.make_options(flags, options, device=device, stream=stream)
        if updatable:
            check(lib().hspmv_create_updatable(C.byref(h), C.byref(csr_dev),
                                               C.byref(maps_dev) if maps_dev is not None else None,
                                               C.byref(opt), dtype_code(self.dtype)), "hspmv_create_updatable")
        elif self.dtype != self.value_dtype:
            check(lib().hspmv_create_mixed(C.byref(h), C.byref(csr_dev),
                                           C.byref(maps_dev) if maps_dev is not None else None,
                                           C.byref(opt), dtype_code(self.dtype)), "hspmv_create_mixed")
        else:
            check(lib().hspmv_create_ex(C.byref(h), C.byref(csr_dev),
                                        C.byref(maps_dev) if maps_dev is not None else None,
                                        C.byref(opt)), "hspmv_create_ex")
        self._h = h
        return self

    # -- new values, same pattern
    @property
    def can_update(self) -> bool:
        """Whether update_values / update_values_device would be taken by this
        handle's plan (hspmv_can_update_values): False for a column-sorted
        handle that was not created with ``updatable=True``."""
        return bool(lib().hspmv_can_update_values(self._h))

    def update_values(self, val: np.ndarray) -> None:
        """New matrix values from host memory, in place (hspmv_update_values):
        ``val`` holds nnz values in A's CSR order and casts to ``value_dtype``;
        the plan and ``info`` stay, and every later y is bit for bit what a new
        handle over the new values gives.  ``op.A`` becomes a CsrMatrix of the
        same pattern arrays with the new values.  ValueError (before any
        library call) for another shape or a dtype that does not cast."""
        val = _check_values(val, self.A.nnz, self.value_dtype)
        check(lib().hspmv_update_values(self._h, _ptr(val), 0), "hspmv_update_values")
        self.A = CsrMatrix(self.A.m, self.A.n, self.A.row_ptr, self.A.col_idx, val, self.A.index_base)

    def update_values_device(self, ptr: Optional[int]) -> None:
        """New values from a device array of nnz ``value_dtype`` entries on the
        handle's device (HSPMV_VALUES_DEVICE; single-device handles), enqueued
        on the handle's stream with no host synchronisation: the array must
        stay unchanged until that work is done.  A handle over borrowed arrays
        (from_device): ``None`` refreshes what the handle derived from the
        array it borrows, after an in-place change; another pointer is the
        borrowed array from then on.  ``op.A`` is left as it is: the new values
        never pass through host memory."""
        check(lib().hspmv_update_values(self._h, ptr, _lib.VALUES_DEVICE), "hspmv_update_values")

    # -- vectors
    def set_x(self, x: np.ndarray) -> None:
        x = np.ascontiguousarray(x, dtype=self.dtype)
        if x.shape[0] != self.A.n:
            raise ValueError(f"x has {x.shape[0]} entries, expected n={self.A.n}")
        check(lib().hspmv_set_x(self._h, _ptr(x)), "hspmv_set_x")

    def set_y(self, y: np.ndarray) -> None:
        """m values into the handle's y in use (hspmv_set_y: its own buffer, or
        the bound array): the y_old of the next :meth:`spmv_axpby`.
        ValueError (before any library call) for another shape than (m,) or a
        dtype that does not cast ``same_kind`` to ``op.dtype``."""
        y = np.asarray(y)
        if y.shape != (self.A.m,):
            raise ValueError(f"y has shape {y.shape}, expected (m,) = ({self.A.m},)")
        if not np.can_cast(y.dtype, self.dtype, casting="same_kind"):
            raise ValueError(f"y has dtype {y.dtype}, which does not cast to {np.dtype(self.dtype)}")
        y = np.ascontiguousarray(y, dtype=self.dtype)
        check(lib().hspmv_set_y(self._h, _ptr(y)), "hspmv_set_y")

    def bind_x_device(self, ptr: Optional[int]) -> None:
        check(lib().hspmv_bind_x_device(self._h, ptr), "hspmv_bind_x_device")

    def bind_y_device(self, ptr: Optional[int]) -> None:
        check(lib().hspmv_bind_y_device(self._h, ptr), "hspmv_bind_y_device")

    def x_device(self, gpu: int = 0) -> int:
        return lib().hspmv_x_device(self._h, gpu) or 0

    def y_device(self, gpu: int = 0) -> int:
        return lib().hspmv_y_device(self._h, gpu) or 0

    # -- compute
    def spmv(self) -> None:
        check(lib().hspmv_spmv(self._h), "hspmv_spmv")

    def spmv_axpby(self, alpha: float = 1.0, beta: float = 0.0) -> None:
        """y = alpha A x + beta y, enqueued like :meth:`spmv`
        (hspmv_spmv_axpby): each of the two products and the sum rounded on
        its own in ``op.dtype``; ``beta == 0`` never reads y.  Single-device
        handles."""
        check(lib().hspmv_spmv_axpby(self._h, float(alpha), float(beta)), "hspmv_spmv_axpby")

    def run_axpby(self, alpha: float, beta: float, warmup: int = 5, iters: int = 20) -> dict:
        """:meth:`run`'s protocol over :meth:`spmv_axpby` (hspmv_run_axpby).  y
        evolves from call to call: keep ``|beta| < 1`` so it stays finite."""
        t = _lib.Timing()
        check(lib().hspmv_run_axpby(self._h, float(alpha), float(beta), int(warmup), int(iters), C.byref(t)),
              "hspmv_run_axpby")
        return {k: getattr(t, k) for k, _ in _lib.Timing._fields_}

    # -- w . y and y . y from the pass that writes y
    def set_w(self, w: np.ndarray) -> None:
        """m values into a buffer the handle owns, the w of the next
        :meth:`spmv_axpby_dot` (hspmv_set_w).  ValueError (before any library
        call) for another shape than (m,) or a dtype that does not cast
        ``same_kind`` to ``op.dtype``."""
        w = np.asarray(w)
        if w.shape != (self.A.m,):
            raise ValueError(f"w has shape {w.shape}, expected (m,) = ({self.A.m},)")
        if not np.can_cast(w.dtype, self.dtype, casting="same_kind"):
            raise ValueError(f"w has dtype {w.dtype}, which does not cast to {np.dtype(self.dtype)}")
        w = np.ascontiguousarray(w, dtype=self.dtype)
        check(lib().hspmv_set_w(self._h, _ptr(w)), "hspmv_set_w")

    def bind_w_device(self, ptr: Optional[int]) -> None:
        """w = a device array of m ``op.dtype`` entries (hspmv_bind_w_device;
        x's pointer gives x . A x); None: back to the handle's own."""
        check(lib().hspmv_bind_w_device(self._h, ptr), "hspmv_bind_w_device")

    def bind_dots_device(self, ptr: Optional[int]) -> None:
        """The two float64 results {wy, yy} go to this device address from the
        next call on (hspmv_bind_dots_device); None: the handle's own pair."""
        check(lib().hspmv_bind_dots_device(self._h, ptr), "hspmv_bind_dots_device")

    @staticmethod
    def _dot_which(wy: bool, yy: bool) -> int:
        which = (_lib.DOT_WY if wy else 0) | (_lib.DOT_YY if yy else 0)
        if not which:
            raise ValueError("spmv_axpby_dot: ask for wy, yy or both")
        return which

    def spmv_axpby_dot(self, alpha: float = 1.0, beta: float = 0.0, wy: bool = False, yy: bool = True) -> None:
        """:meth:`spmv_axpby`, the same bytes of y, and from the same pass
        ``wy`` = w . y and / or ``yy`` = y . y over the y it stores, summed in
        float64 in a fixed order (hspmv_spmv_axpby_dot).  Enqueued; the results
        stay on the device (:meth:`bind_dots_device`), :meth:`get_dots` reads
        them.  ValueError (before any library call) when neither is asked for."""
        which = self._dot_which(wy, yy)
        check(lib().hspmv_spmv_axpby_dot(self._h, float(alpha), float(beta), which), "hspmv_spmv_axpby_dot")

    def get_dots(self):
        """(wy, yy) of the last :meth:`spmv_axpby_dot` as Python floats, after
        synchronising the handle's stream (hspmv_get_dots); the one not asked
        for is 0.0."""
        d = (C.c_double * 2)()
        check(lib().hspmv_get_dots(self._h, d), "hspmv_get_dots")
        return d[0], d[1]

    def run_axpby_dot(self, alpha: float, beta: float, wy: bool = False, yy: bool = True, warmup: int = 5,
                      iters: int = 20) -> dict:
        """:meth:`run_axpby`'s protocol over :meth:`spmv_axpby_dot`
        (hspmv_run_axpby_dot)."""
        which = self._dot_which(wy, yy)
        t = _lib.Timing()
        check(lib().hspmv_run_axpby_dot(self._h, float(alpha), float(beta), which, int(warmup), int(iters),
                                        C.byref(t)), "hspmv_run_axpby_dot")
        return {k: getattr(t, k) for k, _ in _lib.Timing._fields_}

    @property
    def axpby_path(self) -> str:
        """"fused" (the row-slice kernel with the epilogue in its store) or
        "two_pass" (the SpMV into a scratch vector, then one elementwise
        kernel): what the next :meth:`spmv_axpby` runs (hspmv_axpby_path)."""
        rc = lib().hspmv_axpby_path(self._h)
        if rc < 0:
            check(rc, "hspmv_axpby_path")
        return _lib.AXPBY_PATHS[rc]

    def set_axpby_path(self, mode: str) -> None:
        """"auto" (fused where the plan allows it) | "two_pass"
        (hspmv_set_axpby_path); y is the same bytes either way."""
        if mode not in _lib.AXPBY_MODES:
            raise ValueError(f"axpby path {mode!r} (one of {', '.join(_lib.AXPBY_MODES)})")
        check(lib().hspmv_set_axpby_path(self._h, _lib.AXPBY_MODES[mode]), "hspmv_set_axpby_path")

    def synchronize(self) -> None:
        check(lib().hspmv_synchronize(self._h), "hspmv_synchronize")

    def set_sweep(self, mode: str) -> None:
        """"auto" | "forward" | "alternate": whether the row kernel sweeps its
        blocks in the opposite direction on every other SpMV (hspmv_set_sweep;
        y is the same bits either way).  From the next call on."""
        if mode not in _lib.SWEEP:
            raise ValueError(f"sweep mode {mode!r} (one of {', '.join(_lib.SWEEP)})")
        check(lib().hspmv_set_sweep(self._h, _lib.SWEEP[mode]), "hspmv_set_sweep")

    def run(self, warmup: int = 5, iters: int = 20) -> dict:
        t = _lib.Timing()
        check(lib().hspmv_run(self._h, int(warmup), int(iters), C.byref(t)), "hspmv_run")
        return {k: getattr(t, k) for k, _ in _lib.Timing._fields_}

    def get_y(self) -> np.ndarray:
        y = np.empty(self.A.m, dtype=self.dtype)
        check(lib().hspmv_get_y(self._h, _ptr(y)), "hspmv_get_y")
        return y

    def __call__(self, x: np.ndarray) -> np.ndarray:
        self.set_x(x)
        self.spmv()
        return self.get_y()

    def dtypes(self):
        """(value dtype, vector dtype) as the handle reports them (hspmv_get_dtypes)."""
        a, b = C.c_int(), C.c_int()
        check(lib().hspmv_get_dtypes(self._h, C.byref(a), C.byref(b)), "hspmv_get_dtypes")
        return np.dtype(np_dtype(a.value)), np.dtype(np_dtype(b.value))

    def exchange(self):
        b, g = C.c_double(), C.c_double()
        check(lib().hspmv_exchange(self._h, C.byref(b), C.byref(g)), "hspmv_exchange")
        return b.value, g.value

    @property
    def info(self) -> dict:
        i = _lib.Info()
        check(lib().hspmv_get_info_sized(self._h, C.byref(i), C.sizeof(i)), "hspmv_get_info_sized")
        d = {k: getattr(i, k) for k, _ in _lib.Info._fields_}
        d["placement_us"] = [round(v, 3) for v in d["placement_us"][:d["placement_trials"]]]
        d["csort_part_begin"] = [int(v) for v in d["csort_part_begin"][:max(d["csort_parts"], 0)]]
        d["kernel_name"] = KERNEL_NAMES.get(d["kernel"], "?")
        return d

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().hspmv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class SpMM:
    """Multi-vector operator Y = A X for ``k`` right-hand sides (1 <= k <= 32)
    in one pass over A (a libhspmv ``hspmv_mm``).

    X is row-major ``(n, k)`` -- what a contiguous numpy / torch array of that
    shape is -- and Y row-major ``(m, k)``.  On every row of at most
    ``info["serial_max"]`` nonzeros, column c of Y carries the bits
    ``SpMV(A)(X[:, c])`` gives (omp_spmv's order); longer rows are summed in a
    fixed order, bit-identical run to run.  One device; ``stream``: a
    hipStream_t as an int (None: library-owned).
    """

    def __init__(self, A: CsrMatrix, k: int, *, device: int = 0, stream: Optional[int] = None,
                 nontemporal: bool = False):
        self._init_meta(A, k)
        cs = A.c_struct()
        self._create(cs, FLAG_NONTEMPORAL if nontemporal else 0, device, stream)

    def _init_meta(self, A: CsrMatrix, k: int) -> None:
        self._h = None
        self.A = A
        self.k = int(k)
        self.dtype = A.val.dtype
        if not 1 <= self.k <= 32:
            raise ValueError(f"k = {k} right-hand sides (1 <= k <= 32)")

    def _create(self, cs: "_lib.Csr", flags: int, device: int, stream: Optional[int]) -> None:
        opt = _lib.make_options(flags, None, device=device, stream=stream)
        h = C.c_void_p()
        check(lib().hspmv_mm_create(C.byref(h), C.byref(cs), self.k, C.byref(opt)), "hspmv_mm_create")
        self._h = h

    @classmethod
    def from_device(cls, csr_dev: "_lib.Csr", A_meta: CsrMatrix, k: int, *, device: int = 0,
                    stream: Optional[int] = None, nontemporal: bool = False) -> "SpMM":
        """Operator over caller-owned DEVICE arrays (HSPMV_FLAG_DEVICE_PTRS):
        csr_dev holds device pointers; A_meta supplies m, n, dtype."""
        self = cls.__new__(cls)
        self._init_meta(A_meta, k)
        self._create(csr_dev, FLAG_DEVICE_PTRS | (FLAG_NONTEMPORAL if nontemporal else 0), device, stream)
        return self

    # -- new values, same pattern
    def update_values(self, val: np.ndarray) -> None:
        """New matrix values from host memory (hspmv_mm_update_values), as
        :meth:`SpMV.update_values`; ``op.A`` takes the new values."""
        val = _check_values(val, self.A.nnz, self.dtype)
        check(lib().hspmv_mm_update_values(self._h, _ptr(val), 0), "hspmv_mm_update_values")
        self.A = CsrMatrix(self.A.m, self.A.n, self.A.row_ptr, self.A.col_idx, val, self.A.index_base)

    def update_values_device(self, ptr: Optional[int]) -> None:
        """New values from a device array on the operator's device, copied on
        its stream (HSPMV_VALUES_DEVICE); an operator over borrowed arrays
        reads its array on every SpMM: ``None`` does nothing, another pointer
        is the borrowed array from then on.  ``op.A`` is left as it is."""
        check(lib().hspmv_mm_update_values(self._h, ptr, _lib.VALUES_DEVICE), "hspmv_mm_update_values")

    # -- vectors
    def _check_x(self, X) -> np.ndarray:
        """X as a contiguous (n, k) array of the operator's dtype; ValueError
        (before any library call) for another shape or a dtype that does not
        cast to it."""
        X = np.asarray(X)
        if X.ndim != 2 or X.shape != (self.A.n, self.k):
            raise ValueError(f"X has shape {X.shape}, expected (n, k) = ({self.A.n}, {self.k})")
        if not np.can_cast(X.dtype, self.dtype, casting="same_kind"):
            raise ValueError(f"X has dtype {X.dtype}, which does not cast to {np.dtype(self.dtype)}")
        return np.ascontiguousarray(X, dtype=self.dtype)

    def set_x(self, X: np.ndarray) -> None:
        X = self._check_x(X)
        check(lib().hspmv_mm_set_x(self._h, _ptr(X), self.k), "hspmv_mm_set_x")

    def bind_x_device(self, ptr: Optional[int], ldx: Optional[int] = None) -> None:
        """X on the device: n rows of ldx elements (default k); None: the operator's own buffer."""
        check(lib().hspmv_mm_bind_x_device(self._h, ptr, self.k if ldx is None else int(ldx)),
              "hspmv_mm_bind_x_device")

    def bind_y_device(self, ptr: Optional[int], ldy: Optional[int] = None) -> None:
        check(lib().hspmv_mm_bind_y_device(self._h, ptr, self.k if ldy is None else int(ldy)),
              "hspmv_mm_bind_y_device")

    # -- compute
    def spmm(self) -> None:
        check(lib().hspmv_mm_spmm(self._h), "hspmv_mm_spmm")

    def synchronize(self) -> None:
        check(lib().hspmv_mm_synchronize(self._h), "hspmv_mm_synchronize")

    def run(self, warmup: int = 5, iters: int = 20) -> dict:
        t = _lib.Timing()
        check(lib().hspmv_mm_run(self._h, int(warmup), int(iters), C.byref(t)), "hspmv_mm_run")
        return {f: getattr(t, f) for f, _ in _lib.Timing._fields_}

    def get_y(self) -> np.ndarray:
        Y = np.empty((self.A.m, self.k), dtype=self.dtype)
        check(lib().hspmv_mm_get_y(self._h, _ptr(Y), self.k), "hspmv_mm_get_y")
        return Y

    def __call__(self, X: np.ndarray) -> np.ndarray:
        self.set_x(X)
        self.spmm()
        return self.get_y()

    @property
    def info(self) -> dict:
        i = _lib.MmInfo()
        check(lib().hspmv_mm_get_info(self._h, C.byref(i), C.sizeof(i)), "hspmv_mm_get_info")
        return {f: getattr(i, f) for f, _ in _lib.MmInfo._fields_}

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().hspmv_mm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
