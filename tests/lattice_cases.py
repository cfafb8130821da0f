"""The row kernels' template lattice (csrc/row_launch.cuh) as data, and the
matrices that walk it (tests/test_kernel_lattice.py).  A plain module: no
fixtures, no GPU call; the only library calls are host-side planners.

The lattice.  launch_rows picks one instantiation per (NT, U, PF, column
format) and launch_rows_shape the workgroup shape W, the x windows XW and the
padding PAD below it.  ``offered(unit)`` restates those rules -- the
``if constexpr`` and ``static_flag<OFFERED>`` conditions -- in Python: per
(NT, U) 54 kernels without prefetch and 36 with it, for 2 NT x 7 U values and
3 units (stream_f32.hip, stream_f64.hip, stream_f32v64.hip), plus the 4 slice
kernels of each unit (launch_slices: position bits x NT).  ``request(inst)``
is the public request -- SpMV keyword arguments, options, maps, matrix --
that must reach an instantiation, with the ``info`` fields the handle must
then report.

Unreachable instantiations.  None: every offered instantiation has a request.
The ones that need host-planned tables are reached as follows, each a rule of
the planner rather than a knob:
  * CSR3 W in {1, 2, 8} (any format): options csr3_plan = "ssr" with maps of
    11, 5 and 1 super-super-rows over the 705 rows (hspmv_internal.h
    ssr_waves: 64, 141 and 705 rows per SSR); hspmv_tables.cpp build_tasks
    builds a task table for the SSR plan too, so the formats that need
    DevPlan.task_start (group bases, dictionaries) are served.
  * CSR3 dictionary W = 8: hspmv_xdict.cpp xd_block_tasks gives the SSR plan's
    W tasks per dictionary block, so the one-SSR maps make one 8-task block;
    its dictionary is the whole matrix's (the gauntlet's non-split rows touch
    about 2.4 K distinct x entries for that reason).
  * x windows (no option turns them on): hspmv_tables.cpp xwin_table keeps the
    table when at least half the groups / tasks fit 256 entries -- the
    gauntlet's banded groups.
  * PAD: hspmv_plan.cpp plan_launch pads STREAM launches without prefetch
    whose median serial row is a multiple of 16 LDS words long -- the padding
    twins.

The gauntlet (``gauntlet``) is one seeded 705-row matrix built from "special"
rows, whose columns and values do not depend on the filler length, and
"filler" rows of ``fill`` nonzeros, the majority, which set the median serial
row length: 5 in the base matrix (no bank conflicts in either dtype), 8 in the
fp64 / mixed padding twin (16 words) and 32 in the fp32 one (32 words).  Every
special row long enough to be summed cooperatively is preceded, in its run of
non-split rows, by special rows only, so its sums see the same chunk offsets
in a twin as in the base matrix (the fillers and the short special rows are
serial rows: omp_spmv's order wherever they lie).  The ``narrow`` variant
differs in one region's columns only (the far cluster of the plane region,
moved below 65536) and is paired with an x whose entries moved with the
columns, so its products are the base matrix's.

Chunk offsets count from the start of a run of non-split rows inside a
64-row group, and where the groups start depends on the kernel's task layout:
multiples of 64 for STREAM, 64-row steps from each task's first row for CSR3.
``task_starts`` restates the host planner's cut for the plans ``request``
uses (``csr3_task_starts``), so the chunk properties -- four cooperative rows
in one chunk, the 600-nonzero row across a boundary -- are computed per U in
each of the five layouts (``LAYOUTS``).
"""
from __future__ import annotations

from collections import namedtuple
from functools import lru_cache

import numpy as np

import hspmv
from hspmv.api import CsrMatrix, Csr3Maps

# ------------------------------------------------------------------ constants of the library
F64_SERIAL, F32_SERIAL = 40, 56  # hspmv_internal.h kSerialMax / kSerialMaxF32
LONG_ROW = 4096                  # kLongRow: longer rows are split rows
XWIN = 256                       # kXWin
C16_BLOCK = 256                  # 1 << kC16Shift
KERNEL_CODE = {"stream": 2, "csr3": 3}

UNITS = ("f64", "f32", "mixed")
NTS = (0, 1)
US = (2, 3, 4, 5, 6, 8, 16)
FORMATS = ("col32", "col16_block", "col16_group", "dict")
KERNELS = ("stream", "csr3")

Inst = namedtuple("Inst", "unit kernel nt u pf fmt w xw xd pad")
SliceInst = namedtuple("SliceInst", "unit nt pos_bits")
Request = namedtuple("Request", "matrix n_ssr kwargs options expect")


def unit_dtypes(unit):
    """(stored values' dtype, vectors' dtype) of a unit."""
    return {"f64": (np.float64, np.float64), "f32": (np.float32, np.float32),
            "mixed": (np.float32, np.float64)}[unit]


def serial_bound(unit):
    """Rows up to this many nonzeros are summed by one lane in omp_spmv's
    order (the vectors' dtype decides: a mixed handle's is fp64's)."""
    return F32_SERIAL if unit == "f32" else F64_SERIAL


def pad_fill(unit):
    """Filler length of the unit's padding twin: 16 (fp64 vectors) or 32
    (fp32) LDS words."""
    return 32 if unit == "f32" else 8


BASE_FILL = 5


# ------------------------------------------------------------------ the lattice

def offered_shapes(kernel, fmt, pf):
    """(W, XW, PAD) launch_rows_shape instantiates for one (NT, U, PF, format)."""
    xd = fmt == "dict"
    out = []
    if kernel == "stream":
        for w in (1, 2, 4):
            if xd and w != 4:          # if constexpr (!XD || W == 4)
                continue
            for xw in ((0,) if xd else (0, 1)):              # static_flag<!XD>
                for pad in ((0,) if xd or pf else (0, 1)):   # static_flag<!XD && !PF>
                    out.append((w, xw, pad))
    else:
        for w in (1, 2, 4, 8):
            if xd and w < 4:           # if constexpr (!XD || W >= 4)
                continue
            for xw in ((0, 1) if not xd and w == 4 else (0,)):  # static_flag<!XD && W == 4>
                out.append((w, xw, 0))
    return out


def offered(unit):
    """Every row-kernel instantiation of a unit (launch_rows x launch_rows_shape)."""
    out = []
    for nt in NTS:
        for u in US:
            for pf in (0, 1):
                for fmt in FORMATS:
                    for kernel in KERNELS:
                        for w, xw, pad in offered_shapes(kernel, fmt, pf):
                            out.append(Inst(unit, kernel, nt, u, pf, fmt, w, xw, int(fmt == "dict"), pad))
    return out


def offered_slices(unit):
    """launch_slices: static_switch<12, 16> x static_flag(nontemporal)."""
    return [SliceInst(unit, nt, pb) for pb in (12, 16) for nt in NTS]


# maps for the SSR plan: super-super-rows whose mean row count gives W waves
# (ssr_waves: >= 384 rows 8, >= 192 4, >= 96 2, else 1), m = 705
SSR_FOR_W = {1: 11, 2: 5, 4: 3, 8: 1}
DICT_CAP = 32768  # x_dict_cap (bytes): 4096 fp64 / 8192 fp32 entries per block


def request(inst):
    """The public request that reaches ``inst`` and the info it must report.
    NT and PF are not reported by hspmv_info: plan_launch copies them from
    HSPMV_FLAG_NONTEMPORAL / HSPMV_FLAG_PREFETCH (and turns neither on by
    itself here: the matrices fit the Infinity Cache, and a forced U keeps the
    fp64 auto-prefetch rule off)."""
    kwargs = dict(kernel=inst.kernel, chunk_u=inst.u, nontemporal=bool(inst.nt), prefetch=bool(inst.pf))
    opts = {}
    matrix = "pad" if inst.pad else "base"
    if inst.fmt == "col32":
        kwargs["col16"] = False
        opts["x_dict"] = -1
    elif inst.fmt == "col16_block":
        kwargs["col16"] = True
        opts.update(col16_group=-1, x_dict=-1)
    elif inst.fmt == "col16_group":
        kwargs["col16"] = True
        opts.update(col16_group=1, x_dict=-1)
        matrix += "_narrow"
    else:
        opts.update(x_dict=1, x_dict_cap=DICT_CAP, row_slices=-1)
    opts["x_windows"] = 0 if inst.xw else -1
    n_ssr = 0
    if inst.kernel == "stream":
        if not inst.xd:  # dictionaries are planned for 256-row blocks: W = 4 by rule
            opts["stream_waves"] = inst.w
    else:
        n_ssr = SSR_FOR_W[inst.w]
        opts["csr3_plan"] = "aligned" if inst.w == 4 else "ssr"
    expect = dict(kernel=KERNEL_CODE[inst.kernel], chunk_u=inst.u, waves_per_block=inst.w,
                  col16_group=int(inst.fmt == "col16_group"), x_dict=inst.xd, x_windows=inst.xw,
                  lds_pad=inst.pad, row_slices=0, slice_pos_bits=0)
    if inst.fmt == "col32":
        expect["col16"] = 0
    elif inst.fmt in ("col16_group", "dict"):
        expect["col16"] = 1
    # (col16_block: 1 + the planes of the matrix, from col16_planes)
    return Request(matrix, n_ssr, kwargs, opts, expect)


SLICE_CAP = 49152  # x_dict_cap: 6144 fp64 entries, so one block can pass 4096


def slice_request(inst, path):
    """Row slices through the STREAM groups or the CSR3 aligned tasks (the same
    kernel either way).  No chunk_u or prefetch: those keep the chunked kernel
    (hspmv_slices.cpp slices_why HSPMV_SLICES_CHUNKED).  The STREAM path must
    give the position width the matrix is named for; the CSR3 path's blocks
    are cut by the task budget and for occupancy (hspmv_xdict.cpp
    split_xd_blocks), so its width is whatever hspmv_slices_pack says for its
    plan (``host_slice_bits``)."""
    kwargs = dict(kernel=path, nontemporal=bool(inst.nt))
    opts = dict(x_dict=1, row_slices=1, x_dict_cap=SLICE_CAP)
    expect = dict(kernel=KERNEL_CODE[path], x_dict=1, row_slices=1, waves_per_block=4, lds_pad=0,
                  x_windows=0, col16_group=0)
    if path == "stream":
        expect["slice_pos_bits"] = inst.pos_bits
    return Request(f"slices{inst.pos_bits}", 3 if path == "csr3" else 0, kwargs, opts, expect)


def host_slice_bits(unit, req):
    """The position width of the handle ``req`` creates, from the host planner."""
    A = matrix_for(unit, req.matrix)
    _, xdt = unit_dtypes(unit)
    S = hspmv.slices_plan(A, ssr_maps(A.m, req.n_ssr) if req.n_ssr else None, kernel=req.kwargs["kernel"],
                          options=req.options, vector_dtype=xdt if unit == "mixed" else None)
    assert S["why"] == "ok", S["why"]
    return hspmv.slices_pack(S["desc"], S["pos"])["bits"], int(S["pos"].max())


def ssr_maps(m, n_ssr, sr_rows=16):
    """Super-rows of sr_rows rows, cut into n_ssr super-super-rows of (nearly)
    equal super-row counts."""
    inner = np.append(np.arange(0, m, sr_rows), m).astype(np.int32)
    n_sr = len(inner) - 1
    outer = np.round(np.linspace(0, n_sr, n_ssr + 1)).astype(np.int32)
    return Csr3Maps(outer, inner)


# ------------------------------------------------------------------ the gauntlet

N_COLS = 200_000
M_ROWS = 64 * 11 + 1
WIN0, WIN1 = 1000, 3000            # two 256-entry x windows
WIDE_LO, WIDE_W = 20000, 700       # a cluster wider than a window
NEAR_LO, NEAR_W = 500, 600         # the plane region's near cluster ...
FAR_LO, FAR_W = 150000, 600        # ... and its far one (>= 2^16 away)
FAR_NARROW = 50000                 # where the narrow variant puts the far cluster
SPLIT_LO, SPLIT_HI = 80000, 145000  # split rows' columns: no cluster of either variant
SPLIT_ROWS = {192: 4097, 210: 4200, 230: 8300, 231: 4100, 255: 4500}
# rows 65..68 all touch nonzeros [128, 256) of their run: four pieces in one
# chunk already at U = 2 (the first four lengths sum to 254 < 256, the first
# two to 131 > 128)
COOP_ROWS = {64: 61, 65: 70, 66: 60, 67: 63, 68: 100, 69: 90}
CROSS_ROW, CROSS_LEN = 138, 600


def _window(rng, lo, k, width=XWIN):
    return lo + np.sort(rng.choice(width, size=k, replace=False))


def _row(r, fill):
    """(columns, special) of gauntlet row r.  Each row draws from its own
    generator, so a special row is the same in every twin."""
    rng = np.random.default_rng([20240, r])
    g, i = divmod(r, 64)
    filler = lambda lo, width=XWIN: (_window(rng, lo, fill, width), False)
    if g == 0:  # window WIN0: empty rows, every length mod 4, both serial bounds
        if i in (0, 1, 30, 31, 62, 63):
            return np.zeros(0, np.int64), True
        lens = {2: 1, 3: 2, 4: 3, 5: 4, 6: 40, 7: 41, 8: 56, 9: 57, 12: 13, 13: 22}
        if i in lens:
            return _window(rng, WIN0, lens[i]), True
        if i == 10:  # unsorted, with duplicates
            return WIN0 + rng.integers(0, 40, 12), True
        if i == 11:  # cooperative in fp64, serial in fp32; unsorted with duplicates
            return WIN0 + rng.integers(0, XWIN, 48), True
        return filler(WIN0)
    if g == 1:  # window WIN1: six cooperative rows of 60..100 at the group's start
        if r in COOP_ROWS:
            return _window(rng, WIN1, COOP_ROWS[r]), True
        return filler(WIN1)
    if g == 2:  # a ~600-nonzero row 500 nonzeros into its run
        if r < CROSS_ROW:
            return _window(rng, WIDE_LO, 50, WIDE_W), True
        if r == CROSS_ROW:
            return WIDE_LO + rng.integers(0, WIDE_W, CROSS_LEN), True
        return filler(WIDE_LO, WIDE_W)
    if g == 3:  # split rows: first, mid-group, two adjacent, last
        if r in SPLIT_ROWS:
            return rng.integers(SPLIT_LO, SPLIT_HI, SPLIT_ROWS[r]), True
        if r == 193:  # a cooperative row opening the run after a split row
            return _window(rng, WIN1, 70), True
        return filler(WIN1)
    if g == 4:  # every row half in the near and half in the far cluster
        k = 80 if i < 2 else fill
        near = _window(rng, NEAR_LO, (k + 1) // 2, NEAR_W)
        far = _window(rng, FAR_LO, k // 2, FAR_W)
        return np.concatenate([near, far]), i < 2
    if g == 8:  # ragged short rows, a few empty
        if i % 3 == 0:
            return _window(rng, WIN0, int(rng.integers(0, 13))), True
        return filler(WIN0)
    if g == 11:  # the last group: one row
        return _window(rng, WIN0, 7), True
    return filler(WIN1 if g % 2 else WIN0)


Gauntlet = namedtuple("Gauntlet", "A special fill narrow")


@lru_cache(maxsize=None)
def _pattern(fill, narrow):
    cols, special = [], np.zeros(M_ROWS, bool)
    for r in range(M_ROWS):
        c, special[r] = _row(r, fill)
        cols.append(np.asarray(c, np.int64))
    lens = np.array([len(c) for c in cols], np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate(cols)
    if narrow:
        far = (col >= FAR_LO) & (col < FAR_LO + FAR_W)
        col = np.where(far, col - FAR_LO + FAR_NARROW, col)
    # values: one generator per row as well; a few exact zeros in special rows
    val = np.concatenate([np.random.default_rng([777, r]).uniform(-1.0, 1.0, int(lens[r]))
                          for r in range(M_ROWS)])
    for r in (6, 9, 67, CROSS_ROW, 192):
        val[rp[r] + 3] = 0.0
        val[rp[r + 1] - 1] = 0.0
    return rp, col.astype(np.int32), val, special


def gauntlet(fill=BASE_FILL, narrow=False, dtype=np.float64):
    """G_rows: the base matrix (fill = 5) or a padding twin, in the wide
    (col16 planes) or narrow (every group spans < 65536) variant."""
    rp, col, val, special = _pattern(int(fill), bool(narrow))
    return Gauntlet(CsrMatrix(M_ROWS, N_COLS, rp, col, val.astype(dtype)), special, fill, narrow)


def matrix_for(unit, name):
    """The matrix a Request names: base / pad / base_narrow / pad_narrow /
    slices12 / slices16, in the unit's stored dtype."""
    vdt, _ = unit_dtypes(unit)
    if name.startswith("slices"):
        return g_slices(unit, int(name[6:]))
    fill = pad_fill(unit) if name.startswith("pad") else BASE_FILL
    return gauntlet(fill, name.endswith("_narrow"), vdt).A


def x_for(unit, name):
    """x of the unit's vector dtype; the narrow variants' x carries the far
    cluster's entries where their columns went, so every product is the wide
    variant's."""
    from hspmv import gen
    _, xdt = unit_dtypes(unit)
    if name.startswith("slices"):
        return gen.rand_x(matrix_for(unit, name).n, 31).astype(xdt)
    x = gen.rand_x(N_COLS, 42)
    if name.endswith("_narrow"):
        x = x.copy()
        x[FAR_NARROW:FAR_NARROW + FAR_W] = x[FAR_LO:FAR_LO + FAR_W]
    return x.astype(xdt)


# ------------------------------------------------------------------ G_slices

@lru_cache(maxsize=None)
def _slices(bound, stride, dtype_name):
    rng = np.random.default_rng(1000 + bound + stride)
    m = 64 * 5 + 17
    lens = rng.integers(0, bound + 1, m)
    # the first block's rows leave gaps of <= 8 columns (bridged: one run of
    # ~256 * stride entries), but for a few empty rows; the second is sparse
    lens[:256] = np.maximum(lens[:256], 12)
    lens[[0, 63, 64, 200, 300, m - 1]] = 0                 # empty rows, at group edges too
    lens[[1, 2, 3, 4]] = [bound, bound - 1, bound - 2, bound - 3]  # the bound, every length mod 4
    lens[256:320] = rng.integers(0, 6, 64)                 # a narrow slice (w < 8: nothing packs)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([stride * r + np.arange(k) for r, k in enumerate(lens)]).astype(np.int32)
    val = rng.uniform(-1.0, 1.0, int(lens.sum())).astype(dtype_name)
    return CsrMatrix(m, stride * m + bound + 1, rp, col, val)


def g_slices(unit, bits):
    """Ragged rows of 0 .. the unit's serial bound nonzeros, row r at columns
    stride * r ...: a 256-row block stages one run of ~256 * stride entries --
    stride 12: 3 K entries, positions below 4096, the 12-bit stream; stride
    20: 5 K entries, the 16-bit stream (tests/test_slice_pos12.py WIDTH_CASES'
    block_run idea, with ragged rows)."""
    vdt, _ = unit_dtypes(unit)
    return _slices(serial_bound(unit), 12 if bits == 12 else 20, np.dtype(vdt).name)


# ------------------------------------------------------------------ properties, from row_ptr / col_idx

def row_lens(A):
    return np.diff(A.row_ptr.astype(np.int64))


TASK_NNZ = 2048  # hspmv_tables.cpp kTaskNnz: the aligned plan's nonzero budget per task


def csr3_task_starts(A, plan, n_ssr, w):
    """The CSR3 kernel's wave tasks, restated from hspmv_tables.cpp build_tasks
    (the GPU tests hold the count against info's wave_tasks, the dictionary
    test against xdict_plan's blocks).  "aligned": 64-row groups, cut where the
    in-kernel rows pass the budget (cap_task_nnz).  "ssr": W tasks per
    super-super-row, wave k starting at the first row that reaches k / W of
    the SSR's nonzeros (ssr_tasks_rows)."""
    rp, lens, m = A.row_ptr.astype(np.int64), row_lens(A), A.m
    if plan == "aligned":
        assert w == 4
        ts = []
        for g0 in range(0, m, 64):
            ts.append(g0)
            acc = 0
            for r in range(g0, min(m, g0 + 64)):
                k = 0 if lens[r] > LONG_ROW else int(lens[r])
                if r > ts[-1] and acc + k > TASK_NNZ:
                    ts.append(r)
                    acc = 0
                acc += k
        return ts + [m]
    maps = ssr_maps(m, n_ssr)
    ts = []
    for b in range(n_ssr):
        r0, r1 = int(maps.inner[maps.outer[b]]), int(maps.inner[maps.outer[b + 1]])
        k0, k1 = int(rp[r0]), int(rp[r1])
        r = r0
        for k in range(w):
            target = k0 + (k1 - k0) * k // w
            while r < r1 and rp[r] < target:
                r += 1
            ts.append(r0 if k == 0 else r)
    return ts + [m]


# the task layouts the row kernels run the gauntlet in: STREAM's fixed groups
# and the four CSR3 plans of ``request``
LAYOUTS = (("stream", 0),) + tuple(("csr3", w) for w in (1, 2, 4, 8))


def task_starts(A, kernel, w):
    """Rows where a wave starts walking 64-row groups: None for STREAM (fixed
    groups), else the CSR3 tasks of the plan ``request`` asks for W with."""
    if kernel == "stream":
        return None
    return csr3_task_starts(A, "aligned" if w == 4 else "ssr", SSR_FOR_W[w], w)


def kernel_runs(A, starts=None):
    """[(first row, end row)] of the runs of consecutive non-split rows
    (wave_rows' [a, b)) inside the 64-row groups that STREAM (starts None:
    multiples of 64) or a CSR3 wave (64-row steps from its task's first row)
    hands to wave_rows."""
    lens = row_lens(A)
    if starts is None:
        starts = [0, A.m]
    runs = []
    for t0, t1 in zip(starts[:-1], starts[1:]):
        for g0 in range(t0, t1, 64):
            a = g0
            g1 = min(t1, g0 + 64)
            for r in range(g0, g1 + 1):
                if r == g1 or lens[r] > LONG_ROW:
                    if r > a:
                        runs.append((a, r))
                    a = r + 1
    return runs


def stream_runs(A):
    return kernel_runs(A)


def crosses_chunk(A, r, u, runs=None):
    """Row r lies in two chunks of 64 u nonzeros of its run."""
    rp = A.row_ptr.astype(np.int64)
    for a, b in (stream_runs(A) if runs is None else runs):
        if a <= r < b:
            s, e = rp[r] - rp[a], rp[r + 1] - 1 - rp[a]
            return s // (64 * u) != e // (64 * u)
    return False


def coop_rows_per_chunk(A, u, runs=None, lo=60, hi=100):
    """The largest number of rows of lo..hi nonzeros that one chunk of one
    run touches (a lower bound of wave_rows' popcount of cm)."""
    rp = A.row_ptr.astype(np.int64)
    lens = row_lens(A)
    best = 0
    for a, b in (stream_runs(A) if runs is None else runs):
        rows = [r for r in range(a, b) if lo <= lens[r] <= hi]
        if not rows:
            continue
        for c in range(0, int(rp[b] - rp[a]), 64 * u):
            c0, c1 = rp[a] + c, rp[a] + c + 64 * u
            best = max(best, sum(1 for r in rows if rp[r + 1] > c0 and rp[r] < c1))
    return best


def group_spans(A, skip_split=False):
    """Column span (max - min + 1; 0 when empty) of every 64-row group."""
    rp, lens = A.row_ptr.astype(np.int64), row_lens(A)
    out = []
    for g0 in range(0, A.m, 64):
        cs = [A.col_idx[rp[r]:rp[r + 1]] for r in range(g0, min(A.m, g0 + 64))
              if not (skip_split and lens[r] > LONG_ROW)]
        c = np.concatenate(cs) if cs else np.zeros(0, np.int32)
        out.append(int(c.max()) - int(c.min()) + 1 if len(c) else 0)
    return np.array(out)


def col16_planes(A):
    """High-bit planes of the block-base col16 format (hspmv_tables.cpp
    plan_col16): bits of the widest 256-nonzero block's span, less 16."""
    col = A.col_idx.astype(np.int64)
    span = max(int(col[k:k + C16_BLOCK].max() - col[k:k + C16_BLOCK].min())
               for k in range(0, A.nnz, C16_BLOCK))
    return max(0, span.bit_length() - 16)


def median_serial_len(A):
    """hspmv_tables.cpp build_row_tables' serial_len: the median length of the
    rows of 1 .. 40 nonzeros."""
    lens = row_lens(A)
    hist = np.bincount(lens[(lens >= 1) & (lens <= F64_SERIAL)], minlength=F64_SERIAL + 1)
    tot, acc, med = int(hist.sum()), 0, 0
    while med < F64_SERIAL and 2 * acc < tot:
        med += 1
        acc += int(hist[med])
    return med if tot else 0


def pads(unit, A):
    """plan_launch's lds_pad rule for a STREAM launch without prefetch."""
    words = median_serial_len(A) * (1 if unit == "f32" else 2)
    return words > 0 and words % 16 == 0


# ------------------------------------------------------------------ references and the error bound

def exact_products(A, x):
    """val * x[col] in long double: exact for fp32 products (48 bits), rounded
    to 64 bits for fp64 ones -- 2^-11 of the unit's eps."""
    return A.val.astype(np.longdouble) * np.asarray(x)[A.col_idx].astype(np.longdouble)


def reference(A, x, unit):
    """(y_ref, sum |a x|) per row, summed in long double."""
    assert np.finfo(np.longdouble).nmant >= 63, "needs an extended-precision long double"
    p = exact_products(A, x)
    rp = A.row_ptr.astype(np.int64)
    y = np.array([p[rp[r]:rp[r + 1]].sum() for r in range(A.m)], np.longdouble)
    s = np.array([np.abs(p[rp[r]:rp[r + 1]]).sum() for r in range(A.m)], np.longdouble)
    return y, s


def error_bound(A, absum, unit):
    """(len + 2) eps sum|a x|, the bound of any summation order of rounded
    products (each product one rounding, each of the len - 1 additions one,
    the reference's own error in the slack), plus a denormal floor of one
    smallest subnormal per term."""
    _, xdt = unit_dtypes(unit)
    eps = np.longdouble(2.0) ** (-52 if xdt == np.float64 else -23)
    tiny = np.longdouble(np.finfo(xdt).smallest_subnormal)
    lens = row_lens(A).astype(np.longdouble)
    return (lens + 2) * eps * absum + (lens + 2) * tiny


def oracle_y(A, x, unit):
    """oracle.spmv in the unit's vector dtype (a mixed unit: on the widened values)."""
    import oracle
    _, xdt = unit_dtypes(unit)
    return oracle.spmv(A.row_ptr, A.col_idx, A.val.astype(xdt), np.asarray(x, xdt))
