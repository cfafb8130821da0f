"""Every row-kernel instantiation of csrc/row_launch.cuh against the oracle.

CPU: the lattice restated as data (tests/lattice_cases.py) has the counts the
header states; every instantiation has a distinct public request; the
gauntlet matrices keep, per U and per variant, every property the kernels'
inner branches need; the planner-side rules the requests lean on (padding,
x windows, dictionaries, row slices) hold on them; and oracle.spmv itself
stays inside the error bound used below.

GPU: one test per (unit, kernel, column format) walks its instantiations.
For each the handle must report the shape that was asked for (a fallback is a
failure), write every row of a y poisoned with 0xFF bytes, give omp_spmv's
bits on every serially summed row, stay within (len + 2) eps sum|a x| of a
long-double reference on the others, and give the same bits as the plainest
variant of its (unit, kernel, U, W) -- 32-bit columns, nothing else on --
which each test runs for itself and whose task layout it must share (a
dictionary variant may differ in layout; then its serial rows are compared).
The last test checks that the instantiations run are exactly the reachable
set.  Times: pytest --durations; on an MI355X the module takes 4.5 s, its
slowest test 0.54 s.
"""
import numpy as np
import pytest

import hspmv
import lattice_cases as lc
from lattice_cases import Inst
from test_sweep import hip_runtime  # hipMemset on the runtime this process already runs on

# ------------------------------------------------------------------ CPU: the lattice


def test_lattice_counts_match_the_header():
    """54 + 36 per (NT, U), 4 slice kernels, 14 (NT, U) pairs, 3 units."""
    total = 0
    for unit in lc.UNITS:
        insts = lc.offered(unit)
        assert len(set(insts)) == len(insts)
        for nt in lc.NTS:
            for u in lc.US:
                mine = [i for i in insts if i.nt == nt and i.u == u]
                assert sum(1 for i in mine if not i.pf) == 54
                assert sum(1 for i in mine if i.pf) == 36
        assert len(insts) == 14 * 90
        assert len(lc.offered_slices(unit)) == 4
        total += len(insts) + 4
    assert total == 3 * (14 * 90 + 4) == 3792
    # the header's table, per (NT, U, PF = 0) and format
    for fmt in ("col32", "col16_block", "col16_group"):
        assert len(lc.offered_shapes("stream", fmt, 0)) == 12 and len(lc.offered_shapes("stream", fmt, 1)) == 6
        assert len(lc.offered_shapes("csr3", fmt, 0)) == len(lc.offered_shapes("csr3", fmt, 1)) == 5
    assert lc.offered_shapes("stream", "dict", 0) == lc.offered_shapes("stream", "dict", 1) == [(4, 0, 0)]
    assert lc.offered_shapes("csr3", "dict", 1) == [(4, 0, 0), (8, 0, 0)]


def _frozen(req):
    return (req.matrix, req.n_ssr, tuple(sorted(req.kwargs.items())), tuple(sorted(req.options.items())))


def test_every_instantiation_has_its_own_request():
    """No instantiation is unreachable, and no two share a request (so the
    loop below cannot count one launch twice)."""
    for unit in lc.UNITS:
        seen = {}
        for inst in lc.offered(unit):
            req = lc.request(inst)
            assert req.expect["chunk_u"] == inst.u and req.kwargs["chunk_u"] == inst.u  # U is always forced
            assert seen.setdefault(_frozen(req), inst) == inst
            assert (req.n_ssr > 0) == (inst.kernel == "csr3")
            if inst.kernel == "csr3":
                m = lc.M_ROWS
                # the maps give the W asked for (hspmv_internal.h ssr_waves), the aligned plan 4
                w = m / req.n_ssr / 64.0
                want = 8 if w >= 6 else 4 if w >= 3 else 2 if w >= 1.5 else 1
                assert (req.options["csr3_plan"], inst.w) in {("ssr", want), ("aligned", 4)}
                maps = lc.ssr_maps(m, req.n_ssr)
                assert maps.n_ssr == req.n_ssr and maps.inner[-1] == m and maps.outer[-1] == maps.n_sr


# ------------------------------------------------------------------ CPU: the gauntlet

FILLS = sorted({lc.BASE_FILL} | {lc.pad_fill(u) for u in lc.UNITS})
VARIANTS = [(f, n) for f in FILLS for n in (False, True)]


@pytest.mark.parametrize("fill,narrow", VARIANTS)
def test_gauntlet_rows(fill, narrow):
    G = lc.gauntlet(fill, narrow)
    A, lens = G.A, lc.row_lens(G.A)
    assert A.m == 705 and A.m % 64 == 1 and A.n == 200_000 and A.nnz <= 60_000
    # empty rows at the start, in the middle and at the end of a group
    assert not lens[[0, 1, 30, 31, 62, 63]].any() and lens[2] > 0 and lens[61] > 0
    # serial rows of every length mod 4, and both dtypes' serial bounds from both sides
    serial = lens[(lens >= 1) & (lens <= lc.F64_SERIAL)]
    assert {int(v) % 4 for v in serial} == {0, 1, 2, 3}
    assert {40, 41, 56, 57} <= set(lens.tolist())
    assert {1, 2, 3} <= set(lens.tolist())  # ordered_sum's 1-3 element tail alone
    # cooperative rows of 60..100 in one group
    coop = [r for r in range(64, 128) if 60 <= lens[r] <= 100]
    assert len(coop) >= 4 and coop == sorted(lc.COOP_ROWS)
    assert lens[lc.CROSS_ROW] == lc.CROSS_LEN
    # per U and per task layout a kernel runs the matrix in (STREAM's fixed
    # groups; the CSR3 tasks of the aligned plan and of the three SSR plans,
    # whose waves start their 64-row groups wherever the nonzero balance put them)
    for kernel, w in lc.LAYOUTS:
        runs = lc.kernel_runs(A, lc.task_starts(A, kernel, w))
        for u in lc.US:
            # four or more of them in one chunk: wave_rows' row16 path
            # (__popcll(cm) >= 3) with all four of its 16-lane slots taken ...
            assert lc.coop_rows_per_chunk(A, u, runs) >= 4, (kernel, w, u)
            # ... and the ~600-nonzero row in two chunks
            assert lc.crosses_chunk(A, lc.CROSS_ROW, u, runs), (kernel, w, u)
        assert lc.coop_rows_per_chunk(A, 16, runs) >= 5, (kernel, w)  # two rounds of four at the large chunks
    # split rows: first and last row of a group, mid-group, two adjacent
    split = np.flatnonzero(lens > lc.LONG_ROW)
    assert split.tolist() == sorted(lc.SPLIT_ROWS)
    pos = split % 64
    assert 0 in pos and 63 in pos and any(0 < p < 63 for p in pos) and 1 in np.diff(split)
    assert lens.max() > 2 * lc.LONG_ROW  # three chunks of one split row
    runs = lc.stream_runs(A)
    assert sum(1 for a, b in runs if 192 <= a < 256) == 3  # the group's runs between its split rows
    # unsorted columns with duplicates, exact zeros
    rp = A.row_ptr
    unsorted = [r for r in range(A.m) if lens[r] <= lc.LONG_ROW and np.any(np.diff(A.col_idx[rp[r]:rp[r + 1]]) < 0)]
    dups = [r for r in unsorted if len(set(A.col_idx[rp[r]:rp[r + 1]].tolist())) < lens[r]]
    assert {10, 11, lc.CROSS_ROW} <= set(dups)
    assert 5 <= int((A.val == 0).sum()) <= 20
    # a cooperative special row's chunk offsets do not depend on the fillers
    for a, b in runs:
        firsts = [r for r in range(a, b) if not G.special[r]]
        first_filler = firsts[0] if firsts else b
        for r in range(a, b):
            if G.special[r] and lens[r] > lc.F64_SERIAL:
                assert r < first_filler, r
    # the fillers set the median serial row length
    assert lc.median_serial_len(A) == fill and (~G.special).sum() > A.m // 2
    assert np.all(lens[~G.special] == fill) and fill <= lc.F64_SERIAL


@pytest.mark.parametrize("fill", FILLS)
def test_task_layouts_cover_the_rows(fill):
    """The restated CSR3 task cuts: W tasks per super-super-row for the SSR
    plans, 64-row groups cut at the nonzero budget for the aligned one; each
    a non-decreasing cover of the rows."""
    A = lc.gauntlet(fill).A
    for kernel, w in lc.LAYOUTS[1:]:
        ts = lc.task_starts(A, kernel, w)
        assert ts[0] == 0 and ts[-1] == A.m and np.all(np.diff(ts) >= 0)
        if w == 4:
            assert set(range(0, A.m, 64)) <= set(ts) and len(ts) - 1 == (15 if fill == 32 else 12)
        else:
            assert len(ts) - 1 == lc.SSR_FOR_W[w] * w
            assert set(ts[::w]) == set(lc.ssr_maps(A.m, lc.SSR_FOR_W[w]).inner[lc.ssr_maps(A.m, lc.SSR_FOR_W[w]).outer])


@pytest.mark.parametrize("fill,narrow", VARIANTS)
def test_gauntlet_columns(fill, narrow):
    A = lc.gauntlet(fill, narrow).A
    assert A.col_idx.min() >= 0 and A.col_idx.max() < A.n
    spans = lc.group_spans(A)
    fit = (spans > 0) & (spans <= lc.XWIN)
    # x windows: at least half the groups fit 256 entries (xwin_table keeps the
    # table), and some groups inside the XW kernel do not (win.w == 0)
    assert 2 * fit.sum() >= len(spans) and (~fit).sum() >= 3
    assert spans[-1] <= lc.XWIN  # the one-row group
    inner = lc.group_spans(A, skip_split=True)
    planes = lc.col16_planes(A)
    if narrow:
        # group bases: every group, and every task a plan can cut, spans < 65536
        lens = lc.row_lens(A)
        keep = np.repeat(lens <= lc.LONG_ROW, lens)
        c = A.col_idx[keep]
        assert int(c.max()) - int(c.min()) < 65536 and inner.max() < 65536
    else:
        assert 1 <= planes <= 8
        assert inner.max() >= 65536 and (inner < 65536).sum() >= 8  # one region needs planes, the rest do not
    # a 64-lane load that lies in two col16 blocks and two plane words: the
    # plane region's run starts off a multiple of 64 nonzeros (every load of
    # the run, whatever U, covers nonzeros [kb + 64 j, kb + 64 j + 64)), and
    # one of its loads has a multiple of 256 inside
    kb, ke = int(A.row_ptr[256]), int(A.row_ptr[320])
    assert (256, 320) in lc.stream_runs(A) and kb % 64 != 0
    assert any(k // 256 != (min(k + 63, ke - 1)) // 256 for k in range(kb, ke, 64))
    if not narrow:  # ... and both of those blocks carry plane bits
        assert lc.group_spans(A, skip_split=True)[4] >= 65536


def test_twins_and_variants_share_the_special_rows():
    base = lc.gauntlet()
    for unit in lc.UNITS:
        twin = lc.gauntlet(lc.pad_fill(unit))
        assert np.array_equal(base.special, twin.special)
        for r in np.flatnonzero(base.special):
            a0, a1 = base.A.row_ptr[r], base.A.row_ptr[r + 1]
            b0, b1 = twin.A.row_ptr[r], twin.A.row_ptr[r + 1]
            assert np.array_equal(base.A.col_idx[a0:a1], twin.A.col_idx[b0:b1])
            assert np.array_equal(base.A.val[a0:a1], twin.A.val[b0:b1])
    # narrow: the same rows and values, the far cluster's columns moved, x moved with them
    nar = lc.gauntlet(narrow=True)
    assert np.array_equal(base.A.row_ptr, nar.A.row_ptr) and np.array_equal(base.A.val, nar.A.val)
    moved = base.A.col_idx != nar.A.col_idx
    assert moved.any() and np.all(base.A.col_idx[moved] >= lc.FAR_LO)
    assert set(np.flatnonzero(moved).tolist()) <= set(range(base.A.row_ptr[256], base.A.row_ptr[320]))
    xw, xn = lc.x_for("f64", "base"), lc.x_for("f64", "base_narrow")
    assert np.array_equal(xw[base.A.col_idx], xn[nar.A.col_idx])


@pytest.mark.parametrize("unit", lc.UNITS)
def test_padding_follows_the_median_row_length(unit):
    """hspmv_plan.cpp: lds_pad when the median serial row is a multiple of 16
    LDS words long -- the twins' fillers (fp64 / mixed 8, fp32 32), not the base's."""
    assert lc.pad_fill(unit) == (32 if unit == "f32" else 8)
    for narrow in (False, True):
        assert not lc.pads(unit, lc.gauntlet(lc.BASE_FILL, narrow).A)
        assert lc.pads(unit, lc.gauntlet(lc.pad_fill(unit), narrow).A)


@pytest.mark.parametrize("unit", lc.UNITS)
def test_dictionaries_fit_every_block_shape(unit):
    """The dictionary requests are served: STREAM's 256-row blocks, the
    aligned plan's 4-task blocks and the one-SSR plan's single 8-task block
    all stay under the cap (in the vectors' dtype, which sizes the entries)."""
    _, xdt = lc.unit_dtypes(unit)
    A = lc.gauntlet(dtype=xdt).A
    for kernel, w in (("stream", 4), ("csr3", 4), ("csr3", 8)):
        req = lc.request(Inst(unit, kernel, 0, 4, 0, "dict", w, 0, 1, 0))
        maps = lc.ssr_maps(A.m, req.n_ssr) if req.n_ssr else None
        plan = hspmv.xdict_plan(A, maps, kernel=kernel, options=req.options)
        assert plan is not None, (kernel, w)
        blk, runs, pos = plan
        # one dictionary per workgroup: STREAM's 256 rows, or W of the plan's tasks
        # (12 aligned tasks: 3 blocks; the one SSR's 8 tasks: 1) -- the planner's
        # own task table, which lattice_cases restates
        starts = lc.task_starts(A, kernel, w)
        tasks = {("stream", 4): None, ("csr3", 4): 12, ("csr3", 8): 8}[kernel, w]
        assert (starts and len(starts) - 1) == tasks
        assert len(blk) - 1 == (-(-A.m // 256) if kernel == "stream" else -(-tasks // w)) == {4: 3, 8: 1}[w]
        assert int(runs[:, 1].max()) * np.dtype(xdt).itemsize <= lc.DICT_CAP


@pytest.mark.parametrize("unit", lc.UNITS)
def test_slice_matrices_are_eligible_in_both_widths(unit):
    """G_slices: ragged rows up to the serial bound, empty rows, eligible
    (slices_plan's why == "ok") through both paths; the STREAM path gives the
    12-bit stream on one column layout and the 16-bit one on the other."""
    bound = lc.serial_bound(unit)
    for bits in (12, 16):
        A = lc.g_slices(unit, bits)
        lens = lc.row_lens(A)
        assert lens.max() == bound and (lens == 0).sum() >= 5 and A.m % 64 == 17
        assert len({int(v) for v in lens}) > bound // 2  # ragged
        for path in ("stream", "csr3"):
            req = lc.slice_request(lc.SliceInst(unit, 0, bits), path)
            got, top = lc.host_slice_bits(unit, req)  # asserts why == "ok"
            assert got in (12, 16)
            if path == "stream":
                assert got == bits and (top < 4096) == (bits == 12)


ALL_MATRICES = ("base", "base_narrow", "pad", "pad_narrow", "slices12", "slices16")


@pytest.mark.parametrize("unit", lc.UNITS)
def test_oracle_stays_inside_the_bound(unit):
    """omp_spmv's own order is one of the summation orders the bound covers."""
    for name in ALL_MATRICES:
        A, x = lc.matrix_for(unit, name), lc.x_for(unit, name)
        y_ref, absum = lc.reference(A, x, unit)
        bound = lc.error_bound(A, absum, unit)
        err = np.abs(lc.oracle_y(A, x, unit).astype(np.longdouble) - y_ref)
        assert np.all(err <= bound), (name, float((err / np.maximum(bound, 1e-300)).max()))
        # the bound is far below the suite's usual 1e-6 |y| bar on the long rows
        lens = lc.row_lens(A)
        if not name.startswith("slices") and unit != "f32":
            assert np.all(bound[lens > 40] < 1e-9 * absum[lens > 40])


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def need_gpu():
    assert hspmv.device_count() >= 1, "no HIP device visible: the gpu tests must run on the MI355X box"


class Case:
    """A matrix, its x and the three references, computed once per (unit, name)."""
    _cache = {}

    def __init__(self, unit, name):
        self.A, self.x = lc.matrix_for(unit, name), lc.x_for(unit, name)
        self.lens = lc.row_lens(self.A)
        self.serial = self.lens <= lc.serial_bound(unit)
        self.oracle = lc.oracle_y(self.A, self.x, unit)
        self.y_ref, absum = lc.reference(self.A, self.x, unit)
        self.bound = lc.error_bound(self.A, absum, unit)
        self.special = None if name.startswith("slices") else lc.gauntlet(
            lc.pad_fill(unit) if name.startswith("pad") else lc.BASE_FILL, name.endswith("_narrow")).special
        self.maps = {}

    @classmethod
    def get(cls, unit, name):
        key = (unit, name)
        if key not in cls._cache:
            cls._cache[key] = cls(unit, name)
        return cls._cache[key]

    def maps_for(self, n_ssr):
        if not n_ssr:
            return None
        if n_ssr not in self.maps:
            self.maps[n_ssr] = lc.ssr_maps(self.A.m, n_ssr)
        return self.maps[n_ssr]


def run_request(unit, req):
    """One handle, one SpMV into a y of 0xFF bytes: (y, info)."""
    case = Case.get(unit, req.matrix)
    _, xdt = lc.unit_dtypes(unit)
    H = hip_runtime()
    with hspmv.SpMV(case.A, case.maps_for(req.n_ssr), device=0, options=req.options,
                    vector_dtype=xdt if unit == "mixed" else None, **req.kwargs) as op:
        info = op.info
        op.set_x(case.x)
        op.synchronize()
        assert H.hipMemset(op.y_device(0), 0xFF, case.A.m * np.dtype(xdt).itemsize) == 0
        assert H.hipDeviceSynchronize() == 0
        op.spmv()
        y = op.get_y()
    return case, y, info


def check_info(info, expect):
    return [f"info[{k}] = {info[k]}, asked {v}" for k, v in expect.items() if info[k] != v]


def check_y(case, y):
    """Every row written; serial rows omp_spmv's bits; the others within the bound."""
    bad = []
    if np.isnan(y).any():
        bad.append(f"rows not written: {np.flatnonzero(np.isnan(y))[:8].tolist()}")
        return bad
    s = case.serial
    if y[s].tobytes() != case.oracle[s].tobytes():
        rows = np.flatnonzero(s)[y[s] != case.oracle[s]]
        bad.append(f"serial rows differ from omp_spmv: {rows[:8].tolist()} (lens {case.lens[rows[:8]].tolist()})")
    err = np.abs(y.astype(np.longdouble) - case.y_ref)
    over = np.flatnonzero(err > case.bound)
    if len(over):
        worst = over[np.argmax((err / np.maximum(case.bound, np.finfo(np.longdouble).tiny))[over])]
        bad.append(f"rows past (len + 2) eps sum|ax|: {over[:8].tolist()}; row {worst} len {case.lens[worst]} "
                   f"err {float(err[worst]):.3e} bound {float(case.bound[worst]):.3e}")
    return bad


RAN = set()   # (unit, kernel, NT, U, PF, format, W, XW, XD, PAD) and slice tuples run
REFS = {}     # (unit, kernel, U, W) -> (y, task layout) of reference_variant


def full_expect(inst, req, case):
    """req.expect plus what depends on the matrix: the planes of the
    block-base col16 format and, for the CSR3 formats that keep the plan's
    own tasks, their number (which holds lattice_cases' restatement of the
    host planner, on which the per-layout matrix properties are computed,
    against the planner itself)."""
    expect = dict(req.expect)
    if inst.fmt == "col16_block":
        expect["col16"] = 1 + lc.col16_planes(case.A)
    if inst.kernel == "csr3" and not inst.xd:
        expect["wave_tasks"] = len(lc.task_starts(case.A, "csr3", inst.w)) - 1
    return expect


def layout_key(info):
    return (info["blocks"], info["waves_per_block"], info["wave_tasks"])


def reference_variant(unit, kernel, u, w):
    """y and the task layout of the plainest variant of (unit, kernel, U, W):
    32-bit columns, no NT, prefetch, x windows or padding, on the base
    matrix.  Run on demand by whichever test asks first, so a test run alone
    compares against the same reference as the whole module."""
    key = (unit, kernel, u, w)
    if key not in REFS:
        inst = Inst(unit, kernel, 0, u, 0, "col32", w, 0, 0, 0)
        req = lc.request(inst)
        case, y, info = run_request(unit, req)
        bad = check_info(info, full_expect(inst, req, case))
        assert not bad, f"the reference variant {inst} fell back: {bad}"
        REFS[key] = (y, layout_key(info))
    return REFS[key]


def check_identity(inst, case, y, info):
    """The same bits as the reference variant of this (unit, kernel, U, W):
    on every row across NT, PF, XW and the three non-dictionary formats, whose
    task layout must be the reference's; a padding twin on the rows it shares
    with the base matrix (its fillers are serial rows, held to omp_spmv's
    bits already).  The header (row_launch.cuh, row_kernels.cuh): these
    choices change where the data comes from, never the products or their
    summation order.  A dictionary variant with the reference's layout is held
    to every row as well; with another one (its blocks were cut) only its
    serial rows are comparable, and those are omp_spmv's bits in both."""
    y0, layout = reference_variant(inst.unit, inst.kernel, inst.u, inst.w)
    if layout_key(info) != layout:
        return [] if inst.xd else [f"task layout {layout_key(info)}, the 32-bit columns' {layout}"]
    rows = case.special if inst.pad else np.ones(len(y), bool)
    if y[rows].tobytes() == y0[rows].tobytes():
        return []
    diff = np.flatnonzero(rows & (y != y0))
    return [f"bits differ from the reference variant on rows {diff[:8].tolist()} (lens {case.lens[diff[:8]].tolist()})"]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", lc.FORMATS)
@pytest.mark.parametrize("kernel", lc.KERNELS)
@pytest.mark.parametrize("unit", lc.UNITS)
def test_gpu_lattice(need_gpu, unit, kernel, fmt):
    insts = [i for i in lc.offered(unit) if i.kernel == kernel and i.fmt == fmt]
    assert len(insts) == 14 * len(lc.offered_shapes(kernel, fmt, 0)) + 14 * len(lc.offered_shapes(kernel, fmt, 1))
    failures = []
    for inst in insts:
        req = lc.request(inst)
        case, y, info = run_request(unit, req)
        bad = check_info(info, full_expect(inst, req, case))
        if not bad:  # a handle that fell back ran another instantiation: not counted
            RAN.add(tuple(inst))
            bad = check_y(case, y) + check_identity(inst, case, y, info)
        failures += [f"{inst}: {b}" for b in bad]
    assert not failures, f"{len(failures)} failures, first: " + "\n".join(failures[:10])


@pytest.mark.gpu
@pytest.mark.parametrize("unit", lc.UNITS)
def test_gpu_slices(need_gpu, unit):
    """The four slice kernels, through STREAM's groups and the aligned CSR3
    tasks: every row is serial, so every row is omp_spmv's bits."""
    failures = []
    for inst in lc.offered_slices(unit):
        for path in ("stream", "csr3"):
            req = lc.slice_request(inst, path)
            expect = dict(req.expect)
            expect.setdefault("slice_pos_bits", lc.host_slice_bits(unit, req)[0])
            case, y, info = run_request(unit, req)
            assert case.serial.all()
            bad = check_info(info, expect)
            if not bad:
                RAN.add((unit, inst.nt, info["slice_pos_bits"]))
                bad = check_y(case, y)
                if y[case.lens == 0].any():
                    bad.append("an empty row is not 0")
            failures += [f"{inst} via {path}: {b}" for b in bad]
    assert not failures, "\n".join(failures[:10])


@pytest.mark.gpu
def test_gpu_every_reachable_instantiation_ran(need_gpu):
    """The set of tuples run equals the reachable set: all that are offered,
    14 * 90 + 4 per unit."""
    if not RAN:
        pytest.skip("run with the module's other tests: nothing has run in this process")
    reachable = set()
    for unit in lc.UNITS:
        reachable |= {tuple(i) for i in lc.offered(unit)} | {tuple(i) for i in lc.offered_slices(unit)}
    assert RAN <= reachable
    missing = sorted(reachable - RAN, key=str)
    assert not missing, f"{len(missing)} reachable instantiations did not run, first: {missing[:10]}"
    for unit in lc.UNITS:
        assert sum(1 for t in RAN if t[0] == unit) == 14 * 90 + 4, unit

