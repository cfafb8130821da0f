// hspmv_plan.cpp -- the launch planner: which kernel runs a shard and in what
// shape (host only; the kernels are in spmv_kernels.hip, stream_f32/f64.hip
// and csort.hip, the tables the plan is finished from in hspmv_tables.cpp
// build_plan_tables).
#include "hspmv.h"
#include "hspmv_internal.h"

namespace hspmv {
namespace {

constexpr int kWave = 64;

int floor_pow2(double v) {
  int p = 1;
  while (p * 2 <= v && p < 64) p *= 2;
  return p;
}

// Elements per lane per LDS chunk.  Measured on MI355X (profiles/r01_sweep*):
// the chunk must stay small enough for 8 waves/SIMD (U = 4: 62 VGPRs fp64),
// and a 64-row group that fits one chunk of U <= 6 should be done in one.
// fp32 (profiles/r01_ab_f32_u.jsonl): two chunks of U = 6 beat U = 8 on C4's
// 640-nonzero groups (34.3 vs 40.2 us), and long groups take U = 16 (C3's
// 27-point rows: 62.3 vs 67.4 us) -- except on x-slab passes, where U = 8
// measured best (C5: 273 vs 291 us, r01_ab_c5_slabs_u.jsonl).
int pick_u(double nnz_per_pass, int dtype, bool slabs) {
  if (nnz_per_pass <= 128.0) return 2;
  if (nnz_per_pass <= 192.0) return 3;
  if (nnz_per_pass <= 256.0) return 4;
  // 5-nonzero rows fill U = 5 exactly (C2 14.76 -> 14.28 us, l4k 208 -> 199;
  // profiles/r01_ab_u5.jsonl)
  if (nnz_per_pass <= 320.0) return 5;
  if (nnz_per_pass <= 384.0) return 6;
  // two chunks, as full as possible: C4's 640-nonzero groups take 2 x 320
  // (U = 5: fp64 51.1 -> 50.2 us, fp32 35.0 -> 33.0; r01_ab_u5.jsonl)
  if (nnz_per_pass <= 768.0) {
    const int u = (int)((nnz_per_pass + 127.0) / 128.0);
    return u <= 4 ? 4 : (u == 5 ? 5 : 6);
  }
  if (dtype == HSPMV_F64) return 4;
  return slabs ? 8 : 16;
}

}  // namespace

LaunchPlan plan_launch(const DevCSR &A, int dtype, int val_dtype, unsigned flags, double rows_per_ssr,
                       int64_t packed_tasks, const Tuning &t) {
  LaunchPlan p;
  const unsigned k = flag_kernel(flags);
  p.nontemporal = (flags & HSPMV_FLAG_NONTEMPORAL) != 0;
  p.prefetch = (flags & HSPMV_FLAG_PREFETCH) != 0;
  // (with x slabs each pass sees ~d / n_slabs per row, but the chunk size
  // is still picked from d: U = 8 over U = 4/6 on C5's slab passes, 284 vs
  // 320 us -- more gathers in flight per wave; profiles/r01_ab_c5_slabs_u.jsonl)
  const double d = A.m ? (double)A.nnz / (double)A.m : 0.0;
  // XCD block order: a contiguous eighth of the rows per XCD keeps x in that
  // XCD's L2, which pays when the matrix is served from the Infinity Cache;
  // from HBM the dispatch order (the whole chip on one compact window)
  // streams 3-8 % faster (profiles/r01_sweep2-4: C2 full remap 15.6 vs
  // 16.9 us; C3 132 vs 128, C4 70.6 vs 65.4).  Chunked orders in between:
  // xcd_chunk_remap in hspmv_internal.h.
  // sv: bytes of an x entry; sval: of a stored value (a mixed handle: 8 and 4)
  const double sv = dtype == HSPMV_F64 ? 8.0 : 4.0;
  const double sval = val_dtype == HSPMV_F64 ? 8.0 : 4.0;
  const bool resident = mall_resident(A.m, A.n, A.nnz, dtype, val_dtype);
  bool full = false;
  int32_t chunk = 1;
  if (flag_xcd_chunk(flags))
    chunk = flag_xcd_chunk(flags);
  else if (flags & HSPMV_FLAG_NO_XCD_REMAP)
    chunk = 1;
  else if (flags & HSPMV_FLAG_XCD_REMAP)
    full = true;
  else if (resident)
    full = true;
  else if (A.has_xdict || A.has_xdict_tasks)
    // x dictionaries: each XCD takes 4 consecutive workgroups in turn, so the
    // x runs neighbouring workgroups stage are still in that XCD's L2
    // (C3 CSR-3 fp64 112.7 -> 105.2 us, fp32 63.7 -> 62.6; 2 / 8 / 16 / 64
    // blocks: 112.3 / 105.8 / 109.4 / 109.6; profiles/r02k_ab_xcd.jsonl)
    chunk = 4;
  // (packed tasks without super-super-rows: a CSR matrix whose 64-row
  // groups exceed the task budget, hspmv_tables.cpp build_tasks)
  const bool tasks = A.n_ssr > 0 || packed_tasks > 0;
  if (k == kAuto)
    p.kernel = A.has_csort ? kCsort : (tasks && !A.slab_stream ? kCsr3 : kStream);
  else
    p.kernel = (int)k;
  if (p.kernel == kCsort && !A.has_csort) p.kernel = tasks ? kCsr3 : kStream;
  if (p.kernel == kCsr3 && !tasks) p.kernel = kStream;
  const int forced_u = flag_u(flags);
  switch (p.kernel) {
    case kCsort:  // the workgroup shape is fixed; the host tables hold the rest
      p.lanes = kWave;
      p.waves_per_block = kCsortThreads / kWave;
      p.blocks = 0;  // set from the tables (build_plan_tables)
      break;
    case kStream: {
      p.lanes = kWave;
      p.u = forced_u ? forced_u : pick_u(64.0 * (d < kLongRow ? d : kLongRow), dtype, A.n_slabs > 1);
      const int64_t tasks = ((int64_t)A.m + kWave - 1) / kWave;
      p.groups = flag_groups(flags);
      const int64_t waves = (tasks + p.groups - 1) / p.groups;
      // waves per workgroup.  The STREAM waves never meet at a barrier, so
      // small workgroups free their CU slots wave by wave: one wave per
      // workgroup for Infinity-Cache-resident matrices (C2 bench 737 -> 760
      // GFLOP/s), two for HBM-resident ones, where one-wave workgroups run
      // into the per-CU workgroup limit (honeycomb 166.0 -> 161.8 us with
      // two, flat with one; l4k 211.2 -> 207.5; profiles/r01_ab_stream_w.jsonl).
      // LDS-windowed HBM matrices took one wave until r04 (C4 53.2 -> 50.4
      // us in r01); on today's kernel two measure 47.1 vs 47.7-48.0 on C4's
      // 8-rank shard and tie at 4 / 2 / 1 ranks (profiles/r04/
      // sweep_stream_waves.jsonl, 7 rounds, one process).  Four (the
      // dictionaries' 256-row blocks) with x dictionaries.
      p.waves_per_block = A.has_xdict ? 4 : (resident ? 1 : 2);
      if ((t.stream_waves == 1 || t.stream_waves == 2 || t.stream_waves == 4) && !A.has_xdict)
        p.waves_per_block = t.stream_waves;
      p.blocks = (waves + p.waves_per_block - 1) / p.waves_per_block;
      break;
    }
    case kCsr3: {
      p.lanes = kWave;
      double rows_per_task;
      if (packed_tasks > 0) {  // host-planned wave tasks: task_waves per block
        p.waves_per_block = (A.task_waves == 1 || A.task_waves == 2 || A.task_waves == 8) ? A.task_waves : 4;
        rows_per_task = (double)A.m / (double)packed_tasks;
        p.blocks = (packed_tasks + p.waves_per_block - 1) / p.waves_per_block;
      } else {
        // ~64 rows per wave (one lane per row in the ordered sums)
        p.waves_per_block = ssr_waves(rows_per_ssr);
        rows_per_task = rows_per_ssr / p.waves_per_block;
        p.blocks = A.n_ssr;
      }
      const double per_pass = (rows_per_task < 64.0 ? rows_per_task : 64.0) * d;
      p.u = forced_u ? forced_u : pick_u(per_pass < 64.0 * kLongRow ? per_pass : 64.0 * kLongRow, dtype, A.n_slabs > 1);
      break;
    }
  }
  // The STREAM / CSR3 kernels address x and the matrix streams as a 64-bit
  // base plus a 32-bit byte offset (dev_prims.cuh ld_off): x of 4 GiB or
  // more (fp64: n >= 2^29), or -- without split rows -- a row group that
  // could stream 4 GiB, would wrap.  Such matrices take a kernel that
  // indexes through pointers: csort when it was built, else VECTOR.
  const double max_run_bytes =
      (flags & HSPMV_FLAG_NO_SPLIT) ? (double)A.nnz * (sval > 4.0 ? sval : 4.0) : 64.0 * kLongRow * sval;
  if ((p.kernel == kStream || p.kernel == kCsr3) &&
      ((double)A.n * sv > 4294967295.0 || max_run_bytes > 4294967295.0))
    p.kernel = A.has_csort ? kCsort : kVector;
  if (p.kernel == kVector) {
    // lanes per row: HSPMV_LANES(l) when the caller asked for this kernel,
    // else (and for a matrix sent here by the addressing rule) from the mean
    // row length
    int lanes = k == kVector ? flag_lanes(flags) : 0;
    if (lanes == 0) lanes = floor_pow2(d < 2.0 ? 2.0 : d);
    p.lanes = lanes;
    const int64_t blocks = ((int64_t)A.m * lanes + 255) / 256;
    const int64_t cap = 256LL * 8 * 16;  // grid-stride beyond 16 waves/SIMD
    p.blocks = blocks < cap ? blocks : cap;
    if (p.blocks < 1) p.blocks = 1;
  }
  if (p.kernel == kVector || p.kernel == kCsort) {
    full = false;
    chunk = 1;  // dispatch order (csort: the column parts alternate XCDs)
  }
  if (full) {
    const int64_t per_xcd = p.blocks / 8;
    chunk = per_xcd > 1 ? (int32_t)per_xcd : 1;
  }
  p.xcd_chunk = chunk;
  // HBM-resident matrices: nontemporal y stores; and nontemporal col/val
  // streams when the x gather is irregular (column spans of 2^18+ per
  // 256-nonzero block) and x exceeds an XCD's 4 MiB L2, so the streamed
  // bytes do not evict x (C5: -5 %; banded C3/C4: +3-7 %, left off).
  // HSPMV_YNT / HSPMV_NT (0/1) override, for A/B runs.
  p.y_nt = !resident;
  // (not on x-slab passes, whose gathers are L2-resident anyway: C5 284 ->
  // 265 us with plain loads, profiles/r01_ab_nt_slabs.jsonl)
  if (!p.nontemporal && !resident && A.col_span_bits > 17 && (double)A.n * sv > kXcdL2Bytes &&
      A.n_slabs <= 1)
    p.nontemporal = true;
  // fp64 CSR3 tasks with x dictionaries: the next chunk's col/val loads are
  // issued during this chunk's gathers and sums (C3 112.2 -> 105.8 us on one
  // box, 112.4 -> 110.3 on another; slower everywhere else: C3 fp32 +14 %,
  // C4 +13 %, honeycomb +10 %, C2 +14 %; profiles/r02q_ab_c3_u.jsonl,
  // r02r_ab_pf.jsonl)
  // (not the slice kernel, hspmv_slices: it has one pipeline of its own)
  if (!p.prefetch && dtype == HSPMV_F64 && p.kernel == kCsr3 && A.has_xdict_tasks && !forced_u && !A.has_slices)
    p.prefetch = true;
  // Bank-padded product buffers (STREAM, no prefetch): when
  // the typical serially summed row is a multiple of 16 LDS words long
  // (fp32 rows of 16 / 32, fp64 rows of 8 / 16 / 24 / 32 ...), the lanes
  // walking those rows hit at most two banks.  Dense 32x32 blocks: fp64
  // 129.6 -> 95.1 us, fp32 99.6 -> 67.1; fp64 rows of 24: 103.2 -> 95.9;
  // fp32 rows of 24 (8-word multiples) lose 3 % padded, so they are left
  // alone (profiles/r05j/ab_lds_pad.jsonl).  Decided after the A/B
  // overrides, so that hspmv_info.lds_pad reports the launch that runs (the
  // PF variant has no padded form).  Never with x dictionaries: those are
  // sized (hspmv_xdict.cpp xd_target_entries) against unpadded product
  // buffers, and the pad would cost the launch a workgroup per CU.
  if (t.pf >= 0) p.prefetch = t.pf != 0;  // A/B knobs (diagnostic builds only)
  if (t.y_nt >= 0) p.y_nt = t.y_nt != 0;
  if (t.nt >= 0) p.nontemporal = t.nt != 0;
  {
    const int words = A.serial_len * (dtype == HSPMV_F64 ? 2 : 1);
    const bool conflicting = words > 0 && (words % 16) == 0;
    const bool can_pad = p.kernel == kStream && !p.prefetch && !A.has_xdict;
    p.lds_pad = can_pad && conflicting;
    if (t.lds_pad >= 0) p.lds_pad = can_pad && t.lds_pad > 0;
  }
  p.dyn_lds = t.dyn_lds;
  return p;
}

}  // namespace hspmv
