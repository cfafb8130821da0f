// row_kernels.cuh -- the row kernels hspmv_csr_stream and hspmv_csr3 and the
// wave routine they share (wave_rows), instantiated per dtype by the units
// stream_f32.hip / stream_f64.hip / stream_f32v64.hip through row_launch.cuh.
// Device code only.
//
// The hot path of the reference is the row-wise nonzero dot product
//   y[r] = sum_{k=rp[r]}^{rp[r+1]-1} val[k] * x[col[k]]
// (spmv-csr/spmv.c:92-114; GPU forms cuda-spmv-csr/spmv.cu:117-182 and
// cuda-spmv-csrk/hip/csrk.cu:185-390).  It is an HBM-bound gather: 2 flops per
// 12 B (fp64) / 8 B (fp32) of matrix stream, so no MFMA anywhere here.
//
// Both kernels are wave64-native: one wavefront per group of <= 64
// consecutive rows.  The group's nonzeros are contiguous, so the wave streams
// them with fully coalesced loads (U elements per lane per chunk), forms the
// products val*x[col] and stages them in a per-wave LDS slice.  Then
//   - rows of <= serial_max nonzeros: lane i sums row i left to right.
//     Summation order and rounding (product rounded, then sum rounded,
//     starting from 0) are those of omp_spmv, so these rows are BIT-IDENTICAL
//     to the CPU reference;
//   - longer rows: the whole wave sums the row's products in the chunk (DPP
//     tree), accumulated over chunks (fp64 tolerance);
//   - split rows (> long_t nonzeros) are skipped here and summed by the
//     split-row kernels of spmv_kernels.hip.
// The serial bound is an argument (DevPlan.serial_max): kSerialMax
// (hspmv_internal.h), or INT32_MAX for hspmv_options.deterministic = 3, where
// every row is summed serially -- omp_spmv's order for every row.
//
// Blocks are remapped so each of the 8 XCDs (private 4 MiB L2 each) gets a
// contiguous range of row groups: neighbouring rows share x[] lines and the
// edges of val/col lines, which then hit in one L2 instead of eight.  Every
// other SpMV of a handle whose matrix exceeds the Infinity Cache runs that
// order mirrored, last block first (xcd_chunk_remap / sweep_block,
// hspmv_internal.h, shared with the host; hspmv_set_sweep), and so begins on
// the bytes the cache still holds.
#pragma once
#include "dev_diag.cuh"
#include "hspmv_internal.h"

namespace hspmv {
namespace dev {

#ifndef HSPMV_COOP_GROUPS
#define HSPMV_COOP_GROUPS 1
#endif

// PAD: a wave's product buffer holds chunk position i at lds_ix(i) = i + i /
// 32 -- one pad element per 32 -- so that the lanes of an ordered sum, each
// walking its own row with rows one row length apart, do not meet in one
// LDS bank.  Rows of 32 nonzeros put every lane of a chunk on one bank
// (fp32 32-way; fp64 8-way per 256-nonzero chunk), and the ordered sums were
// 40 % of the dense-32x32-block matrix's time (HSPMV_DIAG 1 ablation,
// profiles/r05h/ab_blocks32_ablation.jsonl).  The index math and the bigger
// buffer cost latency and LDS elsewhere (C3 fp32 +8 %, C4 fp32 +8 % with
// padding everywhere, profiles/r05j/ab_lds_pad.jsonl), so the planner pads
// only STREAM launches whose rows are conflicting (LaunchPlan.lds_pad).
template <bool PAD>
__device__ __forceinline__ int32_t lds_ix(int32_t i) { return PAD ? i + (i >> 5) : i; }
template <int U, bool PAD>
constexpr int wave_lds() {  // elements of one wave's product buffer
  return kWave * U + (PAD ? 2 * U : 0);
}

// Ordered sum of lds[lo..hi) into acc, left to right: the LDS reads are
// issued 4 at a time (one LDS latency per 4 nonzeros instead of per nonzero),
// the last 1-3 together (C4's 10-nonzero rows: 54.2 -> 51.7 us,
// profiles/r01_ab_ordered_sum_tail.jsonl), but the additions stay in
// sequence, so the rounding is omp_spmv's.
// (An 8-wide batch for the dictionary kernels measured flat on C3, -0.4 %;
// 8-wide clamped batches everywhere slower: C3 +13 %, honeycomb +5 %.)
// lds holds chunk position i (nonzero c + i) at lds_ix(i).
template <bool PAD, typename T>
__device__ __forceinline__ T ordered_sum(T acc, const T *lds, int32_t c, int32_t lo, int32_t hi) {
  int32_t k = lo;
  for (; k + 4 <= hi; k += 4) {
    const T a0 = lds[lds_ix<PAD>(k - c)], a1 = lds[lds_ix<PAD>(k + 1 - c)], a2 = lds[lds_ix<PAD>(k + 2 - c)],
            a3 = lds[lds_ix<PAD>(k + 3 - c)];
    acc = acc + a0;
    acc = acc + a1;
    acc = acc + a2;
    acc = acc + a3;
  }
  if (k < hi) {  // the last 1-3 in one LDS round trip (clamped reads, selected adds)
    const T a0 = lds[lds_ix<PAD>(k - c)], a1 = lds[lds_ix<PAD>(min(k + 1, hi - 1) - c)],
            a2 = lds[lds_ix<PAD>(min(k + 2, hi - 1) - c)];
    acc = acc + a0;
    if (k + 1 < hi) acc = acc + a1;
    if (k + 2 < hi) acc = acc + a2;
  }
  return acc;
}

// Row bounds of a 64-row group for this lane (0, 0 past g1).  Issued one
// group ahead by the kernels, so a wave's next col/val loads never wait on
// a row-pointer round trip.
__device__ __forceinline__ void group_bounds(const int32_t *__restrict__ rp, int32_t g0,
                                             int32_t g1, int lane, int32_t &beg, int32_t &end) {
  const int32_t row = g0 + lane;
  const bool valid = row < g1;
  beg = valid ? rp[row] : 0;
  end = valid ? rp[row + 1] : 0;
}

// Where a row kernel reads column indices from (DevCSR's col_idx, or the
// 16-bit offsets + block bases + high-bit planes of the col16 format).
struct ColSrc {
  const int32_t *ci;
  const uint16_t *c16;
  const int32_t *cbase;
  const uint64_t *cplanes;
  int32_t n_planes, plane_words;
};

// x window of a STREAM group (XW): x[lo, lo + w) staged in the wave's LDS
// slot `xs`, so the group's gathers are LDS reads; w == 0: global gathers.
template <typename T>
struct XWin {
  const T *xs;
  int32_t lo, w;
};

// The column of the run's element j (byte stream cb, the run starting at
// nonzero kb), in one of the four column formats; XD: its position in the
// block's dictionary instead.  j0: the element the instruction's lane 0 reads
// (wave-uniform).
template <bool NT, int C16, bool XD>
__device__ __forceinline__ int32_t load_col(const ColSrc &cs, const gchar *cb, int32_t kb, int32_t gbase,
                                            uint32_t j, uint32_t j0) {
  if constexpr (XD && diag(kDiagPos8)) {
    return (int32_t)ld_off<NT, uint8_t>(cb, j);  // ablation: 1-byte positions (wrong x)
  } else if constexpr (XD) {
    return (int32_t)ld_off<NT, uint16_t>(cb, j * 2u);  // position in the block's xs
  } else if constexpr (C16 == 2) {
    // group-base offsets: col = the 64-row group's smallest column
    // + 16-bit offset (one scalar load per group, one add here)
    return gbase + (int32_t)ld_off<NT, uint16_t>(cb, j * 2u);
  } else if constexpr (C16 == 1) {
    // col = base of the nonzero's 256-block + 16-bit offset.  The 64
    // lanes of a slice lie in at most two consecutive blocks: one
    // scalar load brings both bases (s_load, no vector memory op)
    const uint32_t e0 = (uint32_t)kb + j0;
    const uint32_t ja = (uint32_t)kb + j;
    const uint32_t b0 = __builtin_amdgcn_readfirstlane(e0 >> kC16Shift);
    const int64_t bp = sload<int64_t>(cs.cbase, (uint64_t)b0 * 4u);
    const int32_t base = ((ja >> kC16Shift) == b0) ? (int32_t)bp : (int32_t)(bp >> 32);
    int32_t high = 0;
    if (cs.n_planes > 0) {  // wave-uniform; the two words a slice spans, by s_load
      const uint32_t w0 = __builtin_amdgcn_readfirstlane(e0 >> 6);
      const bool first = (ja >> 6) == w0;
      for (int p = 0; p < cs.n_planes; ++p) {
        const uint64_t at = ((uint64_t)p * (uint64_t)cs.plane_words + w0) * 8u;
        const uint64_t m0 = (uint64_t)sload<int64_t>(cs.cplanes, at);
        const uint64_t m1 = (uint64_t)sload<int64_t>(cs.cplanes, at + 8u);
        high |= (int32_t)(((first ? m0 : m1) >> (ja & 63u)) & 1u) << p;
      }
    }
    return base + (int32_t)ld_off<NT, uint16_t>(cb, j * 2u) + (high << 16);
  } else {
    return ld_off<NT, int32_t>(cb, j * 4u);
  }
}

// The cooperative rows cm of the chunk [c, c + last] (cm is left empty), one
// row at a time by the whole wave (bounds by readlane: scalar).
template <bool PAD, typename T>
__device__ __forceinline__ T coop_sums_by64(T acc, unsigned long long &cm, const T *lds, int32_t c,
                                            int32_t last, int32_t beg, int32_t end, int lane) {
  while (cm) {
    const int r = __ffsll(cm) - 1;
    cm &= cm - 1;
    const int32_t lo = max(__builtin_amdgcn_readlane(beg, r), c);
    const int32_t hi = min(__builtin_amdgcn_readlane(end, r), c + last + 1);
    if (lo < hi) {  // wave-uniform
      T s = T(0);
      for (int32_t k = lo + lane; k < hi; k += kWave) s += lds[lds_ix<PAD>(k - c)];
      s = wave_sum_dpp(s);
      if (lane == r) acc += s;
    }
  }
  return acc;
}

// y[row] = acc for the lanes that are `live`.  y_nt (HBM-resident y):
// streaming stores (bw_probe3/4: y writes cost ~20 % of time).
template <typename T>
__device__ __forceinline__ void store_y(T *y, int32_t row, T acc, bool live, bool y_nt) {
  if constexpr (diag(kDiagNoStore)) {  // ablation: no y stores (kept live)
    if (live && acc == T(12345.678)) y[row] = acc;
  } else if (live) {
    if (y_nt)
      __builtin_nontemporal_store(acc, y + row);
    else
      y[row] = acc;
  }
}

// One wavefront computes rows [g0, g1), g1 - g0 <= 64, whose bounds
// (group_bounds) are in beg/end; gbase (C16 == 2): the group's base column.
// Rows over long_t nonzeros are left to the split-row kernels, rows over
// serial_max are summed by the whole wave; carry (x slabs, passes after the
// first): the sums start from y.  lds: kWave*U elements private to this wave.
// (The arguments stay scalars: bundled in structs, by value or by reference,
// the kernels compile to other code.)
// Per chunk of 64*U nonzeros: stage A loads col/val (coalesced), stage B
// gathers x[col] (from the LDS window when XW and win.w > 0), stage C forms
// the products into LDS; then the row sums.  PF
// (software pipelining): the next chunk's stage A is issued between this
// chunk's stage B and C, so its latency overlaps the gather and the sums.
// TV: the type the values are stored and streamed in (T, or float under
// T = double: the mixed handles); each value is widened to T once, before its
// product, so the products and sums are T's.
template <typename T, bool NT, int U, bool PF, int C16, bool XW, bool XD, bool GROUPS, bool PAD = false,
          typename TV = T>
__device__ __forceinline__ void wave_rows(int32_t g0, int32_t g1, int32_t beg, int32_t end,
                                          int32_t long_t, int32_t serial_max, const ColSrc &cs,
                                          const TV *__restrict__ val, const T *__restrict__ x,
                                          T *__restrict__ y, T *lds, int lane,
                                          const XWin<T> &win, bool y_nt, bool carry,
                                          int32_t gbase, trace_t *ts = nullptr) {
  const int32_t row = g0 + lane;
  const bool valid = row < g1;
  const int32_t len = end - beg;
  (void)ts;
  (void)win;
  const bool skip = len > long_t;
  const unsigned long long skipmask = __ballot(valid && skip);
  const unsigned long long coopmask = __ballot(valid && !skip && len > serial_max);
  const bool serial = valid && !skip && len <= serial_max;
  const gchar *xb = uniform_ptr(x);
  const bool inwin = (XW && win.w > 0) || XD;
  // x slabs: passes after the first continue each row's sum from y, so a
  // row's products are still added left to right from 0 across the passes
  T acc = (carry && valid && !skip) ? y[row] : T(0);
  // Runs of consecutive non-split rows [a, b); normally one run = the group.
  int32_t a = g0;
  while (a < g1) {
    const unsigned long long rest = skipmask & bits_from(a - g0);
    const int32_t b = rest ? g0 + (__ffsll(rest) - 1) : g1;
    if (b > a) {
      const int32_t kb = __builtin_amdgcn_readfirstlane(__shfl(beg, a - g0, kWave));
      const int32_t ke = __builtin_amdgcn_readfirstlane(__shfl(end, b - 1 - g0, kWave));
      const int32_t n_run = ke - kb;
      const unsigned long long coop = coopmask & bits_from(a - g0) & ~bits_from(b - g0);
      const bool mine = serial && row >= a && row < b;
      int32_t col[U];
      TV v[U];
      const gchar *cb = (C16 || XD) ? uniform_ptr(cs.c16 + kb) : uniform_ptr(cs.ci + kb);
      const gchar *vb = uniform_ptr(val + kb);
      // (A raw-buffer form -- SGPR descriptors bounded to the run, no
      // clamp VALU -- measured 0-2.5 % slower in one-process A/B runs,
      // tools/ab.py, profiles/r01_ab_buffer_loads.jsonl.)
      auto stage_a = [&](int32_t c0, int32_t last) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          // clamp instead of branching: every load issues back to back
          const uint32_t j = (uint32_t)(c0 + min(u * kWave + lane, last));
          col[u] = load_col<NT, C16, XD>(cs, cb, kb, gbase, j, (uint32_t)(c0 + min(u * kWave, last)));
          v[u] = ld_off<NT, TV>(vb, j * (uint32_t)sizeof(TV));
        }
      };
      if constexpr (PF) {
        if (n_run > 0) stage_a(0, min(kWave * U, n_run) - 1);
      }
      for (int32_t c0 = 0; c0 < n_run; c0 += kWave * U) {
        const int32_t last = min(kWave * U, n_run - c0) - 1;
        if constexpr (!PF) stage_a(c0, last);
        if (c0 == 0) wave_trace_stamp(ts, lane, 2);
        T xv[U], vv[U];
        if (inwin) {
#pragma unroll
          for (int u = 0; u < U; ++u) {
            xv[u] = XD ? win.xs[col[u]] : win.xs[col[u] - win.lo];
            vv[u] = (T)v[u];
          }
        } else {
#pragma unroll
          for (int u = 0; u < U; ++u) {
            if constexpr (diag(kDiagNoGather))
              xv[u] = T(col[u] & 1) + T(1);
            else
              xv[u] = ld_off<false, T>(xb, (uint32_t)col[u] * (uint32_t)sizeof(T));
            vv[u] = (T)v[u];
          }
        }
        if constexpr (PF) {
          __builtin_amdgcn_sched_barrier(0);
          const int32_t cn = c0 + kWave * U;
          stage_a(cn < n_run ? cn : n_run - 1, cn < n_run ? min(kWave * U, n_run - cn) - 1 : 0);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (c0 == 0) wave_trace_stamp(ts, lane, 3);
#pragma unroll
        for (int u = 0; u < U; ++u) lds[lds_ix<PAD>(u * kWave + lane)] = vv[u] * xv[u];
        wave_sync();
        const int32_t c = kb + c0;
        if constexpr (diag(kDiagNoRowSums)) {
          if (mine && max(beg, c) < min(end, c + last + 1)) acc += lds[lds_ix<PAD>(max(beg, c) - c)];
        } else {
          if (mine) acc = ordered_sum<PAD>(acc, lds, c, max(beg, c), min(end, c + last + 1));
        }
        // only the cooperative rows this chunk touches (rows are contiguous:
        // the others would add nothing)
        unsigned long long cm = coop ? coop & __ballot(end > c && beg <= c + last) : 0ull;
        // three or more pieces (rows of 33..~100 nonzeros): four at a time,
        // one 16-lane DPP row each.  CSR3 kernel only -- the tasks that
        // mid-density CSR matrices run as (hspmv_tables.cpp build_tasks): in
        // the STREAM kernel the extra code cost the honeycomb matrix 4 %
        // (161 -> 168 us) with no such rows at all (r02z9).  d33 173 ->
        // 137 us, d48 132 -> 109, d64 103 -> 95 (profiles/r02z8).
        // (Left in place: as a function of its own, like coop_sums_by64, it
        // compiles to other code in the CSR3 kernels.)
        if (GROUPS && __popcll(cm) >= 3) {
          const int g = lane >> 4, gl = lane & 15;
          while (cm) {
            int rq[4];
            int32_t lq[4], hq[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              rq[q] = -1;
              lq[q] = 0;
              hq[q] = 0;
              if (cm) {  // wave-uniform
                rq[q] = __ffsll(cm) - 1;
                cm &= cm - 1;
                lq[q] = max(__builtin_amdgcn_readlane(beg, rq[q]), c);
                hq[q] = min(__builtin_amdgcn_readlane(end, rq[q]), c + last + 1);
              }
            }
            const int32_t lo = g == 0 ? lq[0] : (g == 1 ? lq[1] : (g == 2 ? lq[2] : lq[3]));
            const int32_t hi = g == 0 ? hq[0] : (g == 1 ? hq[1] : (g == 2 ? hq[2] : hq[3]));
            T s = T(0);
            for (int32_t k = lo + gl; k < hi; k += 16) s += lds[lds_ix<PAD>(k - c)];
            s = row16_sum_dpp(s);
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (rq[q] >= 0) {  // wave-uniform
                const T t = lane_value(s, 16 * q + 15);
                if (lane == rq[q]) acc += t;
              }
          }
        }
        acc = coop_sums_by64<PAD>(acc, cm, lds, c, last, beg, end, lane);
        wave_sync();
        if (c0 == 0) wave_trace_stamp(ts, lane, 4);
        if (c0 + kWave * U >= n_run) wave_trace_put(ts, lane, 7, (trace_t)(c0 / (kWave * U) + 1));
      }
    }
    a = b + 1;
  }
  wave_trace_stamp(ts, lane, 5);
  store_y(y, row, acc, valid && !skip, y_nt);
}

// Stages x[lo, lo + w) (w <= kXWin) into the wave's LDS window slot.  The
// loads are contiguous (coalesced), unlike the gathers they replace.
template <typename T>
__device__ __forceinline__ void stage_xwin(T *xs, const T *__restrict__ x, int32_t lo, int32_t w,
                                           int lane) {
  const gchar *xb = uniform_ptr(x + lo);
  T t[kXWin / kWave];
#pragma unroll
  for (int i = 0; i < kXWin / kWave; ++i) {
    const int32_t e = min(i * kWave + lane, w - 1);
    t[i] = ld_off<false, T>(xb, (uint32_t)e * (uint32_t)sizeof(T));
  }
#pragma unroll
  for (int i = 0; i < kXWin / kWave; ++i) xs[i * kWave + lane] = t[i];
  wave_sync();
}

// Block x dictionary (XD): the x entries a workgroup's rows reference,
// as runs of consecutive columns.  blk[b], blk[b+1] bound block b's records
// in runs: {x_start, lds_off} per run, then a sentinel {0, total}; run i
// stages x[x_start, x_start + len) at xs[lds_off ...], len = the next
// record's lds_off - lds_off.  The col stream then holds each nonzero's
// 16-bit position in xs (the host builds both, hspmv_xdict.cpp build_xdict).
struct XDict {
  const int32_t *blk;
  const int2 *runs;
};

// The workgroup stages its dictionary into xs (NTH threads, contiguous loads
// per run instead of one gather per nonzero) and waits at a block barrier.
// Every wave of the block must call this (before any early return).
template <typename T, int NTH>
__device__ __forceinline__ void stage_xdict(T *xs, const T *__restrict__ x, const XDict &xd,
                                            int64_t blk, int tid) {
  constexpr int kBatch = 8;
  if constexpr (diag(kDiagNoStaging)) return;
  if constexpr (diag(kDiagBarrierOnly)) {
    __syncthreads();
    return;
  }
  if constexpr (diag(kDiagStagePrio3)) __builtin_amdgcn_s_setprio(3);
  if constexpr (diag(kDiagStagePrio1)) __builtin_amdgcn_s_setprio(1);
  const int64_t rr = sload<int64_t>(xd.blk, (uint64_t)blk * 4u);
  const int32_t r0 = (int32_t)rr;
  const int32_t nr = (int32_t)(rr >> 32) - r0 - 1;  // runs (<= 63), then the sentinel
  const int lane = tid & (kWave - 1);
  int2 rec = make_int2(0, 0);
  if (nr >= 0 && lane <= nr) rec = xd.runs[r0 + lane];
  const int32_t total = nr >= 0 ? __builtin_amdgcn_readlane(rec.y, nr) : 0;
  const int32_t delta = rec.x - rec.y;  // x index = xs index + delta inside the run
  const gchar *xb = uniform_ptr(x);
  for (int32_t e0 = 0; e0 < total; e0 += NTH * kBatch) {  // block-uniform
    int32_t e[kBatch], d[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      e[j] = e0 + j * NTH + tid;
      d[j] = 0;
    }
    for (int r = 0; r < nr; ++r) {  // runs are sorted by lds_off: the last run starting <= e
      const int32_t o = __builtin_amdgcn_readlane(rec.y, r);
      const int32_t dl = __builtin_amdgcn_readlane(delta, r);
#pragma unroll
      for (int j = 0; j < kBatch; ++j) d[j] = e[j] >= o ? dl : d[j];
    }
    T v[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j)
      v[j] = ld_off<false, T>(xb, (uint32_t)(min(e[j], total - 1) + d[j]) * (uint32_t)sizeof(T));
#pragma unroll
    for (int j = 0; j < kBatch; ++j)
      if (e[j] < total) xs[e[j]] = v[j];
  }
  __syncthreads();
  if constexpr (diag(kDiagStagePrio3 | kDiagStagePrio1)) __builtin_amdgcn_s_setprio(0);
}

// Where a wave's gathers read x: the block's dictionary (XD, xdyn), or the x
// window xwin[idx] = {lo, w} of the wave's group or task (XW), staged here in
// the wave's slot of xlds when it fits (w > 0); neither: x itself.
template <bool XW, bool XD, typename T>
__device__ __forceinline__ XWin<T> x_source(const unsigned char *xdyn, T *xlds, const int2 *xwin, int64_t idx,
                                            const T *x, int wid, int lane) {
  XWin<T> win{XD ? reinterpret_cast<const T *>(xdyn) : nullptr, 0, 0};
  if constexpr (XW) {
    const int64_t wv = sload<int64_t>(xwin, (uint64_t)idx * 8u);
    win.lo = (int32_t)wv;
    win.w = (int32_t)(wv >> 32);
    win.xs = xlds + wid * kXWin;
    if (win.w > 0) stage_xwin(xlds + wid * kXWin, x, win.lo, win.w, lane);
  }
  return win;
}

// STREAM (HSPMV_KERNEL_STREAM, the default for CSR): wave w walks `groups`
// consecutive 64-row groups starting at row w * groups * 64, loading the next
// group's row pointers before streaming the current one.  XW: groups whose x
// window (xwin[g] = {lo, w}) fits kXWin entries gather from an LDS copy of
// it.  Replaces cuda_spmv's thread-per-row scalar loop (uncoalesced) with a
// CSR-stream scheme (coalesced stream + LDS segmented sums).
template <typename T, bool NT, int U, bool PF, int C16, bool XW, bool XD, int W = 4, bool PAD = false,
          typename TV = T>
__global__ __launch_bounds__(W * 64) void hspmv_csr_stream(
    int32_t m, int32_t long_t, int32_t serial_max, uint32_t blk_order, int32_t groups, int32_t y_nt,
    int32_t carry,
    const int32_t *__restrict__ rp, ColSrc cs, const int2 *__restrict__ xwin, XDict xd,
    const TV *__restrict__ val, const T *__restrict__ x, T *__restrict__ y) {
  static_assert(!XD || W == 4, "dictionaries are planned for 256-row blocks");
  __shared__ T lds[W * wave_lds<U, PAD>()];
  __shared__ T xlds[XW ? W * kXWin : 1];
  extern __shared__ __attribute__((aligned(16))) unsigned char xdyn[];  // XD: the block's xs
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t blk = sweep_block(blockIdx.x, gridDim.x, blk_order);
  // XD (groups == 1): the block's 256 rows share one staged dictionary; the
  // only block barrier of the kernel is at the end of the staging.
  if constexpr (XD) stage_xdict<T, 256>(reinterpret_cast<T *>(xdyn), x, xd, blk, threadIdx.x);
  int64_t g0 = (blk * W + wid) * (int64_t)groups * kWave;
  if (g0 >= m) return;  // wave-uniform
  const int64_t gend = min<int64_t>(g0 + (int64_t)groups * kWave, m);
  T *my = lds + wid * wave_lds<U, PAD>();
  trace_t *ts = trace_slots<kDiagWaveTrace>(blk * W + wid);
  wave_trace_stamp(ts, lane, 0);
  wave_trace_hw_id(ts, lane, 6);
  int32_t beg, end;
  group_bounds(rp, (int32_t)g0, (int32_t)min<int64_t>(g0 + kWave, gend), lane, beg, end);
  wave_trace_stamp(ts, lane, 1);
  while (true) {
    const int32_t g1 = (int32_t)min<int64_t>(g0 + kWave, gend);
    const XWin<T> win = x_source<XW, XD>(xdyn, xlds, xwin, g0 / kWave, x, wid, lane);
    int32_t nbeg = 0, nend = 0;
    if (g1 < gend) group_bounds(rp, g1, (int32_t)min<int64_t>(g1 + kWave, gend), lane, nbeg, nend);
    int32_t gbase = 0;
    if constexpr (C16 == 2) gbase = (int32_t)sload<int64_t>(cs.cbase, (uint64_t)(g0 / kWave) * 4u);
    wave_rows<T, NT, U, PF, C16, XW, XD, false, PAD, TV>(
        (int32_t)g0, g1, beg, end, long_t, serial_max,  // the group and its rows' bounds, the row-length rules
        cs, val, x, y, my, lane, win,                   // the streams, this wave's LDS, its x source
        y_nt != 0, carry != 0, gbase, ts);
    ts = nullptr;  // trace the first group only
    if (g1 >= gend) break;
    g0 = g1;
    beg = nbeg;
    end = nend;
  }
}

// CSR3 (HSPMV_KERNEL_CSR3): wave tasks planned on the host, W per workgroup:
// 64-row aligned groups by default (cache-line-aligned y stores), super-rows
// packed into <= 64-row tasks (HSPMV_TASK_FILL=0), or one workgroup of W
// waves per super-super-row whose super-rows are split W ways by nonzeros
// (HSPMV_CSR3_PLAN=ssr); each wave runs wave_rows over its task
// (hspmv_tables.cpp build_tasks).  Replaces cuSpMV_3 / cuSpMV_3_vec (thread
// or sub-warp per row inside (8,12)-thread blocks, csrk.cu:185-319) and
// cuSpMV_2 (degenerate outer level).
template <typename T, bool NT, int U, bool PF, int C16, int W, bool XW, bool XD, typename TV = T>
__global__ __launch_bounds__(W * 64) void hspmv_csr3(
    int32_t n_tasks, int32_t long_t, int32_t serial_max, uint32_t blk_order, int32_t y_nt, int32_t carry,
    int32_t align,
    const int32_t *__restrict__ task_start, const int2 *__restrict__ xwin, XDict xd,
    const int32_t *__restrict__ rp, ColSrc cs, const TV *__restrict__ val,
    const T *__restrict__ x, T *__restrict__ y) {
  __shared__ T lds[W * wave_lds<U, false>()];
  __shared__ T xlds[XW ? W * kXWin : 1];
  extern __shared__ __attribute__((aligned(16))) unsigned char xdyn[];  // XD: the block's xs
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t blk = sweep_block(blockIdx.x, gridDim.x, blk_order);
  trace_t *bt = block_trace_begin(blk);
  // XD: the W packed tasks of the block share one staged dictionary (loads
  // of the task / row bounds and of the first chunk issued ahead of the
  // staging measured -0.3 ... -0.6 % and cost 20 VGPRs: profiles/r05c,
  // r05d; removed)
  if constexpr (XD) stage_xdict<T, W * 64>(reinterpret_cast<T *>(xdyn), x, xd, blk, threadIdx.x);
  const int64_t t = blk * W + wid;
  if (t >= n_tasks) return;
  const trace_t t_start = wave_trace_now();
  // both task bounds in one scalar load (K$), not a vector round trip
  const int64_t tb = sload<int64_t>(task_start, (uint64_t)t * 4u);
  const int32_t r0 = (int32_t)tb;
  const int32_t r1 = (int32_t)(tb >> 32);
  if (r0 >= r1) return;
  T *my = lds + wid * wave_lds<U, false>();
  // group-base columns: one base per packed task
  int32_t gbase = 0;
  if constexpr (C16 == 2) gbase = (int32_t)sload<int64_t>(cs.cbase, (uint64_t)t * 4u);
  // the task's x window (packed tasks: <= 64 rows)
  const XWin<T> win = x_source<XW, XD>(xdyn, xlds, xwin, t, x, wid, lane);
  trace_t *ts = trace_slots<kDiagWaveTrace>(t);
  wave_trace_put(ts, lane, 0, t_start);
  wave_trace_put(ts, lane, 6, (trace_t)(r1 - r0));
  // align: groups end on multiples of 64 rows (the SSR plan's aligned
  // pieces: every y store but an SSR's first and last covers whole lines)
  const int32_t g1_first = min(align ? (r0 & ~(kWave - 1)) + kWave : r0 + kWave, r1);
  int32_t beg, end;
  group_bounds(rp, r0, g1_first, lane, beg, end);
  wave_trace_stamp(ts, lane, 1);
  for (int32_t g0 = r0, g1 = g1_first; g0 < r1; g0 = g1, g1 = min(g1 + kWave, r1)) {
    int32_t nbeg = 0, nend = 0;
    if (g1 < r1) group_bounds(rp, g1, min(g1 + kWave, r1), lane, nbeg, nend);
    wave_rows<T, NT, U, PF, C16, XW, XD, HSPMV_COOP_GROUPS != 0, false, TV>(
        g0, g1, beg, end, long_t, serial_max,  // the group and its rows' bounds, the row-length rules
        cs, val, x, y, my, lane, win,          // the streams, this wave's LDS, its x source
        y_nt != 0, carry != 0, gbase, ts);
    ts = nullptr;
    beg = nbeg;
    end = nend;
  }
  block_trace_wave_end(bt, lane, wid);
}

}  // namespace dev
}  // namespace hspmv
