// spmv_device.cuh -- device building blocks of the row kernels (STREAM and
// CSR3), included by the per-dtype instantiation units stream_f32.hip /
// stream_f64.hip (split so hipcc compiles them in parallel).  The design is
// described in spmv_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "hspmv_internal.h"

namespace hspmv {
namespace dev {

// Ablation builds only (make diag): 1 = skip the ordered row sums, 2 = skip
// the x gather (x[col] := 1), 3 = both; 16 = skip the x-dictionary staging
// (and its barrier), 32 = the barrier without the staging loads, 256 = no y
// stores (the sums kept live), 1024 = 1-byte dictionary positions (half the
// index bytes; the bound on any position compression: C3 107.3 -> 102.7 us,
// fp32 62.1 -> 51.2, profiles/r03/ab_c3_1byte_positions_ablation.jsonl --
// run-coded positions (a run-start mask per 64 nonzeros + 2 bytes per run,
// 0.86 B/nnz on C3) measured 108.7 -> 114.2 us, fp32 62.2 -> 99.4: the
// decode's dependent loads cost more than the bytes).  Results are wrong in
// those builds.
#ifndef HSPMV_DIAG
#define HSPMV_DIAG 0
#endif

// HSPMV_DIAG & 8: per-wave phase timestamps (s_memtime) of the STREAM
// kernel into g_trace (read back by hspmv_diag_trace, stream_f64.hip).  Each
// stamp first waits for all of the wave's outstanding loads, so the traced
// build measures a serialised wave; results are correct.
constexpr int kTraceWaves = 1 << 17;
constexpr int kTraceSlots = 8;
#if (HSPMV_DIAG & 8)
static __device__ unsigned long long g_trace[kTraceWaves * kTraceSlots];
__device__ __forceinline__ unsigned long long diag_stamp() {
  unsigned long long t;
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)"
               : "=s"(t)::"memory");
  return t;
}
#define HSPMV_TRACE(ts, i, v)            \
  do {                                   \
    if ((ts) != nullptr && lane == 0) (ts)[i] = (v); \
  } while (0)
#else
#define HSPMV_TRACE(ts, i, v) \
  do {                        \
  } while (0)
#endif
// HSPMV_DIAG & 512: per-workgroup timeline of the CSR3 kernel -- slot 0 the
// workgroup's start, 1..4 each wave's end (after its y store is issued), 6
// HW_ID, 7 XCC_ID (s_memrealtime, 100 MHz; no waits, results correct) --
// into g_trace[block * kTraceSlots] (tools/block_trace.py).
#if (HSPMV_DIAG & 512)
#if !(HSPMV_DIAG & 8)
static __device__ unsigned long long g_trace[kTraceWaves * kTraceSlots];
#endif
__device__ __forceinline__ unsigned long long diag_realtime() {
  unsigned long long t;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
#endif

constexpr int kWave = 64;
#ifndef HSPMV_COOP_GROUPS
#define HSPMV_COOP_GROUPS 1
#endif
// kSerialMax (hspmv_internal.h): the longest row summed serially by one lane.
// The kernels take the bound as an argument (DevPlan.serial_max): kSerialMax,
// or INT32_MAX for hspmv_options.deterministic = 3, where every row is summed
// serially -- omp_spmv's order for every row, the long ones by one lane.

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

template <bool NT, typename T>
__device__ __forceinline__ T ldg(const T *p) {
  if constexpr (NT)
    return __builtin_nontemporal_load(p);
  else
    return *p;
}

// Orders a wave's LDS writes before its other lanes' LDS reads (the
// wave-scope equivalent of a barrier; no s_barrier involved).
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// One DPP move of v (both dwords for fp64); lanes the pattern does not feed
// read 0.
template <int CTRL, int ROW_MASK, typename T>
__device__ __forceinline__ T dpp_move(T v) {
  if constexpr (sizeof(T) == 8) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(b >> 32), CTRL, ROW_MASK, 0xf, false);
    return __builtin_bit_cast(T, ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
  } else {
    return __builtin_bit_cast(
        T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false));
  }
}

// Wave sum by DPP (row_shr 1/2/4/8 inside each 16-lane row, then
// row_bcast 15/31 across rows: an inclusive scan whose lane 63 holds the
// total), returned wave-uniform.  No LDS round trips, unlike __shfl_xor
// (ds_bpermute): the cooperative rows' reductions are on the critical path
// of each chunk (mid-density rows, profiles/r02z*).
// Lane l's value of v, wave-uniform (v_readlane; l wave-uniform).
template <typename T>
__device__ __forceinline__ T lane_value(T v, int l) {
  if constexpr (sizeof(T) == 8) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)b, l);
    const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), l);
    return __builtin_bit_cast(T, ((uint64_t)hi << 32) | lo);
  } else {
    return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
  }
}

// Sums of the four 16-lane DPP rows: lane 16 q + 15 holds row q's total.
template <typename T>
__device__ __forceinline__ T row16_sum_dpp(T v) {
  v += dpp_move<0x111, 0xf>(v);
  v += dpp_move<0x112, 0xf>(v);
  v += dpp_move<0x114, 0xf>(v);
  v += dpp_move<0x118, 0xf>(v);
  return v;
}

template <typename T>
__device__ __forceinline__ T wave_sum_dpp(T v) {
  v += dpp_move<0x111, 0xf>(v);
  v += dpp_move<0x112, 0xf>(v);
  v += dpp_move<0x114, 0xf>(v);
  v += dpp_move<0x118, 0xf>(v);
  v += dpp_move<0x142, 0xa>(v);
  v += dpp_move<0x143, 0xc>(v);
  return lane_value(v, 63);
}

// Block order: xcd_chunk_remap / sweep_block (hspmv_internal.h), shared with
// the host.

__device__ __forceinline__ unsigned long long bits_from(int i) {
  return i >= 64 ? 0ull : (~0ull << i);
}

// Loads through a wave-uniform GLOBAL (address_space 1) base pointer plus a
// 32-bit byte offset, so hipcc emits global_load ... v_off, s[base:base+1]
// (one offset VGPR per load, no 64-bit address pairs, and no flat_load,
// which would force vmcnt(0) + lgkmcnt(0) waits).
typedef __attribute__((address_space(1))) const char gchar;

template <bool NT, typename T>
__device__ __forceinline__ T ld_off(const gchar *base, uint32_t byte_off) {
  const __attribute__((address_space(1))) T *p =
      (const __attribute__((address_space(1))) T *)(base + byte_off);
  if constexpr (NT)
    return __builtin_nontemporal_load(p);
  else
    return *p;
}

template <typename T>
__device__ __forceinline__ const gchar *uniform_ptr(const T *p) {
  const uint64_t v = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (const gchar *)(((uint64_t)hi << 32) | lo);
}

// Scalar (s_load) read of 8 bytes at p + byte_off; p and byte_off must be
// wave-uniform.
__device__ __forceinline__ int64_t sload_i64(const void *p, uint64_t byte_off) {
  const uint64_t v = reinterpret_cast<uint64_t>(p) + byte_off;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  typedef __attribute__((address_space(4))) const int64_t ci64;
  return *(ci64 *)(((uint64_t)hi << 32) | lo);
}

// The same for 4 bytes.
__device__ __forceinline__ int32_t sload_i32(const void *p, uint64_t byte_off) {
  const uint64_t v = reinterpret_cast<uint64_t>(p) + byte_off;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  typedef __attribute__((address_space(4))) const int32_t ci32;
  return *(ci32 *)(((uint64_t)hi << 32) | lo);
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

// One wavefront computes rows [g0, g1), g1 - g0 <= 64, whose bounds
// (group_bounds) are in beg/end.  lds: kWave*U elements private to this
// wave.  Per chunk of 64*U nonzeros: stage A loads col/val (coalesced),
// stage B gathers x[col] (from the LDS window when XW and win.w > 0), stage
// C forms the products into LDS; then the row sums.  PF (software
// pipelining): the next chunk's stage A is issued between this chunk's
// stage B and C, so its latency overlaps the gather and the sums.
// TV: the type the values are stored and streamed in (T, or float under
// T = double: the mixed handles); each value is widened to T once, before its
// product, so the products and sums are T's.
template <typename T, bool NT, int U, bool PF, int C16, bool XW, bool XD, bool GROUPS, bool PAD = false,
          typename TV = T>
__device__ __forceinline__ void wave_rows(int32_t g0, int32_t g1, int32_t beg, int32_t end,
                                          int32_t long_t, int32_t serial_max, const ColSrc &cs,
                                          const TV *__restrict__ val,
                                          const T *__restrict__ x,
                                          T *__restrict__ y, T *lds, int lane,
                                          const XWin<T> &win, bool y_nt, bool carry,
                                          int32_t gbase, unsigned long long *ts = nullptr) {
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
          if constexpr (XD && (HSPMV_DIAG & 1024) != 0) {
            col[u] = (int32_t)ld_off<NT, uint8_t>(cb, j);  // ablation: 1-byte positions (wrong x)
          } else if constexpr (XD) {
            col[u] = (int32_t)ld_off<NT, uint16_t>(cb, j * 2u);  // position in the block's xs
          } else if constexpr (C16 == 2) {
            // group-base offsets: col = the 64-row group's smallest column
            // + 16-bit offset (one scalar load per group, one add here)
            col[u] = gbase + (int32_t)ld_off<NT, uint16_t>(cb, j * 2u);
          } else if constexpr (C16 == 1) {
            // col = base of the nonzero's 256-block + 16-bit offset.  The 64
            // lanes of a slice lie in at most two consecutive blocks: one
            // scalar load brings both bases (s_load, no vector memory op)
            const uint32_t e0 = (uint32_t)kb + (uint32_t)(c0 + min(u * kWave, last));
            const uint32_t ja = (uint32_t)kb + j;
            const uint32_t b0 = __builtin_amdgcn_readfirstlane(e0 >> kC16Shift);
            const int64_t bp = sload_i64(cs.cbase, (uint64_t)b0 * 4u);
            const int32_t base = ((ja >> kC16Shift) == b0) ? (int32_t)bp : (int32_t)(bp >> 32);
            int32_t high = 0;
            if (cs.n_planes > 0) {  // wave-uniform; the two words a slice spans, by s_load
              const uint32_t w0 = __builtin_amdgcn_readfirstlane(e0 >> 6);
              const bool first = (ja >> 6) == w0;
              for (int p = 0; p < cs.n_planes; ++p) {
                const uint64_t at = ((uint64_t)p * (uint64_t)cs.plane_words + w0) * 8u;
                const uint64_t m0 = (uint64_t)sload_i64(cs.cplanes, at);
                const uint64_t m1 = (uint64_t)sload_i64(cs.cplanes, at + 8u);
                high |= (int32_t)(((first ? m0 : m1) >> (ja & 63u)) & 1u) << p;
              }
            }
            col[u] = base + (int32_t)ld_off<NT, uint16_t>(cb, j * 2u) + (high << 16);
          } else {
            col[u] = ld_off<NT, int32_t>(cb, j * 4u);
          }
          v[u] = ld_off<NT, TV>(vb, j * (uint32_t)sizeof(TV));
        }
      };
      if constexpr (PF) {
        if (n_run > 0) stage_a(0, min(kWave * U, n_run) - 1);
      }
      for (int32_t c0 = 0; c0 < n_run; c0 += kWave * U) {
        const int32_t last = min(kWave * U, n_run - c0) - 1;
        if constexpr (!PF) stage_a(c0, last);
#if (HSPMV_DIAG & 8)
        if (c0 == 0) HSPMV_TRACE(ts, 2, diag_stamp());
#endif
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
            if constexpr ((HSPMV_DIAG & 2) != 0)
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
#if (HSPMV_DIAG & 8)
        if (c0 == 0) HSPMV_TRACE(ts, 3, diag_stamp());
#endif
#pragma unroll
        for (int u = 0; u < U; ++u) lds[lds_ix<PAD>(u * kWave + lane)] = vv[u] * xv[u];
        wave_sync();
        const int32_t c = kb + c0;
        if constexpr ((HSPMV_DIAG & 1) != 0) {
          if (mine && max(beg, c) < min(end, c + last + 1)) acc += lds[lds_ix<PAD>(max(beg, c) - c)];
        } else {
          if (mine) acc = ordered_sum<PAD>(acc, lds, c, max(beg, c), min(end, c + last + 1));
        }
        // only the cooperative rows this chunk touches (rows are contiguous:
        // the others would add nothing), bounds by readlane (scalar)
        unsigned long long cm = coop ? coop & __ballot(end > c && beg <= c + last) : 0ull;
        // three or more pieces (rows of 33..~100 nonzeros): four at a time,
        // one 16-lane DPP row each.  CSR3 kernel only -- the tasks that
        // mid-density CSR matrices run as (hspmv_tables.cpp build_tasks): in
        // the STREAM kernel the extra code cost the honeycomb matrix 4 %
        // (161 -> 168 us) with no such rows at all (r02z9).  d33 173 ->
        // 137 us, d48 132 -> 109, d64 103 -> 95 (profiles/r02z8).
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
        wave_sync();
#if (HSPMV_DIAG & 8)
        if (c0 == 0) HSPMV_TRACE(ts, 4, diag_stamp());
        if (c0 + kWave * U >= n_run) HSPMV_TRACE(ts, 7, (unsigned long long)(c0 / (kWave * U) + 1));
#endif
      }
    }
    a = b + 1;
  }
#if (HSPMV_DIAG & 8)
  HSPMV_TRACE(ts, 5, diag_stamp());
#endif
  if constexpr ((HSPMV_DIAG & 256) != 0) {  // ablation: no y stores (kept live)
    if (valid && !skip && acc == T(12345.678)) y[row] = acc;
  } else if (valid && !skip) {
    if (y_nt)  // HBM-resident: streaming stores (bw_probe3/4: y writes cost ~20 % of time)
      __builtin_nontemporal_store(acc, y + row);
    else
      y[row] = acc;
  }
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
  if constexpr ((HSPMV_DIAG & 16) != 0) return;  // ablation: no staging, no barrier
  if constexpr ((HSPMV_DIAG & 32) != 0) {        // ablation: the barrier only
    __syncthreads();
    return;
  }
  // HSPMV_DIAG & 64 / 128 (A/B, results correct): the staging waves at
  // issue priority 3 / 1 until the barrier, ahead of other blocks' streams
  if constexpr ((HSPMV_DIAG & 64) != 0) __builtin_amdgcn_s_setprio(3);
  if constexpr ((HSPMV_DIAG & 128) != 0) __builtin_amdgcn_s_setprio(1);
  const int64_t rr = sload_i64(xd.blk, (uint64_t)blk * 4u);
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
  if constexpr ((HSPMV_DIAG & (64 | 128)) != 0) __builtin_amdgcn_s_setprio(0);
}

// STREAM: wave w walks `groups` consecutive 64-row groups starting at row
// w * groups * 64, loading the next group's row pointers before streaming
// the current one.  XW: groups whose x window (xwin[g] = {lo, w}) fits
// kXWin entries gather from an LDS copy of it.
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
  unsigned long long *ts = nullptr;
#if (HSPMV_DIAG & 8)
  const int64_t wv = blk * W + wid;
  if (wv < kTraceWaves) ts = g_trace + wv * kTraceSlots;
  HSPMV_TRACE(ts, 0, diag_stamp());
  {
    unsigned hw;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    HSPMV_TRACE(ts, 6, (unsigned long long)hw);
  }
#endif
  int32_t beg, end;
  group_bounds(rp, (int32_t)g0, (int32_t)min<int64_t>(g0 + kWave, gend), lane, beg, end);
#if (HSPMV_DIAG & 8)
  HSPMV_TRACE(ts, 1, diag_stamp());
#endif
  while (true) {
    const int32_t g1 = (int32_t)min<int64_t>(g0 + kWave, gend);
    XWin<T> win{XD ? reinterpret_cast<const T *>(xdyn) : nullptr, 0, 0};
    if constexpr (XW) {
      const int64_t wv = sload_i64(xwin, (uint64_t)(g0 / kWave) * 8u);
      win.lo = (int32_t)wv;
      win.w = (int32_t)(wv >> 32);
      win.xs = xlds + wid * kXWin;
      if (win.w > 0) stage_xwin(xlds + wid * kXWin, x, win.lo, win.w, lane);
    }
    int32_t nbeg = 0, nend = 0;
    if (g1 < gend) group_bounds(rp, g1, (int32_t)min<int64_t>(g1 + kWave, gend), lane, nbeg, nend);
    int32_t gbase = 0;
    if constexpr (C16 == 2) gbase = (int32_t)sload_i64(cs.cbase, (uint64_t)(g0 / kWave) * 4u);
    wave_rows<T, NT, U, PF, C16, XW, XD, false, PAD, TV>((int32_t)g0, g1, beg, end, long_t, serial_max, cs, val,
                                                     x, y, my,
                                         lane, win, y_nt != 0, carry != 0, gbase, ts);
    ts = nullptr;  // trace the first group only
    if (g1 >= gend) break;
    g0 = g1;
    beg = nbeg;
    end = nend;
  }
}

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
#if (HSPMV_DIAG & 512)
  unsigned long long *bt = blk < kTraceWaves ? g_trace + blk * kTraceSlots : nullptr;
  if (bt && threadIdx.x == 0) {
    bt[0] = diag_realtime();
    bt[6] = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_ID
    bt[7] = __builtin_amdgcn_s_getreg((31 << 11) | 20);  // XCC_ID
  }
#endif
  // XD: the W packed tasks of the block share one staged dictionary (loads
  // of the task / row bounds and of the first chunk issued ahead of the
  // staging measured -0.3 ... -0.6 % and cost 20 VGPRs: profiles/r05c,
  // r05d; removed)
  if constexpr (XD) stage_xdict<T, W * 64>(reinterpret_cast<T *>(xdyn), x, xd, blk, threadIdx.x);
  const int64_t t = blk * W + wid;
  if (t >= n_tasks) return;
#if (HSPMV_DIAG & 8)
  const unsigned long long tb_stamp = diag_stamp();
#endif
  // both task bounds in one scalar load (K$), not a vector round trip
  const int64_t tb = sload_i64(task_start, (uint64_t)t * 4u);
  const int32_t r0 = (int32_t)tb;
  const int32_t r1 = (int32_t)(tb >> 32);
  if (r0 >= r1) return;
  T *my = lds + wid * wave_lds<U, false>();
  // group-base columns: one base per packed task
  int32_t gbase = 0;
  if constexpr (C16 == 2) gbase = (int32_t)sload_i64(cs.cbase, (uint64_t)t * 4u);
  XWin<T> win{XD ? reinterpret_cast<const T *>(xdyn) : nullptr, 0, 0};
  if constexpr (XW) {  // the task's x window (packed tasks: <= 64 rows)
    const int64_t wv = sload_i64(xwin, (uint64_t)t * 8u);
    win.lo = (int32_t)wv;
    win.w = (int32_t)(wv >> 32);
    win.xs = xlds + wid * kXWin;
    if (win.w > 0) stage_xwin(xlds + wid * kXWin, x, win.lo, win.w, lane);
  }
  unsigned long long *ts = nullptr;
#if (HSPMV_DIAG & 8)
  if (t < kTraceWaves) ts = g_trace + t * kTraceSlots;
  HSPMV_TRACE(ts, 0, tb_stamp);
  HSPMV_TRACE(ts, 6, (unsigned long long)(r1 - r0));
#endif
  // align: groups end on multiples of 64 rows (the SSR plan's aligned
  // pieces: every y store but an SSR's first and last covers whole lines)
  const int32_t g1_first = min(align ? (r0 & ~(kWave - 1)) + kWave : r0 + kWave, r1);
  int32_t beg, end;
  group_bounds(rp, r0, g1_first, lane, beg, end);
#if (HSPMV_DIAG & 8)
  HSPMV_TRACE(ts, 1, diag_stamp());
#endif
  for (int32_t g0 = r0, g1 = g1_first; g0 < r1; g0 = g1, g1 = min(g1 + kWave, r1)) {
    int32_t nbeg = 0, nend = 0;
    if (g1 < r1) group_bounds(rp, g1, min(g1 + kWave, r1), lane, nbeg, nend);
    wave_rows<T, NT, U, PF, C16, XW, XD, HSPMV_COOP_GROUPS != 0, false, TV>(g0, g1, beg, end, long_t, serial_max, cs, val,
                                                                 x, y, my, lane,
                                         win, y_nt != 0, carry != 0, gbase, ts);
    ts = nullptr;
    beg = nbeg;
    end = nend;
  }
#if (HSPMV_DIAG & 512)
  if (bt && lane == 0 && wid < 4) bt[1 + wid] = diag_realtime();
#endif
}

// ------------------------------------------------------------------ row slices
//
// The transposed (sliced-ELL) shape of the dictionary kernels, for handles
// whose every row is summed serially anyway (hspmv_slices.cpp holds the
// format and the eligibility rules).  A wave's task of <= 64 rows is stored
// column-major: lane i owns row i, slot k of all 64 rows lies together, so
// one load instruction brings 16 bytes of values (2 fp64 / 4 fp32
// consecutive slots of the lane's row) or 8 bytes of positions (4 slots) per
// lane, and the lane multiplies and adds its own row left to right -- the
// order and rounding of the ordered sums, with no product buffer in LDS, no
// wave_sync and no row pointers.  Slot k of a slice starts at element 64 * k
// of the slice in both streams (groups and the trailing single columns
// alike).  Slots past a row's end are masked by its length, never added.
//
// PB = 12 (a handle whose positions all fit 12 bits, hspmv_slices_pack): a
// whole batch of 8 slots reads one 12-byte position group per lane, eight
// 12-bit fields, at 96 bytes per slot column; the slice's last w mod 8 slots
// follow in the 16-bit layout, and the slice starts at 128 * ppre[t] bytes.
#ifndef HSPMV_SLICE_BATCH
#define HSPMV_SLICE_BATCH 8  // slots per load batch (a multiple of 4)
#endif

struct Slices {
  const int32_t *desc;  // {prefix, first row} per task, closed by {total, m}
  const uint8_t *len;   // nonzeros per row
  const uint16_t *pos;  // dictionary positions, 64 * prefix elements per slice start
  const int32_t *ppre;  // PB = 12: the packed positions' start per task, 128-byte units
};

typedef int32_t sl_i4 __attribute__((ext_vector_type(4), aligned(4)));

// Scalar (s_load) read of 16 bytes at p + byte_off, both wave-uniform.
__device__ __forceinline__ sl_i4 sload_i128(const void *p, uint64_t byte_off) {
  const uint64_t v = reinterpret_cast<uint64_t>(p) + byte_off;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  typedef __attribute__((address_space(4))) const sl_i4 ci128;
  return *(ci128 *)(((uint64_t)hi << 32) | lo);
}

typedef uint32_t sl_u3 __attribute__((ext_vector_type(3), aligned(4)));

template <typename TV, int B>
struct SliceBatch {
  TV v[B];              // slot k0 + i of the lane's row, as stored
  uint32_t pq[B / 2];   // positions of whole 4-slot groups, two per register (PB = 12: 3 per 8 slots)
  uint32_t ps[3];       // positions of the slice's last 1-3 slots (single columns)
};

// A whole batch: slots [k0, k0 + B) all lie in 16-byte value groups and
// 8-byte (PB = 12: 12-byte) position groups.  vb / pb: the slice's streams.
template <typename TV, bool NT, int B, int PB>
__device__ __forceinline__ void slice_load_full(SliceBatch<TV, B> &q, const gchar *vb, const gchar *pb,
                                                int32_t k0, int lane) {
  constexpr int G = 16 / (int)sizeof(TV);
  typedef TV tv __attribute__((ext_vector_type(G)));
  typedef uint32_t u2 __attribute__((ext_vector_type(2)));
  const gchar *vbb = vb + (uint64_t)(uint32_t)k0 * (kWave * sizeof(TV));
  const gchar *pbb = pb + (uint64_t)(uint32_t)k0 * (kWave * PB / 8u);
#pragma unroll
  for (int j = 0; j < B / G; ++j) {
    const tv t = ld_off<NT, tv>(vbb, (uint32_t)(j * kWave + lane) * 16u);
#pragma unroll
    for (int e = 0; e < G; ++e) q.v[j * G + e] = t[e];
  }
  if constexpr (PB == 12) {
    // (sizeof(sl_u3) is 16: the groups are addressed in bytes)
#pragma unroll
    for (int g = 0; g < B / 8; ++g) {
      const sl_u3 t = ld_off<NT, sl_u3>(pbb, (uint32_t)(g * kWave + lane) * 12u);
      q.pq[3 * g] = t[0];
      q.pq[3 * g + 1] = t[1];
      q.pq[3 * g + 2] = t[2];
    }
  } else {
#pragma unroll
    for (int g = 0; g < B / 4; ++g) {
      const u2 t = ld_off<NT, u2>(pbb, (uint32_t)(g * kWave + lane) * 8u);
      q.pq[2 * g] = t[0];
      q.pq[2 * g + 1] = t[1];
    }
  }
}

// The slice's last, partial batch: slots [k0, w), w - k0 < B; whole groups
// as above, the rest from the single columns.  Slots past w read as value 0
// at position 0 (and are masked like every slot past a row's end).  The
// tail's positions are 16-bit for either PB; PB sets where they start.
template <typename TV, bool NT, int B, int PB>
__device__ __forceinline__ void slice_load_tail(SliceBatch<TV, B> &q, const gchar *vb, const gchar *pb,
                                                int32_t k0, int32_t w, int lane) {
  constexpr int G = 16 / (int)sizeof(TV);
  typedef TV tv __attribute__((ext_vector_type(G)));
  typedef uint32_t u2 __attribute__((ext_vector_type(2)));
  const gchar *vbb = vb + (uint64_t)(uint32_t)k0 * (kWave * sizeof(TV));
  const gchar *pbb = pb + (uint64_t)(uint32_t)k0 * (kWave * PB / 8u);
#pragma unroll
  for (int i = 0; i < B; ++i) q.v[i] = TV(0);
#pragma unroll
  for (int i = 0; i < B / 2; ++i) q.pq[i] = 0u;
#pragma unroll
  for (int i = 0; i < 3; ++i) q.ps[i] = 0u;
#pragma unroll
  for (int j = 0; j < B / G; ++j) {
    if (k0 + j * G + G <= w) {  // wave-uniform
      const tv t = ld_off<NT, tv>(vbb, (uint32_t)(j * kWave + lane) * 16u);
#pragma unroll
      for (int e = 0; e < G; ++e) q.v[j * G + e] = t[e];
    } else {
#pragma unroll
      for (int e = 0; e < G - 1; ++e)
        if (k0 + j * G + e < w)
          q.v[j * G + e] = ld_off<NT, TV>(vbb, (uint32_t)((j * G + e) * kWave + lane) * (uint32_t)sizeof(TV));
    }
  }
#pragma unroll
  for (int g = 0; g < B / 4; ++g) {
    if (k0 + 4 * g + 4 <= w) {
      const u2 t = ld_off<NT, u2>(pbb, (uint32_t)(g * kWave + lane) * 8u);
      q.pq[2 * g] = t[0];
      q.pq[2 * g + 1] = t[1];
    } else {
#pragma unroll
      for (int r = 0; r < 3; ++r)
        if (k0 + 4 * g + r < w)
          q.ps[r] = (uint32_t)ld_off<NT, uint16_t>(pbb, (uint32_t)((4 * g + r) * kWave + lane) * 2u);
    }
  }
}

// Position of slot i of a whole batch.
template <int PB>
__device__ __forceinline__ uint32_t slice_pos(const uint32_t *pq, int i) {
  if constexpr (PB == 12) {
    const int d = 3 * (i / 8) + 12 * (i % 8) / 32, sh = 12 * (i % 8) % 32;
    uint32_t v = pq[d] >> sh;
    if (sh > 20) v |= pq[d + 1] << (32 - sh);
    return v & 0xfffu;
  } else {
    return (pq[i / 2] >> (16 * (i & 1))) & 0xffffu;
  }
}

// Adds the batch's slots to acc in slot order: the product rounded on its
// own (-ffp-contract=off), then the add; a slot at or past the row's end
// leaves acc as it is.  full: every position comes from pq, PB bits each
// (a tail batch's are 16-bit).  A value stored narrower than T (TV) is
// widened here, once, before its product.
template <typename T, int B, int PB, typename TV>
__device__ __forceinline__ T slice_consume(T acc, const SliceBatch<TV, B> &q, const T *xs, int32_t k0,
                                           int32_t w, int32_t len, bool full) {
  T xv[B];
#pragma unroll
  for (int i = 0; i < B; ++i) {
    const int g = i / 4, r = i % 4;
    const uint32_t p = (full || k0 + 4 * g + 4 <= w) ? slice_pos<PB>(q.pq, i) : q.ps[r < 3 ? r : 0];
    xv[i] = xs[p];
  }
#pragma unroll
  for (int i = 0; i < B; ++i) {
    const T p = (T)q.v[i] * xv[i];
    acc = (k0 + i < len) ? acc + p : acc;
  }
  return acc;
}

// One workgroup = one dictionary block (four wave tasks, or a half block's
// two and two empty ones), staged by stage_xdict exactly as in the chunked
// kernels.  Each wave reads its slice's descriptor (one scalar load) and its
// rows' lengths before the staging; after the barrier it walks the slot
// columns in batches of B, the next batch's loads issued before the current
// one is consumed.  LDS: the dictionary alone.
template <typename T, bool NT, int B, int PB, typename TV = T>
__global__ __launch_bounds__(256) void hspmv_slices(int32_t n_slices, uint32_t blk_order, int32_t y_nt,
                                                    Slices sl, XDict xd, const TV *__restrict__ val,
                                                    const T *__restrict__ x, T *__restrict__ y) {
  static_assert(B % 4 == 0 && B >= 4, "batches hold whole position groups");
  static_assert(PB == 16 || (PB == 12 && B % 8 == 0), "12-bit positions come in groups of 8 slots");
  static_assert(B % (16 / (int)sizeof(TV)) == 0, "batches hold whole 16-byte value groups");
  extern __shared__ __attribute__((aligned(16))) unsigned char xdyn[];
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t blk = sweep_block(blockIdx.x, gridDim.x, blk_order);
  const int64_t t = blk * 4 + wid;
  int32_t off = 0, poff = 0, w = 0, r0 = 0, nr = 0;
  if (t < n_slices) {  // wave-uniform
    const sl_i4 d = sload_i128(sl.desc, (uint64_t)t * 8u);
    off = d[0];
    r0 = d[1];
    w = d[2] - d[0];
    nr = d[3] - d[1];
    poff = PB == 12 ? sload_i32(sl.ppre, (uint64_t)t * 4u) : off;
  }
  int32_t len = 0;
  if (lane < nr) len = (int32_t)sl.len[r0 + lane];
  stage_xdict<T, 256>(reinterpret_cast<T *>(xdyn), x, xd, blk, threadIdx.x);
  if (nr <= 0) return;
  const T *xs = reinterpret_cast<const T *>(xdyn);
  const gchar *vb = uniform_ptr(val + (int64_t)off * kWave);
  const gchar *pb = uniform_ptr(sl.pos + (int64_t)poff * kWave);
  const int32_t wf = w & ~(B - 1);  // slots in whole batches
  T acc = T(0);
  SliceBatch<TV, B> cur, nxt, tail;
  int32_t k0 = 0;
  if (wf > 0) slice_load_full<TV, NT, B, PB>(cur, vb, pb, 0, lane);
  for (; k0 + 3 * B <= wf; k0 += 2 * B) {
    slice_load_full<TV, NT, B, PB>(nxt, vb, pb, k0 + B, lane);
    __builtin_amdgcn_sched_barrier(0);
    acc = slice_consume<T, B, PB>(acc, cur, xs, k0, w, len, true);
    __builtin_amdgcn_sched_barrier(0);
    slice_load_full<TV, NT, B, PB>(cur, vb, pb, k0 + 2 * B, lane);
    __builtin_amdgcn_sched_barrier(0);
    acc = slice_consume<T, B, PB>(acc, nxt, xs, k0 + B, w, len, true);
    __builtin_amdgcn_sched_barrier(0);
  }
  if (k0 + 2 * B <= wf) {
    slice_load_full<TV, NT, B, PB>(nxt, vb, pb, k0 + B, lane);
    __builtin_amdgcn_sched_barrier(0);
    acc = slice_consume<T, B, PB>(acc, cur, xs, k0, w, len, true);
    __builtin_amdgcn_sched_barrier(0);
    cur = nxt;
    k0 += B;
  }
  // cur: the last whole batch (at wf - B), not yet added
  if (w > wf) slice_load_tail<TV, NT, B, PB>(tail, vb, pb, wf, w, lane);
  __builtin_amdgcn_sched_barrier(0);
  if (wf > 0) acc = slice_consume<T, B, PB>(acc, cur, xs, wf - B, w, len, true);
  if (w > wf) acc = slice_consume<T, B, 16>(acc, tail, xs, wf, w, len, false);
  if constexpr ((HSPMV_DIAG & 256) != 0) {  // ablation: no y stores (kept live)
    if (lane < nr && acc == T(12345.678)) y[r0 + lane] = acc;
  } else if (lane < nr) {
    if (y_nt)
      __builtin_nontemporal_store(acc, y + r0 + lane);
    else
      y[r0 + lane] = acc;
  }
}

// ------------------------------------------------------------------ launchers

// The kernels' block-order argument: the XCD chunk, and the sweep direction
// of this launch in the top bit (sweep_block).
inline uint32_t block_order(const LaunchPlan &p) {
  return (uint32_t)p.xcd_chunk | (p.reverse ? kSweepReverse : 0u);
}

template <typename T, int PB, typename TV>
void launch_slices_pb(const DevPlan &dp, const LaunchPlan &p, const T *x, T *y, hipStream_t st) {
  const Slices sl{dp.sl_desc, dp.sl_len, dp.sl_pos, dp.sl_ppre};
  const XDict xd{dp.xd_blk, reinterpret_cast<const int2 *>(dp.xd_runs)};
  const unsigned dyn = (unsigned)dp.xd_lds_bytes + (unsigned)p.dyn_lds;
  const TV *val = static_cast<const TV *>(dp.sl_val);
  if (p.nontemporal)
    hipLaunchKernelGGL((hspmv_slices<T, true, HSPMV_SLICE_BATCH, PB, TV>), dim3((unsigned)p.blocks), dim3(256), dyn,
                       st, dp.n_slices, block_order(p), (int32_t)p.y_nt, sl, xd, val, x, y);
  else
    hipLaunchKernelGGL((hspmv_slices<T, false, HSPMV_SLICE_BATCH, PB, TV>), dim3((unsigned)p.blocks), dim3(256), dyn,
                       st, dp.n_slices, block_order(p), (int32_t)p.y_nt, sl, xd, val, x, y);
}

template <typename T, typename TV>
hipError_t launch_slices(const DevPlan &dp, const LaunchPlan &p, const T *x, T *y, hipStream_t st) {
  if (!dp.xd_blk || !dp.sl_len || !dp.sl_pos || !dp.sl_val || p.waves_per_block != 4 ||
      p.blocks != ((int64_t)dp.n_slices + 3) / 4 ||
      !(dp.sl_pos_bits == 16 || (dp.sl_pos_bits == 12 && dp.sl_ppre)))
    return hipErrorInvalidValue;  // the host built the slices for another block shape
  if (dp.sl_pos_bits == 12)
    launch_slices_pb<T, 12, TV>(dp, p, x, y, st);
  else
    launch_slices_pb<T, 16, TV>(dp, p, x, y, st);
  return hipGetLastError();
}

inline ColSrc col_src(const DevCSR &A) {
  return ColSrc{A.col_idx, A.col16, A.cbase, A.cplanes, A.n_cplanes, A.cplane_words};
}

template <typename T, bool NT, int U, bool PF, int C16, bool XD, typename TV>
void launch_rows_u(const DevCSR &A, const DevPlan &dp, const LaunchPlan &p, const T *x, T *y,
                   hipStream_t st) {
  const TV *val = static_cast<const TV *>(A.val);
  const ColSrc cs = col_src(A);
  const XDict xd{dp.xd_blk, reinterpret_cast<const int2 *>(dp.xd_runs)};
  // dynamic LDS: the block's x dictionary (XD), or occupancy experiments (HSPMV_DYNLDS)
  const unsigned dyn = XD ? (unsigned)dp.xd_lds_bytes + (unsigned)p.dyn_lds : (unsigned)p.dyn_lds;
  if (p.kernel == kStream) {
    const int2 *xw = reinterpret_cast<const int2 *>(dp.xwin);
#define HSPMV_STREAM(C, XW, XDX, W, PAD)                                                            \
  hipLaunchKernelGGL((hspmv_csr_stream<T, NT, U, PF, C, XW, XDX, W, PAD, TV>), dim3((unsigned)p.blocks), \
                     dim3(W * 64), dyn, st, A.m, dp.long_t, dp.serial_max, block_order(p),       \
                     (int32_t)p.groups,                                                               \
                     (int32_t)p.y_nt, p.carry, A.row_ptr, cs, xw, xd, val, x, y)
    if constexpr (XD) {  // never padded (plan_launch: dictionaries are sized unpadded)
      HSPMV_STREAM(false, false, true, 4, false);
      return;
    }
    // padded product buffers (LaunchPlan.lds_pad): conflicting row lengths,
    // no prefetch variant (the planner never pairs them)
    if constexpr (!PF) {
      if (p.lds_pad) {
        if (p.waves_per_block == 1 && xw) HSPMV_STREAM(C16, true, false, 1, true);
        else if (p.waves_per_block == 1) HSPMV_STREAM(C16, false, false, 1, true);
        else if (p.waves_per_block != 4 && xw) HSPMV_STREAM(C16, true, false, 2, true);
        else if (p.waves_per_block != 4) HSPMV_STREAM(C16, false, false, 2, true);
        else if (xw) HSPMV_STREAM(C16, true, false, 4, true);
        else HSPMV_STREAM(C16, false, false, 4, true);
        return;
      }
    }
    if (p.waves_per_block == 1 && xw) HSPMV_STREAM(C16, true, false, 1, false);
    else if (p.waves_per_block == 1) HSPMV_STREAM(C16, false, false, 1, false);
    else if (p.waves_per_block != 4 && xw) HSPMV_STREAM(C16, true, false, 2, false);
    else if (p.waves_per_block != 4) HSPMV_STREAM(C16, false, false, 2, false);
    else if (xw) HSPMV_STREAM(C16, true, false, 4, false);
    else HSPMV_STREAM(C16, false, false, 4, false);
#undef HSPMV_STREAM
    return;
  }
  {
  const int2 *xw = reinterpret_cast<const int2 *>(dp.xwin);
#define HSPMV_CSR3(W, C, XW, X)                                                               \
  hipLaunchKernelGGL((hspmv_csr3<T, NT, U, PF, C, W, XW, X, TV>), dim3((unsigned)p.blocks),      \
                     dim3(W * 64), dyn, st, dp.n_tasks, dp.long_t, dp.serial_max,             \
                     block_order(p),                                                   \
                     (int32_t)p.y_nt, p.carry, dp.task_align, dp.task_start, xw, xd, A.row_ptr, cs, \
                     val, x, y)
  if constexpr (XD) {  // packed tasks only (4 or 8 per block)
    if (p.waves_per_block == 8)
      HSPMV_CSR3(8, false, false, true);
    else
      HSPMV_CSR3(4, false, false, true);
    return;
  } else {
    if (xw && p.waves_per_block == 4) {  // x windows: packed tasks only (4 per block)
      HSPMV_CSR3(4, C16, true, false);
      return;
    }
    switch (p.waves_per_block) {
      case 1: HSPMV_CSR3(1, C16, false, false); break;
      case 2: HSPMV_CSR3(2, C16, false, false); break;
      case 4: HSPMV_CSR3(4, C16, false, false); break;
      default: HSPMV_CSR3(8, C16, false, false); break;
    }
  }
#undef HSPMV_CSR3
  }
}

template <typename T, bool NT, bool PF, int C16, bool XD, typename TV>
hipError_t launch_rows_pf(const DevCSR &A, const DevPlan &dp, const LaunchPlan &p, const T *x,
                          T *y, hipStream_t st) {
  switch (p.u) {
    case 2: launch_rows_u<T, NT, 2, PF, C16, XD, TV>(A, dp, p, x, y, st); break;
    case 3: launch_rows_u<T, NT, 3, PF, C16, XD, TV>(A, dp, p, x, y, st); break;
    case 4: launch_rows_u<T, NT, 4, PF, C16, XD, TV>(A, dp, p, x, y, st); break;
    case 5: launch_rows_u<T, NT, 5, PF, C16, XD, TV>(A, dp, p, x, y, st); break;
    case 6: launch_rows_u<T, NT, 6, PF, C16, XD, TV>(A, dp, p, x, y, st); break;
    case 8: launch_rows_u<T, NT, 8, PF, C16, XD, TV>(A, dp, p, x, y, st); break;
    case 16: launch_rows_u<T, NT, 16, PF, C16, XD, TV>(A, dp, p, x, y, st); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template <typename T, int C16, bool XD, typename TV>
hipError_t launch_rows_c(const DevCSR &A, const DevPlan &dp, const LaunchPlan &p, const T *x,
                         T *y, hipStream_t st) {
  if (p.nontemporal)
    return p.prefetch ? launch_rows_pf<T, true, true, C16, XD, TV>(A, dp, p, x, y, st)
                      : launch_rows_pf<T, true, false, C16, XD, TV>(A, dp, p, x, y, st);
  return p.prefetch ? launch_rows_pf<T, false, true, C16, XD, TV>(A, dp, p, x, y, st)
                    : launch_rows_pf<T, false, false, C16, XD, TV>(A, dp, p, x, y, st);
}

// XD (block x dictionaries) replaces both the 32-bit columns and the col16
// offsets: its col stream is the 16-bit xs positions.  TV: the stored type of
// A.val / dp.sl_val (the mixed handles: float under T = double).
template <typename T, typename TV = T>
hipError_t launch_rows(const DevCSR &A, const DevPlan &dp, const LaunchPlan &p, const T *x, T *y,
                       hipStream_t st) {
  if (dp.sl_desc) return launch_slices<T, TV>(dp, p, x, y, st);  // row slices of a dictionary handle
  if (dp.xd_blk) {
    if (!A.col16 || (p.kernel == kStream && p.groups != 1) ||
        (p.kernel == kCsr3 && (!dp.task_start || (p.waves_per_block != 4 && p.waves_per_block != 8))))
      return hipErrorInvalidValue;  // the host built the dictionary for another block shape
    return launch_rows_c<T, 0, true, TV>(A, dp, p, x, y, st);
  }
  if (A.col16 && A.c16_mode == 2) {
    if (p.kernel == kCsr3 && !dp.task_start)
      return hipErrorInvalidValue;  // built for the host-planned wave tasks (one base per task)
    return launch_rows_c<T, 2, false, TV>(A, dp, p, x, y, st);
  }
  return A.col16 ? launch_rows_c<T, 1, false, TV>(A, dp, p, x, y, st)
                 : launch_rows_c<T, 0, false, TV>(A, dp, p, x, y, st);
}

}  // namespace dev
}  // namespace hspmv
