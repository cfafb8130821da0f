// dev_diag.cuh -- the row and slice kernels' diagnostic builds (make diag
// DIAGS=<bits>): the HSPMV_DIAG bits by name, and the trace helpers the
// kernels call.  In the product build (HSPMV_DIAG = 0) every helper here is
// empty and compiles to nothing.
#pragma once
#include "dev_prims.cuh"

#ifndef HSPMV_DIAG
#define HSPMV_DIAG 0
#endif

namespace hspmv {
namespace dev {

// Ablations: results are wrong in those builds.
constexpr int kDiagNoRowSums = 1;    // skip the ordered row sums
constexpr int kDiagNoGather = 2;     // skip the x gather (x[col] := 1 or 2); 3 = both
constexpr int kDiagNoStaging = 16;   // skip the x-dictionary staging (and its barrier)
constexpr int kDiagBarrierOnly = 32; // the staging's barrier without its loads
constexpr int kDiagNoStore = 256;    // no y stores (the sums kept live)
// 1-byte dictionary positions (half the index bytes; the bound on any
// position compression: C3 107.3 -> 102.7 us, fp32 62.1 -> 51.2,
// profiles/r03/ab_c3_1byte_positions_ablation.jsonl -- run-coded positions
// (a run-start mask per 64 nonzeros + 2 bytes per run, 0.86 B/nnz on C3)
// measured 108.7 -> 114.2 us, fp32 62.2 -> 99.4: the decode's dependent loads
// cost more than the bytes).
constexpr int kDiagPos8 = 1024;
// A/B, results correct: the dictionary-staging waves at issue priority 3 / 1
// until the barrier, ahead of other blocks' streams.
constexpr int kDiagStagePrio3 = 64;
constexpr int kDiagStagePrio1 = 128;
// Traces, results correct.  kDiagWaveTrace: per-wave phase timestamps
// (s_memtime) of the row kernels into g_trace (read back by hspmv_diag_trace,
// stream_f64.hip; tools/wave_trace.py).  Each stamp first waits for all of the
// wave's outstanding loads, so the traced build measures a serialised wave.
// Slots: 0 start, 1 first row bounds, 2 first chunk loaded, 3 gathered, 4
// summed, 5 all chunks done, 6 HW_ID (STREAM) / rows of the task (CSR3), 7
// chunks of the first run.
constexpr int kDiagWaveTrace = 8;
// kDiagBlockTrace: per-workgroup timeline of the CSR3 kernel -- slot 0 the
// workgroup's start, 1..4 each wave's end (after its y store is issued), 6
// HW_ID, 7 XCC_ID (s_memrealtime, 100 MHz; no waits) -- into
// g_trace[block * kTraceSlots] (tools/block_trace.py).
constexpr int kDiagBlockTrace = 512;

constexpr bool diag(int bits) { return (HSPMV_DIAG & bits) != 0; }

constexpr int kTraceWaves = 1 << 17;
constexpr int kTraceSlots = 8;
typedef unsigned long long trace_t;

#if (HSPMV_DIAG & (8 | 512))
static __device__ trace_t g_trace[kTraceWaves * kTraceSlots];
#endif

// The trace slots of wave / workgroup `id` (nullptr: not traced).
template <int BIT>
__device__ __forceinline__ trace_t *trace_slots(int64_t id) {
#if (HSPMV_DIAG & (8 | 512))
  if constexpr (diag(BIT)) return id < kTraceWaves ? g_trace + id * kTraceSlots : nullptr;
#endif
  return nullptr;
}

// kDiagWaveTrace: the time now, all of the wave's loads landed (0 when off).
__device__ __forceinline__ trace_t wave_trace_now() {
  trace_t t = 0;
#if (HSPMV_DIAG & 8)
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
#endif
  return t;
}
__device__ __forceinline__ void wave_trace_put(trace_t *ts, int lane, int slot, trace_t v) {
  if constexpr (diag(kDiagWaveTrace))
    if (ts != nullptr && lane == 0) ts[slot] = v;
}
__device__ __forceinline__ void wave_trace_stamp(trace_t *ts, int lane, int slot) {
  if constexpr (diag(kDiagWaveTrace)) wave_trace_put(ts, lane, slot, wave_trace_now());
}
__device__ __forceinline__ void wave_trace_hw_id(trace_t *ts, int lane, int slot) {
#if (HSPMV_DIAG & 8)
  unsigned hw;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  wave_trace_put(ts, lane, slot, (trace_t)hw);
#endif
}

// kDiagBlockTrace: the workgroup's start, and where it runs.
__device__ __forceinline__ trace_t block_trace_now() {
  trace_t t = 0;
#if (HSPMV_DIAG & 512)
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
#endif
  return t;
}
__device__ __forceinline__ trace_t *block_trace_begin(int64_t blk) {
  trace_t *bt = trace_slots<kDiagBlockTrace>(blk);
  if constexpr (diag(kDiagBlockTrace)) {
    if (bt && threadIdx.x == 0) {
      bt[0] = block_trace_now();
      bt[6] = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_ID
      bt[7] = __builtin_amdgcn_s_getreg((31 << 11) | 20);  // XCC_ID
    }
  }
  return bt;
}
__device__ __forceinline__ void block_trace_wave_end(trace_t *bt, int lane, int wid) {
  if constexpr (diag(kDiagBlockTrace))
    if (bt && lane == 0 && wid < 4) bt[1 + wid] = block_trace_now();
}

}  // namespace dev
}  // namespace hspmv
