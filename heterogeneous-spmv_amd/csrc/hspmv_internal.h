// Internal interfaces shared by the host runtime (hspmv_runtime.h units), the
// launch planner (hspmv_plan.cpp) and the HIP kernels (spmv_kernels.hip).  Not
// part of the C ABI.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <vector>

#include "hspmv.h"

namespace hspmv {

// Device view of one CSR shard (rows [0, m) of the shard; global columns).
struct DevCSR {
  int32_t m = 0;
  int64_t n = 0;
  int64_t nnz = 0;
  const int32_t *row_ptr = nullptr;
  const int32_t *col_idx = nullptr;
  const void *val = nullptr;
  int32_t n_ssr = 0, n_sr = 0;          // CSR-3 maps (0 = none)
  const int32_t *outer = nullptr;
  const int32_t *inner = nullptr;
  // 16-bit column offsets (row kernels): col[k] = cbase[k >> kC16Shift] + col16[k]
  // plus bit 16+p of (col - base) in plane p: bit k&63 of cplanes[p*cplane_words + k/64]
  const uint16_t *col16 = nullptr;
  const int32_t *cbase = nullptr;
  const uint64_t *cplanes = nullptr;
  int32_t n_cplanes = 0, cplane_words = 0;
  // c16_mode 2 (STREAM only): col[k] = cbase[g] + col16[k] with g = the
  // nonzero's 64-row group, when every group's columns span < 65536
  int32_t c16_mode = 1;
  int32_t col_span_bits = 0;  // bits of the widest 256-nonzero block's column span (0 = unknown)
  // planner hints from the host tables: STREAM x windows / block x
  // dictionaries were built for this shard
  bool has_xwin = false, has_xdict = false;
  bool has_xdict_tasks = false;  // x dictionaries built for packed CSR3 tasks
  bool has_slices = false;       // ... and stored as row slices (DevPlan.sl)
  int32_t n_slabs = 1;        // x slabs: the row kernel's passes (each sees ~nnz / n_slabs)
  int32_t task_waves = 4;     // CSR3 wave tasks per workgroup: 4 (8 with 8-task dictionary
                              // blocks); the SSR plan: ssr_waves() per super-super-row
  bool has_csort = false;     // column-sorted row blocks were built (irregular gathers)
  bool slab_stream = false;   // x-slab passes with CSR-3 tasks: AUTO runs STREAM (slab_kernel_rule)
  int32_t serial_len = 0;     // median length of the rows summed serially (<= kSerialMax), 0 = none
};

// Planner choices of one handle.  The first block mirrors hspmv_options
// (include/hspmv.h; 0 = the library's choice); the second holds A/B-only
// knobs that product builds never change: only a diagnostic build
// (make diag-env: -DHSPMV_ENV_KNOBS) reads them, and the public fields, from
// HSPMV_* environment variables (tuning_from_env, hspmv_options.cpp), so a
// production handle's kernel choice cannot move with the environment.
struct Tuning {
  int csr3_plan = 0;        // 0/1 aligned 64-row tasks, 2 packed super-rows, 3 workgroup per SSR
  int task_nnz = 0;         // wave-task nonzero budget (0: 2048)
  int x_windows = 0;        // -1 off, 0 auto
  int x_dict = 0;           // -1 off, 0 auto, 1 whenever it fits
  int x_dict_cap = 0;       // LDS bytes per dictionary block (0: 20 KiB; <= 64 KiB)
  int x_slabs = 0;          // -1 off, 0 auto, B > 0 forced
  int col16_group = 0;      // -1 off, 0 auto, 1 whenever it fits
  int csort = 0;            // -1 off, 0 auto, 1 whenever it can be built
  int csort_parts = 0;      // 0 auto, 1/2/4
  int csort_u = 0;          // 0 auto, 4/8/16
  int stream_waves = 0;     // 0 auto, 1/2/4
  int deterministic = 0;    // 1: ordered row kernels (omp_spmv's order); 2: reproducible (fixed-point csort allowed)
  int serial_max = 0;       // A/B: the row kernels' serial bound (0: kSerialMax)
  int placement_trials = 0; // 0/1 off, K <= 8 array sets
  int row_slices = 0;       // -1 off, 0 auto, 1 whenever eligible (hspmv_slices.cpp)
  int ssr_w = 0;            // SSR plan waves per workgroup (0: ssr_waves(); A/B)
  int ssr_align = -1;       // SSR plan wave cut: 2 row-granular nnz balance (-1: default), 0 super-rows, 1 aligned pieces
  // A/B only (diagnostic builds)
  int contig = 0;           // hipDeviceMallocContiguous allocations
  int xd_waves = 0;         // packed CSR3 tasks per dictionary block (0: 4; 8)
  int xd_blocks_per_cu = 0; // CSR3 dictionary blocks sized for this many per CU (0: 6; -1: no cuts)
  double xslab_bytes = 0;   // x bytes per slab (0: 2 MiB)
  int csort_nt = -1, csort_pf = -1;      // -1: the library's choice
  int csort_blocks_per_cu = 0;           // row blocks per CU and part (0: 1)
  int csort_slot32 = -1;                 // fp32 LDS row slots (fp32 data)
  int csort_wide = -1;                   // 16-byte entry loads (interleaved layout)
  int csort_lds_cap = 0;                 // LDS bytes per workgroup for the row slots (0: all)
  int csort_seg = -1;                    // segmented chunks: 0 never, 2 always (-1: by conflicts)
  int csort_seg_extra = 0;               // serialised same-slot lanes that flag a chunk (0: default)
  int csort_trace = 0;                   // per-workgroup timestamps (hspmv_diag_csort_trace)
  int csort_long = 0;                    // rows above this many nonzeros are sliced (0: kLongRow)
  int csort_balance = 0;                 // -1: equal-width column parts, nnz-balanced rows (r03)
  int csort_fin_rows = 0;                // rows per finishing-pass thread (0: default; 1, 2, 4)
  int csort_dyn = -1;                    // chunks claimed from an LDS queue (-1: the library's choice)
  double csort_sweep_w = 0;              // column-part cost of a column per row block (0: kSweepPerRowBlock)
  double csort_slack = 0;                // widest column part / (n / H) when balancing (0: kPartSlack)
  int csort_part32 = -1;                 // fp32 row partials over fp64 slots (fp32 data; -1: on, 0 off)
  int lds_pad = -1;                      // STREAM padded product buffers (-1: by row length, 0 off, 1 on)
  int pf = -1, y_nt = -1, nt = -1;       // row kernels: prefetch, nt y stores, nt col/val
  int dyn_lds = 0;
  // internal (hspmv_create_updatable; no hspmv_options field): column-sorted
  // tables are built with their source-index table (CsortPlan::src)
  int csort_src = 0;
};

constexpr int kC16Shift = 8;  // 256 nonzeros per column-base block
constexpr int kXWin = 256;    // largest LDS-staged x window of a row group (entries)

enum Kernel : int { kAuto = 0, kVector = 1, kStream = 2, kCsr3 = 3, kCsort = 4 };

// Rows longer than this many nonzeros ("split rows") are cut into chunks of
// kLongChunk nonzeros, each summed by its own workgroup, and the chunk sums
// are added per row by a second small kernel (deterministic order).
constexpr int32_t kLongRow = 4096;
// Rows of up to this many nonzeros are summed serially (omp_spmv's order) by
// one lane in the row kernels; longer ones cooperatively (fixed DPP trees) --
// unless DevPlan.serial_max raises the bound (deterministic = 3).
constexpr int32_t kSerialMax = 40;
// fp32 data: 56 -- rows of 41-56 nonzeros summed serially ran 15-27 % faster
// than in the cooperative trees (d41 113.7 -> 83.0 us, d48 106.3 -> 90.2 at
// 48, profiles/r06s3/ab_serial48_f32.jsonl; d50 104.7 -> 81.8, d52 100.4 ->
// 80.4, d56 94.8 -> 80.2 at 56, r06s5), every other shape flat; 64 lost on
// d64 (+31 %, r06s2).  fp64 rows of 48 serially met in LDS banks (d48 +41 %,
// r06s2), so fp64 keeps 40.
constexpr int32_t kSerialMaxF32 = 56;
constexpr int32_t kLongChunk = 4096;

// ---- planner rules shared by plan_launch and the host tables: one
// definition each, asked with the shape or the flags

// Rows with more nonzeros than this are split rows (none: HSPMV_FLAG_NO_SPLIT).
inline int32_t split_threshold(unsigned flags) {
  return (flags & HSPMV_FLAG_NO_SPLIT) ? INT32_MAX : kLongRow;
}

// A matrix whose bytes stay under this is served from the 256 MiB Infinity
// Cache across back-to-back SpMVs (the planner's "resident" test).
constexpr double kMallResident = 192.0 * 1024 * 1024;
// The bytes one SpMV touches: values + 32-bit columns, row pointers + y, x.
// dtype: x and y; val_dtype: the stored values (a mixed handle's are fp32).
inline double footprint_bytes(int64_t m, int64_t n, int64_t nnz, int dtype, int val_dtype) {
  const double sx = dtype == HSPMV_F64 ? 8.0 : 4.0;
  const double sv = val_dtype == HSPMV_F64 ? 8.0 : 4.0;
  return (double)nnz * (sv + 4.0) + (double)m * (sx + 4.0) + (double)n * sx;
}
inline bool mall_resident(int64_t m, int64_t n, int64_t nnz, int dtype, int val_dtype) {
  return footprint_bytes(m, n, nnz, dtype, val_dtype) <= kMallResident;
}
// The L2 of one XCD: gathers from an x (or a row group's slice of x) beyond
// it miss L2.
constexpr double kXcdL2Bytes = 4.0 * 1024 * 1024;

// ---- the row kernels' block order: one definition for the kernels and the
// host (hspmv_block_order, tests/test_sweep.py)
#if defined(__HIPCC__)
#define HSPMV_HD __host__ __device__ __forceinline__
#else
#define HSPMV_HD inline
#endif
constexpr uint32_t kNumXcd = 8;

// Bijective XCD-aware block order (cdna_hip_programming.md §5 "XCD swizzle
// must be bijective").  Blocks b and b+8 share an XCD under round-robin
// dispatch; with chunk s > 1 each XCD takes s consecutive logical blocks in
// turn, so at any moment the 8 XCDs work on 8 adjacent runs of s blocks:
// s = nb/8 gives each XCD one contiguous eighth of the rows (x stays in
// that XCD's L2), small s keeps the whole chip's read front compact (HBM
// page locality) while rows still share x lines within an XCD.  s <= 1 is
// the dispatch order.  Blocks past the last full 8*s span keep their index.
HSPMV_HD uint32_t xcd_chunk_remap(uint32_t b, uint32_t nb, uint32_t s) {
  if (s <= 1) return b;
  const uint32_t span = kNumXcd * s;
  if (b >= (nb / span) * span) return b;
  const uint32_t i = b / kNumXcd, x = b % kNumXcd;
  return (i / s) * span + x * s + (i % s);
}

// The sweep direction rides in the top bit of the kernels' block-order
// argument (the chunk is at most 2^30): set, the remapped order is mirrored,
// grid index b runs logical block nb - 1 - remap(b).  The mirror comes after
// the remap, so consecutive logical blocks still share an XCD turn and the
// rows of y are the same bits: a row's sum never leaves its block.  A launch
// that sweeps the matrix against the direction of the one before it starts
// on the bytes that one touched last, which the 256 MiB Infinity Cache still
// holds (hspmv_set_sweep).
constexpr uint32_t kSweepReverse = 0x80000000u;
HSPMV_HD uint32_t sweep_block(uint32_t b, uint32_t nb, uint32_t order) {
  const uint32_t blk = xcd_chunk_remap(b, nb, order & ~kSweepReverse);
  return (order & kSweepReverse) ? nb - 1u - blk : blk;
}

// The fields of hspmv_options.flags (include/hspmv.h): the kernel code,
// HSPMV_LANES(l), HSPMV_U(u) (5 bits below HSPMV_FLAG_PREFETCH),
// HSPMV_XCD_CHUNK(s) (5 bits; 0 = automatic) and HSPMV_GROUPS(g) (3 bits; 1
// when unset), the last two decoded from their log2 + 1 codes.
inline unsigned flag_kernel(unsigned flags) { return flags & HSPMV_KERNEL_MASK; }
inline int flag_lanes(unsigned flags) { return (int)((flags & HSPMV_LANES_MASK) >> HSPMV_LANES_SHIFT); }
inline int flag_u(unsigned flags) { return (int)((flags >> HSPMV_U_SHIFT) & 0x1Fu); }
inline int32_t flag_xcd_chunk(unsigned flags) {
  const unsigned code = (flags >> HSPMV_XCD_CHUNK_SHIFT) & 0x1Fu;
  return code ? 1 << (code - 1) : 0;
}
inline int32_t flag_groups(unsigned flags) {
  const unsigned code = (flags >> HSPMV_GROUPS_SHIFT) & 0x7u;
  return code ? 1 << (code - 1) : 1;
}

// Column-sorted row blocks (csort.hip): workgroup b works on column part
// b % H (a fixed slice of x) and walks chunks [blk_c[b], blk_c[b+1]) of 64*u
// entries in column order; its rows are [blk_r[2b], blk_r[2b+1]) (each part
// has its own row partition) and its long-row slices vslice[blk_v[b] ..
// blk_v[b+1]).  Built by build_csort (hspmv_csort_build.cpp).
constexpr int kCsortThreads = 1024;
constexpr int kCsortMaxLds = 160 * 1024;
// the kernel's static LDS (its chunk-queue head, 16 B with alignment) comes
// out of the same budget as the row slots (build_csort)
constexpr int kCsortStaticLds = 16;
// Diagnostic trace of a csort launch (DevCsort.trace, HSPMV_CSORT_TRACE=1):
// per workgroup kCsortTraceSlots u64 = {start, end, XCC_ID | HW_ID << 32,
// after the slot-zeroing barrier, then per wave: its end (after its last
// chunk), then per wave: the chunks it ran} (s_memrealtime, 100 MHz).
constexpr int kCsortTraceSlots = 4 + 2 * (kCsortThreads / 64);
// Fixed-point slots: every product rounds to an integer below 2^kCsortFixBits
// (values scaled to |v'| < 1 per row, x to |x'| < 2^kCsortFixBits), so a slot
// of <= 4096 products stays below 2^62; the pre-pass runs kCsortXexpBlocks
// workgroups at most.
constexpr int kCsortFixBits = 50;
constexpr int kCsortXexpBlocks = 256;
constexpr int64_t kCsortXexpChunk = 8192;  // x entries per pre-pass block and chunk
constexpr int32_t kCsortXexpNonFinite = 0x7fffffff;
struct DevCsort {
  int32_t n_wg = 0, H = 1, u = 16, direct = 0, n_long = 0;
  bool nontemporal = true;
  bool prefetch = false;  // next chunk's entries loaded during this chunk's gathers
  bool slot32 = false;    // fp32 LDS row slots and partials (fp32 data; A/B)
  bool wide = false;      // 16-byte entry loads (host-interleaved layout)
  bool dyn = false;       // waves claim the workgroup's chunks from an LDS queue
  bool part32 = false;    // fp32 row partials over fp64 slots (fp32 data; the default)
  // Reproducible (fixed-point) row sums (hspmv_options.deterministic = 2):
  // the slots are int64 sums of each product rounded to an integer at scale
  // 2^(kCsortFixBits - xexp - rexp[row]); xexp = the max exponent of |x|,
  // found per SpMV by hspmv_csort_xexp into xexp_part[n_xexp] (csort.hip)
  bool fixed = false;
  const int16_t *rexp = nullptr;  // per row: the exponent its values were scaled by (2^rexp)
  const int16_t *sexp = nullptr;  // per long-row slice: its row's rexp
  int32_t *xexp_part = nullptr;   // per pre-pass block: max frexp exponent of |x| (INT32_MAX: non-finite)
  int32_t n_xexp = 0;
  int64_t n_x = 0;                // x entries the pre-pass reads
  int32_t fin_rows = 0;   // rows per finishing-pass thread (0: 4, or the most m allows)
  int64_t m = 0;
  int32_t lds_bytes = 0;
  const int32_t *blk_c = nullptr, *blk_r = nullptr, *blk_v = nullptr, *vslice = nullptr;
  int32_t row_blocks = 0;  // blocks per column part (the parts' own row partitions)
  unsigned long long *trace = nullptr;  // diagnostic builds: per-workgroup {start, end, hw_id} (s_memrealtime)
  const int32_t *cbase = nullptr;
  const void *ent = nullptr;  // fp32: {idx, val} records; fp64: idx
  const void *val = nullptr;  // fp64 values (nullptr for fp32)
  void *part = nullptr, *spart = nullptr;  // partial sums in the slot type
  const uint32_t *long_mask = nullptr;
  const int32_t *long_row = nullptr, *long_cs = nullptr;
  // Updatable handles only (hspmv_create_updatable; else nullptr): per
  // entry-stream position, at the position of the entry's VALUE, the CSR index
  // of the nonzero stored there, kCsortSrcPad for padding (refresh.hip)
  const uint32_t *src = nullptr;
  int64_t chunks = 0;    // all workgroups' chunks (blk_c[n_wg])
  int32_t n_slices = 0;  // long-row slices (long_cs[n_long])
  int32_t long_t = 0;    // rows above this many nonzeros are long rows (the `extra` term of rexp)
};
constexpr uint32_t kCsortSrcPad = 0xFFFFFFFFu;

// Device-side tables the host planner builds once per shard (all optional),
// one record per table family: the upload that builds a family fills its
// record, and a launch reads the records build_plan_tables selected.
// CSR-3: wave task t covers rows [start[t], start[t+1]); either super-rows
// packed into <= 64-row tasks (default), or waves_per_block tasks per
// super-super-row, nnz-balanced on super-row boundaries (HSPMV_CSR3_PLAN=ssr).
struct DevTasks {
  const int32_t *start = nullptr;
  int32_t n = 0;
  // 1: a task's 64-row groups end on multiples of 64 (its first group may be
  // shorter) -- the SSR plan's aligned cut (ssr_tasks_aligned); 0: groups of
  // 64 rows from the task's first row
  int32_t align = 0;
};
// split rows
struct DevSplit {
  int32_t long_t = 0x7fffffff;  // rows with more nonzeros are split rows
  int32_t n_long = 0, n_chunks = 0;
  bool long_serial = false;  // split rows summed in order by hspmv_long_serial (deterministic = 3)
  // ... on a stream of their own, forked from and joined back into the
  // launch stream, so they run beside the row kernel instead of after it
  hipStream_t long_stream = nullptr;
  hipEvent_t long_fork = nullptr, long_join = nullptr;
  const int32_t *long_row = nullptr;    // n_long row ids (shard-local)
  const int32_t *long_cstart = nullptr; // n_long+1, chunk ranges per split row
  const int32_t *chunk_k = nullptr;     // 2*n_chunks: [k0, k1) per chunk
  void *partials = nullptr;             // n_chunks partial sums (dtype)
};
// Block x dictionaries (STREAM with one group per wave: 256-row blocks;
// CSR3: blocks of four packed tasks): blk[b], blk[b+1] bound block b's
// {x_start, lds_off} run records in runs (int2), the last a sentinel
// {0, entries}; col16 then holds each nonzero's position in the staged xs.
// lds_bytes = the largest block's dictionary (dynamic LDS per block).
struct DevXdict {
  const int32_t *blk = nullptr;
  const void *runs = nullptr;
  int32_t lds_bytes = 0;
};
// Row slices (hspmv_slices.cpp): the dictionary handle's matrix stored per
// 64-row wave task column-major, one lane per row (hspmv_slices,
// slice_kernel.cuh).  desc: {prefix, first row} per task and a closing pair
// ({padded slot columns, m}); slice t's values start at val + 64 * prefix
// elements; len: one length per row.  Positions: pos_bits = 16, slice t's
// start at pos + 64 * prefix; 12, the packed stream, slice t's at
// 128 * ppre[t] bytes.  DevPlan.sl is set only when the launch runs the slice
// kernel.
struct DevSlices {
  const int32_t *desc = nullptr;
  const uint8_t *len = nullptr;
  const uint16_t *pos = nullptr;
  const int32_t *ppre = nullptr;
  int32_t pos_bits = 0;
  void *val = nullptr;  // (the value refresh writes it, refresh.hip)
  int32_t n = 0;  // descriptors (= wave tasks, the empty ones included)
};
// x slabs (irregular gathers, x larger than an XCD's L2): the columns are
// cut into n equal ranges and the row kernel runs once per slab over a
// slab-major copy of the matrix -- pass b reads rows
// [rp[b*(m+1) + r], rp[b*(m+1) + r + 1]) of col / val, so its gathers stay
// inside one L2-sized slice of x.  Split rows have empty slab segments (the
// split-row kernels sum them from the CSR).
struct DevSlabs {
  int32_t n = 0;
  const int32_t *rp = nullptr;
  const int32_t *col = nullptr;
  void *val = nullptr;  // (the value refresh writes it, refresh.hip)
};
struct DevPlan {
  DevTasks tasks;
  DevSplit split;
  int32_t serial_max = kSerialMax;  // rows up to this length are summed serially (fp32: kSerialMaxF32)
  // x windows per row group (STREAM: 64-row groups; CSR3: packed tasks):
  // {lo, w} (int32), w = 0 when the group's columns span more than kXWin
  // entries (then it gathers from global x)
  const void *xwin = nullptr;
  DevXdict xd;
  DevSlices sl;
  DevSlabs slabs;
  DevCsort cs;  // kCsort
};

struct LaunchPlan {
  int kernel = kStream;
  int lanes = 64;          // VECTOR: lanes per row; STREAM/CSR3: 64 rows per wave pass
  int waves_per_block = 4; // CSR3: waves per super-super-row workgroup
  int u = 8;               // STREAM/CSR3: elements per lane per LDS chunk
  bool nontemporal = false;
  bool prefetch = false;   // STREAM/CSR3: next chunk's col/val issued early
  bool y_nt = false;       // STREAM/CSR3: nontemporal y stores
  int32_t dyn_lds = 0;     // extra dynamic LDS per block (occupancy experiments)
  int32_t xcd_chunk = 1;   // blocks per XCD turn (1 = dispatch order; see xcd_chunk_remap)
  bool reverse = false;    // STREAM/CSR3/slices: this launch sweeps the blocks last to first (launch_spmv)
  int32_t groups = 1;      // STREAM: 64-row groups per wave (next group's rp prefetched)
  int32_t carry = 0;       // STREAM/CSR3: rows start from y (x-slab passes after the first)
  bool lds_pad = false;     // STREAM: bank-padded product buffers (row_kernels.cuh lds_ix)
  bool row_slices = false;  // STREAM/CSR3 with dictionaries: the lane-per-row slice kernel
  int64_t blocks = 0;
};

// Waves of the workgroup-per-super-super-row CSR-3 plan: ~64 rows per wave
// (one lane per row in the ordered sums), from the mean rows per SSR.
inline int ssr_waves(double rows_per_ssr) {
  const double w = rows_per_ssr / 64.0;
  return w >= 6.0 ? 8 : (w >= 3.0 ? 4 : (w >= 1.5 ? 2 : 1));
}

// Chooses kernel / lanes / block shape for a shard (host-side heuristic,
// hspmv_plan.cpp).
// rows_per_ssr: mean rows per super-super-row (CSR-3 workgroup-per-SSR plan);
// packed_tasks > 0: CSR-3 tasks packed from super-rows (4 per workgroup).
// dtype: the vectors' (every launch-shape rule follows it: the LDS product
// buffers hold it); val_dtype: the stored values' (the footprint, the matrix
// streams' addressing).
LaunchPlan plan_launch(const DevCSR &A, int dtype, int val_dtype, unsigned flags, double rows_per_ssr,
                       int64_t packed_tasks, const Tuning &t);

// STREAM / CSR3 row kernels (stream_f32.hip / stream_f64.hip).
hipError_t launch_rows_f32(const DevCSR &A, const DevPlan &dp, const LaunchPlan &p,
                           const float *x, float *y, hipStream_t st);
hipError_t launch_rows_f64(const DevCSR &A, const DevPlan &dp, const LaunchPlan &p,
                           const double *x, double *y, hipStream_t st);
// ... of a mixed handle: A.val / dp.sl.val / dp.slabs.val hold float
// (stream_f32v64.hip)
hipError_t launch_rows_f32v64(const DevCSR &A, const DevPlan &dp, const LaunchPlan &p,
                              const double *x, double *y, hipStream_t st);

// Column-sorted row-block kernel + its finishing pass (csort.hip).
hipError_t launch_csort(const DevCsort &c, int dtype, const void *x, void *y, hipStream_t st);

// Enqueues one y = A*x (main kernel + split-row kernels when present).
// reverse: the STREAM / CSR3 / slice row kernel (each x-slab pass of it)
// sweeps its blocks last to first; the launches keep their order, and the
// vector, column-sorted and split-row kernels always run forward.
// dtype: x, y, products and sums; val_dtype: the stored values (equal, or
// HSPMV_F32 under HSPMV_F64: the mixed handles).
hipError_t launch_spmv(const DevCSR &A, const DevPlan &dp, int dtype, int val_dtype, const LaunchPlan &plan,
                       const void *x, void *y, hipStream_t stream, bool reverse = false);

// ---- y = alpha (A x) + beta y (hspmv_spmv_axpby).  The
// scalars as the caller gave them; each launch converts them to the vectors'
// type once, on the host.
struct AxpbyScalars {
  double alpha, beta;
};
// Whether the fused path can run the shard: its launch is the slice kernel
// alone (no x slabs, no split rows beside it).
inline bool axpby_fusable(const DevCSR &A, const DevPlan &dp) {
  return A.m > 0 && dp.sl.desc && dp.slabs.n == 0 && dp.split.n_long == 0;
}
// The fused path: hspmv_slices_axpby in place of hspmv_slices (the stream_*
// units hold the instantiations); y is read (beta != 0) and written.
hipError_t launch_slices_axpby_f32(const DevPlan &dp, const LaunchPlan &p, const AxpbyScalars &ab,
                                   const float *x, float *y, hipStream_t st);
hipError_t launch_slices_axpby_f64(const DevPlan &dp, const LaunchPlan &p, const AxpbyScalars &ab,
                                   const double *x, double *y, hipStream_t st);
hipError_t launch_slices_axpby_f32v64(const DevPlan &dp, const LaunchPlan &p, const AxpbyScalars &ab,
                                      const double *x, double *y, hipStream_t st);
// launch_spmv's counterpart for a shard that is axpby_fusable (else
// hipErrorInvalidValue): one kernel, the sweep direction as there.
hipError_t launch_spmv_axpby(const DevCSR &A, const DevPlan &dp, int dtype, int val_dtype, const LaunchPlan &plan,
                             const AxpbyScalars &ab, const void *x, void *y, hipStream_t stream,
                             bool reverse = false);
// The two-pass path's second pass (axpby.hip): y[i] = alpha s[i] + beta y[i]
// for m elements of dtype, y never read when beta converts to 0; y_nt: the
// plan's nontemporal y stores.  s and y must not overlap.
hipError_t launch_axpby(int dtype, int64_t m, const AxpbyScalars &ab, bool y_nt, const void *s, void *y,
                        hipStream_t stream);

// ---- w . y and y . y from the pass that writes y (hspmv_spmv_axpby_dot,
// DESIGN.md §5f).  What one launch reads and writes beside y:
struct DotArgs {
  const void *w;     // m entries of the vector dtype; nullptr: w . y not asked for (never read)
  bool yy;           // y . y asked for
  double *partials;  // {wy, yy} pairs, 16-byte aligned: one per slice (fused) / per workgroup (two-pass)
};
// A shard's three buffers of the dot calls (Shard::dot), each allocated
// through its DevCtx by the first call that needs it and freed with it.
// partials: n_fused pairs for the slice kernel (one per wave task, zeroed
// once: a task without rows never writes its pair), then n_2p pairs for the
// two-pass kernel's workgroups.
struct DevDot {
  void *d_w = nullptr;         // own w (m entries; hspmv_set_w)
  const void *w = nullptr;     // w in use (own or bound); nullptr: none yet
  double *d_part = nullptr;
  int64_t n_fused = 0, n_2p = 0;
  double *d_out = nullptr;     // own {wy, yy}
  double *out = nullptr;       // bound results (hspmv_bind_dots_device); nullptr: d_out
  double *last = nullptr;      // where the last dot call wrote (hspmv_get_dots); nullptr: no call yet
};
// Workgroups hspmv_axpby_dot runs for m rows at most (its partials).
inline int64_t axpby_dot_blocks(int64_t m) { return (m + 255) / 256; }
// The fused path's kernel: launch_spmv_axpby with hspmv_slices_axpby_dot;
// dot.partials holds dp.sl.n pairs.
hipError_t launch_slices_axpby_dot_f32(const DevPlan &dp, const LaunchPlan &p, const AxpbyScalars &ab,
                                       const DotArgs &dot, const float *x, float *y, hipStream_t st);
hipError_t launch_slices_axpby_dot_f64(const DevPlan &dp, const LaunchPlan &p, const AxpbyScalars &ab,
                                       const DotArgs &dot, const double *x, double *y, hipStream_t st);
hipError_t launch_slices_axpby_dot_f32v64(const DevPlan &dp, const LaunchPlan &p, const AxpbyScalars &ab,
                                          const DotArgs &dot, const double *x, double *y, hipStream_t st);
hipError_t launch_spmv_axpby_dot(const DevCSR &A, const DevPlan &dp, int dtype, int val_dtype,
                                 const LaunchPlan &plan, const AxpbyScalars &ab, const DotArgs &dot, const void *x,
                                 void *y, hipStream_t stream, bool reverse = false);
// The two-pass path's second pass (axpby.hip): launch_axpby's update and
// stores, and each workgroup's pair into dot.partials[block] (at most
// axpby_dot_blocks(m) of them); *n_partials: how many it wrote.
hipError_t launch_axpby_dot(int dtype, int64_t m, const AxpbyScalars &ab, bool y_nt, const void *s, void *y,
                            const DotArgs &dot, int64_t *n_partials, hipStream_t stream);
// Both paths' last launch: out[0..1] (8-byte aligned) = the sums of the n
// pairs, in an order that depends on n alone (one workgroup of 1024 threads).
hipError_t launch_dot_finish(const double *partials, int64_t n, double *out, hipStream_t stream);

// ---- value refresh (refresh.hip; hspmv_update_values, hspmv_update.cpp):
// the derived copies of the values rebuilt on the device from src, the new
// values in the shard's CSR order (val_dtype: the stored values').  Both
// enqueue one kernel on st, or nothing for an empty table.
// The row slices' value stream dst (DevSlices.val) of n_slices descriptors
// desc with the row lengths len; row_ptr: the shard's CSR row pointers.
hipError_t launch_refresh_slices(int val_dtype, int64_t n_slices, const int32_t *desc, const uint8_t *len,
                                 const int32_t *row_ptr, const void *src, void *dst, hipStream_t st);
// The x slabs' slab-major values dst (DevSlabs.val) of the n_slabs
// row-pointer arrays slab_rp, m + 1 entries each.
hipError_t launch_refresh_slabs(int val_dtype, int32_t m, int64_t nnz, int32_t n_slabs, const int32_t *row_ptr,
                                const int32_t *slab_rp, const void *src, void *dst, hipStream_t st);

// The column-sorted entry stream of an updatable shard (c.src set): every
// value of c.ent (fp32 records) / c.val (fp64) rewritten from src_val through
// c.src, scaled by 2^rexp of its row under fixed-point slots; padding 0.
// Writes the shard's own tables (the views of DevCsort are const for the SpMV).
hipError_t launch_refresh_csort(int val_dtype, const DevCsort &c, const void *src_val, hipStream_t st);
// Fixed-point shards: c.rexp and c.sexp restated from src_val (row_scales,
// hspmv_csort_build.cpp); enqueue it before launch_refresh_csort.
hipError_t launch_refresh_row_scales(int val_dtype, const DevCsort &c, const int32_t *row_ptr,
                                     const void *src_val, hipStream_t st);

// ---- multi-vector SpMM (spmm.hip, hspmv_mm.cpp): Y = A X, X row-major n x k
constexpr int32_t kMmMaxRhs = 32;
// Lanes one row takes: the smallest power of two >= k (k in [1, kMmMaxRhs]).
inline int32_t mm_lanes_per_row(int32_t k) {
  int32_t kp = 1;
  while (kp < k) kp *= 2;
  return kp;
}
// Grid of the row kernel: four waves per workgroup, 64 / kp rows per wave.
inline int64_t mm_blocks(int64_t m, int32_t kp) {
  const int64_t rows = 4 * (64 / kp);
  return (m + rows - 1) / rows;
}
// Rows up to this many nonzeros carry omp_spmv's bits: the single-vector
// kernels' serial bound of the dtype.
inline int32_t mm_serial_max(int dtype) { return dtype == HSPMV_F64 ? kSerialMax : kSerialMaxF32; }
// The ids of the rows over serial_max nonzeros, ascending (host only, no
// device call: tools/spmm_plan_check.cpp runs it under the sanitizers).
void mm_long_rows(const int32_t *row_ptr, int64_t m, int32_t serial_max, std::vector<int32_t> &rows);
struct DevMM {
  int32_t m = 0;
  int64_t nnz = 0;
  int32_t k = 1, lanes_per_row = 1;
  int32_t serial_max = kSerialMax;
  bool nontemporal = false;
  const int32_t *row_ptr = nullptr;
  const int32_t *col_idx = nullptr;
  const void *val = nullptr;
  const int32_t *long_row = nullptr;  // n_long row ids for the wave-per-row kernel
  int32_t n_long = 0;
};
// Enqueues one Y = A X (the row kernel, then the long-row kernel when the
// table is not empty).  Checks m, nnz, the leading dimensions and the grid
// first: HSPMV_OK or an HSPMV_E_* code with the message set.
int launch_spmm(const DevMM &d, int dtype, const void *X, int64_t ldx, void *Y, int64_t ldy,
                hipStream_t stream);

}  // namespace hspmv
