// hspmv_runtime.h -- the host runtime's internal state and the functions its
// units share (not part of the C ABI).  The runtime is split by concern:
//   hspmv_options.cpp      hspmv_options -> Tuning (+ diagnostic env knobs)
//   hspmv_plan.cpp         plan_launch: the kernel and launch shape of a shard
//                          (sees hspmv_internal.h only, not this header)
//   hspmv_shard.cpp        DevCtx (the owner of device memory, streams and
//                          events), upload, launch-plan finish and placement
//                          trials of one row-range shard, the checks and the
//                          timing loop the single- and multi-vector paths share
//   hspmv_tables.cpp       host planner tables: 16-bit columns, wave tasks,
//                          x windows, x slabs, split rows, CSR-3 SSR tasks;
//                          host-only planners (plan_col16, plan_col16g ->
//                          Col16Plan; plan_xslabs -> XslabPlan; plan_split_rows
//                          -> SplitPlan; median_serial_len, wants_csort,
//                          c16_saved_of over SavedTerms), their uploads
//                          (upload_col16, upload_xslabs, upload_split_rows) and
//                          the two sequences build_row_tables (fills the
//                          records of Shard::built) / build_plan_tables
//                          (selects the ones the launch reads into Shard::dp)
//   hspmv_xdict.cpp        block x dictionaries (+ hspmv_xdict_plan), the
//                          plan entry points' shared preamble (plan_shape)
//   hspmv_slices.cpp       row slices of dictionary handles (+ hspmv_slices_plan)
//   hspmv_csort_build.cpp  column-sorted row blocks (csort.hip's tables):
//                          plan_csort (host only), upload_csort, build_csort
//   hspmv_update.cpp       new values for a planned shard (hspmv_update_values)
//   hspmv_multi.cpp        the row-range partition over devices, RCCL
//   hspmv_api.cpp          the C ABI entry points
//
// Replaces the CSRk_Graph device plumbing of the reference
// (cuda-spmv-csrk/hip/csrk.cu:92-113, 531-641, 722-870): device buffers are
// owned by a handle instead of process globals, every HIP/RCCL status is
// checked, and there is one stream per GPU instead of the default stream +
// hipDeviceSynchronize.
#pragma once
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdint>
#include <functional>
#include <thread>
#include <vector>

#include "hspmv_common.h"
#include "hspmv_internal.h"

#define HIP_TRY(expr)                                                              \
  do {                                                                             \
    hipError_t _e = (expr);                                                        \
    if (_e != hipSuccess)                                                          \
      return set_error(HSPMV_E_HIP, "%s failed: %s (%s:%d)", #expr,                \
                       hipGetErrorString(_e), __FILE__, __LINE__);                 \
  } while (0)

namespace hspmv {

// The owner of one device's side of a shard or an SpMM operator.  The
// ownership rule of the whole runtime: what a DevCtx allocated or created it
// frees -- early through release(), else in its destructor -- and nothing
// else is ever freed.  Every other device pointer (Shard::d_*, the matrix
// arrays; DevCSR; the table records of Shard::built and Shard::dp, DevCsort
// among them; DevMM) is a view: into one of these allocations, or a caller's
// borrowed array, which never enters a context.
// alloc / upload / open / new_* expect `device` to be the current device.
struct DevCtx {
  int device = 0;
  hipStream_t stream = nullptr;  // launches: the caller's, or one this context created
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // the timing pair (open)
  // Tuning.contig (A/B, diagnostic builds): physically contiguous allocations
  // (hipDeviceMallocContiguous; the plain allocation when that fails)
  bool contig = false;

  DevCtx() = default;
  DevCtx(DevCtx &&o) noexcept;  // leaves o empty
  DevCtx(const DevCtx &) = delete;
  DevCtx &operator=(const DevCtx &) = delete;
  // Frees every live allocation, owned event and owned stream on `device`;
  // does not synchronise.
  ~DevCtx();

  // bytes of device memory (16 for a size of 0) into *p, recorded as owned
  template <typename T>
  int alloc(T **p, size_t bytes) {
    void *q = nullptr;
    const int rc = alloc_raw(&q, bytes);
    *p = static_cast<T *>(q);
    return rc;
  }
  // alloc + the host-to-device copy of the same bytes (none when bytes == 0)
  template <typename T>
  int upload(T **p, const void *src, size_t bytes) {
    void *q = nullptr;
    const int rc = upload_raw(&q, src, bytes);
    *p = static_cast<T *>(q);
    return rc;
  }
  // Frees one owned allocation now and forgets it; a pointer this context
  // does not own (a borrowed array, nullptr) is left alone.
  void release(const void *p);
  int64_t bytes() const;  // the live allocations' recorded sizes (hspmv_info.device_bytes)
  // The launch stream -- the caller's, or a new non-blocking one -- and ev0 / ev1.
  int open(void *caller_stream);
  // An extra owned non-blocking stream / event without timing (the serial
  // long-row fork and join).
  int new_stream(hipStream_t *st);
  int new_event(hipEvent_t *ev, unsigned flags = hipEventDisableTiming);

 private:
  struct Block {
    void *ptr;
    size_t bytes;
  };
  std::vector<Block> blocks_;
  std::vector<hipStream_t> streams_;
  std::vector<hipEvent_t> events_;
  int alloc_raw(void **p, size_t bytes);
  int upload_raw(void **p, const void *src, size_t bytes);
};

// What a launch reads instead of the 32-bit CSR streams, and the numbers the
// bytes it saves are worked out from (c16_saved_of: Shard::c16_saved).
enum SavedFormat { kFmtCol32 = 0, kFmtCsort, kFmtSlices, kFmtDict, kFmtGroup16, kFmtBlock16, kFmtSlabs };
struct SavedTerms {
  int dtype = HSPMV_F64, val_dtype = HSPMV_F64;
  int64_t m = 0, nnz = 0, long_nnz = 0, x_entries = 0;
  double csort_format_bytes = 0.0;                      // kFmtCsort
  int64_t sl_padded = 0, sl_pos_bytes = 0, sl_desc_n = 0;  // kFmtSlices
  int64_t xd_runs_n = 0, xd_entries = 0, blocks = 0;    // kFmtSlices, kFmtDict
  int64_t groups = 0;                                   // kFmtGroup16: the bases read
  int n_cplanes = 0, n_slabs = 0;                       // kFmtBlock16; kFmtSlabs
};

// The host copies a shard is planned from.  upload_shard (a borrowed matrix:
// create_single) fills rp, outer and inner; build_row_tables the wave tasks
// (build_xdict may cut them) and the x windows, which it empties again when
// another table is taken.  build_plan_tables reads them last: finish_shard
// releases the whole record once that has returned.
struct HostTables {
  std::vector<int32_t> rp, outer, inner;  // row pointers and CSR-3 maps, rebased to the shard
  std::vector<int32_t> tasks;             // CSR-3 wave tasks (build_tasks)
  std::vector<int32_t> xwin, xwin_t;      // x windows per 64-row group / per packed CSR-3 task
};

// One row-range shard on one GPU: views, host tables and the plan; dev owns
// the device side.
struct Shard {
  DevCtx dev;
  int64_t row0 = 0;  // first global row
  int64_t nnz0 = 0;  // first global nonzero (hspmv_update_values: the shard's range of val)
  // dtype: x, y, the products and the sums; val_dtype: the stored values
  // (A.val, the slab and slice copies).  Equal, or HSPMV_F32 under HSPMV_F64
  // (hspmv_create_mixed).  Set before upload_shard / build_row_tables.
  int dtype = HSPMV_F64, val_dtype = HSPMV_F64;
  DevCSR A;          // device view (rows rebased to 0)
  LaunchPlan plan;
  double mean_rows_per_ssr = 0.0;
  // views of dev's allocations: the matrix arrays, and the 16-bit column trio
  // (writable slots: the placement trials repoint them)
  int32_t *d_rp = nullptr, *d_ci = nullptr, *d_outer = nullptr, *d_inner = nullptr;
  uint16_t *d_c16 = nullptr;  // 16-bit column offsets
  int32_t *d_cbase = nullptr;
  uint64_t *d_cplanes = nullptr;
  // Every other device table has one record (DevPlan's, hspmv_internal.h),
  // filled once by the upload_* / build_* that makes the table: into `built`,
  // what this shard has on the device.  dp is what the launch reads:
  // build_plan_tables takes a record of `built` whole, or leaves dp's empty
  // when the planned launch shape cannot read that table.
  DevPlan built, dp;
  int64_t xd_cut = 0;                // CSR3 dictionary blocks cut in two (split_xd_blocks)
  int xd_shape = 0;                  // 0 none, kStream (256-row blocks), kCsr3 (4 packed tasks)
  // The report's numbers (c16_saved_of, hspmv_info): each upload writes its
  // table's terms, build_plan_tables those of the planned launch.
  SavedTerms saved;
  int64_t csort_chunks = 0, csort_seg_chunks = 0;  // chunks, and those stored slot-sorted
  std::vector<int64_t> csort_wg_stats;  // diagnostic builds: 8 cost terms per workgroup
  int64_t csort_part_begin[4] = {0, 0, 0, 0};  // first column of each column part
  int c16g_shape = 0;                // group-base columns built for kStream groups / kCsr3 tasks
  HostTables host;
  void *d_val = nullptr;   // own values (none for a borrowed matrix)
  void *d_x = nullptr;     // own x (n entries)
  void *d_y = nullptr;     // own y (m_shard entries) -- or a view into d_yfull
  void *d_yfull = nullptr; // multi-GPU: padded all-gather buffer P*max_rows
  void *d_axpby = nullptr; // hspmv_spmv_axpby's two-pass scratch (m entries; from the first such call on)
  DevDot dot;              // hspmv_spmv_axpby_dot's w, partials and results (each from the first call that needs it)
  const void *x = nullptr; // x in use (own or bound)
  void *y = nullptr;       // y in use (own or bound)
  int64_t x_entries = 0;   // distinct columns of this shard
  double c16_saved = 0.0;  // bytes per SpMV the 16-bit column offsets save
  // placement trials (place_shard): SpMV time of each array set, the kept one
  std::vector<double> place_us;
  int place_pick = 0;
  double heavy_frac = -1.0;  // x-slab handles with CSR3 tasks: nonzeros in heavy 64-row groups (slab_kernel_rule)
  Tuning tune;  // the handle's planner choices (hspmv_options)
};

}  // namespace hspmv

struct hspmv_handle {
  std::vector<hspmv::Shard> shards;
  int64_t m = 0, n = 0, nnz = 0;
  int dtype = HSPMV_F64;      // x, y, products and sums
  int val_dtype = HSPMV_F64;  // the stored matrix values (hspmv_create_mixed: HSPMV_F32 under HSPMV_F64)
  int64_t n_ssr = 0, n_sr = 0;
  unsigned flags = 0;
  bool x_set = false;
  int64_t max_rows = 0;   // multi-GPU padding for the y all-gather
  bool sharded = false;   // row-range partition (hspmv_create_sharded / num_gpus > 1)
  int64_t x_entries() const {
    int64_t t = 0;
    for (auto &s : shards) t += s.x_entries;
    return t;
  }
  std::vector<ncclComm_t> comms;
  int rccl_version = 0;   // ncclGetVersion of the RCCL this process resolved
  // hspmv_set_sweep: the mode, and the parity of the SpMV calls so far (one
  // flip per hspmv_spmv / hspmv_run iteration, the same for every shard)
  int sweep_mode = HSPMV_SWEEP_AUTO;
  bool sweep_phase = false;
  int axpby_mode = HSPMV_AXPBY_AUTO;  // hspmv_set_axpby_path
};

namespace hspmv {

// The host tables' thread pool: body(lo, hi, t) over [0, n) cut into nt equal
// ranges, one thread each, nt = n / grain, at least 1 (which runs inline)
// and at most 16.
template <typename F>
inline void parallel_ranges(int64_t n, int64_t grain, F &&body) {
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(16, n / grain));
  if (nt == 1) return (void)body((int64_t)0, n, 0);
  std::vector<std::thread> th;
  for (int t = 0; t < nt; ++t) th.emplace_back([&, t]() { body(n * t / nt, n * (t + 1) / nt, t); });
  for (auto &x : th) x.join();
}

// ---- hspmv_options.cpp
int tuning_from_options(const hspmv_options *o, Tuning *t);
void tuning_from_env(Tuning *t);
Tuning default_tuning();
int check_deterministic(unsigned flags, const Tuning &t);

// ---- hspmv_shard.cpp
// HSPMV_E_NODEV unless `device` is one of the visible devices (*ndev of them).
int check_device(int device, int *ndev = nullptr);
// A borrowed device CSR (HSPMV_FLAG_DEVICE_PTRS) on the current device: the
// description, then what the kernels index with -- the row pointers and the
// columns, read back into rp and cols -- validated on the host before the
// first launch.  The values are only null-checked.
int read_device_csr(const hspmv_csr *A, std::vector<int32_t> &rp, std::vector<int32_t> &cols);
// The reference timing protocol (hspmv_run, hspmv_mm_run): enqueue(p) puts
// one iteration's work of devs[p] on its stream.  `warmup` iterations, each
// synchronised, then `iters` timed ones: device time ev0 -> ev1 (the maximum
// over devs) and wall time, min / max / mean into out's t_*, wall_* and
// iters; everything else in *out is zeroed.
int timed_run(const std::vector<DevCtx *> &devs, int warmup, int iters,
              const std::function<int(size_t)> &enqueue, hspmv_timing *out);
int upload_shard(Shard &s, const hspmv_csr *A, const hspmv_csr3_maps *mp, int64_t r0, int64_t r1,
                 int64_t ssr0, int64_t ssr1, int64_t y_rows_alloc, unsigned flags);
int finish_shard(Shard &s, unsigned flags, void *stream);
int place_shard(Shard &s, int64_t n);

// ---- hspmv_tables.cpp
int64_t count_distinct_cols(const int32_t *col, int64_t nnz, int64_t n);
bool csr3_packed(const Tuning &t);
bool csr3_fill(const Tuning &t);
void build_tasks(const int32_t *rp, int64_t m, const std::vector<int32_t> *inner,
                 const std::vector<int32_t> *outer, unsigned flags, const Tuning &tune,
                 std::vector<int32_t> &ts, int *waves);
bool irregular_gathers(const int32_t *rp, const int32_t *col, int64_t m, double sv);
// The row kernels' tables are planned on the host apart from their upload:
// the plan_* functions make no HIP call and touch no Shard, fill a plain
// struct and return whether the table is taken (dtype: the vectors',
// val_dtype: the stored values'); the upload_* functions hold the uploads and
// allocations and fill the table's record in Shard::built, its terms in
// Shard::saved and its DevCSR hints, nothing else.  A plan is a local that
// dies once its upload returns.
// tools/row_tables_check.cpp decodes every table back into the matrix
// (make asan-row-tables; tests/test_row_tables_plan.py).
//
// 16-bit column offsets (DevCSR.col16 / cbase / cplanes).
struct Col16Plan {
  int mode = 1;                  // DevCSR.c16_mode: 1 a base per 2^kC16Shift nonzeros, 2 per row group
  std::vector<uint16_t> off;     // per nonzero
  std::vector<int32_t> base;     // per block / group, + 1 pad entry
  std::vector<uint64_t> planes;  // mode 1: n_planes x plane_words (the last word a pad)
  int n_planes = 0;
  int32_t plane_words = 0;
  int span_bits = 0;  // bits of the widest block's / group's column span (0: not scanned)
  int shape = 0;      // mode 2: kStream (64-row groups) or kCsr3 (the wave tasks)
};
bool plan_col16(const int32_t *col, int64_t nnz, int64_t m, int64_t n, int dtype, int val_dtype,
                unsigned flags, Col16Plan &P);
// starts: the CSR-3 wave tasks, or nullptr for STREAM's 64-row groups
bool plan_col16g(const int32_t *rp, const int32_t *col, int64_t m, int64_t n, int dtype, int val_dtype,
                 unsigned flags, const Tuning &tune, const std::vector<int32_t> *starts, Col16Plan &P);
int upload_col16(Shard &s, const Col16Plan &P);
// x slabs: slab b's row pointers are rp[b * (m + 1) ..], into the slab-major col / val
struct XslabPlan {
  int B = 0;
  std::vector<int32_t> rp, col;
  std::vector<char> val;  // the stored dtype's bytes
};
bool plan_xslabs(const int32_t *rp, const int32_t *col, const void *val, int64_t m, int64_t n, int dtype,
                 int val_dtype, unsigned flags, const Tuning &tune, XslabPlan &P);
int upload_xslabs(Shard &s, const XslabPlan &P);
// split rows (serial order uploads long_row alone)
struct SplitPlan {
  std::vector<int32_t> long_row, long_cs{0}, chunk_k;
  int64_t long_nnz = 0;
  int32_t long_t = 0;  // split_threshold(flags)
};
bool plan_split_rows(const int32_t *rp, int64_t m, unsigned flags, SplitPlan &P);
int upload_split_rows(Shard &s, const SplitPlan &P);
int32_t median_serial_len(const int32_t *rp, int64_t m);
bool wants_csort(const int32_t *rp, const int32_t *col, int64_t m, int64_t n, int dtype, int val_dtype,
                 unsigned flags, const Tuning &tune);
// (SavedFormat, SavedTerms: above Shard, which holds the terms)
double c16_saved_of(int format, const SavedTerms &t);
// (the vectors' and the values' dtypes: s.dtype, s.val_dtype)
int build_row_tables(Shard &s, const int32_t *rp, const int32_t *col, const void *val, int64_t m,
                     int64_t n, unsigned flags);
int build_plan_tables(Shard &s, unsigned flags);

// ---- hspmv_xdict.cpp
// Which row kernel the planner will pick for a shard with n_ssr
// super-super-rows and (CSR-3) wave tasks.
int kernel_for_tables(int64_t n_ssr, bool have_tasks, unsigned flags);
int build_xdict(Shard &s, const int32_t *rp, const int32_t *col, const void *val, int64_t m, int64_t n,
                unsigned flags, bool have_xwin);
// The dictionaries of the workgroups whose rows are [bs[b], bs[b+1]).
struct XdPlan {
  std::vector<int32_t> blk;  // nb + 1 record ranges
  std::vector<int32_t> rec;  // {x_start, lds_off} per run, sentinel {0, entries} per block
  std::vector<uint16_t> pos; // per nonzero: position in its block's staged x (0 for split rows)
  std::vector<int32_t> total;  // entries per block
  int64_t entries = 0, in_kernel_nnz = 0;
  int32_t tmax = 0;
};
int xd_block_tasks(const Tuning &t, int task_waves);
// What hspmv_xdict_plan_ex and hspmv_slices_plan plan for: the options as
// Tuning + flags, the validated matrix's wave tasks (build_tasks), the tasks
// per dictionary block W and the row kernel.
struct PlanShape {
  Tuning tune;
  unsigned flags = 0;
  std::vector<int32_t> tasks;
  int W = 4, kern = kStream;
};
int plan_shape(const hspmv_csr *A, const hspmv_csr3_maps *maps, const hspmv_options *opt, PlanShape &ps);
// The pair a create / plan entry point was given: HSPMV_OK when vector_dtype
// equals val_dtype or is HSPMV_F64 over HSPMV_F32 values, else E_INVALID.
int check_dtype_pair(int val_dtype, int vector_dtype);
int64_t xdict_cap_entries(int dtype, const Tuning &t);
// slices: the workgroups' LDS is the dictionary alone (the slice kernel)
bool plan_xdict_for(const int32_t *rp, const int32_t *col, int kern, int64_t m,
                    std::vector<int32_t> &tasks, int W, int32_t long_t, int64_t cap, int dtype,
                    const Tuning &tune, bool slices, bool fill, XdPlan &P, int64_t *cut);

// ---- hspmv_slices.cpp
struct SliceCounts {
  int64_t n_desc = 0, n_slices = 0;  // wave tasks, and those with rows
  int64_t padded = 0;                // sum of the slices' widths (x 64 = padded entries)
  int64_t max_rows = 0, max_len = 0;
};
struct SlicePlan {
  std::vector<int32_t> desc;
  std::vector<uint8_t> len;
  std::vector<uint16_t> pos;
  std::vector<char> val;
  int64_t padded = 0;
};
// Row ranges of the wave tasks of `kern`: the CSR3 task table, or STREAM's 64-row groups.
std::vector<int32_t> slice_starts(int kern, int64_t m, const std::vector<int32_t> &tasks);
// HSPMV_SLICES_OK when a handle with these options and rows takes the slice
// format (dictionaries permitting), else the first rule it fails.
// dtype: the vectors' (the serial bound); val_dtype: the stored values' (the
// byte rule, the residence test; build_slices: the value groups).
int slices_why(const Tuning &t, unsigned flags, int kern, int W, const int32_t *rp, int64_t m,
               int64_t n, int dtype, int val_dtype, const std::vector<int32_t> &starts, SliceCounts *out);
void build_slices(const int32_t *rp, const uint16_t *pos, const void *val, int64_t m, int val_dtype,
                  const std::vector<int32_t> &starts, SlicePlan &P);
int upload_slices(Shard &s, const SlicePlan &P);
void drop_slices(Shard &s);

// ---- hspmv_csort_build.cpp
// What the device says: its CUs, and the LDS bytes a workgroup's row slots may take.
struct CsortLimits {
  int cus;
  int lds_bytes;
};
// The column-sorted tables of one shard on the host: what upload_csort puts on
// the device or into the shard's report, and nothing else (DevCsort,
// hspmv_internal.h, says what the tables and the launch scalars mean).
struct CsortPlan {
  int64_t m = 0, n = 0;
  int dtype = HSPMV_F64;
  std::vector<int32_t> blk_c, blk_r, blk_v, vslice, cbase;
  std::vector<uint64_t> rec;   // the entry stream, fp32: {idx, val} records
  std::vector<uint32_t> idx;   // ... fp64: indices
  std::vector<double> val64;   // ... and values
  std::vector<uint32_t> long_mask;
  std::vector<int32_t> long_row, long_cs;  // (empty without long rows)
  std::vector<int16_t> rexp, sexp;         // (empty unless fixed)
  // Tuning.csort_src only (else empty): per entry-stream position, where the
  // entry's value is stored (ch * C + at(wide, q, 2), both dtypes), the CSR
  // index k it came from; kCsortSrcPad for padding
  std::vector<uint32_t> src;
  int32_t long_t = 0;                      // rows above this many nonzeros are long rows
  int32_t n_wg = 0, H = 1, u = 16, n_long = 0;
  bool direct = false, nontemporal = true, prefetch = false, slot32 = false, part32 = false, wide = false,
       dyn = false, fixed = false;
  int32_t fin_rows = 0, lds_bytes = 0, row_blocks = 0, n_xexp = 0;
  // bytes of the device-only arrays (0: none): part, spart, xexp_part, trace
  size_t part_bytes = 0, spart_bytes = 0, xexp_part_bytes = 0, trace_bytes = 0;
  int64_t chunks = 0, seg_chunks = 0;  // chunks, and those stored slot-sorted
  int64_t part_begin[4] = {0, 0, 0, 0};  // first column of each column part
  std::vector<int64_t> wg_stats;  // Tuning.csort_trace: 8 cost terms per workgroup
  double format_bytes = 0.0;      // bytes one SpMV moves, x apart (upload_csort adds the shard's)
};
// The host-only planner (no HIP call, no Shard): false when the matrix does
// not take this path (an empty shape, no values, too many long-row slices or
// rows for the LDS slots, chunk counts past the index types), P then
// unspecified.  tools/csort_plan_check.cpp decodes its tables back into the
// matrix (make asan-csort; tests/test_csort_plan.py).
bool plan_csort(const int32_t *rp, const int32_t *col, const void *val, int64_t m, int64_t n, int dtype,
                unsigned flags, const Tuning &tune, const CsortLimits &lim, CsortPlan &P);
// Uploads and allocations only: fills s.built.cs, the shard's csort_* report
// fields, s.saved.csort_format_bytes (with the x term of s.x_entries) and
// s.A.has_csort.
int upload_csort(Shard &s, const CsortPlan &P);
// The device's two limits, plan_csort, upload_csort; HSPMV_OK without tables
// (s.A.has_csort stays false) when the planner declines.
int build_csort(Shard &s, const int32_t *rp, const int32_t *col, const void *val, int64_t m,
                int64_t n, int dtype, unsigned flags);

// ---- hspmv_update.cpp
// Whether the shard's plan can take new values: every plan but a
// column-sorted one without its source-index table (a handle not created by
// hspmv_create_updatable).  No device call, no error set.
bool shard_can_update(const Shard &s);
// HSPMV_OK when shard_can_update, else HSPMV_E_INVALID with the message set.
int update_values_why(const Shard &s);
// HSPMV_E_INVALID when the shard scales its values per row (fixed-point
// column-sorted slots) and val, its nnz new values in host memory, holds an
// Inf or NaN: a new handle over them would not be fixed-point.  No device call.
int update_values_finite(const Shard &s, const void *val);
// New values for the shard: val = its nnz values in CSR order (host memory,
// or on_device: on the shard's device); borrowed: the shard reads the
// caller's device array -- val (NULL: the array as it is) is that array from
// now on.  Copies into the CSR-order values the shard owns and rebuilds the
// row slices' and the x slabs' copies on the shard's stream; a host val is
// consumed before return.  The arguments were checked by the caller.
int update_shard_values(Shard &s, const void *val, bool on_device, bool borrowed);

// ---- hspmv_multi.cpp
// (equal dtypes only: hspmv_create_mixed refuses more than one device)
int create_sharded(hspmv_handle **hp, const hspmv_csr *A, const hspmv_csr3_maps *maps,
                   const std::vector<int> &devs, unsigned flags, const Tuning &tune);
int bcast_x(hspmv_handle *h);
int gather_y(hspmv_handle *h);

}  // namespace hspmv
