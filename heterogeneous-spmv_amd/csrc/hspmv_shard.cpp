// hspmv_shard.cpp -- DevCtx (the owner of device memory, streams and events); one
// row-range shard: upload, plan finish, placement; the shared checks and timing loop
// (see hspmv_runtime.h for the split of the host runtime).
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <thread>
#include <vector>

#include "hspmv_runtime.h"

namespace hspmv {

DevCtx::DevCtx(DevCtx &&o) noexcept
    : device(o.device), stream(o.stream), ev0(o.ev0), ev1(o.ev1), contig(o.contig),
      blocks_(std::move(o.blocks_)), streams_(std::move(o.streams_)), events_(std::move(o.events_)) {
  o.stream = nullptr;
  o.ev0 = o.ev1 = nullptr;
}

DevCtx::~DevCtx() {
  if (blocks_.empty() && streams_.empty() && events_.empty()) return;  // owns nothing: no HIP call
  (void)hipSetDevice(device);
  for (const Block &b : blocks_) (void)hipFree(b.ptr);
  for (hipEvent_t e : events_) (void)hipEventDestroy(e);
  for (hipStream_t st : streams_) (void)hipStreamDestroy(st);
}

int DevCtx::alloc_raw(void **p, size_t bytes) {
  *p = nullptr;
  if (bytes == 0) bytes = 16;
  hipError_t e = hipErrorMemoryAllocation;
  if (contig) {
    e = hipExtMallocWithFlags(p, bytes, hipDeviceMallocContiguous);
    if (e != hipSuccess) (void)hipGetLastError();
  }
  if (e != hipSuccess) e = hipMalloc(p, bytes);
  if (e != hipSuccess)
    return set_error(HSPMV_E_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  blocks_.push_back({*p, bytes});
  return HSPMV_OK;
}

int DevCtx::upload_raw(void **p, const void *src, size_t bytes) {
  const int rc = alloc_raw(p, bytes);
  if (rc) return rc;
  if (bytes) HIP_TRY(hipMemcpy(*p, src, bytes, hipMemcpyHostToDevice));
  return HSPMV_OK;
}

void DevCtx::release(const void *p) {
  for (size_t i = 0; p && i < blocks_.size(); ++i)
    if (blocks_[i].ptr == p) {
      (void)hipFree(blocks_[i].ptr);
      blocks_.erase(blocks_.begin() + (ptrdiff_t)i);
      return;
    }
}

int64_t DevCtx::bytes() const {
  int64_t t = 0;
  for (const Block &b : blocks_) t += (int64_t)b.bytes;
  return t;
}

int DevCtx::new_stream(hipStream_t *st) {
  HIP_TRY(hipStreamCreateWithFlags(st, hipStreamNonBlocking));
  streams_.push_back(*st);
  return HSPMV_OK;
}

int DevCtx::new_event(hipEvent_t *ev, unsigned flags) {
  HIP_TRY(hipEventCreateWithFlags(ev, flags));
  events_.push_back(*ev);
  return HSPMV_OK;
}

int DevCtx::open(void *caller_stream) {
  int rc;
  if (caller_stream)
    stream = (hipStream_t)caller_stream;
  else if ((rc = new_stream(&stream)))
    return rc;
  if ((rc = new_event(&ev0, hipEventDefault)) || (rc = new_event(&ev1, hipEventDefault))) return rc;
  return HSPMV_OK;
}

int check_device(int device, int *ndev_out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return set_error(HSPMV_E_NODEV, "no HIP device available");
  if (ndev_out) *ndev_out = ndev;
  if (device < 0 || device >= ndev)
    return set_error(HSPMV_E_NODEV, "device %d out of range (have %d)", device, ndev);
  return HSPMV_OK;
}

int read_device_csr(const hspmv_csr *A, std::vector<int32_t> &rp, std::vector<int32_t> &cols) {
  if (A->m < 0 || A->n < 0 || A->nnz < 0 || A->m >= INT32_MAX || A->nnz >= INT32_MAX ||
      (A->dtype != HSPMV_F32 && A->dtype != HSPMV_F64) || !A->row_ptr)
    return set_error(HSPMV_E_INVALID, "bad device matrix description");
  rp.resize((size_t)(A->m + 1));
  HIP_TRY(hipMemcpy(rp.data(), A->row_ptr, 4 * rp.size(), hipMemcpyDeviceToHost));
  hspmv_csr view = *A;  // device col/val are only null-checked, never read here
  view.row_ptr = rp.data();
  int rc;
  if ((rc = validate_host_csr(&view, false))) return rc;
  cols.resize((size_t)A->nnz);
  if (A->nnz) HIP_TRY(hipMemcpy(cols.data(), A->col_idx, 4 * cols.size(), hipMemcpyDeviceToHost));
  for (int32_t c : cols)
    if (c < 0 || c >= A->n)
      return set_error(HSPMV_E_INVALID, "device col_idx %d out of [0, %lld)", c, (long long)A->n);
  return HSPMV_OK;
}

int timed_run(const std::vector<DevCtx *> &devs, int warmup, int iters,
              const std::function<int(size_t)> &enqueue, hspmv_timing *out) {
  int rc;
  for (int i = 0; i < warmup; ++i) {
    for (size_t p = 0; p < devs.size(); ++p) {
      HIP_TRY(hipSetDevice(devs[p]->device));
      if ((rc = enqueue(p))) return rc;
    }
    for (DevCtx *d : devs) {
      HIP_TRY(hipSetDevice(d->device));
      HIP_TRY(hipStreamSynchronize(d->stream));
    }
  }
  double tmin = 1e30, tmax = 0, tsum = 0, wmin = 1e30, wmax = 0, wsum = 0;
  for (int i = 0; i < iters; ++i) {
    auto tic = std::chrono::steady_clock::now();
    for (size_t p = 0; p < devs.size(); ++p) {
      DevCtx *d = devs[p];
      HIP_TRY(hipSetDevice(d->device));
      HIP_TRY(hipEventRecord(d->ev0, d->stream));
      if ((rc = enqueue(p))) return rc;
      HIP_TRY(hipEventRecord(d->ev1, d->stream));
    }
    double dev = 0.0;
    for (DevCtx *d : devs) {
      HIP_TRY(hipSetDevice(d->device));
      HIP_TRY(hipEventSynchronize(d->ev1));
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, d->ev0, d->ev1));
      dev = std::max(dev, (double)ms * 1e-3);
    }
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - tic).count();
    tmin = std::min(tmin, dev); tmax = std::max(tmax, dev); tsum += dev;
    wmin = std::min(wmin, wall); wmax = std::max(wmax, wall); wsum += wall;
  }
  memset(out, 0, sizeof(*out));
  out->t_min = tmin; out->t_max = tmax; out->t_avg = tsum / iters;
  out->wall_min = wmin; out->wall_max = wmax; out->wall_avg = wsum / iters;
  out->iters = iters;
  return HSPMV_OK;
}

// Uploads rows [r0, r1) of A (and the matching slice of the maps) to shard s.
int upload_shard(Shard &s, const hspmv_csr *A, const hspmv_csr3_maps *mp, int64_t r0, int64_t r1,
                 int64_t ssr0, int64_t ssr1, int64_t y_rows_alloc, unsigned flags) {
  const size_t sv = dtype_size(s.val_dtype), sx = dtype_size(s.dtype);  // stored values; x and y
  const int64_t m = r1 - r0;
  const int64_t k0 = A->row_ptr[r0], k1 = A->row_ptr[r1];
  const int64_t nnz = k1 - k0;
  HIP_TRY(hipSetDevice(s.dev.device));
  s.row0 = r0;
  s.nnz0 = k0;
  int rc;
  std::vector<int32_t> &rp = s.host.rp;
  rp.resize((size_t)(m + 1));
  for (int64_t i = 0; i <= m; ++i) rp[i] = (int32_t)(A->row_ptr[r0 + i] - k0);
  if ((rc = s.dev.upload(&s.d_rp, rp.data(), 4 * (size_t)(m + 1)))) return rc;
  if ((rc = s.dev.upload(&s.d_ci, A->col_idx + k0, 4 * (size_t)nnz))) return rc;
  if ((rc = s.dev.upload(&s.d_val, (const char *)A->val + sv * k0, sv * (size_t)nnz))) return rc;
  if ((rc = s.dev.alloc(&s.d_x, sx * (size_t)A->n))) return rc;
  if (y_rows_alloc > 0) {
    if ((rc = s.dev.alloc(&s.d_y, sx * (size_t)y_rows_alloc))) return rc;
  }
  s.x_entries = count_distinct_cols(A->col_idx + k0, nnz, A->n);
  s.A.m = (int32_t)m;
  s.A.n = A->n;
  s.A.nnz = nnz;
  s.A.row_ptr = s.d_rp;
  s.A.col_idx = s.d_ci;
  s.A.val = s.d_val;
  if (mp && mp->n_ssr > 0) {
    const int64_t nssr = ssr1 - ssr0;
    const int64_t sr0 = mp->outer[ssr0], sr1 = mp->outer[ssr1];
    const int64_t nsr = sr1 - sr0;
    std::vector<int32_t> &o = s.host.outer, &in = s.host.inner;
    o.resize((size_t)(nssr + 1));
    in.resize((size_t)(nsr + 1));
    for (int64_t i = 0; i <= nssr; ++i) o[i] = (int32_t)(mp->outer[ssr0 + i] - sr0);
    for (int64_t i = 0; i <= nsr; ++i) in[i] = (int32_t)(mp->inner[sr0 + i] - r0);
    if ((rc = s.dev.upload(&s.d_outer, o.data(), 4 * o.size()))) return rc;
    if ((rc = s.dev.upload(&s.d_inner, in.data(), 4 * in.size()))) return rc;
    s.A.n_ssr = (int32_t)nssr;
    s.A.n_sr = (int32_t)nsr;
    s.A.outer = s.d_outer;
    s.A.inner = s.d_inner;
    s.mean_rows_per_ssr = nssr ? (double)m / (double)nssr : 0.0;
  }
  return build_row_tables(s, rp.data(), A->col_idx + k0, (const char *)A->val + sv * k0, m, A->n, flags);
}

int finish_shard(Shard &s, unsigned flags, void *stream) {
  HIP_TRY(hipSetDevice(s.dev.device));
  int rc;
  if ((rc = s.dev.open(stream))) return rc;
  // CSR-3 block size from the mean rows per super-super-row (sizing on the
  // 90th percentile doubled C3's waves for a 7-12 % loss, r01_ab_csr3_tasks)
  const double ssr_rows = s.mean_rows_per_ssr;
  s.plan = plan_launch(s.A, s.dtype, s.val_dtype, flags, ssr_rows,
                       s.host.tasks.empty() ? 0 : (int64_t)s.host.tasks.size() - 1, s.tune);
  if ((rc = build_plan_tables(s, flags))) return rc;
  s.x = s.d_x;
  s.y = s.d_y;
  s.host = HostTables();  // every host copy the plan was built from
  return HSPMV_OK;
}

// Mean SpMV time (us) of the shard's current arrays: 2 warm-up launches, then
// the best of 3 event-timed runs of 5 launches.  < 0 on a launch error.
static double time_shard(Shard &s) {
  for (int i = 0; i < 2; ++i)
    if (launch_spmv(s.A, s.dp, s.dtype, s.val_dtype, s.plan, s.x, s.y, s.dev.stream) != hipSuccess) return -1.0;
  double best = 1e30;
  for (int r = 0; r < 3; ++r) {
    if (hipEventRecord(s.dev.ev0, s.dev.stream) != hipSuccess) return -1.0;
    for (int i = 0; i < 5; ++i)
      if (launch_spmv(s.A, s.dp, s.dtype, s.val_dtype, s.plan, s.x, s.y, s.dev.stream) != hipSuccess) return -1.0;
    float ms = 0.0f;
    if (hipEventRecord(s.dev.ev1, s.dev.stream) != hipSuccess || hipEventSynchronize(s.dev.ev1) != hipSuccess ||
        hipEventElapsedTime(&ms, s.dev.ev0, s.dev.ev1) != hipSuccess)
      return -1.0;
    best = std::min(best, 1000.0 * (double)ms / 5.0);
  }
  return best;
}

// Placement trials.  Where a handle's streamed arrays land in HBM moves the
// HBM-bound row kernels by up to ~10 %: identical C3 handles created one
// after another in one process ran 101.0, 105.4 and 110.8 us, each stable
// over its own rounds (profiles/r02ad_ab_placement.jsonl).  So the shard's
// streamed arrays -- row pointers, the column stream the kernel reads (16-bit
// positions/offsets or 32-bit columns), values, x and y -- are copied into
// trials-1 fresh allocations in turn (all held until the end, so each lands
// elsewhere), every set is timed over a few SpMVs, and the fastest is kept;
// the others are released.  The kernel, its tables and every bit of y are the
// same for all sets.  Single-GPU handles with owned arrays whose row kernel
// (STREAM / CSR3) streams from HBM; Tuning.placement_trials = K sets the number of sets
// (0 or 1 = off); memory for the extra sets must be free, else fewer are
// tried.  Off by default: with 4 sets per handle no faster placement turned
// up on C3 (the first set won 8 of 8 handles; the trial sets ran 111-117 us
// against 109-111) and C4's picks did not carry over to the steady state
// (49.5 vs 49.4 us without trials; profiles/r02ae_ab_placement_trials.jsonl),
// so what made some handles fast in r02ad is not the placement of these
// arrays alone.
static constexpr int kPlacementTrials = 0;

int place_shard(Shard &s, int64_t n) {
  int trials = s.tune.placement_trials > 0 ? std::min(8, s.tune.placement_trials) : kPlacementTrials;
  if (trials <= 1 || (s.plan.kernel != kStream && s.plan.kernel != kCsr3) || s.A.m == 0) return HSPMV_OK;
  if (s.dp.sl.desc) return HSPMV_OK;  // row slices: the trial sets copy the CSR-order streams
  const size_t sv = dtype_size(s.dtype), sval = dtype_size(s.val_dtype);  // x and y; the stored values
  const int64_t m = s.A.m, nnz = s.A.nnz;
  if (mall_resident(m, n, nnz, s.dtype, s.val_dtype)) return HSPMV_OK;  // served from the Infinity Cache: placement does not matter
  struct Arr { void **slot; size_t bytes; };
  std::vector<Arr> arrs = {{(void **)&s.d_rp, 4 * (size_t)(m + 1)},
                           {(void **)&s.d_val, sval * (size_t)nnz},
                           {(void **)&s.d_x, sv * (size_t)n},
                           {(void **)&s.d_y, sv * (size_t)m}};
  if (s.A.col16)
    arrs.push_back({(void **)&s.d_c16, 2 * (size_t)nnz});
  else
    arrs.push_back({(void **)&s.d_ci, 4 * (size_t)nnz});
  size_t set_bytes = 0;
  for (auto &a : arrs) set_bytes += a.bytes;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  const size_t margin = (size_t)1 << 30;
  const int fit = free_b > margin ? (int)std::min<size_t>(8, (free_b - margin) / set_bytes) : 0;
  trials = std::min(trials, 1 + fit);
  if (trials <= 1) return HSPMV_OK;
  auto point = [&]() {
    s.A.row_ptr = s.d_rp;
    s.A.col_idx = s.d_ci;
    s.A.val = s.d_val;
    if (s.A.col16) s.A.col16 = s.d_c16;
    s.x = s.d_x;
    s.y = s.d_y;
  };
  HIP_TRY(hipMemsetAsync(s.d_x, 0, sv * (size_t)n, s.dev.stream));
  std::vector<std::vector<void *>> sets(1);
  for (auto &a : arrs) sets[0].push_back(*a.slot);
  s.place_us.assign(1, time_shard(s));
  if (s.place_us[0] < 0) return set_error(HSPMV_E_HIP, "placement trial: launch failed");
  int rc = HSPMV_OK;
  for (int k = 1; k < trials && rc == HSPMV_OK; ++k) {
    std::vector<void *> set;
    for (auto &a : arrs) {
      void *p = nullptr;
      if (s.dev.alloc(&p, a.bytes) != HSPMV_OK) break;
      set.push_back(p);
      if (hipMemcpyAsync(p, *a.slot, a.bytes, hipMemcpyDeviceToDevice, s.dev.stream) != hipSuccess) {
        rc = set_error(HSPMV_E_HIP, "placement trial: copy failed");
        break;
      }
    }
    if (rc != HSPMV_OK || set.size() != arrs.size()) {  // out of memory or a failed copy: stop
      (void)hipStreamSynchronize(s.dev.stream);
      for (void *p : set) s.dev.release(p);
      (void)hipGetLastError();
      if (rc == HSPMV_OK) clear_error();  // out of memory only ends the trials
      break;
    }
    for (size_t i = 0; i < arrs.size(); ++i) *arrs[i].slot = set[i];
    point();
    const double t = time_shard(s);
    sets.push_back(set);
    s.place_us.push_back(t);
    if (t < 0) rc = set_error(HSPMV_E_HIP, "placement trial: launch failed");
  }
  HIP_TRY(hipStreamSynchronize(s.dev.stream));
  int pick = 0;
  for (int k = 1; k < (int)sets.size(); ++k)
    if (s.place_us[(size_t)k] >= 0 && s.place_us[(size_t)k] < s.place_us[(size_t)pick]) pick = k;
  for (int k = 0; k < (int)sets.size(); ++k)
    if (k != pick)
      for (void *p : sets[(size_t)k]) s.dev.release(p);
  for (size_t i = 0; i < arrs.size(); ++i) *arrs[i].slot = sets[(size_t)pick][i];
  point();
  s.place_pick = pick;
  return rc;
}

}  // namespace hspmv
