// hspmv_mm.cpp -- the multi-vector operator Y = A X (hspmv_mm_*,
// include/hspmv.h): creation, X / Y binding, the launch, the timing protocol
// and the report.  The kernels are in spmm.hip.  The operator keeps its
// device state in a Shard (hspmv_runtime.h) -- the CSR arrays, the long-row
// table in d_long_row, its own X (n * k) in d_x and Y (m * k) in d_y, the
// stream and the events -- so allocation accounting, upload and release are
// the single-vector handle's (dev_alloc, upload, free_shard).
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <memory>
#include <vector>

#include "hspmv_runtime.h"

using namespace hspmv;

struct hspmv_mm {
  Shard s;
  DevMM d;
  int64_t m = 0, n = 0, nnz = 0;
  int dtype = HSPMV_F64;
  int32_t k = 1;
  int64_t ldx = 1, ldy = 1;  // leading dimensions of s.x / s.y
  bool x_set = false;
  bool borrowed = false;     // HSPMV_FLAG_DEVICE_PTRS: matrix arrays not owned
};

namespace hspmv {

void mm_long_rows(const int32_t *row_ptr, int64_t m, int32_t serial_max, std::vector<int32_t> &rows) {
  rows.clear();
  for (int64_t r = 0; r < m; ++r)
    if (row_ptr[r + 1] - row_ptr[r] > serial_max) rows.push_back((int32_t)r);
}

}  // namespace hspmv

namespace {

int check_mm(hspmv_mm *mm) {
  if (!mm) return set_error(HSPMV_E_INVALID, "mm is NULL");
  return HSPMV_OK;
}

double mm_alg_bytes(const hspmv_mm *mm) {
  const double sv = (double)dtype_size(mm->dtype);
  return (double)mm->nnz * (sv + 4.0) + (double)(mm->m + 1) * 4.0 +
         (double)(mm->s.x_entries + mm->m) * (double)mm->k * sv;
}

// Everything after the argument checks; on an error the caller frees the shard.
int build_mm(hspmv_mm *mm, const hspmv_csr *A, int device, void *stream) {
  Shard &s = mm->s;
  const size_t sv = dtype_size(A->dtype);
  int rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return set_error(HSPMV_E_NODEV, "no HIP device available");
  if (device < 0 || device >= ndev)
    return set_error(HSPMV_E_NODEV, "device %d out of range (have %d)", device, ndev);
  s.device = device;
  HIP_TRY(hipSetDevice(device));
  std::vector<int32_t> long_rows;
  const int32_t serial_max = mm_serial_max(A->dtype);
  if (!mm->borrowed) {
    if ((rc = validate_host_csr(A, true))) return rc;
    if ((rc = upload(s, &s.d_rp, A->row_ptr, 4 * (size_t)(A->m + 1)))) return rc;
    if ((rc = upload(s, &s.d_ci, A->col_idx, 4 * (size_t)A->nnz))) return rc;
    if ((rc = upload(s, &s.d_val, A->val, sv * (size_t)A->nnz))) return rc;
    s.owns_csr = true;
    s.x_entries = count_distinct_cols(A->col_idx, A->nnz, A->n);
    mm_long_rows(A->row_ptr, A->m, serial_max, long_rows);
  } else {
    // Borrowed device arrays: validate what the kernels index with on the
    // host before the first launch, as hspmv_create_ex does.
    if (A->m < 0 || A->n < 0 || A->nnz < 0 || A->m >= INT32_MAX || A->nnz >= INT32_MAX ||
        (A->dtype != HSPMV_F32 && A->dtype != HSPMV_F64) || !A->row_ptr ||
        (A->nnz > 0 && (!A->col_idx || !A->val)))
      return set_error(HSPMV_E_INVALID, "bad device matrix description");
    std::vector<int32_t> rp((size_t)(A->m + 1));
    HIP_TRY(hipMemcpy(rp.data(), A->row_ptr, 4 * rp.size(), hipMemcpyDeviceToHost));
    hspmv_csr view = *A;  // device col/val are only null-checked, never read here
    view.row_ptr = rp.data();
    if ((rc = validate_host_csr(&view, false))) return rc;
    std::vector<int32_t> cols((size_t)A->nnz);
    if (A->nnz) HIP_TRY(hipMemcpy(cols.data(), A->col_idx, 4 * cols.size(), hipMemcpyDeviceToHost));
    for (int32_t c : cols)
      if (c < 0 || c >= A->n)
        return set_error(HSPMV_E_INVALID, "device col_idx %d out of [0, %lld)", c, (long long)A->n);
    s.x_entries = count_distinct_cols(cols.data(), A->nnz, A->n);
    s.d_rp = const_cast<int32_t *>(A->row_ptr);
    s.d_ci = const_cast<int32_t *>(A->col_idx);
    s.d_val = const_cast<void *>(A->val);
    mm_long_rows(rp.data(), A->m, serial_max, long_rows);
  }
  if ((rc = upload(s, &s.d_long_row, long_rows.data(), 4 * long_rows.size()))) return rc;
  if ((rc = dev_alloc(&s.d_x, sv * (size_t)A->n * (size_t)mm->k, &s.bytes))) return rc;
  if ((rc = dev_alloc(&s.d_y, sv * (size_t)A->m * (size_t)mm->k, &s.bytes))) return rc;
  if (stream) {
    s.stream = (hipStream_t)stream;
    s.own_stream = false;
  } else {
    HIP_TRY(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    s.own_stream = true;
  }
  HIP_TRY(hipEventCreate(&s.ev0));
  HIP_TRY(hipEventCreate(&s.ev1));
  s.x = s.d_x;
  s.y = s.d_y;
  mm->ldx = mm->ldy = mm->k;
  DevMM &d = mm->d;
  d.m = (int32_t)A->m;
  d.nnz = A->nnz;
  d.k = mm->k;
  d.lanes_per_row = mm_lanes_per_row(mm->k);
  d.serial_max = serial_max;
  d.row_ptr = s.d_rp;
  d.col_idx = s.d_ci;
  d.val = s.d_val;
  d.long_row = s.d_long_row;
  d.n_long = (int32_t)long_rows.size();
  return HSPMV_OK;
}

int enqueue(hspmv_mm *mm) {
  return launch_spmm(mm->d, mm->dtype, mm->s.x, mm->ldx, mm->s.y, mm->ldy, mm->s.stream);
}

}  // namespace

extern "C" {

int hspmv_mm_create(hspmv_mm **out, const hspmv_csr *A, int32_t k, const hspmv_options *opt) {
  clear_error();
  // refusals before any device is touched
  if (!out) return set_error(HSPMV_E_INVALID, "mm (the operator pointer) is NULL");
  *out = nullptr;
  if (!A) return set_error(HSPMV_E_INVALID, "A (the matrix) is NULL");
  if (k < 1 || k > kMmMaxRhs)
    return set_error(HSPMV_E_INVALID, "k = %d right-hand sides (1 <= k <= %d)", k, kMmMaxRhs);
  hspmv_options v;
  memset(&v, 0, sizeof(v));
  if (opt) {
    if (opt->struct_size < offsetof(hspmv_options, csr3_plan))
      return set_error(HSPMV_E_INVALID, "hspmv_options.struct_size %u too small", opt->struct_size);
    memcpy(&v, opt, std::min<size_t>(opt->struct_size, sizeof(v)));
  }
  if (flag_kernel(v.flags) != HSPMV_KERNEL_AUTO)
    return set_error(HSPMV_E_INVALID, "flags: kernel code %u (the SpMM has one kernel: HSPMV_KERNEL_AUTO)",
                     flag_kernel(v.flags));
  if (v.n_devices > 1)
    return set_error(HSPMV_E_INVALID, "n_devices = %d (the SpMM runs on one device)", v.n_devices);
  std::unique_ptr<hspmv_mm> mm(new hspmv_mm());
  mm->m = A->m; mm->n = A->n; mm->nnz = A->nnz; mm->dtype = A->dtype; mm->k = k;
  mm->borrowed = (v.flags & HSPMV_FLAG_DEVICE_PTRS) != 0;
  mm->d.nontemporal = (v.flags & HSPMV_FLAG_NONTEMPORAL) != 0;
  const int rc = build_mm(mm.get(), A, v.device, v.stream);
  if (rc) {
    free_shard(mm->s, mm->borrowed);
    return rc;
  }
  *out = mm.release();
  return HSPMV_OK;
}

int hspmv_mm_set_x(hspmv_mm *mm, const void *X_host, int64_t ldx) {
  clear_error();
  int rc;
  if ((rc = check_mm(mm))) return rc;
  if (ldx < mm->k) return set_error(HSPMV_E_INVALID, "ldx = %lld below k = %d", (long long)ldx, mm->k);
  if (!X_host && mm->n > 0) return set_error(HSPMV_E_INVALID, "X is NULL");
  Shard &s = mm->s;
  const size_t sv = dtype_size(mm->dtype);
  HIP_TRY(hipSetDevice(s.device));
  if (mm->n && ldx == mm->k)
    HIP_TRY(hipMemcpyAsync(s.d_x, X_host, sv * (size_t)mm->k * (size_t)mm->n, hipMemcpyHostToDevice, s.stream));
  else if (mm->n)
    HIP_TRY(hipMemcpy2DAsync(s.d_x, sv * (size_t)mm->k, X_host, sv * (size_t)ldx, sv * (size_t)mm->k,
                             (size_t)mm->n, hipMemcpyHostToDevice, s.stream));
  HIP_TRY(hipStreamSynchronize(s.stream));
  s.x = s.d_x;
  mm->ldx = mm->k;
  mm->x_set = true;
  return HSPMV_OK;
}

int hspmv_mm_bind_x_device(hspmv_mm *mm, const void *X_dev, int64_t ldx) {
  clear_error();
  int rc;
  if ((rc = check_mm(mm))) return rc;
  if (X_dev && ldx < mm->k)
    return set_error(HSPMV_E_INVALID, "ldx = %lld below k = %d", (long long)ldx, mm->k);
  mm->s.x = X_dev ? X_dev : mm->s.d_x;
  mm->ldx = X_dev ? ldx : mm->k;
  mm->x_set = X_dev != nullptr || mm->x_set;
  return HSPMV_OK;
}

int hspmv_mm_bind_y_device(hspmv_mm *mm, void *Y_dev, int64_t ldy) {
  clear_error();
  int rc;
  if ((rc = check_mm(mm))) return rc;
  if (Y_dev && ldy < mm->k)
    return set_error(HSPMV_E_INVALID, "ldy = %lld below k = %d", (long long)ldy, mm->k);
  mm->s.y = Y_dev ? Y_dev : mm->s.d_y;
  mm->ldy = Y_dev ? ldy : mm->k;
  return HSPMV_OK;
}

int hspmv_mm_spmm(hspmv_mm *mm) {
  int rc;
  if ((rc = check_mm(mm))) return rc;
  if (!mm->x_set) return set_error(HSPMV_E_STATE, "X not set (hspmv_mm_set_x / hspmv_mm_bind_x_device)");
  HIP_TRY(hipSetDevice(mm->s.device));
  return enqueue(mm);
}

int hspmv_mm_synchronize(hspmv_mm *mm) {
  clear_error();
  int rc;
  if ((rc = check_mm(mm))) return rc;
  HIP_TRY(hipSetDevice(mm->s.device));
  HIP_TRY(hipStreamSynchronize(mm->s.stream));
  return HSPMV_OK;
}

int hspmv_mm_run(hspmv_mm *mm, int warmup, int iters, hspmv_timing *out) {
  clear_error();
  int rc;
  if ((rc = check_mm(mm))) return rc;
  if (!out || iters < 1 || warmup < 0) return set_error(HSPMV_E_INVALID, "bad arguments");
  if (!mm->x_set) return set_error(HSPMV_E_STATE, "X not set (hspmv_mm_set_x / hspmv_mm_bind_x_device)");
  Shard &s = mm->s;
  HIP_TRY(hipSetDevice(s.device));
  for (int i = 0; i < warmup; ++i) {
    if ((rc = enqueue(mm))) return rc;
    HIP_TRY(hipStreamSynchronize(s.stream));
  }
  double tmin = 1e30, tmax = 0, tsum = 0, wmin = 1e30, wmax = 0, wsum = 0;
  for (int i = 0; i < iters; ++i) {
    auto tic = std::chrono::steady_clock::now();
    HIP_TRY(hipEventRecord(s.ev0, s.stream));
    if ((rc = enqueue(mm))) return rc;
    HIP_TRY(hipEventRecord(s.ev1, s.stream));
    HIP_TRY(hipEventSynchronize(s.ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s.ev0, s.ev1));
    const double dev = (double)ms * 1e-3;
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - tic).count();
    tmin = std::min(tmin, dev); tmax = std::max(tmax, dev); tsum += dev;
    wmin = std::min(wmin, wall); wmax = std::max(wmax, wall); wsum += wall;
  }
  memset(out, 0, sizeof(*out));
  out->t_min = tmin; out->t_max = tmax; out->t_avg = tsum / iters;
  out->wall_min = wmin; out->wall_max = wmax; out->wall_avg = wsum / iters;
  out->gflops = tmin > 0 ? 2.0 * (double)mm->nnz * (double)mm->k / tmin * 1e-9 : 0.0;
  out->gbps_alg = tmin > 0 ? mm_alg_bytes(mm) / tmin * 1e-9 : 0.0;
  out->iters = iters;
  out->num_gpus = 1;
  return HSPMV_OK;
}

int hspmv_mm_get_y(hspmv_mm *mm, void *Y_host, int64_t ldy) {
  clear_error();
  int rc;
  if ((rc = check_mm(mm))) return rc;
  if (ldy < mm->k) return set_error(HSPMV_E_INVALID, "ldy = %lld below k = %d", (long long)ldy, mm->k);
  if (!mm->x_set) return set_error(HSPMV_E_STATE, "X not set: there is no Y yet");
  if (!Y_host && mm->m > 0) return set_error(HSPMV_E_INVALID, "Y is NULL");
  Shard &s = mm->s;
  const size_t sv = dtype_size(mm->dtype);
  HIP_TRY(hipSetDevice(s.device));
  if (mm->m && ldy == mm->k && mm->ldy == mm->k)
    HIP_TRY(hipMemcpyAsync(Y_host, s.y, sv * (size_t)mm->k * (size_t)mm->m, hipMemcpyDeviceToHost, s.stream));
  else if (mm->m)
    HIP_TRY(hipMemcpy2DAsync(Y_host, sv * (size_t)ldy, s.y, sv * (size_t)mm->ldy, sv * (size_t)mm->k,
                             (size_t)mm->m, hipMemcpyDeviceToHost, s.stream));
  HIP_TRY(hipStreamSynchronize(s.stream));
  return HSPMV_OK;
}

int hspmv_mm_get_info(hspmv_mm *mm, hspmv_mm_info *out, uint32_t out_size) {
  clear_error();
  int rc;
  if ((rc = check_mm(mm))) return rc;
  if (!out) return set_error(HSPMV_E_INVALID, "NULL output");
  hspmv_mm_info full;
  memset(&full, 0, sizeof(full));
  full.k = mm->k;
  full.lanes_per_row = mm->d.lanes_per_row;
  full.rows_per_wave = 64 / mm->d.lanes_per_row;
  full.waves_per_block = 4;
  full.blocks = mm_blocks(mm->m, mm->d.lanes_per_row);
  full.long_rows = mm->d.n_long;
  full.serial_max = mm->d.serial_max;
  full.alg_bytes = mm_alg_bytes(mm);
  full.flops = 2.0 * (double)mm->nnz * (double)mm->k;
  full.device_bytes = mm->s.bytes;
  memcpy(out, &full, std::min<size_t>(out_size, sizeof(full)));
  return HSPMV_OK;
}

void hspmv_mm_destroy(hspmv_mm *mm) {
  if (!mm) return;
  (void)hipSetDevice(mm->s.device);
  if (mm->s.stream) (void)hipStreamSynchronize(mm->s.stream);
  free_shard(mm->s, mm->borrowed);
  delete mm;
}

}  // extern "C"
