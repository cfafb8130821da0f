// hspmv_mm.cpp -- the multi-vector operator Y = A X (hspmv_mm_*,
// include/hspmv.h): creation, X / Y binding, the launch, the timing protocol
// and the report.  The kernels are in spmm.hip.  A DevCtx (hspmv_runtime.h)
// owns the operator's device side -- the CSR arrays of an owned matrix, the
// long-row table, its own X (n * k) and Y (m * k), the stream and the events;
// a borrowed matrix's arrays are views in DevMM only.
#include <string.h>

#include <algorithm>
#include <cstddef>
#include <memory>
#include <vector>

#include "hspmv_runtime.h"

using namespace hspmv;

struct hspmv_mm {
  DevCtx dev;
  DevMM d;
  void *d_x = nullptr, *d_y = nullptr;  // own X and Y
  const void *x = nullptr;              // X / Y in use (own or bound)
  void *y = nullptr;
  int64_t x_entries = 0;                // distinct columns
  int64_t m = 0, n = 0, nnz = 0;
  int dtype = HSPMV_F64;
  int32_t k = 1;
  int64_t ldx = 1, ldy = 1;  // leading dimensions of x / y
  bool x_set = false;
  bool borrowed = false;                // HSPMV_FLAG_DEVICE_PTRS: d.val is the caller's
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
         (double)(mm->x_entries + mm->m) * (double)mm->k * sv;
}

// Everything after the argument checks.  borrowed: HSPMV_FLAG_DEVICE_PTRS,
// the matrix arrays are the caller's.
int build_mm(hspmv_mm *mm, const hspmv_csr *A, bool borrowed, int device, void *stream) {
  DevCtx &dev = mm->dev;
  DevMM &d = mm->d;
  const size_t sv = dtype_size(A->dtype);
  int rc;
  mm->borrowed = borrowed;
  if ((rc = check_device(device))) return rc;
  dev.device = device;
  HIP_TRY(hipSetDevice(device));
  std::vector<int32_t> long_rows;
  const int32_t serial_max = mm_serial_max(A->dtype);
  if (!borrowed) {
    if ((rc = validate_host_csr(A, true))) return rc;
    if ((rc = dev.upload(&d.row_ptr, A->row_ptr, 4 * (size_t)(A->m + 1)))) return rc;
    if ((rc = dev.upload(&d.col_idx, A->col_idx, 4 * (size_t)A->nnz))) return rc;
    if ((rc = dev.upload(&d.val, A->val, sv * (size_t)A->nnz))) return rc;
    mm->x_entries = count_distinct_cols(A->col_idx, A->nnz, A->n);
    mm_long_rows(A->row_ptr, A->m, serial_max, long_rows);
  } else {
    std::vector<int32_t> rp, cols;
    if ((rc = read_device_csr(A, rp, cols))) return rc;
    mm->x_entries = count_distinct_cols(cols.data(), A->nnz, A->n);
    d.row_ptr = A->row_ptr;
    d.col_idx = A->col_idx;
    d.val = A->val;
    mm_long_rows(rp.data(), A->m, serial_max, long_rows);
  }
  if ((rc = dev.upload(&d.long_row, long_rows.data(), 4 * long_rows.size()))) return rc;
  if ((rc = dev.alloc(&mm->d_x, sv * (size_t)A->n * (size_t)mm->k))) return rc;
  if ((rc = dev.alloc(&mm->d_y, sv * (size_t)A->m * (size_t)mm->k))) return rc;
  if ((rc = dev.open(stream))) return rc;
  mm->x = mm->d_x;
  mm->y = mm->d_y;
  mm->ldx = mm->ldy = mm->k;
  d.m = (int32_t)A->m;
  d.nnz = A->nnz;
  d.k = mm->k;
  d.lanes_per_row = mm_lanes_per_row(mm->k);
  d.serial_max = serial_max;
  d.n_long = (int32_t)long_rows.size();
  return HSPMV_OK;
}

int enqueue(hspmv_mm *mm) {
  return launch_spmm(mm->d, mm->dtype, mm->x, mm->ldx, mm->y, mm->ldy, mm->dev.stream);
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
  mm->d.nontemporal = (v.flags & HSPMV_FLAG_NONTEMPORAL) != 0;
  // (an error return unwinds mm: its DevCtx frees what it holds)
  const int rc = build_mm(mm.get(), A, (v.flags & HSPMV_FLAG_DEVICE_PTRS) != 0, v.device, v.stream);
  if (rc) return rc;
  *out = mm.release();
  return HSPMV_OK;
}

int hspmv_mm_set_x(hspmv_mm *mm, const void *X_host, int64_t ldx) {
  clear_error();
  int rc;
  if ((rc = check_mm(mm))) return rc;
  if (ldx < mm->k) return set_error(HSPMV_E_INVALID, "ldx = %lld below k = %d", (long long)ldx, mm->k);
  if (!X_host && mm->n > 0) return set_error(HSPMV_E_INVALID, "X is NULL");
  hipStream_t st = mm->dev.stream;
  const size_t sv = dtype_size(mm->dtype);
  HIP_TRY(hipSetDevice(mm->dev.device));
  if (mm->n && ldx == mm->k)
    HIP_TRY(hipMemcpyAsync(mm->d_x, X_host, sv * (size_t)mm->k * (size_t)mm->n, hipMemcpyHostToDevice, st));
  else if (mm->n)
    HIP_TRY(hipMemcpy2DAsync(mm->d_x, sv * (size_t)mm->k, X_host, sv * (size_t)ldx, sv * (size_t)mm->k,
                             (size_t)mm->n, hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  mm->x = mm->d_x;
  mm->ldx = mm->k;
  mm->x_set = true;
  return HSPMV_OK;
}

int hspmv_mm_update_values(hspmv_mm *mm, const void *val, unsigned flags) {
  clear_error();
  int rc;
  if ((rc = check_mm(mm))) return rc;
  if (flags & ~HSPMV_VALUES_DEVICE)
    return set_error(HSPMV_E_INVALID, "unknown flag bits 0x%x (HSPMV_VALUES_DEVICE or 0)",
                     flags & ~HSPMV_VALUES_DEVICE);
  const bool on_device = (flags & HSPMV_VALUES_DEVICE) != 0;
  if (mm->borrowed && !on_device)
    return set_error(HSPMV_E_INVALID, "an operator over borrowed device arrays (HSPMV_FLAG_DEVICE_PTRS) "
                                      "takes device values only: pass HSPMV_VALUES_DEVICE");
  if (mm->nnz == 0) return HSPMV_OK;
  if (mm->borrowed) {  // the kernels read the caller's array: nothing derived from it
    if (val) mm->d.val = val;
    return HSPMV_OK;
  }
  if (!val) return set_error(HSPMV_E_INVALID, "val is NULL");
  hipStream_t st = mm->dev.stream;
  HIP_TRY(hipSetDevice(mm->dev.device));
  HIP_TRY(hipMemcpyAsync(const_cast<void *>(mm->d.val), val, dtype_size(mm->dtype) * (size_t)mm->nnz,
                         on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  if (!on_device) HIP_TRY(hipStreamSynchronize(st));  // the host array is the caller's again
  return HSPMV_OK;
}

int hspmv_mm_bind_x_device(hspmv_mm *mm, const void *X_dev, int64_t ldx) {
  clear_error();
  int rc;
  if ((rc = check_mm(mm))) return rc;
  if (X_dev && ldx < mm->k)
    return set_error(HSPMV_E_INVALID, "ldx = %lld below k = %d", (long long)ldx, mm->k);
  mm->x = X_dev ? X_dev : mm->d_x;
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
  mm->y = Y_dev ? Y_dev : mm->d_y;
  mm->ldy = Y_dev ? ldy : mm->k;
  return HSPMV_OK;
}

int hspmv_mm_spmm(hspmv_mm *mm) {
  int rc;
  if ((rc = check_mm(mm))) return rc;
  if (!mm->x_set) return set_error(HSPMV_E_STATE, "X not set (hspmv_mm_set_x / hspmv_mm_bind_x_device)");
  HIP_TRY(hipSetDevice(mm->dev.device));
  return enqueue(mm);
}

int hspmv_mm_synchronize(hspmv_mm *mm) {
  clear_error();
  int rc;
  if ((rc = check_mm(mm))) return rc;
  HIP_TRY(hipSetDevice(mm->dev.device));
  HIP_TRY(hipStreamSynchronize(mm->dev.stream));
  return HSPMV_OK;
}

int hspmv_mm_run(hspmv_mm *mm, int warmup, int iters, hspmv_timing *out) {
  clear_error();
  int rc;
  if ((rc = check_mm(mm))) return rc;
  if (!out || iters < 1 || warmup < 0) return set_error(HSPMV_E_INVALID, "bad arguments");
  if (!mm->x_set) return set_error(HSPMV_E_STATE, "X not set (hspmv_mm_set_x / hspmv_mm_bind_x_device)");
  if ((rc = timed_run({&mm->dev}, warmup, iters, [&](size_t) { return enqueue(mm); }, out))) return rc;
  const double tmin = out->t_min;
  out->gflops = tmin > 0 ? 2.0 * (double)mm->nnz * (double)mm->k / tmin * 1e-9 : 0.0;
  out->gbps_alg = tmin > 0 ? mm_alg_bytes(mm) / tmin * 1e-9 : 0.0;
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
  hipStream_t st = mm->dev.stream;
  const size_t sv = dtype_size(mm->dtype);
  HIP_TRY(hipSetDevice(mm->dev.device));
  if (mm->m && ldy == mm->k && mm->ldy == mm->k)
    HIP_TRY(hipMemcpyAsync(Y_host, mm->y, sv * (size_t)mm->k * (size_t)mm->m, hipMemcpyDeviceToHost, st));
  else if (mm->m)
    HIP_TRY(hipMemcpy2DAsync(Y_host, sv * (size_t)ldy, mm->y, sv * (size_t)mm->ldy, sv * (size_t)mm->k,
                             (size_t)mm->m, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
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
  full.device_bytes = mm->dev.bytes();
  memcpy(out, &full, std::min<size_t>(out_size, sizeof(full)));
  return HSPMV_OK;
}

void hspmv_mm_destroy(hspmv_mm *mm) {
  if (!mm) return;
  (void)hipSetDevice(mm->dev.device);
  if (mm->dev.stream) (void)hipStreamSynchronize(mm->dev.stream);
  delete mm;
}

}  // extern "C"
