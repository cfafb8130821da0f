// hspmv_update.cpp -- new matrix values for a planned shard, in place
// (hspmv_update_values; see hspmv_runtime.h for the split of the host runtime).
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "hspmv_runtime.h"

namespace hspmv {

// The plan of a shard depends on the sparsity pattern alone; the values sit in
// up to three device arrays:
//   CSR order   d_val (A.val): what the chunked STREAM / CSR3 kernels (32- or
//               16-bit columns, dictionaries, x windows), VECTOR, the split-row
//               and the serial long-row kernels read.  A row-slice shard has
//               released it, a borrowed one never had it (A.val is the caller's);
//   row slices  dp.sl.val, slice-major (build_slices);
//   x slabs     dp.slabs.val, slab-major (plan_xslabs); split rows stay in A.val;
//   column-sorted  the entry stream (dp.cs.ent / dp.cs.val), sorted by column
//               inside each workgroup and, under fixed-point slots, scaled per
//               row by 2^rexp, which follows the values (build_csort).  Only a
//               shard that kept the source index of every stream position
//               (hspmv_create_updatable: dp.cs.src) can restate it.
// An update puts the new CSR-order values where A.val points -- a copy into
// d_val, or the caller's array itself for a borrowed shard -- and rebuilds, on
// the shard's stream, each derived copy the DevPlan launches from
// (refresh.hip).  A row-slice shard that owns its matrix has no CSR-order
// array to copy into: a device source is read where it is, a host source goes
// through a staging allocation that lives for this call only.
// Everything is enqueued on the shard's stream, after the SpMVs enqueued so
// far and before the later ones; a host source is consumed (the stream
// synchronised) before return.

static int refresh_derived(Shard &s, const void *src) {
  hipStream_t st = s.dev.stream;
  if (s.dp.sl.desc) {
    const hipError_t e = launch_refresh_slices(s.val_dtype, s.dp.sl.n, s.dp.sl.desc, s.dp.sl.len,
                                               s.A.row_ptr, src, s.dp.sl.val, st);
    if (e != hipSuccess)
      return set_error(HSPMV_E_HIP, "row-slice value refresh on GPU %d failed: %s", s.dev.device,
                       hipGetErrorString(e));
  }
  if (s.dp.slabs.n) {
    const hipError_t e = launch_refresh_slabs(s.val_dtype, s.A.m, s.A.nnz, s.dp.slabs.n, s.A.row_ptr,
                                              s.dp.slabs.rp, src, s.dp.slabs.val, st);
    if (e != hipSuccess)
      return set_error(HSPMV_E_HIP, "x-slab value refresh on GPU %d failed: %s", s.dev.device,
                       hipGetErrorString(e));
  }
  if (s.plan.kernel == kCsort) {  // the row scales first: the entry stream is scaled by them
    hipError_t e = launch_refresh_row_scales(s.val_dtype, s.dp.cs, s.A.row_ptr, src, st);
    if (e == hipSuccess) e = launch_refresh_csort(s.val_dtype, s.dp.cs, src, st);
    if (e != hipSuccess)
      return set_error(HSPMV_E_HIP, "column-sorted value refresh on GPU %d failed: %s", s.dev.device,
                       hipGetErrorString(e));
  }
  return HSPMV_OK;
}

bool shard_can_update(const Shard &s) { return s.plan.kernel != kCsort || s.dp.cs.src != nullptr; }

int update_values_why(const Shard &s) {
  if (!shard_can_update(s))
    return set_error(HSPMV_E_INVALID,
                     "the column-sorted kernel's tables cannot take new values (its entries are sorted by "
                     "column inside each block, and the fixed-point row scales follow the values): create the "
                     "handle with hspmv_options.csort = -1 or deterministic = 1 to update it in place, or "
                     "with hspmv_create_updatable, which keeps the entries' source indices");
  return HSPMV_OK;
}

int update_values_finite(const Shard &s, const void *val) {
  if (s.plan.kernel != kCsort || !s.dp.cs.fixed || !val) return HSPMV_OK;
  // an exponent field of all ones: Inf or NaN.  Integer tests under one OR,
  // no branch in the loop, so it vectorises.
  unsigned bad = 0;
  if (s.val_dtype == HSPMV_F32) {
    const char *v = static_cast<const char *>(val);
    for (int64_t k = 0; k < s.A.nnz; ++k) {
      uint32_t b;
      memcpy(&b, v + 4 * k, 4);
      bad |= (b & 0x7f800000u) == 0x7f800000u;
    }
  } else {
    const char *v = static_cast<const char *>(val);
    for (int64_t k = 0; k < s.A.nnz; ++k) {
      uint64_t b;
      memcpy(&b, v + 8 * k, 8);
      bad |= (b & 0x7ff0000000000000ull) == 0x7ff0000000000000ull;
    }
  }
  if (bad)
    return set_error(HSPMV_E_INVALID,
                     "the new values hold an Inf or NaN and this handle's column-sorted slots are fixed-point "
                     "(deterministic = 2): a new handle over them would keep fp64 slots, so they cannot be "
                     "taken in place; create a new handle");
  return HSPMV_OK;
}

int update_shard_values(Shard &s, const void *val, bool on_device, bool borrowed) {
  if (s.A.nnz == 0) return HSPMV_OK;
  const size_t bytes = dtype_size(s.val_dtype) * (size_t)s.A.nnz;
  HIP_TRY(hipSetDevice(s.dev.device));
  hipStream_t st = s.dev.stream;
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  const void *src = nullptr;
  void *staging = nullptr;
  int rc = HSPMV_OK;
  if (borrowed) {  // the caller's device array: the one in use, or a new one from now on
    if (val) s.A.val = val;
    src = s.A.val;
  } else if (s.d_val) {
    HIP_TRY(hipMemcpyAsync(s.d_val, val, bytes, kind, st));
    src = s.d_val;
  } else if (on_device) {
    src = val;
  } else {
    if ((rc = s.dev.alloc(&staging, bytes))) return rc;
    const hipError_t e = hipMemcpyAsync(staging, val, bytes, kind, st);
    if (e != hipSuccess)
      rc = set_error(HSPMV_E_HIP, "hipMemcpyAsync of the staged values failed: %s", hipGetErrorString(e));
    src = staging;
  }
  if (rc == HSPMV_OK) rc = refresh_derived(s, src);
  if (!on_device) {  // the host array is the caller's again on return
    const hipError_t e = hipStreamSynchronize(st);
    s.dev.release(staging);
    if (e != hipSuccess && rc == HSPMV_OK)
      rc = set_error(HSPMV_E_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
  }
  return rc;
}

}  // namespace hspmv
