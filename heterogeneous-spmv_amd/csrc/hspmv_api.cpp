// hspmv_api.cpp -- the C ABI entry points (include/hspmv.h): handle
// creation, x/y binding, the SpMV launch, the reference timing protocol,
// y gathering and the handle report.  The runtime behind them is in the
// other hspmv_*.cpp units (hspmv_runtime.h).
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <memory>
#include <vector>

#include "hspmv_runtime.h"

using namespace hspmv;

namespace {

int check_handle(hspmv_handle *h) {
  if (!h || h->shards.empty()) return set_error(HSPMV_E_INVALID, "invalid handle");
  return HSPMV_OK;
}

// vec_dtype: the type of x, y, the products and the sums; < 0: A->dtype (the
// stored values' type).  hspmv_create_mixed passes HSPMV_F64 over fp32 values.
int create_single(hspmv_handle **hp, const hspmv_csr *A, const hspmv_csr3_maps *maps, int device,
                  void *stream, unsigned flags, const Tuning &tune, int vec_dtype = -1) {
  if (int rc0 = check_deterministic(flags, tune)) return rc0;
  const bool devptrs = (flags & HSPMV_FLAG_DEVICE_PTRS) != 0;
  if (!A) return set_error(HSPMV_E_INVALID, "matrix is NULL");
  if (vec_dtype < 0) vec_dtype = A->dtype;
  int rc;
  if ((rc = check_device(device))) return rc;
  // (an error return unwinds h: the shard's DevCtx frees what it holds)
  std::unique_ptr<hspmv_handle> h(new hspmv_handle());
  h->m = A->m; h->n = A->n; h->nnz = A->nnz; h->dtype = vec_dtype; h->val_dtype = A->dtype; h->flags = flags;
  h->shards.resize(1);
  Shard &s = h->shards[0];
  s.dev.device = device;
  s.dev.contig = tune.contig == 1;
  s.tune = tune;
  s.dtype = vec_dtype;
  s.val_dtype = A->dtype;
  if (!devptrs) {
    if ((rc = validate_host_csr(A, true))) return rc;
    if ((rc = validate_host_maps(maps, A->m))) return rc;
    if (maps && maps->n_ssr > 0) { h->n_ssr = maps->n_ssr; h->n_sr = maps->n_sr; }
    if ((rc = upload_shard(s, A, maps, 0, A->m, 0, maps ? maps->n_ssr : 0, A->m, flags))) return rc;
  } else {
    // Borrowed device arrays: validate what the kernels index with (row_ptr,
    // the columns and the maps) on the host before the first launch.  They go
    // into the views only, never into s.dev.
    HIP_TRY(hipSetDevice(device));
    std::vector<int32_t> cols;  // host copy until the row tables are built
    if ((rc = read_device_csr(A, s.host.rp, cols))) return rc;
    s.A.m = (int32_t)A->m; s.A.n = A->n; s.A.nnz = A->nnz;
    s.A.row_ptr = A->row_ptr; s.A.col_idx = A->col_idx; s.A.val = A->val;
    s.x_entries = count_distinct_cols(cols.data(), A->nnz, A->n);
    if (maps && maps->n_ssr > 0) {
      std::vector<int32_t> &o = s.host.outer, &in = s.host.inner;
      o.resize((size_t)(maps->n_ssr + 1));
      in.resize((size_t)(maps->n_sr + 1));
      HIP_TRY(hipMemcpy(o.data(), maps->outer, 4 * o.size(), hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(in.data(), maps->inner, 4 * in.size(), hipMemcpyDeviceToHost));
      hspmv_csr3_maps mv = {maps->n_ssr, maps->n_sr, o.data(), in.data()};
      if ((rc = validate_host_maps(&mv, A->m))) return rc;
      s.A.n_ssr = (int32_t)maps->n_ssr; s.A.n_sr = (int32_t)maps->n_sr;
      s.A.outer = maps->outer; s.A.inner = maps->inner;
      s.mean_rows_per_ssr = (double)A->m / (double)maps->n_ssr;
      h->n_ssr = maps->n_ssr; h->n_sr = maps->n_sr;
    }
    // the values come back to the host too: the x slabs copy them slab-major
    std::vector<char> vals(dtype_size(A->dtype) * (size_t)A->nnz);
    if (A->nnz) HIP_TRY(hipMemcpy(vals.data(), A->val, vals.size(), hipMemcpyDeviceToHost));
    if ((rc = build_row_tables(s, s.host.rp.data(), cols.data(), vals.data(), A->m, A->n, flags))) return rc;
    std::vector<char>().swap(vals);
    std::vector<int32_t>().swap(cols);
    const size_t sv = dtype_size(vec_dtype);
    if ((rc = s.dev.alloc(&s.d_x, sv * (size_t)A->n)) || (rc = s.dev.alloc(&s.d_y, sv * (size_t)A->m)))
      return rc;
  }
  if ((rc = finish_shard(s, flags, stream))) return rc;
  if (!devptrs && (rc = place_shard(s, A->n))) return rc;
  (void)ncclGetVersion(&h->rccl_version);
  *hp = h.release();
  return HSPMV_OK;
}

// Whether this shard's row kernel changes direction from one SpMV to the
// next (hspmv_set_sweep).  The vector and column-sorted kernels never do.
// AUTO: a single row-kernel launch (no x slabs) over a matrix the Infinity
// Cache does not hold whole -- a resident one is served from it in either
// direction.
bool shard_alternates(const hspmv_handle *h, const Shard &s) {
  if (h->sweep_mode == HSPMV_SWEEP_FORWARD || s.A.m == 0) return false;
  if (s.plan.kernel != kStream && s.plan.kernel != kCsr3) return false;
  if (h->sweep_mode == HSPMV_SWEEP_ALTERNATE) return true;
  return s.dp.slabs.n == 0 && !mall_resident(s.A.m, h->n, s.A.nnz, h->dtype, h->val_dtype);
}

// The direction of the next SpMV on s; the caller flips h->sweep_phase once
// per call, after every shard has been launched.
bool shard_reverse(const hspmv_handle *h, const Shard &s) {
  return h->sweep_phase && shard_alternates(h, s);
}

// One SpMV of shard s on its stream (its device is the current one), into
// y (nullptr: the shard's y in use).
int launch_shard(const hspmv_handle *h, Shard &s, void *y = nullptr) {
  hipError_t e = launch_spmv(s.A, s.dp, h->dtype, h->val_dtype, s.plan, s.x, y ? y : s.y, s.dev.stream,
                             shard_reverse(h, s));
  if (e != hipSuccess)
    return set_error(HSPMV_E_HIP, "SpMV launch on GPU %d failed: %s", s.dev.device, hipGetErrorString(e));
  return HSPMV_OK;
}

// ---- y = alpha A x + beta y (hspmv_spmv_axpby)

// The refusal every axpby entry point and hspmv_set_y share: a handle, and one
// shard.  No device call.
int check_single_shard(hspmv_handle *h, const char *what) {
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (h->shards.size() > 1)
    return set_error(HSPMV_E_INVALID, "%s needs a single-device handle (this one has %d shards)", what,
                     (int)h->shards.size());
  return HSPMV_OK;
}

// Whether the next hspmv_spmv_axpby runs hspmv_slices_axpby (else SpMV into
// the scratch vector, then hspmv_axpby).
bool axpby_fused(const hspmv_handle *h) {
  const Shard &s = h->shards[0];
  return h->axpby_mode == HSPMV_AXPBY_AUTO && (s.plan.kernel == kStream || s.plan.kernel == kCsr3) &&
         axpby_fusable(s.A, s.dp);
}

// Everything an axpby call decides before its first launch: the refusals,
// and the two-pass path's scratch vector (allocated once, then kept).  The
// shard's device is the current one on return.
int prepare_axpby(hspmv_handle *h, const char *what) {
  int rc;
  if ((rc = check_single_shard(h, what))) return rc;
  if (!h->x_set) return set_error(HSPMV_E_STATE, "x not set (hspmv_set_x / hspmv_bind_x_device)");
  Shard &s = h->shards[0];
  if (s.x == s.y && h->m > 0)
    return set_error(HSPMV_E_INVALID, "%s: x and y are the same device array (y is read and written row by row "
                                      "while other rows still gather from x)", what);
  HIP_TRY(hipSetDevice(s.dev.device));
  if (!axpby_fused(h) && !s.d_axpby && (rc = s.dev.alloc(&s.d_axpby, dtype_size(h->dtype) * (size_t)h->m)))
    return rc;
  return HSPMV_OK;
}

// One y = alpha A x + beta y on the shard's stream (prepare_axpby has passed);
// flips the sweep phase as one hspmv_spmv does.
int enqueue_axpby(hspmv_handle *h, const AxpbyScalars &ab) {
  Shard &s = h->shards[0];
  hipError_t e;
  if (axpby_fused(h)) {
    e = launch_spmv_axpby(s.A, s.dp, h->dtype, h->val_dtype, s.plan, ab, s.x, s.y, s.dev.stream,
                          shard_reverse(h, s));
  } else {
    if (int rc = launch_shard(h, s, s.d_axpby)) return rc;
    e = launch_axpby(h->dtype, h->m, ab, s.plan.y_nt, s.d_axpby, s.y, s.dev.stream);
  }
  if (e != hipSuccess)
    return set_error(HSPMV_E_HIP, "axpby launch on GPU %d failed: %s", s.dev.device, hipGetErrorString(e));
  h->sweep_phase = !h->sweep_phase;
  return HSPMV_OK;
}

// ---- ... and w . y, y . y from the same pass (hspmv_spmv_axpby_dot)

int check_dot_which(unsigned which) {
  if (which == 0 || (which & ~(HSPMV_DOT_WY | HSPMV_DOT_YY)))
    return set_error(HSPMV_E_INVALID, "which = 0x%x (HSPMV_DOT_WY, HSPMV_DOT_YY or both)", which);
  return HSPMV_OK;
}

// prepare_axpby, the dot call's own refusals, and the buffers this call needs
// that the shard does not have yet: the partial pairs (both paths' share in
// one allocation, so a change of path allocates nothing) and the own result.
int prepare_axpby_dot(hspmv_handle *h, const char *what, unsigned which) {
  int rc;
  if ((rc = check_dot_which(which))) return rc;
  if ((rc = check_single_shard(h, what))) return rc;
  Shard &s = h->shards[0];
  DevDot &d = s.dot;
  if (which & HSPMV_DOT_WY) {
    if (!d.w) return set_error(HSPMV_E_STATE, "%s: HSPMV_DOT_WY with no w (hspmv_set_w / hspmv_bind_w_device)", what);
    if (d.w == s.y && h->m > 0)
      return set_error(HSPMV_E_INVALID, "%s: w and y are the same device array (ask for HSPMV_DOT_YY)", what);
  }
  if ((rc = prepare_axpby(h, what))) return rc;
  if (!d.d_part) {
    d.n_fused = axpby_fusable(s.A, s.dp) ? s.dp.sl.n : 0;
    d.n_2p = axpby_dot_blocks(h->m);
    const size_t bytes = 16 * (size_t)(d.n_fused + d.n_2p);
    if ((rc = s.dev.alloc(&d.d_part, bytes))) return rc;
    // (a wave task without rows never writes its pair: it stays 0.0)
    if (bytes) HIP_TRY(hipMemsetAsync(d.d_part, 0, bytes, s.dev.stream));
  }
  if (!d.out && !d.d_out && (rc = s.dev.alloc(&d.d_out, 2 * sizeof(double)))) return rc;
  return HSPMV_OK;
}

// enqueue_axpby with the dots (prepare_axpby_dot has passed): the path's
// kernel(s), then the finish kernel over the partials that path wrote.
int enqueue_axpby_dot(hspmv_handle *h, const AxpbyScalars &ab, unsigned which) {
  Shard &s = h->shards[0];
  DevDot &d = s.dot;
  double *out = d.out ? d.out : d.d_out;
  DotArgs da{(which & HSPMV_DOT_WY) ? d.w : nullptr, (which & HSPMV_DOT_YY) != 0, d.d_part};
  int64_t n = 0;
  hipError_t e;
  if (axpby_fused(h)) {
    n = d.n_fused;
    e = launch_spmv_axpby_dot(s.A, s.dp, h->dtype, h->val_dtype, s.plan, ab, da, s.x, s.y, s.dev.stream,
                              shard_reverse(h, s));
  } else {
    if (int rc = launch_shard(h, s, s.d_axpby)) return rc;
    da.partials = d.d_part + 2 * d.n_fused;
    e = launch_axpby_dot(h->dtype, h->m, ab, s.plan.y_nt, s.d_axpby, s.y, da, &n, s.dev.stream);
  }
  if (e == hipSuccess) e = launch_dot_finish(da.partials, n, out, s.dev.stream);
  if (e != hipSuccess)
    return set_error(HSPMV_E_HIP, "axpby_dot launch on GPU %d failed: %s", s.dev.device, hipGetErrorString(e));
  d.last = out;
  h->sweep_phase = !h->sweep_phase;
  return HSPMV_OK;
}

int check_devices(const int *devices, int n, int *ndev_out) {
  int rc;
  if ((rc = check_device(0, ndev_out))) return rc;  // any device at all, and how many
  for (int p = 0; devices && p < n; ++p)
    if ((rc = check_device(devices[p]))) return rc;
  return HSPMV_OK;
}

}  // namespace

extern "C" {

int hspmv_rccl_version(int *version) {
  clear_error();
  if (!version) return set_error(HSPMV_E_INVALID, "NULL argument");
  *version = 0;
  ncclResult_t r = ncclGetVersion(version);
  if (r != ncclSuccess) return set_error(HSPMV_E_RCCL, "ncclGetVersion: %s", ncclGetErrorString(r));
  return HSPMV_OK;
}

int hspmv_device_count(int *count) {
  clear_error();
  if (!count) return set_error(HSPMV_E_INVALID, "NULL argument");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *count = 0;
    return set_error(HSPMV_E_NODEV, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  *count = c;
  return HSPMV_OK;
}

}  // extern "C"

extern "C" {

int hspmv_create_on_device(hspmv_handle **hp, const hspmv_csr *A, const hspmv_csr3_maps *maps,
                           int device, void *stream, unsigned flags) {
  clear_error();
  if (!hp) return set_error(HSPMV_E_INVALID, "NULL handle pointer");
  *hp = nullptr;
  return create_single(hp, A, maps, device, stream, flags, default_tuning());
}

}  // extern "C"

namespace {

// hspmv_create_ex; updatable: column-sorted tables keep their source indices
// (hspmv_create_updatable)
int create_ex(hspmv_handle **hp, const hspmv_csr *A, const hspmv_csr3_maps *maps, const hspmv_options *opt,
              bool updatable) {
  Tuning t;
  int rc;
  if ((rc = tuning_from_options(opt, &t))) return rc;
  tuning_from_env(&t);  // diagnostic builds only
  t.csort_src = updatable ? 1 : 0;
  const unsigned flags = opt ? opt->flags : 0u;
  if (opt && opt->devices) {
    if (flags & HSPMV_FLAG_DEVICE_PTRS)
      return set_error(HSPMV_E_INVALID, "device pointers need a single-device handle");
    if (opt->n_devices < 1) return set_error(HSPMV_E_INVALID, "need n_devices >= 1");
    int ndev = 0;
    if ((rc = check_devices(opt->devices, opt->n_devices, &ndev))) return rc;
    return create_sharded(hp, A, maps, std::vector<int>(opt->devices, opt->devices + opt->n_devices),
                          flags, t);
  }
  return create_single(hp, A, maps, opt ? opt->device : 0, opt ? opt->stream : nullptr, flags, t);
}

// hspmv_create_mixed (a mixed handle builds no column-sorted tables, so
// `updatable` matters for equal dtypes only)
int create_mixed(hspmv_handle **hp, const hspmv_csr *A, const hspmv_csr3_maps *maps, const hspmv_options *opt,
                 int vector_dtype, bool updatable) {
  if (!A) return set_error(HSPMV_E_INVALID, "matrix is NULL");
  // every refusal below comes before the first HIP call (no device needed)
  int rc;
  if ((rc = check_dtype_pair(A->dtype, vector_dtype))) return rc;
  if (vector_dtype == A->dtype) return create_ex(hp, A, maps, opt, updatable);
  Tuning t;
  if ((rc = tuning_from_options(opt, &t))) return rc;
  tuning_from_env(&t);  // diagnostic builds only
  const unsigned flags = opt ? opt->flags : 0u;
  if (opt && (opt->n_devices > 1 || (opt->devices && opt->n_devices != 1)))
    return set_error(HSPMV_E_INVALID, "a mixed handle (fp32 values, fp64 vectors) runs on one device: "
                                      "n_devices = %d", opt->n_devices);
  if (flag_kernel(flags) == kCsort || t.csort > 0)
    return set_error(HSPMV_E_INVALID, "a mixed handle (fp32 values, fp64 vectors) has no column-sorted "
                                      "kernel: HSPMV_KERNEL_CSORT / csort = 1 need equal dtypes");
  const int device = opt ? (opt->devices ? opt->devices[0] : opt->device) : 0;
  return create_single(hp, A, maps, device, opt ? opt->stream : nullptr, flags, t, vector_dtype);
}

}  // namespace

extern "C" {

int hspmv_create_ex(hspmv_handle **hp, const hspmv_csr *A, const hspmv_csr3_maps *maps,
                    const hspmv_options *opt) {
  clear_error();
  if (!hp) return set_error(HSPMV_E_INVALID, "NULL handle pointer");
  *hp = nullptr;
  return create_ex(hp, A, maps, opt, false);
}

int hspmv_create_mixed(hspmv_handle **hp, const hspmv_csr *A, const hspmv_csr3_maps *maps,
                       const hspmv_options *opt, int vector_dtype) {
  clear_error();
  if (!hp) return set_error(HSPMV_E_INVALID, "NULL handle pointer");
  *hp = nullptr;
  return create_mixed(hp, A, maps, opt, vector_dtype, false);
}

int hspmv_create_updatable(hspmv_handle **hp, const hspmv_csr *A, const hspmv_csr3_maps *maps,
                           const hspmv_options *opt, int vector_dtype) {
  clear_error();
  if (!hp) return set_error(HSPMV_E_INVALID, "NULL handle pointer");
  *hp = nullptr;
  return create_mixed(hp, A, maps, opt, vector_dtype, true);
}

int hspmv_get_dtypes(hspmv_handle *h, int *value_dtype, int *vector_dtype) {
  clear_error();
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (value_dtype) *value_dtype = h->val_dtype;
  if (vector_dtype) *vector_dtype = h->dtype;
  return HSPMV_OK;
}

int hspmv_create(hspmv_handle **hp, const hspmv_csr *A, const hspmv_csr3_maps *maps, int num_gpus,
                 unsigned flags) {
  clear_error();
  if (!hp) return set_error(HSPMV_E_INVALID, "NULL handle pointer");
  *hp = nullptr;
  if (flags & HSPMV_FLAG_DEVICE_PTRS)
    return set_error(HSPMV_E_INVALID, "device pointers need hspmv_create_on_device");
  int ndev = 0, rc;
  if ((rc = check_devices(nullptr, 0, &ndev))) return rc;
  if (num_gpus <= 0) num_gpus = ndev;
  if (num_gpus > ndev)
    return set_error(HSPMV_E_NODEV, "%d GPUs requested, %d visible", num_gpus, ndev);
  if (num_gpus == 1) return create_single(hp, A, maps, 0, nullptr, flags, default_tuning());
  std::vector<int> devs((size_t)num_gpus);
  for (int p = 0; p < num_gpus; ++p) devs[(size_t)p] = p;
  return create_sharded(hp, A, maps, devs, flags, default_tuning());
}

int hspmv_create_sharded(hspmv_handle **hp, const hspmv_csr *A, const hspmv_csr3_maps *maps,
                         const int *devices, int n_shards, unsigned flags) {
  clear_error();
  if (!hp) return set_error(HSPMV_E_INVALID, "NULL handle pointer");
  *hp = nullptr;
  if (flags & HSPMV_FLAG_DEVICE_PTRS)
    return set_error(HSPMV_E_INVALID, "device pointers need hspmv_create_on_device");
  if (!devices || n_shards < 1) return set_error(HSPMV_E_INVALID, "need n_shards >= 1 devices");
  int ndev = 0, rc;
  if ((rc = check_devices(devices, n_shards, &ndev))) return rc;
  return create_sharded(hp, A, maps, std::vector<int>(devices, devices + n_shards), flags,
                        default_tuning());
}

int hspmv_set_x(hspmv_handle *h, const void *x_host) {
  clear_error();
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (!x_host && h->n > 0) return set_error(HSPMV_E_INVALID, "x is NULL");
  const size_t bytes = dtype_size(h->dtype) * (size_t)h->n;
  Shard &s0 = h->shards[0];
  HIP_TRY(hipSetDevice(s0.dev.device));
  if (bytes) {
    HIP_TRY(hipMemcpyAsync(s0.d_x, x_host, bytes, hipMemcpyHostToDevice, s0.dev.stream));
    HIP_TRY(hipStreamSynchronize(s0.dev.stream));
  }
  if ((rc = bcast_x(h))) return rc;
  for (auto &s : h->shards) {
    HIP_TRY(hipSetDevice(s.dev.device));
    HIP_TRY(hipStreamSynchronize(s.dev.stream));
    s.x = s.d_x;
  }
  h->x_set = true;
  return HSPMV_OK;
}

int hspmv_update_values(hspmv_handle *h, const void *val, unsigned flags) {
  clear_error();
  int rc;
  // every refusal, for every shard, before the first device call
  if ((rc = check_handle(h))) return rc;
  if (flags & ~HSPMV_VALUES_DEVICE)
    return set_error(HSPMV_E_INVALID, "unknown flag bits 0x%x (HSPMV_VALUES_DEVICE or 0)",
                     flags & ~HSPMV_VALUES_DEVICE);
  const bool on_device = (flags & HSPMV_VALUES_DEVICE) != 0;
  const bool borrowed = (h->flags & HSPMV_FLAG_DEVICE_PTRS) != 0;
  if (borrowed && !on_device)
    return set_error(HSPMV_E_INVALID, "a handle over borrowed device arrays (HSPMV_FLAG_DEVICE_PTRS) takes "
                                      "device values only: pass HSPMV_VALUES_DEVICE");
  if (on_device && h->shards.size() > 1)
    return set_error(HSPMV_E_INVALID, "HSPMV_VALUES_DEVICE needs a single-device handle (this one has %d "
                                      "shards): pass the global values from host memory",
                     (int)h->shards.size());
  for (const Shard &s : h->shards)
    if ((rc = update_values_why(s))) return rc;
  if (h->nnz == 0) return HSPMV_OK;
  if (!val && !borrowed) return set_error(HSPMV_E_INVALID, "val is NULL");
  const size_t sv = dtype_size(h->val_dtype);
  if (!on_device)  // (a device source: finite values are the caller's duty, include/hspmv.h)
    for (const Shard &s : h->shards)
      if ((rc = update_values_finite(s, (const char *)val + sv * (size_t)s.nnz0))) return rc;
  for (Shard &s : h->shards) {
    const void *v = val ? (const char *)val + sv * (size_t)s.nnz0 : nullptr;
    if ((rc = update_shard_values(s, v, on_device, borrowed))) return rc;
  }
  return HSPMV_OK;
}

int hspmv_can_update_values(const hspmv_handle *h) {
  if (!h || h->shards.empty()) return 0;
  for (const Shard &s : h->shards)
    if (!shard_can_update(s)) return 0;
  return 1;
}

int hspmv_bind_x_device(hspmv_handle *h, const void *x_dev) {
  clear_error();
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (h->sharded) return set_error(HSPMV_E_STATE, "bind needs a single-device handle");
  h->shards[0].x = x_dev ? x_dev : h->shards[0].d_x;
  h->x_set = x_dev != nullptr || h->x_set;
  return HSPMV_OK;
}

int hspmv_bind_y_device(hspmv_handle *h, void *y_dev) {
  clear_error();
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (h->sharded) return set_error(HSPMV_E_STATE, "bind needs a single-device handle");
  h->shards[0].y = y_dev ? y_dev : h->shards[0].d_y;
  return HSPMV_OK;
}

void *hspmv_x_device(hspmv_handle *h, int gpu) {
  if (!h || gpu < 0 || gpu >= (int)h->shards.size()) return nullptr;
  return (void *)h->shards[gpu].x;
}

void *hspmv_y_device(hspmv_handle *h, int gpu) {
  if (!h || gpu < 0 || gpu >= (int)h->shards.size()) return nullptr;
  return h->shards[gpu].y;
}

int hspmv_spmv(hspmv_handle *h) {
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (!h->x_set) return set_error(HSPMV_E_STATE, "x not set (hspmv_set_x / hspmv_bind_x_device)");
  for (auto &s : h->shards) {
    HIP_TRY(hipSetDevice(s.dev.device));
    if ((rc = launch_shard(h, s))) return rc;
  }
  h->sweep_phase = !h->sweep_phase;
  return HSPMV_OK;
}

int hspmv_spmv_axpby(hspmv_handle *h, double alpha, double beta) {
  int rc;
  if ((rc = prepare_axpby(h, "hspmv_spmv_axpby"))) return rc;
  return enqueue_axpby(h, AxpbyScalars{alpha, beta});
}

int hspmv_run_axpby(hspmv_handle *h, double alpha, double beta, int warmup, int iters, hspmv_timing *out) {
  clear_error();
  int rc;
  if ((rc = check_single_shard(h, "hspmv_run_axpby"))) return rc;
  if (!out || iters < 1 || warmup < 0) return set_error(HSPMV_E_INVALID, "bad arguments");
  if ((rc = prepare_axpby(h, "hspmv_run_axpby"))) return rc;
  const AxpbyScalars ab{alpha, beta};
  std::vector<DevCtx *> devs{&h->shards[0].dev};
  if ((rc = timed_run(devs, warmup, iters, [&](size_t) { return enqueue_axpby(h, ab); }, out))) return rc;
  const double tmin = out->t_min;
  // the SpMV's algorithmic bytes plus the one pass the general form adds: y_old
  const double bytes = alg_bytes_of(h->m, h->x_entries(), h->nnz, h->dtype, h->val_dtype, h->n_ssr, h->n_sr) +
                       ((beta != 0.0) ? (double)dtype_size(h->dtype) * (double)h->m : 0.0);
  out->gflops = tmin > 0 ? 2.0 * (double)h->nnz / tmin * 1e-9 : 0.0;
  out->gbps_alg = tmin > 0 ? bytes / tmin * 1e-9 : 0.0;
  out->num_gpus = 1;
  return HSPMV_OK;
}

int hspmv_spmv_axpby_dot(hspmv_handle *h, double alpha, double beta, unsigned which) {
  int rc;
  if ((rc = prepare_axpby_dot(h, "hspmv_spmv_axpby_dot", which))) return rc;
  return enqueue_axpby_dot(h, AxpbyScalars{alpha, beta}, which);
}

int hspmv_run_axpby_dot(hspmv_handle *h, double alpha, double beta, unsigned which, int warmup, int iters,
                        hspmv_timing *out) {
  clear_error();
  int rc;
  if ((rc = check_dot_which(which))) return rc;
  if ((rc = check_single_shard(h, "hspmv_run_axpby_dot"))) return rc;
  if (!out || iters < 1 || warmup < 0) return set_error(HSPMV_E_INVALID, "bad arguments");
  if ((rc = prepare_axpby_dot(h, "hspmv_run_axpby_dot", which))) return rc;
  const AxpbyScalars ab{alpha, beta};
  std::vector<DevCtx *> devs{&h->shards[0].dev};
  if ((rc = timed_run(devs, warmup, iters, [&](size_t) { return enqueue_axpby_dot(h, ab, which); }, out)))
    return rc;
  const double tmin = out->t_min;
  // hspmv_run_axpby's bytes plus the one pass over w
  const double sv = (double)dtype_size(h->dtype);
  const double bytes = alg_bytes_of(h->m, h->x_entries(), h->nnz, h->dtype, h->val_dtype, h->n_ssr, h->n_sr) +
                       ((beta != 0.0) ? sv * (double)h->m : 0.0) +
                       ((which & HSPMV_DOT_WY) ? sv * (double)h->m : 0.0);
  out->gflops = tmin > 0 ? 2.0 * (double)h->nnz / tmin * 1e-9 : 0.0;
  out->gbps_alg = tmin > 0 ? bytes / tmin * 1e-9 : 0.0;
  out->num_gpus = 1;
  return HSPMV_OK;
}

int hspmv_set_w(hspmv_handle *h, const void *w_host) {
  clear_error();
  int rc;
  if ((rc = check_single_shard(h, "hspmv_set_w"))) return rc;
  if (!w_host && h->m > 0) return set_error(HSPMV_E_INVALID, "w is NULL");
  Shard &s = h->shards[0];
  const size_t bytes = dtype_size(h->dtype) * (size_t)h->m;
  HIP_TRY(hipSetDevice(s.dev.device));
  if (!s.dot.d_w && (rc = s.dev.alloc(&s.dot.d_w, bytes))) return rc;
  if (bytes) {
    HIP_TRY(hipMemcpyAsync(s.dot.d_w, w_host, bytes, hipMemcpyHostToDevice, s.dev.stream));
    HIP_TRY(hipStreamSynchronize(s.dev.stream));
  }
  s.dot.w = s.dot.d_w;
  return HSPMV_OK;
}

int hspmv_bind_w_device(hspmv_handle *h, const void *w_dev) {
  clear_error();
  int rc;
  if ((rc = check_single_shard(h, "hspmv_bind_w_device"))) return rc;
  DevDot &d = h->shards[0].dot;
  d.w = w_dev ? w_dev : d.d_w;  // (no own w yet: none in use)
  return HSPMV_OK;
}

int hspmv_bind_dots_device(hspmv_handle *h, double *dots_dev) {
  clear_error();
  int rc;
  if ((rc = check_single_shard(h, "hspmv_bind_dots_device"))) return rc;
  if (reinterpret_cast<uintptr_t>(dots_dev) % 8 != 0)
    return set_error(HSPMV_E_INVALID, "hspmv_bind_dots_device: the two doubles must be 8-byte aligned");
  h->shards[0].dot.out = dots_dev;
  return HSPMV_OK;
}

int hspmv_get_dots(hspmv_handle *h, double out[2]) {
  clear_error();
  int rc;
  if ((rc = check_single_shard(h, "hspmv_get_dots"))) return rc;
  if (!out) return set_error(HSPMV_E_INVALID, "NULL output");
  Shard &s = h->shards[0];
  if (!s.dot.last)
    return set_error(HSPMV_E_STATE, "hspmv_get_dots before any hspmv_spmv_axpby_dot on this handle");
  HIP_TRY(hipSetDevice(s.dev.device));
  HIP_TRY(hipMemcpyAsync(out, s.dot.last, 2 * sizeof(double), hipMemcpyDeviceToHost, s.dev.stream));
  HIP_TRY(hipStreamSynchronize(s.dev.stream));
  return HSPMV_OK;
}

int hspmv_set_axpby_path(hspmv_handle *h, int mode) {
  clear_error();
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (mode != HSPMV_AXPBY_AUTO && mode != HSPMV_AXPBY_TWO_PASS)
    return set_error(HSPMV_E_INVALID, "axpby path %d (HSPMV_AXPBY_AUTO or _TWO_PASS)", mode);
  h->axpby_mode = mode;
  return HSPMV_OK;
}

int hspmv_axpby_path(hspmv_handle *h) {
  clear_error();
  int rc;
  if ((rc = check_single_shard(h, "hspmv_axpby_path"))) return rc;
  return axpby_fused(h) ? HSPMV_AXPBY_PATH_FUSED : HSPMV_AXPBY_PATH_TWO_PASS;
}

int hspmv_set_y(hspmv_handle *h, const void *y_host) {
  clear_error();
  int rc;
  if ((rc = check_single_shard(h, "hspmv_set_y"))) return rc;
  if (!y_host && h->m > 0) return set_error(HSPMV_E_INVALID, "y is NULL");
  Shard &s = h->shards[0];
  const size_t bytes = dtype_size(h->dtype) * (size_t)h->m;
  HIP_TRY(hipSetDevice(s.dev.device));
  if (bytes) {
    HIP_TRY(hipMemcpyAsync(s.y, y_host, bytes, hipMemcpyHostToDevice, s.dev.stream));
    HIP_TRY(hipStreamSynchronize(s.dev.stream));
  }
  return HSPMV_OK;
}

int hspmv_set_sweep(hspmv_handle *h, int mode) {
  clear_error();
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (mode != HSPMV_SWEEP_AUTO && mode != HSPMV_SWEEP_FORWARD && mode != HSPMV_SWEEP_ALTERNATE)
    return set_error(HSPMV_E_INVALID, "sweep mode %d (HSPMV_SWEEP_AUTO, _FORWARD or _ALTERNATE)", mode);
  h->sweep_mode = mode;
  return HSPMV_OK;
}

int hspmv_block_order(int64_t n_blocks, int32_t xcd_chunk, int reverse, int32_t *order) {
  clear_error();
  if (n_blocks < 0 || n_blocks > INT32_MAX || xcd_chunk < 0 || (n_blocks > 0 && !order))
    return set_error(HSPMV_E_INVALID, "bad block-order arguments");
  // a chunk with no full span of 8 * chunk blocks is the dispatch order (and
  // 8 * chunk stays inside 32 bits for the ones that reach the remap)
  const uint32_t chunk = (int64_t)xcd_chunk * kNumXcd > n_blocks ? 1u : (uint32_t)xcd_chunk;
  const uint32_t arg = chunk | (reverse ? kSweepReverse : 0u);
  for (int64_t b = 0; b < n_blocks; ++b)
    order[b] = (int32_t)sweep_block((uint32_t)b, (uint32_t)n_blocks, arg);
  return HSPMV_OK;
}

int hspmv_synchronize(hspmv_handle *h) {
  clear_error();
  int rc;
  if ((rc = check_handle(h))) return rc;
  for (auto &s : h->shards) {
    HIP_TRY(hipSetDevice(s.dev.device));
    HIP_TRY(hipStreamSynchronize(s.dev.stream));
  }
  return HSPMV_OK;
}

int hspmv_run(hspmv_handle *h, int warmup, int iters, hspmv_timing *out) {
  clear_error();
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (!out || iters < 1 || warmup < 0) return set_error(HSPMV_E_INVALID, "bad arguments");
  // (as ever, only a warm-up launch asks for x)
  if (warmup > 0 && !h->x_set) return set_error(HSPMV_E_STATE, "x not set (hspmv_set_x / hspmv_bind_x_device)");
  std::vector<DevCtx *> devs;
  for (auto &s : h->shards) devs.push_back(&s.dev);
  // one SpMV of shard p; the direction flips once per iteration, after the last shard
  auto enqueue = [&](size_t p) -> int {
    const int e = launch_shard(h, h->shards[p]);
    if (p + 1 == h->shards.size()) h->sweep_phase = !h->sweep_phase;
    return e;
  };
  if ((rc = timed_run(devs, warmup, iters, enqueue, out))) return rc;
  const double tmin = out->t_min;
  out->gflops = tmin > 0 ? 2.0 * (double)h->nnz / tmin * 1e-9 : 0.0;
  out->gbps_alg = tmin > 0 ? alg_bytes_of(h->m, h->x_entries(), h->nnz, h->dtype, h->val_dtype, h->n_ssr, h->n_sr) / tmin * 1e-9 : 0.0;
  out->num_gpus = (int32_t)h->shards.size();
  return HSPMV_OK;
}

int hspmv_get_y(hspmv_handle *h, void *y_host) {
  clear_error();
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (!y_host && h->m > 0) return set_error(HSPMV_E_INVALID, "y is NULL");
  const size_t sv = dtype_size(h->dtype);
  if (!h->sharded) {
    Shard &s = h->shards[0];
    HIP_TRY(hipSetDevice(s.dev.device));
    if (h->m) HIP_TRY(hipMemcpyAsync(y_host, s.y, sv * (size_t)h->m, hipMemcpyDeviceToHost, s.dev.stream));
    HIP_TRY(hipStreamSynchronize(s.dev.stream));
    return HSPMV_OK;
  }
  // RCCL all-gather of the padded shards, then unpad GPU 0's copy.
  if ((rc = gather_y(h))) return rc;
  if ((rc = hspmv_synchronize(h))) return rc;
  Shard &s0 = h->shards[0];
  HIP_TRY(hipSetDevice(s0.dev.device));
  std::vector<char> full(sv * (size_t)(h->max_rows * (int64_t)h->shards.size()));
  HIP_TRY(hipMemcpy(full.data(), s0.d_yfull, full.size(), hipMemcpyDeviceToHost));
  for (size_t p = 0; p < h->shards.size(); ++p) {
    const Shard &s = h->shards[p];
    memcpy((char *)y_host + sv * (size_t)s.row0, full.data() + sv * (size_t)(h->max_rows * (int64_t)p),
           sv * (size_t)s.A.m);
  }
  return HSPMV_OK;
}

int hspmv_exchange(hspmv_handle *h, double *bcast_s, double *gather_s) {
  clear_error();
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (bcast_s) {
    if ((rc = hspmv_synchronize(h))) return rc;
    auto tic = std::chrono::steady_clock::now();
    if ((rc = bcast_x(h))) return rc;
    if ((rc = hspmv_synchronize(h))) return rc;
    *bcast_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - tic).count();
  }
  if (gather_s) {
    if ((rc = hspmv_synchronize(h))) return rc;
    auto tic = std::chrono::steady_clock::now();
    if ((rc = gather_y(h))) return rc;
    if ((rc = hspmv_synchronize(h))) return rc;
    *gather_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - tic).count();
  }
  return HSPMV_OK;
}

}  // extern "C"

// The full report (this header's hspmv_info).
static int fill_info(hspmv_handle *h, hspmv_info *out) {
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (!out) return set_error(HSPMV_E_INVALID, "NULL output");
  memset(out, 0, sizeof(*out));
  const Shard &s = h->shards[0];
  out->kernel = s.plan.kernel;
  out->lanes = s.plan.lanes;
  out->waves_per_block = s.plan.waves_per_block;
  out->num_gpus = (int32_t)h->shards.size();
  out->blocks = s.plan.blocks;
  out->x_entries = h->x_entries();
  out->alg_bytes = alg_bytes_of(h->m, out->x_entries, h->nnz, h->dtype, h->val_dtype, h->n_ssr, h->n_sr);
  out->flops = 2.0 * (double)h->nnz;
  for (auto &sh : h->shards) out->device_bytes += sh.dev.bytes();
  out->chunk_u = s.plan.u;
  out->n_split_rows = s.dp.split.n_long;
  out->xcd_remap = s.plan.xcd_chunk;
  out->groups_per_wave = s.plan.kernel == kStream ? s.plan.groups : 1;
  out->format_bytes = out->alg_bytes;
  for (auto &sh : h->shards) out->format_bytes -= sh.c16_saved;
  out->col16 = s.A.col16 ? 1 + s.A.n_cplanes : 0;
  out->wave_tasks = s.plan.kernel == kCsr3 ? s.dp.tasks.n : 0;
  out->x_windows = s.dp.xwin ? 1 : 0;
  out->x_dict = s.dp.xd.blk ? 1 : 0;
  out->x_slabs = s.dp.slabs.n;
  out->col16_group = (s.A.col16 && s.A.c16_mode == 2) ? 1 : 0;
  out->csort_parts = s.plan.kernel == kCsort ? s.dp.cs.H : 0;
  out->n_split_rows = s.plan.kernel == kCsort ? s.dp.cs.n_long : out->n_split_rows;
  for (auto &sh : h->shards) out->x_dict_entries += sh.dp.xd.blk ? sh.saved.xd_entries : 0;
  out->placement_trials = (int32_t)s.place_us.size();
  out->placement_pick = s.place_pick;
  for (size_t k = 0; k < s.place_us.size() && k < 8; ++k) out->placement_us[k] = s.place_us[k];
  out->deterministic = 1;
  for (auto &sh : h->shards) out->deterministic &= (sh.plan.kernel == kCsort && !sh.dp.cs.fixed) ? 0 : 1;
  // the maps-driven plans need maps; a CSR matrix whose heavy 64-row groups
  // sent it to the CSR3 kernel runs build_tasks' row groups
  out->csr3_plan = s.plan.kernel != kCsr3 ? 0
                   : s.A.n_ssr == 0 ? HSPMV_CSR3_PLAN_ROW_GROUPS
                   : s.tune.csr3_plan == HSPMV_CSR3_PLAN_SSR ? HSPMV_CSR3_PLAN_SSR
                   : csr3_fill(s.tune) ? HSPMV_CSR3_PLAN_ALIGNED : HSPMV_CSR3_PLAN_PACKED;
  out->csort_slot_bytes = s.plan.kernel == kCsort ? (s.dp.cs.slot32 ? 4 : 8) : 0;
  out->csort_row_blocks = s.plan.kernel == kCsort ? s.dp.cs.row_blocks : 0;
  out->rccl_version = h->rccl_version;
  out->slab_kernel_rule = s.heavy_frac < 0 ? 0 : (s.A.slab_stream ? 2 : 1);
  out->heavy_group_frac = s.heavy_frac < 0 ? 0.0 : s.heavy_frac;
  out->lds_pad = s.plan.lds_pad ? 1 : 0;
  out->csort_fixed_point = s.plan.kernel == kCsort && s.dp.cs.fixed ? 1 : 0;
  out->serial_order = 1;
  for (auto &sh : h->shards) out->serial_order &= sh.dp.serial_max == INT32_MAX ? 1 : 0;
  out->row_slices = s.dp.sl.desc ? 1 : 0;
  out->slice_pos_bits = s.dp.sl.pos_bits;
  out->sweep = shard_alternates(h, s) ? 1 : 0;
  if (s.plan.kernel == kCsort)
    for (int hh = 0; hh < 4; ++hh) out->csort_part_begin[hh] = s.csort_part_begin[hh];
  for (auto &sh : h->shards)
    if (sh.plan.kernel == kCsort) {
      out->csort_chunks += sh.csort_chunks;
      out->csort_seg_chunks += sh.csort_seg_chunks;
    }
  return HSPMV_OK;
}

extern "C" {

// The 1.0 layout only (HSPMV_INFO_SIZE_1_0 bytes, frozen for major 1): a
// 1.0 caller's struct is that large whatever this library's hspmv_info is.
static_assert(sizeof(hspmv_info) >= HSPMV_INFO_SIZE_1_0, "hspmv_info shrank below its 1.0 layout");
static_assert(offsetof(hspmv_info, heavy_group_frac) + sizeof(double) == HSPMV_INFO_SIZE_1_0,
              "HSPMV_INFO_SIZE_1_0 must end at the last 1.0 field");

int hspmv_get_info(hspmv_handle *h, hspmv_info *out) {
  clear_error();
  if (!out) return set_error(HSPMV_E_INVALID, "NULL output");
  hspmv_info full;
  const int rc = fill_info(h, &full);
  if (rc) return rc;
  memcpy(out, &full, HSPMV_INFO_SIZE_1_0);
  return HSPMV_OK;
}

#ifdef HSPMV_ENV_KNOBS
// Diagnostic builds only (not in hspmv.h): the last csort launch's
// per-workgroup trace (kCsortTraceSlots u64 each, hspmv_internal.h),
// when the handle was created with HSPMV_CSORT_TRACE=1.  Returns the
// workgroup count (0: no trace).
int hspmv_diag_csort_trace(hspmv_handle *h, unsigned long long *out, int max_wg) {
  if (!h || h->shards.empty()) return 0;
  const Shard &s = h->shards[0];
  if (s.plan.kernel != kCsort || !s.dp.cs.trace) return 0;
  const int n = std::min(max_wg, s.dp.cs.n_wg);
  if (hipSetDevice(s.dev.device) != hipSuccess || hipStreamSynchronize(s.dev.stream) != hipSuccess ||
      hipMemcpy(out, s.dp.cs.trace, 8 * kCsortTraceSlots * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
    return 0;
  return n;
}

// Diagnostic builds only: build_csort's per-workgroup cost terms {rows,
// slices, chunks, entries, gather quad-sectors, gather sectors, segmented
// chunks, 0} (8 int64 per workgroup).  Returns the workgroup count.
int hspmv_diag_csort_stats(hspmv_handle *h, long long *out, int max_wg) {
  if (!h || h->shards.empty()) return 0;
  const Shard &s = h->shards[0];
  const int n = std::min<int>(max_wg, (int)(s.csort_wg_stats.size() / 8));
  memcpy(out, s.csort_wg_stats.data(), 8 * 8 * (size_t)n);
  return n;
}
#endif

int hspmv_get_info_sized(hspmv_handle *h, hspmv_info *out, uint32_t out_size) {
  clear_error();
  if (!out) return set_error(HSPMV_E_INVALID, "NULL output");
  hspmv_info full;
  int rc = fill_info(h, &full);
  if (rc) return rc;
  memcpy(out, &full, std::min<size_t>(out_size, sizeof(full)));
  return HSPMV_OK;
}

void hspmv_destroy(hspmv_handle *h) {
  if (!h) return;
  for (auto &s : h->shards) {
    (void)hipSetDevice(s.dev.device);
    if (s.dev.stream) (void)hipStreamSynchronize(s.dev.stream);
  }
  for (auto c : h->comms) (void)ncclCommDestroy(c);
  delete h;  // after the communicators: each shard's DevCtx frees what it holds
}

}  // extern "C"
