// spmv_kernels.hip -- launch_spmv, the entry of every single-vector SpMV, and
// the kernels that are not row kernels (those: row_kernels.cuh and
// slice_kernel.cuh, instantiated by the stream_* units; csort.hip):
//
//  * hspmv_csr_vector<T, L, NT>   (HSPMV_KERNEL_VECTOR)
//      L lanes (a sub-wave, L | 64) per row, lanes stride the row's nonzeros
//      with FMA, reduced by __shfl_xor inside the L-lane group.  Replaces
//      cuSpMV_3_vec's veclevel lanes + barrier-free volatile-LDS tree
//      (csrk.cu:222-240) with a wave64-safe shuffle reduction; L = 1 is the
//      thread-per-row cuda_spmv shape.
//
//  * the split rows (> kLongRow nonzeros) that the row kernels skip:
//    hspmv_long_chunks + hspmv_long_reduce (many workgroups per row), or with
//    hspmv_options.deterministic = 3 hspmv_long_serial (one workgroup per
//    row, the adds still in order, on a stream forked beside the row kernel)
//    + hspmv_long_scatter.
//
// Build: hipcc --offload-arch=gfx950 -ffp-contract=off.  Contraction is off so
// that only the explicit fma() calls (vector kernel, long rows) fuse.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "dev_prims.cuh"
#include "hspmv_internal.h"
#include "static_switch.h"

namespace hspmv {
namespace {

using dev::kWave;
using dev::ldg;
using dev::wave_sum;

// TV (here and in the split-row kernels): the stored type of val -- T, or
// float under T = double for the mixed handles; a value is widened to T before
// its product.
template <typename T, int L, bool NT, typename TV = T>
__global__ __launch_bounds__(256) void hspmv_csr_vector(
    int32_t m, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
    const TV *__restrict__ val, const T *__restrict__ x, T *__restrict__ y) {
  const int lane = threadIdx.x & (L - 1);
  int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / L;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x / L;
  for (; row < m; row += stride) {
    const int32_t beg = rp[row];
    const int32_t end = rp[row + 1];
    T s = T(0);
    for (int32_t k = beg + lane; k < end; k += L)
      s = fma((T)ldg<NT>(val + k), x[ldg<NT>(ci + k)], s);
#pragma unroll
    for (int off = L / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, L);
    if (lane == 0) y[row] = s;
  }
}

// Split rows, step 1: one 256-thread workgroup per chunk of <= kLongChunk
// nonzeros of one long row -> partials[chunk].
template <typename T, bool NT, typename TV = T>
__global__ __launch_bounds__(256) void hspmv_long_chunks(
    int32_t n_chunks, const int32_t *__restrict__ chunk_k, const int32_t *__restrict__ ci,
    const TV *__restrict__ val, const T *__restrict__ x, T *__restrict__ partials) {
  __shared__ T red[4];
  const int c = blockIdx.x;
  if (c >= n_chunks) return;  // block-uniform
  const int32_t k0 = chunk_k[2 * c], k1 = chunk_k[2 * c + 1];
  T s0 = T(0), s1 = T(0);
  int32_t k = k0 + threadIdx.x;
  for (; k + 256 < k1; k += 512) {
    s0 = fma((T)ldg<NT>(val + k), x[ldg<NT>(ci + k)], s0);
    s1 = fma((T)ldg<NT>(val + k + 256), x[ldg<NT>(ci + k + 256)], s1);
  }
  if (k < k1) s0 = fma((T)ldg<NT>(val + k), x[ldg<NT>(ci + k)], s0);
  const T s = wave_sum(s0 + s1);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[c] = (red[0] + red[1]) + (red[2] + red[3]);
}

// Split rows, step 2: one wave per long row adds its chunk partials.
template <typename T>
__global__ __launch_bounds__(256) void hspmv_long_reduce(
    int32_t n_long, const int32_t *__restrict__ long_row, const int32_t *__restrict__ cstart,
    const T *__restrict__ partials, T *__restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n_long) return;
  const int32_t c0 = cstart[j], c1 = cstart[j + 1];
  T s = T(0);
  for (int32_t c = c0 + lane; c < c1; c += kWave) s += partials[c];
  s = wave_sum(s);
  if (lane == 0) y[long_row[j]] = s;
}

// Serial order (hspmv_options.deterministic = 3), rows over kLongRow
// nonzeros: one 256-thread workgroup per row adds the row's products left
// to right from 0, as omp_spmv does -- which no number of lanes can share.
// Waves 1-3 form the next 16 KiB of products (multiply rounded on its
// own, no fma: -ffp-contract=off) into one LDS buffer while lane 0 of wave 0
// adds the current one: 32 products per step, read as 16-byte LDS loads
// issued one step ahead of the dependent adds, so the add chain (not the
// LDS round trip) bounds the row.  In the row kernels such a row was walked by
// one lane through its wave's product chunks, one LDS round trip per four
// adds (C5's 144 616-nonzero hub row: 2.1 ms for the launch).
constexpr int kLongSerialBytes = 16384;  // per LDS buffer (two: 32 KiB)

template <typename T, bool NT, typename TV = T>
__global__ __launch_bounds__(256) void hspmv_long_serial(
    int32_t n_long, const int32_t *__restrict__ long_row, const int32_t *__restrict__ rp,
    const int32_t *__restrict__ ci, const TV *__restrict__ val, const T *__restrict__ x,
    T *__restrict__ y, T *__restrict__ lsum) {
  constexpr int32_t kLongSerialChunk = kLongSerialBytes / (int)sizeof(T);
  __shared__ __attribute__((aligned(16))) T buf[2][kLongSerialChunk];
  const int j = blockIdx.x;
  if (j >= n_long) return;  // block-uniform
  const int32_t r = long_row[j];
  const int32_t k0 = rp[r], k1 = rp[r + 1];
  auto fill = [&](T *dst, int32_t c, int t, int nt) {
    const int32_t n = min(k1 - c, kLongSerialChunk);
    for (int32_t i = t; i < n; i += nt) {
      const T p = (T)ldg<NT>(val + c + i) * x[ldg<NT>(ci + c + i)];
      dst[i] = p;
    }
  };
  fill(buf[0], k0, threadIdx.x, 256);
  __syncthreads();
  T acc = T(0);
  int s = 0;
  for (int32_t c = k0; c < k1; c += kLongSerialChunk, s ^= 1) {
    if (threadIdx.x >= kWave) {
      if (c + kLongSerialChunk < k1) fill(buf[s ^ 1], c + kLongSerialChunk, threadIdx.x - kWave, 256 - kWave);
    } else if (threadIdx.x == 0) {
      const int32_t n = min(k1 - c, kLongSerialChunk);
      const T *b = buf[s];
      constexpr int V = 16 / (int)sizeof(T), B = 32;
      typedef T tv __attribute__((ext_vector_type(V)));
      int32_t i = 0;
      // two register sets, no copies: each step's loads go out (a
      // sched_barrier keeps them there) before the other set's adds
      auto load = [&](tv(&q)[B / V], int32_t at) {
#pragma unroll
        for (int v = 0; v < B / V; ++v) q[v] = *reinterpret_cast<const tv *>(b + at + v * V);
      };
      auto add = [&](const tv(&q)[B / V]) {
#pragma unroll
        for (int v = 0; v < B / V; ++v)
#pragma unroll
          for (int e = 0; e < V; ++e) acc = acc + q[v][e];
      };
      if (n >= 2 * B) {
        tv q0[B / V], q1[B / V];
        load(q0, 0);
        for (; i + 2 * B <= n; i += 2 * B) {
          load(q1, i + B);
          __builtin_amdgcn_sched_barrier(0);
          add(q0);
          __builtin_amdgcn_sched_barrier(0);
          load(q0, i + 3 * B <= n ? i + 2 * B : i);  // (a harmless reload at the end)
          __builtin_amdgcn_sched_barrier(0);
          add(q1);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      for (; i < n; ++i) acc = acc + b[i];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (lsum)
      lsum[j] = acc;  // forked: hspmv_long_scatter writes y after the row kernel
    else
      y[r] = acc;
  }
}

// The forked long rows' sums into y, on the launch stream after the row
// kernel (whose x-slab passes also write those rows: empty segments).
template <typename T>
__global__ __launch_bounds__(256) void hspmv_long_scatter(int32_t n_long, const int32_t *__restrict__ long_row,
                                                          const T *__restrict__ lsum, T *__restrict__ y) {
  const int32_t j = (int32_t)(blockIdx.x * 256 + threadIdx.x);
  if (j < n_long) y[long_row[j]] = lsum[j];
}

// ------------------------------------------------------------------ dispatch

// The row kernels' instantiation unit for vectors of T and values stored as TV.
template <typename TV>
hipError_t launch_rows_of(const DevCSR &A, const DevPlan &dp, const LaunchPlan &p, const double *x, double *y,
                          hipStream_t st) {
  if constexpr (sizeof(TV) == 8)
    return launch_rows_f64(A, dp, p, x, y, st);
  else
    return launch_rows_f32v64(A, dp, p, x, y, st);
}
template <typename TV>
hipError_t launch_rows_of(const DevCSR &A, const DevPlan &dp, const LaunchPlan &p, const float *x, float *y,
                          hipStream_t st) {
  return launch_rows_f32(A, dp, p, x, y, st);
}

template <typename T, bool NT, typename TV = T>
hipError_t launch_typed(const DevCSR &A, const DevPlan &dp, const LaunchPlan &p, const T *x,
                        T *y, hipStream_t st) {
  if (A.m == 0) return hipSuccess;
  const int32_t *rp = A.row_ptr;
  const int32_t *ci = A.col_idx;
  const TV *val = static_cast<const TV *>(A.val);
  hipError_t e = hipSuccess;
  const DevSplit &sp = dp.split;
  // serial order: the long rows' workgroups start first, on their own
  // stream (forked from st, joined back below), beside the row kernel, and
  // leave their sums in sp.partials for hspmv_long_scatter -- C5: 289 us of
  // x-slab passes and a 497 us add chain otherwise in sequence
  const bool fork = sp.n_long > 0 && sp.long_serial && sp.long_stream;
  if (fork) {
    if ((e = hipEventRecord(sp.long_fork, st)) != hipSuccess ||
        (e = hipStreamWaitEvent(sp.long_stream, sp.long_fork, 0)) != hipSuccess)
      return e;
    hipLaunchKernelGGL((hspmv_long_serial<T, NT, TV>), dim3((unsigned)sp.n_long), dim3(256), 0, sp.long_stream,
                       sp.n_long, sp.long_row, rp, ci, val, x, y, static_cast<T *>(sp.partials));
    if ((e = hipGetLastError()) != hipSuccess || (e = hipEventRecord(sp.long_join, sp.long_stream)) != hipSuccess)
      return e;
  }
  switch (p.kernel) {
    case kVector:
      if (!static_switch<1, 2, 4, 8, 16, 32, 64>(p.lanes, [&](auto L) {
            hipLaunchKernelGGL((hspmv_csr_vector<T, L, NT, TV>), dim3((unsigned)p.blocks), dim3(256), 0, st, A.m,
                               rp, ci, val, x, y);
          }))
        return hipErrorInvalidValue;
      return hipGetLastError();  // the vector kernel sums split rows itself
    case kStream:
    case kCsr3:
      if (dp.slabs.n > 0) {  // one pass per x slab, each continuing the rows from y
        DevCSR As = A;
        As.col_idx = dp.slabs.col;
        As.val = dp.slabs.val;
        As.col16 = nullptr;
        As.cbase = nullptr;
        As.cplanes = nullptr;
        As.n_cplanes = 0;
        LaunchPlan ps = p;
        for (int32_t b = 0; b < dp.slabs.n && e == hipSuccess; ++b) {
          As.row_ptr = dp.slabs.rp + (size_t)b * (size_t)(A.m + 1);
          ps.carry = b > 0;
          e = launch_rows_of<TV>(As, dp, ps, x, y, st);  // (mixed: slab_val is fp32 as well)
        }
      } else {
        e = launch_rows_of<TV>(A, dp, p, x, y, st);
      }
      if (e != hipSuccess) return e;
      break;
    case kCsort:
      if constexpr (sizeof(TV) != sizeof(T)) return hipErrorInvalidValue;  // no mixed csort tables
      return launch_csort(dp.cs, sizeof(T) == 8 ? 1 : 0, x, y, st);
    default:
      return hipErrorInvalidValue;
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (fork) {
    if ((e = hipStreamWaitEvent(st, sp.long_join, 0)) != hipSuccess) return e;
    hipLaunchKernelGGL((hspmv_long_scatter<T>), dim3((unsigned)((sp.n_long + 255) / 256)), dim3(256), 0, st,
                       sp.n_long, sp.long_row, static_cast<const T *>(sp.partials), y);
    e = hipGetLastError();
  } else if (sp.n_long > 0 && sp.long_serial) {
    hipLaunchKernelGGL((hspmv_long_serial<T, NT, TV>), dim3((unsigned)sp.n_long), dim3(256), 0, st, sp.n_long,
                       sp.long_row, rp, ci, val, x, y, static_cast<T *>(nullptr));
    e = hipGetLastError();
  } else if (sp.n_long > 0) {
    hipLaunchKernelGGL((hspmv_long_chunks<T, NT, TV>), dim3((unsigned)sp.n_chunks), dim3(256), 0, st,
                       sp.n_chunks, sp.chunk_k, ci, val, x, static_cast<T *>(sp.partials));
    hipLaunchKernelGGL((hspmv_long_reduce<T>), dim3((unsigned)((sp.n_long + 3) / 4)), dim3(256), 0, st, sp.n_long,
                       sp.long_row, sp.long_cstart, static_cast<const T *>(sp.partials), y);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace

hipError_t launch_spmv(const DevCSR &A, const DevPlan &dp, int dtype, int val_dtype, const LaunchPlan &fwd,
                       const void *x, void *y, hipStream_t stream, bool reverse) {
  LaunchPlan plan = fwd;
  plan.reverse = reverse && (fwd.kernel == kStream || fwd.kernel == kCsr3);
  if (dtype == HSPMV_F64 && val_dtype == HSPMV_F32) {  // mixed: fp32 values under fp64 vectors and sums
    return plan.nontemporal
               ? launch_typed<double, true, float>(A, dp, plan, (const double *)x, (double *)y, stream)
               : launch_typed<double, false, float>(A, dp, plan, (const double *)x, (double *)y, stream);
  }
  if (dtype != val_dtype) return hipErrorInvalidValue;
  if (dtype == 1) {
    return plan.nontemporal
               ? launch_typed<double, true>(A, dp, plan, (const double *)x, (double *)y, stream)
               : launch_typed<double, false>(A, dp, plan, (const double *)x, (double *)y, stream);
  }
  return plan.nontemporal
             ? launch_typed<float, true>(A, dp, plan, (const float *)x, (float *)y, stream)
             : launch_typed<float, false>(A, dp, plan, (const float *)x, (float *)y, stream);
}

hipError_t launch_spmv_axpby(const DevCSR &A, const DevPlan &dp, int dtype, int val_dtype, const LaunchPlan &fwd,
                             const AxpbyScalars &ab, const void *x, void *y, hipStream_t stream, bool reverse) {
  if (!axpby_fusable(A, dp) || (fwd.kernel != kStream && fwd.kernel != kCsr3)) return hipErrorInvalidValue;
  LaunchPlan plan = fwd;
  plan.reverse = reverse;
  if (dtype == HSPMV_F64 && val_dtype == HSPMV_F32)
    return launch_slices_axpby_f32v64(dp, plan, ab, (const double *)x, (double *)y, stream);
  if (dtype != val_dtype) return hipErrorInvalidValue;
  if (dtype == HSPMV_F64) return launch_slices_axpby_f64(dp, plan, ab, (const double *)x, (double *)y, stream);
  return launch_slices_axpby_f32(dp, plan, ab, (const float *)x, (float *)y, stream);
}

hipError_t launch_spmv_axpby_dot(const DevCSR &A, const DevPlan &dp, int dtype, int val_dtype,
                                 const LaunchPlan &fwd, const AxpbyScalars &ab, const DotArgs &dot, const void *x,
                                 void *y, hipStream_t stream, bool reverse) {
  if (!axpby_fusable(A, dp) || (fwd.kernel != kStream && fwd.kernel != kCsr3)) return hipErrorInvalidValue;
  LaunchPlan plan = fwd;
  plan.reverse = reverse;
  if (dtype == HSPMV_F64 && val_dtype == HSPMV_F32)
    return launch_slices_axpby_dot_f32v64(dp, plan, ab, dot, (const double *)x, (double *)y, stream);
  if (dtype != val_dtype) return hipErrorInvalidValue;
  if (dtype == HSPMV_F64)
    return launch_slices_axpby_dot_f64(dp, plan, ab, dot, (const double *)x, (double *)y, stream);
  return launch_slices_axpby_dot_f32(dp, plan, ab, dot, (const float *)x, (float *)y, stream);
}

}  // namespace hspmv
