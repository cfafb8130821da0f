// axpby.hip -- hspmv_axpby, the second pass of hspmv_spmv_axpby's two-pass
// path: after launch_spmv has left s = A x in the handle's
// scratch vector,
//     y[i] = fl(fl(alpha * s[i]) + fl(beta * y[i]))      beta != 0
//     y[i] = fl(alpha * s[i])                            beta == 0
// elementwise over the m rows.  Every operation is rounded on its own
// (-ffp-contract=off, like every kernel unit), so the bytes are those of the
// fused epilogue in slice_kernel.cuh and of the host model.  beta == 0 is a
// kernel-uniform branch that issues no load of y: a NaN or Inf there does not
// propagate.
//
// One thread per 16-byte group (2 fp64 / 4 fp32) while y is 16-byte aligned
// -- the scratch vector always is, a bound y may not be -- and the last m mod G
// elements, or all of them under a misaligned y, one thread each.
//
// hspmv_axpby_dot is that pass with the two dot products of
// hspmv_spmv_axpby_dot, and hspmv_dot_finish sums the partials of either path
// (DESIGN.md §5f).
#include <hip/hip_runtime.h>

#include "dev_prims.cuh"
#include "hspmv_internal.h"

namespace hspmv {
namespace {

template <typename T, typename V>
__device__ __forceinline__ V axpby_of(T alpha, T beta, bool read_y, V s, const V *y) {
  V r = alpha * s;
  if (read_y) {  // kernel-uniform
    const V by = beta * *y;
    r = r + by;
  }
  return r;
}

template <typename V>
__device__ __forceinline__ void axpby_store(V r, V *y, int32_t y_nt) {
  if (y_nt)
    __builtin_nontemporal_store(r, y);
  else
    *y = r;
}

// groups: 16-byte groups at the front of s and y (0 under a misaligned y);
// thread i < groups takes group i, thread groups + j element G * groups + j.
template <typename T>
__global__ __launch_bounds__(256) void hspmv_axpby(int64_t m, int64_t groups, T alpha, T beta, int32_t y_nt,
                                                   const T *__restrict__ s, T *__restrict__ y) {
  constexpr int G = 16 / (int)sizeof(T);
  typedef T tv __attribute__((ext_vector_type(G)));
  const bool read_y = beta != T(0);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < groups) {
    tv *yp = reinterpret_cast<tv *>(y) + i;
    const tv sv = *(reinterpret_cast<const tv *>(s) + i);
    axpby_store(axpby_of<T, tv>(alpha, beta, read_y, sv, yp), yp, y_nt);
  } else {
    const int64_t e = G * groups + (i - groups);
    if (e < m) axpby_store(axpby_of<T, T>(alpha, beta, read_y, s[e], y + e), y + e, y_nt);
  }
}

// hspmv_axpby with the dots of hspmv_spmv_axpby_dot's two-pass path (DESIGN.md
// §5f): the same update and stores, thread for thread, and from the values
// stored the workgroup's pair {sum w[e] y[e], sum y[e]^2}, products and sums
// in double, into partials[blockIdx.x].  w: nullptr when w . y is not asked
// for (never read then); yy == 0: no y . y; the slot not asked for is 0.0.
// The order is fixed: a thread adds its group's elements in index order, a
// wave its lanes by wave_sum_dpp, thread 0 the four waves' sums in wave order.
// A thread past the last element brings 0.0.  (w may be x, never y: y keeps no
// __restrict__ against it.)
typedef double dot2 __attribute__((ext_vector_type(2)));
typedef double dot2_a8 __attribute__((ext_vector_type(2), aligned(8)));

template <typename T>
__global__ __launch_bounds__(256) void hspmv_axpby_dot(int64_t m, int64_t groups, T alpha, T beta, int32_t y_nt,
                                                       uint32_t yy, const T *__restrict__ s, const T *w, T *y,
                                                       dot2 *__restrict__ partials) {
  constexpr int G = 16 / (int)sizeof(T);
  typedef T tv __attribute__((ext_vector_type(G)));
  __shared__ dot2 red[4];
  const bool read_y = beta != T(0);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double twy = 0.0, tyy = 0.0;
  if (i < groups) {
    tv *yp = reinterpret_cast<tv *>(y) + i;
    const tv sv = *(reinterpret_cast<const tv *>(s) + i);
    T wv[G];
#pragma unroll
    for (int e = 0; e < G; ++e) wv[e] = w ? w[G * i + e] : T(0);
    const tv r = axpby_of<T, tv>(alpha, beta, read_y, sv, yp);
    axpby_store(r, yp, y_nt);
#pragma unroll
    for (int e = 0; e < G; ++e) {
      const double yd = (double)r[e];
      if (w) twy = twy + (double)wv[e] * yd;
      if (yy) tyy = tyy + yd * yd;
    }
  } else {
    const int64_t e = G * groups + (i - groups);
    if (e < m) {
      const T wv = w ? w[e] : T(0);
      const T r = axpby_of<T, T>(alpha, beta, read_y, s[e], y + e);
      axpby_store(r, y + e, y_nt);
      const double yd = (double)r;
      if (w) twy = (double)wv * yd;
      if (yy) tyy = yd * yd;
    }
  }
  const double a = dev::wave_sum_dpp<double>(twy);
  const double b = dev::wave_sum_dpp<double>(tyy);
  if ((threadIdx.x & (dev::kWave - 1)) == 0) red[threadIdx.x >> 6] = dot2{a, b};
  __syncthreads();
  if (threadIdx.x == 0) {
    dot2 t = red[0];
    t = t + red[1];
    t = t + red[2];
    t = t + red[3];
    partials[blockIdx.x] = t;
  }
}

// The last launch of both paths: the n pairs summed into out[0..1].  One
// workgroup of 1024 threads whatever the device and the call: thread t adds
// partials[t], partials[t + 1024], ... in index order (one 16-byte load
// each), a fixed LDS tree halves the 1024 sums ten times, and thread 0 stores
// the pair.  n = 0 stores {0.0, 0.0}.
__global__ __launch_bounds__(1024) void hspmv_dot_finish(const dot2 *__restrict__ partials, int64_t n,
                                                         double *__restrict__ out) {
  __shared__ dot2 red[1024];
  const int t = threadIdx.x;
  dot2 a = dot2{0.0, 0.0};
  // eight loads in flight, added in index order; a pair past n counts as
  // +0.0, which changes no bit of a sum that started from +0.0
  constexpr int kInFlight = 8;
  for (int64_t i = t; i < n; i += 1024 * kInFlight) {
    dot2 v[kInFlight];
#pragma unroll
    for (int k = 0; k < kInFlight; ++k) {
      const int64_t j = i + 1024 * (int64_t)k;
      v[k] = j < n ? partials[j] : dot2{0.0, 0.0};
    }
#pragma unroll
    for (int k = 0; k < kInFlight; ++k) a = a + v[k];
  }
  red[t] = a;
  for (int st = 512; st > 0; st >>= 1) {
    __syncthreads();
    if (t < st) red[t] = red[t] + red[t + st];
  }
  if (t == 0) *reinterpret_cast<dot2_a8 *>(out) = red[0];
}

template <typename T>
hipError_t launch_axpby_dot_typed(int64_t m, const AxpbyScalars &ab, bool y_nt, const T *s, T *y,
                                  const DotArgs &dot, int64_t *n_partials, hipStream_t st) {
  constexpr int G = 16 / (int)sizeof(T);
  const int64_t groups = reinterpret_cast<uintptr_t>(y) % 16 == 0 ? m / G : 0;
  const int64_t threads = groups + (m - G * groups);
  const int64_t blocks = (threads + 255) / 256;
  if (blocks > INT32_MAX || blocks > axpby_dot_blocks(m)) return hipErrorInvalidValue;
  hipLaunchKernelGGL((hspmv_axpby_dot<T>), dim3((unsigned)blocks), dim3(256), 0, st, m, groups, (T)ab.alpha,
                     (T)ab.beta, (int32_t)y_nt, (uint32_t)dot.yy, s, static_cast<const T *>(dot.w), y,
                     reinterpret_cast<dot2 *>(dot.partials));
  *n_partials = blocks;
  return hipGetLastError();
}

template <typename T>
hipError_t launch_axpby_typed(int64_t m, const AxpbyScalars &ab, bool y_nt, const T *s, T *y, hipStream_t st) {
  constexpr int G = 16 / (int)sizeof(T);
  const int64_t groups = reinterpret_cast<uintptr_t>(y) % 16 == 0 ? m / G : 0;
  const int64_t threads = groups + (m - G * groups);
  const int64_t blocks = (threads + 255) / 256;
  if (blocks > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL((hspmv_axpby<T>), dim3((unsigned)blocks), dim3(256), 0, st, m, groups, (T)ab.alpha, (T)ab.beta,
                     (int32_t)y_nt, s, y);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_axpby(int dtype, int64_t m, const AxpbyScalars &ab, bool y_nt, const void *s, void *y,
                        hipStream_t stream) {
  if (m <= 0) return hipSuccess;
  if (!s || !y || reinterpret_cast<uintptr_t>(s) % 16 != 0) return hipErrorInvalidValue;
  return dtype == HSPMV_F64 ? launch_axpby_typed<double>(m, ab, y_nt, (const double *)s, (double *)y, stream)
                            : launch_axpby_typed<float>(m, ab, y_nt, (const float *)s, (float *)y, stream);
}

hipError_t launch_axpby_dot(int dtype, int64_t m, const AxpbyScalars &ab, bool y_nt, const void *s, void *y,
                            const DotArgs &dot, int64_t *n_partials, hipStream_t stream) {
  *n_partials = 0;
  if (m <= 0) return hipSuccess;
  if (!s || !y || reinterpret_cast<uintptr_t>(s) % 16 != 0 || !dot.partials ||
      reinterpret_cast<uintptr_t>(dot.partials) % 16 != 0)
    return hipErrorInvalidValue;
  return dtype == HSPMV_F64
             ? launch_axpby_dot_typed<double>(m, ab, y_nt, (const double *)s, (double *)y, dot, n_partials, stream)
             : launch_axpby_dot_typed<float>(m, ab, y_nt, (const float *)s, (float *)y, dot, n_partials, stream);
}

hipError_t launch_dot_finish(const double *partials, int64_t n, double *out, hipStream_t stream) {
  if (n < 0 || !out || reinterpret_cast<uintptr_t>(out) % 8 != 0 ||
      (n > 0 && (!partials || reinterpret_cast<uintptr_t>(partials) % 16 != 0)))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(hspmv_dot_finish, dim3(1), dim3(1024), 0, stream, reinterpret_cast<const dot2 *>(partials), n,
                     out);
  return hipGetLastError();
}

}  // namespace hspmv
