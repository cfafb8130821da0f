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
#include <hip/hip_runtime.h>

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

}  // namespace hspmv
