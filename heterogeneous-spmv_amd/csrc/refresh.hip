// refresh.hip -- rebuilds the copies of the matrix values a handle derived at
// creation from new CSR-order values, on the device (hspmv_update_values,
// include/hspmv.h; the host side is hspmv_update.cpp).
//
// The values of a handle live in up to three places: the CSR-order array the
// chunked, vector and split-row kernels read (a plain copy: no kernel here),
// the row slices' value stream and the x slabs' slab-major copy.  The last
// two are permutations of the CSR order that depend on the sparsity pattern
// alone, and every table that describes them is already on the device:
//
//  * hspmv_refresh_slices<TV>   the value stream of the row slices
//      One wave per slice descriptor, lane i owns row first + i (as in
//      hspmv_slices, slice_kernel.cuh).  The lane walks its row's CSR values
//      left to right and the wave writes the slice in build_slices' layout
//      (hspmv_slices.cpp, slot_at): the w / G whole groups of G = 16 /
//      sizeof(TV) slots as one 16-byte store per lane (1 KiB contiguous per
//      wave store), the last w mod G slots as single 64-lane columns.  Slots
//      at or past the row's length and lanes past the slice's rows store 0,
//      so the stream is byte for byte what a new handle would upload, padding
//      included.  A slice's rows are one contiguous CSR range of at most 64
//      rows x the serial bound: the wave copies it into its part of the
//      workgroup's LDS with coalesced loads and the lanes walk their rows
//      there (STAGE).  The direct form, every lane reading global memory at a
//      stride of its row length, measured 1.6x (fp64) to 2.0x (fp32 values)
//      slower on C3 and stays as the path of a slice that
//      would not fit the LDS part.  Positions, descriptors and lengths are
//      only read.
//
//  * hspmv_refresh_slabs<TV, L>  the slab-major copy of the x slabs
//      L lanes per row.  Segment b of row r is the next slab_rp_b[r + 1] -
//      slab_rp_b[r] CSR entries of the row (build_xslabs, hspmv_tables.cpp),
//      so the lanes walk the B row-pointer arrays in slab order and copy each
//      segment with consecutive lanes on consecutive entries.  Split rows have
//      empty segments in every slab: nothing is copied for them (the split-row
//      kernels read the CSR order).
//
// Values move as stored (TV: float or double; a mixed handle's are float), bit
// for bit: no arithmetic touches them.  Plain HIP C++ with vector stores,
// static LDS only, no atomics.
#include "dev_prims.cuh"
#include "hspmv_common.h"
#include "hspmv_internal.h"
#include "static_switch.h"

namespace hspmv {
namespace {

using dev::kWave;

constexpr int kRefreshWaves = 4;  // waves per 256-thread workgroup

// HSPMV_REFRESH_STAGE = 1: the wave first copies its slice's CSR range, one
// contiguous run of at most 64 rows x the serial bound, into LDS with coalesced
// loads and the lanes walk their rows there, instead of reading global memory
// at a stride of the row length (the A/B of DESIGN.md 5d).
#ifndef HSPMV_REFRESH_STAGE
#define HSPMV_REFRESH_STAGE 1
#endif
constexpr int kStageWaves = 2;  // waves per workgroup of the staged form (static LDS <= 64 KiB)
template <typename TV>
constexpr int stage_cap() {  // values a wave stages: 64 rows of the serial bound of the widest vectors TV goes with
  return kWave * (sizeof(TV) == 8 ? kSerialMax : kSerialMaxF32);
}

template <typename TV, bool STAGE>
__global__ __launch_bounds__(STAGE ? kStageWaves * kWave : 256) void hspmv_refresh_slices(
    int32_t n_slices, const int32_t *__restrict__ desc, const uint8_t *__restrict__ len,
    const int32_t *__restrict__ row_ptr, const TV *__restrict__ src, TV *__restrict__ dst) {
  constexpr int G = 16 / (int)sizeof(TV);
  constexpr int W = STAGE ? kStageWaves : kRefreshWaves;
  typedef TV tv __attribute__((ext_vector_type(G)));
  __shared__ TV stage[STAGE ? W * stage_cap<TV>() : 1];
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x >> 6;
  const int64_t t = (int64_t)blockIdx.x * W + wid;
  if (t >= n_slices) return;  // wave-uniform
  // {prefix, first row} of this task and of the next (the closing pair after the last)
  const int32_t off = desc[2 * t], r0 = desc[2 * t + 1];
  const int32_t w = desc[2 * t + 2] - off, nr = desc[2 * t + 3] - r0;
  if (w <= 0 || nr <= 0) return;
  int32_t n = 0, k0 = 0;
  if (lane < nr) {
    n = (int32_t)len[r0 + lane];
    k0 = row_ptr[r0 + lane];
  }
  const TV *row = src + k0;
  TV *out = dst + (int64_t)off * kWave;
  const int32_t ng = w / G;
  if constexpr (STAGE) {
    // the slice's rows are the CSR range [beg, end); one that would not fit the
    // wave's LDS (no handle builds such a slice) takes the direct path below
    const int32_t beg = row_ptr[r0], end = row_ptr[r0 + nr];
    if (end - beg <= stage_cap<TV>()) {  // wave-uniform
      TV *mine = stage + wid * stage_cap<TV>();
      for (int32_t i = lane; i < end - beg; i += kWave) mine[i] = src[(int64_t)beg + i];
      dev::wave_sync();
      const TV *lrow = mine + (lane < nr ? k0 - beg : 0);
      for (int32_t g = 0; g < ng; ++g) {
        tv v;
#pragma unroll
        for (int e = 0; e < G; ++e) {
          const int32_t k = g * G + e;
          v[e] = k < n ? lrow[k] : TV(0);
        }
        *reinterpret_cast<tv *>(out + ((int64_t)g * kWave + lane) * G) = v;
      }
      for (int32_t k = ng * G; k < w; ++k) out[(int64_t)k * kWave + lane] = k < n ? lrow[k] : TV(0);
      return;
    }
  }
  for (int32_t g = 0; g < ng; ++g) {
    tv v;
#pragma unroll
    for (int e = 0; e < G; ++e) {
      const int32_t k = g * G + e;
      v[e] = k < n ? row[k] : TV(0);
    }
    *reinterpret_cast<tv *>(out + ((int64_t)g * kWave + lane) * G) = v;
  }
  for (int32_t k = ng * G; k < w; ++k) out[(int64_t)k * kWave + lane] = k < n ? row[k] : TV(0);
}

template <typename TV, int L>
__global__ __launch_bounds__(256) void hspmv_refresh_slabs(int32_t m, int32_t n_slabs,
                                                           const int32_t *__restrict__ row_ptr,
                                                           const int32_t *__restrict__ slab_rp,
                                                           const TV *__restrict__ src, TV *__restrict__ dst) {
  const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) / L;
  const int32_t sub = (int32_t)(threadIdx.x % L);
  if (r >= m) return;
  int64_t k = row_ptr[r];
  const int32_t *p = slab_rp + r;
  for (int32_t b = 0; b < n_slabs; ++b, p += (int64_t)m + 1) {
    const int32_t o0 = p[0], o1 = p[1];
    for (int32_t i = sub; i < o1 - o0; i += L) dst[(int64_t)o0 + i] = src[k + i];
    k += o1 - o0;
  }
}

template <typename F>
hipError_t with_value_type(int val_dtype, F &&f) {
  hipError_t e = hipErrorInvalidValue;  // the stored values: fp32 or fp64
  static_switch<HSPMV_F32, HSPMV_F64>(val_dtype, [&](auto DT) {
    using TV = std::conditional_t<DT == HSPMV_F64, double, float>;
    e = f(TV());
  });
  return e;
}

}  // namespace

hipError_t launch_refresh_slices(int val_dtype, int64_t n_slices, const int32_t *desc, const uint8_t *len,
                                 const int32_t *row_ptr, const void *src, void *dst, hipStream_t st) {
  if (n_slices <= 0) return hipSuccess;
  constexpr bool kStage = HSPMV_REFRESH_STAGE != 0;
  constexpr int kWaves = kStage ? kStageWaves : kRefreshWaves;
  const int64_t blocks = (n_slices + kWaves - 1) / kWaves;
  if (n_slices > INT32_MAX || !desc || !len || !row_ptr || !src || !dst) return hipErrorInvalidValue;
  return with_value_type(val_dtype, [&](auto tv) {
    using TV = decltype(tv);
    hipLaunchKernelGGL((hspmv_refresh_slices<TV, kStage>), dim3((unsigned)blocks), dim3(kWaves * kWave), 0, st,
                       (int32_t)n_slices, desc, len, row_ptr, static_cast<const TV *>(src),
                       static_cast<TV *>(dst));
    return hipGetLastError();
  });
}

hipError_t launch_refresh_slabs(int val_dtype, int32_t m, int64_t nnz, int32_t n_slabs, const int32_t *row_ptr,
                                const int32_t *slab_rp, const void *src, void *dst, hipStream_t st) {
  if (m <= 0 || nnz <= 0 || n_slabs <= 0) return hipSuccess;
  if (!row_ptr || !slab_rp || !src || !dst) return hipErrorInvalidValue;
  // lanes per row: about four entries per lane on the mean row, at least 8
  // (a row at the split threshold is then 512 strided copies per lane, 64 on
  // matrices whose mean row is long)
  const int64_t mean = nnz / m;
  const int lanes = mean > 128 ? 64 : (mean > 64 ? 32 : (mean > 32 ? 16 : 8));
  const int64_t blocks = ((int64_t)m * lanes + 255) / 256;
  if (blocks > INT32_MAX) return hipErrorInvalidValue;
  return with_value_type(val_dtype, [&](auto tv) {
    using TV = decltype(tv);
    hipError_t e = hipErrorInvalidValue;
    static_switch<8, 16, 32, 64>(lanes, [&](auto L) {
      hipLaunchKernelGGL((hspmv_refresh_slabs<TV, L>), dim3((unsigned)blocks), dim3(256), 0, st, m, n_slabs,
                         row_ptr, slab_rp, static_cast<const TV *>(src), static_cast<TV *>(dst));
      e = hipGetLastError();
    });
    return e;
  });
}

}  // namespace hspmv
