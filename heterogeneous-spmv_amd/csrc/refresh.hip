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
//      slab_rp_b[r] CSR entries of the row (plan_xslabs, hspmv_tables.cpp),
//      so the lanes walk the B row-pointer arrays in slab order and copy each
//      segment with consecutive lanes on consecutive entries.  Split rows have
//      empty segments in every slab: nothing is copied for them (the split-row
//      kernels read the CSR order).
//
//  * hspmv_refresh_csort<TV, WIDE, FIXP>  the entry stream of the
//      column-sorted tables (csort.hip), for a handle that kept its
//      source-index table (hspmv_create_updatable; DevCsort.src)
//      One 1024-thread workgroup per csort workgroup b; each wave walks whole
//      chunks of [blk_c[b], blk_c[b+1]), 64 consecutive stream positions per
//      step, so src is read and the stream written in full 64-lane lines.
//      src[p] is the CSR index of the value stored at position p: fp32 loads
//      the 8-byte {idx, val} record, replaces the value word and stores the
//      record whole (a 4-byte store at stride 8 would write half sectors);
//      fp64 stores into the value array.  Padding (kCsortSrcPad) stores 0.
//      FIXP (fixed-point slots): the value is scaled by 2^e, e = the rexp of
//      the slot's row or the sexp of its long-row slice (slot = idx >> 16, the
//      tables the SpMV's finishing code reads), in fp64 and narrowed once, so
//      a result below the type's normal range is rounded once to nearest even
//      as std::ldexp does on the host (Values, hspmv_csort_build.cpp).  The
//      fp64 index word of a WIDE stream sits at another position than its
//      value (4 per lane against 2): idx_of_val.
//
//  * hspmv_refresh_row_scales<TV, L>  rexp of a fixed-point handle, L lanes per
//      row (a row over 256 nonzeros: the whole wave): -(ilogb(max |v|) + 1) -
//      extra, extra from the row's length alone (row_scales,
//      hspmv_csort_build.cpp); 0 for a zero or empty row.
//    hspmv_refresh_long_scales<TV>   one workgroup per long row (the rows the
//      kernel slices): its rexp and sexp[slice] = that for each of its slices.
//
// Values move as stored (TV: float or double; a mixed handle's are float), bit
// for bit: no arithmetic touches them but the fixed-point power-of-two scale.
// Plain HIP C++ with vector stores, static LDS only, no atomics.
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

constexpr int kCsortRefreshThreads = 1024;

// WIDE fp64 streams: the position, within its chunk, of the index word of the
// entry whose value is stored at pl (`at`, hspmv_csort_build.cpp: values are
// interleaved 2 per lane, indices 4 per lane)
__device__ __forceinline__ int32_t idx_of_val(int32_t pl) {
  const int32_t u = (pl >> 7) * 2 + (pl & 1), lane = (pl & 127) >> 1;
  return (u >> 2) * 256 + lane * 4 + (u & 3);
}

template <typename TV, bool WIDE, bool FIXP>
__global__ __launch_bounds__(kCsortRefreshThreads) void hspmv_refresh_csort(
    int32_t C, const int32_t *__restrict__ blk_c, const int32_t *__restrict__ blk_r,
    const int32_t *__restrict__ blk_v, const int32_t *__restrict__ vslice, const int16_t *__restrict__ rexp,
    const int16_t *__restrict__ sexp, const uint32_t *__restrict__ src, const TV *__restrict__ val,
    void *__restrict__ ent, TV *__restrict__ out) {
  const int32_t b = (int32_t)blockIdx.x;
  const int32_t c0 = blk_c[b], c1 = blk_c[b + 1];
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
  int32_t r0 = 0, nr = 0, v0 = 0;
  if constexpr (FIXP) {
    r0 = blk_r[2 * b];
    nr = blk_r[2 * b + 1] - r0;
    v0 = blk_v[b];
  }
  // the scale of slot `slot` of this workgroup (never asked for the dummy
  // slot: padding is known by its src)
  auto scale = [&](uint32_t slot) -> int {
    return (int32_t)slot < nr ? (int)rexp[r0 + (int32_t)slot] : (int)sexp[vslice[v0 + (int32_t)slot - nr]];
  };
  // four 64-position steps at a time (a chunk holds 4, 8 or 16 of them): the
  // source indices first, then the gathers and the records, so that a wave
  // has four of each in flight
  constexpr int G = 4;
  for (int32_t c = c0 + wid; c < c1; c += kCsortRefreshThreads / kWave) {  // wave-uniform
    const int64_t base = (int64_t)c * C;
    for (int32_t g = 0; g < C; g += G * kWave) {
      uint32_t k[G];
      TV v[G];
      uint2 e[G];
#pragma unroll
      for (int j = 0; j < G; ++j) k[j] = src[base + g + j * kWave + lane];
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const int32_t pl = g + j * kWave + lane;
        if constexpr (sizeof(TV) == 4) {
          e[j] = static_cast<const uint2 *>(ent)[base + pl];
        } else if constexpr (FIXP) {
          e[j].x = static_cast<const uint32_t *>(ent)[base + (WIDE ? idx_of_val(pl) : pl)];
        }
        v[j] = k[j] != kCsortSrcPad ? val[k[j]] : TV(0);
      }
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const int64_t p = base + g + j * kWave + lane;
        if constexpr (FIXP) {  // in fp64, narrowed once: std::ldexp's single rounding
          if (k[j] != kCsortSrcPad) v[j] = (TV)ldexp((double)v[j], scale(e[j].x >> 16));
        }
        if constexpr (sizeof(TV) == 4) {
          e[j].y = __float_as_uint(v[j]);
          static_cast<uint2 *>(ent)[p] = e[j];
        } else {
          out[p] = v[j];
        }
      }
    }
  }
}

constexpr int32_t kScaleWaveRow = 256;  // rows over this many nonzeros take the whole wave

template <typename TV, int L>
__global__ __launch_bounds__(256) void hspmv_refresh_row_scales(int32_t m, int32_t long_t,
                                                                const int32_t *__restrict__ row_ptr,
                                                                const TV *__restrict__ val,
                                                                int16_t *__restrict__ rexp) {
  const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) / L;
  const int32_t sub = (int32_t)(threadIdx.x % L), lane = (int32_t)(threadIdx.x & (kWave - 1));
  int32_t k0 = 0, k1 = 0;
  if (r < m) {
    k0 = row_ptr[r];
    k1 = row_ptr[r + 1];
  }
  // (no lane leaves before the wave-wide steps below)
  const bool mine = r < m && k1 - k0 <= long_t;  // a long row: hspmv_refresh_long_scales
  const bool whole = mine && k1 - k0 > kScaleWaveRow;
  double mx = 0.0;
  if (mine && !whole)
    for (int32_t k = k0 + sub; k < k1; k += L) mx = fmax(mx, fabs((double)val[k]));
#pragma unroll
  for (int d = L / 2; d > 0; d >>= 1) mx = fmax(mx, __shfl_xor(mx, d, L));
  // the rows of this wave that L lanes would walk for hundreds of steps, one
  // after the other with all 64 lanes
  unsigned long long todo = __ballot(whole && sub == 0);
  while (todo) {  // wave-uniform
    const int l = __ffsll(todo) - 1;
    todo &= todo - 1;
    const int32_t a = __shfl(k0, l, kWave), b = __shfl(k1, l, kWave);
    double w = 0.0;
    for (int32_t k = a + lane; k < b; k += kWave) w = fmax(w, fabs((double)val[k]));
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) w = fmax(w, __shfl_xor(w, d, kWave));
    if (lane == l) mx = w;
  }
  if (!mine || sub != 0) return;
  int e = 0;
  if (mx > 0.0) {
    const int64_t len = k1 - k0;
    int extra = 0;  // a row kept whole over 4096 nonzeros (row_scales)
    while (len <= long_t && ((int64_t)4096 << extra) < len) ++extra;
    e = -(ilogb(mx) + 1) - extra;
  }
  rexp[r] = (int16_t)e;
}

// One workgroup per long row j (> long_t nonzeros, so its `extra` is 0): the
// row's rexp and the sexp of its slices [long_cs[j], long_cs[j + 1]).
template <typename TV>
__global__ __launch_bounds__(256) void hspmv_refresh_long_scales(const int32_t *__restrict__ long_row,
                                                                 const int32_t *__restrict__ long_cs,
                                                                 const int32_t *__restrict__ row_ptr,
                                                                 const TV *__restrict__ val,
                                                                 int16_t *__restrict__ rexp,
                                                                 int16_t *__restrict__ sexp) {
  __shared__ double wmx[256 / kWave];
  const int32_t j = (int32_t)blockIdx.x, r = long_row[j];
  const int32_t k0 = row_ptr[r], k1 = row_ptr[r + 1];
  double mx = 0.0;
  for (int32_t k = k0 + (int32_t)threadIdx.x; k < k1; k += 256) mx = fmax(mx, fabs((double)val[k]));
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) mx = fmax(mx, __shfl_xor(mx, d, kWave));
  if ((threadIdx.x & (kWave - 1)) == 0) wmx[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmax(fmax(wmx[0], wmx[1]), fmax(wmx[2], wmx[3]));
  const int16_t e = mx > 0.0 ? (int16_t)(-(ilogb(mx) + 1)) : (int16_t)0;
  if (threadIdx.x == 0) rexp[r] = e;
  for (int32_t sl = long_cs[j] + (int32_t)threadIdx.x; sl < long_cs[j + 1]; sl += 256) sexp[sl] = e;
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

// (The SpMV reads these tables through DevCsort's const views; the shard's
// DevCtx owns them, and the refresh is what writes them.)
hipError_t launch_refresh_csort(int val_dtype, const DevCsort &c, const void *src_val, hipStream_t st) {
  if (c.n_wg <= 0 || c.chunks <= 0) return hipSuccess;
  const bool f32 = val_dtype == HSPMV_F32;
  if (!c.src || !src_val || !c.blk_c || !c.ent || (!f32 && !c.val) || (c.u != 4 && c.u != 8 && c.u != 16))
    return hipErrorInvalidValue;
  if (c.fixed && (!c.rexp || !c.sexp || !c.blk_r || !c.blk_v || !c.vslice)) return hipErrorInvalidValue;
  return with_value_type(val_dtype, [&](auto tv) {
    using TV = decltype(tv);
    static_flag(c.fixed, [&](auto FIXP) {
      // (only the fp64 fixed-point form looks an index word up by its value's
      // position: the one pair for which a WIDE kernel exists)
      static_flag<sizeof(TV) == 8 && decltype(FIXP)::value>(c.wide, [&](auto WIDE) {
        hipLaunchKernelGGL((hspmv_refresh_csort<TV, WIDE, FIXP>), dim3((unsigned)c.n_wg),
                           dim3(kCsortRefreshThreads), 0, st, (int32_t)(kWave * c.u), c.blk_c, c.blk_r, c.blk_v,
                           c.vslice, c.rexp, c.sexp, c.src, static_cast<const TV *>(src_val),
                           const_cast<void *>(c.ent), static_cast<TV *>(const_cast<void *>(c.val)));
      });
    });
    return hipGetLastError();
  });
}

hipError_t launch_refresh_row_scales(int val_dtype, const DevCsort &c, const int32_t *row_ptr,
                                     const void *src_val, hipStream_t st) {
  if (!c.fixed || c.m <= 0) return hipSuccess;
  if (!c.rexp || !c.sexp || !row_ptr || !src_val || c.m > INT32_MAX) return hipErrorInvalidValue;
  if (c.n_long > 0 && (!c.long_row || !c.long_cs)) return hipErrorInvalidValue;
  constexpr int kLanes = 8;  // per row: the rows of these matrices are short (long ones: 64-byte strides)
  const int64_t blocks = (c.m * kLanes + 255) / 256;
  if (blocks > INT32_MAX) return hipErrorInvalidValue;
  int16_t *rexp = const_cast<int16_t *>(c.rexp);
  return with_value_type(val_dtype, [&](auto tv) {
    using TV = decltype(tv);
    hipLaunchKernelGGL((hspmv_refresh_row_scales<TV, kLanes>), dim3((unsigned)blocks), dim3(256), 0, st,
                       (int32_t)c.m, c.long_t, row_ptr, static_cast<const TV *>(src_val), rexp);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && c.n_long > 0) {
      hipLaunchKernelGGL((hspmv_refresh_long_scales<TV>), dim3((unsigned)c.n_long), dim3(256), 0, st, c.long_row,
                         c.long_cs, row_ptr, static_cast<const TV *>(src_val), rexp,
                         const_cast<int16_t *>(c.sexp));
      e = hipGetLastError();
    }
    return e;
  });
}

}  // namespace hspmv
