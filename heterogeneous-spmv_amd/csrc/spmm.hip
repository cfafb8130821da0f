// spmm.hip -- multi-vector SpMM for gfx950: Y = A X for k <= 32 right-hand
// sides in one pass over A (hspmv_mm_*, include/hspmv.h).
//
// X is row-major n x k with leading dimension ldx (the k values of one row
// of X contiguous), Y row-major m x k with ldy.  A is plain CSR: none of the
// single-vector formats (16-bit columns, dictionaries, row slices) applies.
// KP = the smallest power of two >= k is the lanes one row takes; lanes with
// c >= k stay idle and the padding columns of X and Y are never touched.
//
//  * hspmv_mm_rows<T, KP, NT>   rows of <= serial_max nonzeros
//      A wave owns R = 64 / KP consecutive rows; lane (r, c), c the fastest
//      lane index, owns Y[row r, column c].  The R rows' nonzeros are one
//      contiguous range: the wave reads it coalesced, mm_chunk<KP>() entries
//      at a time on 64-entry boundaries, into its slice of a static LDS buffer.
//      Each lane then walks its own row's entries of the chunk left to right
//      (the KP lanes of a row read the same LDS word: a broadcast) and
//      gathers X[col * ldx + c], kMmBatch gathers in flight, so one wave
//      instruction touches R segments of k * sizeof(T) contiguous bytes.
//      sum = sum + (v * x) from 0 with a rounded product and a separate add
//      (-ffp-contract=off, no fma): the
//      operations and the order of omp_spmv (spmv-csr/spmv.c:92-114), so
//      column c of Y is bit for bit what omp_spmv -- and hspmv_spmv on these
//      rows -- gives for x = X[:, c].  An empty row stores +0.0.  Chunks that
//      lie wholly inside longer rows are skipped unread.
//
//  * hspmv_mm_long<T, KP, NT>   rows over serial_max (the host's table)
//      One wave per listed row, lanes (s, c) with S = 64 / KP slots: slot s
//      adds entries beg + s, beg + s + S, ... in order, then a fixed xor tree
//      runs over s and the s == 0 lanes store.  Deterministic, bit-identical
//      run to run; within the project's tolerance of omp_spmv, not its bits.
//      Rows over 4096 nonzeros stay on their one wave in this version (the
//      single-vector library splits them over workgroups).
//
// All index arithmetic into X and Y is 64-bit (n * ldx may exceed 2^31).
// LDS is static only.  Out of scope here: multi-GPU shards, k > 32, CSR-3
// maps, x dictionaries or row slices for X, column-major X, alpha / beta.
#include "dev_prims.cuh"
#include "hspmv_common.h"
#include "hspmv_internal.h"
#include "static_switch.h"

namespace hspmv {
namespace {

using dev::ldg;
using dev::wave_sync;

constexpr int kMmWaves = 4;     // waves per 256-thread workgroup
constexpr int kMmBatch = 8;     // gathers a lane keeps in flight
// Nonzeros a wave stages per pass.  A lane works only while the chunk holds
// entries of its own row, so the chunk should cover the wave's R rows: with
// 256 entries and R = 32 rows of 27, a third of the lanes had work per pass
// and the passes' gather latencies added up (C3 fp64 k = 2: 300 us).
constexpr int kMmMaxChunk = 768;
template <int KP>
constexpr int mm_chunk() {
  return KP <= 2 ? kMmMaxChunk : (KP == 4 ? 512 : 256);
}

template <typename T, int KP, bool NT>
__global__ __launch_bounds__(256) void hspmv_mm_rows(int32_t m, int32_t k, int32_t serial_max,
                                                     const int32_t *__restrict__ rp,
                                                     const int32_t *__restrict__ ci,
                                                     const T *__restrict__ val, const T *__restrict__ X,
                                                     int64_t ldx, T *__restrict__ Y, int64_t ldy) {
  constexpr int R = 64 / KP;
  constexpr int kMmChunk = mm_chunk<KP>();
  __shared__ int32_t s_col[kMmWaves][kMmChunk];
  __shared__ T s_val[kMmWaves][kMmChunk];
  static_assert(kMmChunk % 64 == 0 && kMmChunk <= kMmMaxChunk, "chunks are whole 64-entry loads");
  static_assert(sizeof(int32_t) * kMmWaves * kMmChunk + sizeof(T) * kMmWaves * kMmChunk <= 36 * 1024,
                "static LDS of the SpMM row kernel must stay well below the 64 KiB limit");
  const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
  const int c = lane & (KP - 1), r = lane / KP;
  // whole waves leave here and the kernel has no workgroup barrier
  const int64_t r0 = ((int64_t)blockIdx.x * kMmWaves + w) * R;
  if (r0 >= m) return;
  const int64_t row = r0 + r;
  const int32_t rend = (int32_t)(r0 + R < m ? r0 + R : m);
  const int32_t k0 = rp[r0], k1 = rp[rend];  // the wave's nonzeros (wave-uniform)
  int32_t beg = 0, end = 0;
  if (row < m) {
    beg = rp[row];
    end = rp[row + 1];
  }
  // a lane without work: past m, a padding column, or a row of the long-row kernel
  const bool mine = row < m && c < k && end - beg <= serial_max;
  if (!mine) end = beg;
  int32_t *scol = s_col[w];
  T *sval = s_val[w];
  T sum = 0;
  for (int32_t cb = k0 & ~63; cb < k1; cb += kMmChunk) {
    const int32_t lo = beg > cb ? beg : cb;
    const int32_t hi = end < cb + kMmChunk ? end : cb + kMmChunk;
    if (!__any(lo < hi)) continue;  // inside long rows: nothing to stage
    wave_sync();  // the previous chunk's reads are done
#pragma unroll
    for (int u = 0; u < kMmChunk / 64; ++u) {
      const int32_t i = cb + u * 64 + lane;
      if (i >= k0 && i < k1) {
        scol[u * 64 + lane] = ldg<NT>(ci + i);
        sval[u * 64 + lane] = ldg<NT>(val + i);
      }
    }
    wave_sync();
    for (int32_t j = lo; j < hi; j += kMmBatch) {
      T v[kMmBatch], xv[kMmBatch];
#pragma unroll
      for (int q = 0; q < kMmBatch; ++q) {  // nothing is loaded past the row's end
        v[q] = 0;
        xv[q] = 0;
        if (j + q < hi) {
          v[q] = sval[j + q - cb];
          xv[q] = X[(int64_t)scol[j + q - cb] * ldx + c];
        }
      }
#pragma unroll
      for (int q = 0; q < kMmBatch; ++q)
        if (j + q < hi) sum = sum + (v[q] * xv[q]);
    }
  }
  if (mine) Y[row * ldy + c] = sum;
}

template <typename T, int KP, bool NT>
__global__ __launch_bounds__(256) void hspmv_mm_long(int32_t n_long, int32_t k,
                                                     const int32_t *__restrict__ long_row,
                                                     const int32_t *__restrict__ rp,
                                                     const int32_t *__restrict__ ci,
                                                     const T *__restrict__ val, const T *__restrict__ X,
                                                     int64_t ldx, T *__restrict__ Y, int64_t ldy) {
  constexpr int S = 64 / KP;
  const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
  const int64_t t = (int64_t)blockIdx.x * kMmWaves + w;
  if (t >= n_long) return;
  const int64_t row = long_row[t];
  const int32_t beg = rp[row], end = rp[row + 1];
  const int c = lane & (KP - 1), s = lane / KP;
  // padding lanes gather column 0 (in bounds) and never store
  const bool live = c < k;
  const int cc = live ? c : 0;
  T sum = 0;
  for (int32_t i = beg + s; i < end; i += kMmBatch * S) {
    T v[kMmBatch], xv[kMmBatch];
#pragma unroll
    for (int q = 0; q < kMmBatch; ++q) {
      const int32_t ii = i + q * S < end ? i + q * S : i;
      v[q] = ldg<NT>(val + ii);
      xv[q] = X[(int64_t)ldg<NT>(ci + ii) * ldx + cc];
    }
#pragma unroll
    for (int q = 0; q < kMmBatch; ++q)
      if (i + q * S < end) sum = sum + (v[q] * xv[q]);
  }
#pragma unroll
  for (int off = 32; off >= KP; off >>= 1) sum = sum + __shfl_xor(sum, off, 64);
  if (s == 0 && live) Y[row * ldy + c] = sum;
}

template <typename T, int KP, bool NT>
hipError_t launch_kp(const DevMM &d, int64_t blocks, const T *X, int64_t ldx, T *Y, int64_t ldy,
                     hipStream_t st) {
  const T *val = static_cast<const T *>(d.val);
  hipLaunchKernelGGL((hspmv_mm_rows<T, KP, NT>), dim3((unsigned)blocks), dim3(256), 0, st, d.m, d.k,
                     d.serial_max, d.row_ptr, d.col_idx, val, X, ldx, Y, ldy);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || d.n_long == 0) return e;
  hipLaunchKernelGGL((hspmv_mm_long<T, KP, NT>), dim3((unsigned)((d.n_long + kMmWaves - 1) / kMmWaves)),
                     dim3(256), 0, st, d.n_long, d.k, d.long_row, d.row_ptr, d.col_idx, val, X, ldx, Y,
                     ldy);
  return hipGetLastError();
}

template <typename T, bool NT>
hipError_t launch_typed(const DevMM &d, int64_t blocks, const T *X, int64_t ldx, T *Y, int64_t ldy,
                        hipStream_t st) {
  hipError_t e = hipErrorInvalidValue;  // lanes per row: a power of two up to 32
  static_switch<1, 2, 4, 8, 16, 32>(d.lanes_per_row,
                                    [&](auto KP) { e = launch_kp<T, KP, NT>(d, blocks, X, ldx, Y, ldy, st); });
  return e;
}

}  // namespace

int launch_spmm(const DevMM &d, int dtype, const void *X, int64_t ldx, void *Y, int64_t ldy,
                hipStream_t st) {
  if (d.k < 1 || d.k > kMmMaxRhs || d.lanes_per_row != mm_lanes_per_row(d.k))
    return set_error(HSPMV_E_INVALID, "SpMM launch: k = %d with %d lanes per row", d.k, d.lanes_per_row);
  if (d.m < 0 || d.nnz < 0 || d.nnz > (int64_t)INT32_MAX - 2 * kMmMaxChunk)
    return set_error(HSPMV_E_INVALID, "SpMM launch: m = %d, nnz = %lld beyond the kernel's 32-bit nonzero index",
                     d.m, (long long)d.nnz);
  if (ldx < d.k || ldy < d.k)
    return set_error(HSPMV_E_INVALID, "SpMM launch: ldx = %lld, ldy = %lld below k = %d", (long long)ldx,
                     (long long)ldy, d.k);
  const int64_t blocks = mm_blocks(d.m, d.lanes_per_row);
  if (blocks > INT32_MAX || d.n_long < 0 || d.n_long > d.m)
    return set_error(HSPMV_E_INVALID, "SpMM launch: grid of %lld blocks, %d long rows", (long long)blocks,
                     d.n_long);
  if (d.m == 0) return HSPMV_OK;
  hipError_t e;
  if (dtype == HSPMV_F64)
    e = d.nontemporal ? launch_typed<double, true>(d, blocks, (const double *)X, ldx, (double *)Y, ldy, st)
                      : launch_typed<double, false>(d, blocks, (const double *)X, ldx, (double *)Y, ldy, st);
  else
    e = d.nontemporal ? launch_typed<float, true>(d, blocks, (const float *)X, ldx, (float *)Y, ldy, st)
                      : launch_typed<float, false>(d, blocks, (const float *)X, ldx, (float *)Y, ldy, st);
  if (e != hipSuccess) return set_error(HSPMV_E_HIP, "SpMM launch failed: %s", hipGetErrorString(e));
  return HSPMV_OK;
}

}  // namespace hspmv
