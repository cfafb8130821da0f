// slice_kernel.cuh -- hspmv_slices, the lane-per-row kernel of dictionary
// handles with row slices (STREAM / CSR3 handles; instantiated beside the row
// kernels, row_launch.cuh), hspmv_slices_axpby, its twin whose store is the
// y = alpha (A x) + beta y epilogue, and hspmv_slices_axpby_dot, which also
// sums w . y and y . y over the values it stores.  Device code only.
//
// The transposed (sliced-ELL) shape of the dictionary kernels, for handles
// whose every row is summed serially anyway (hspmv_slices.cpp holds the
// format and the eligibility rules).  A wave's task of <= 64 rows is stored
// column-major: lane i owns row i, slot k of all 64 rows lies together, so
// one load instruction brings 16 bytes of values (2 fp64 / 4 fp32
// consecutive slots of the lane's row) or 8 bytes of positions (4 slots) per
// lane, and the lane multiplies and adds its own row left to right -- the
// order and rounding of the ordered sums, with no product buffer in LDS, no
// wave_sync and no row pointers.  Slot k of a slice starts at element 64 * k
// of the slice in both streams (groups and the trailing single columns
// alike).  Slots past a row's end are masked by its length, never added.
//
// PB = 12 (a handle whose positions all fit 12 bits, dictionaries of <= 4096
// entries, hspmv_slices_pack): a whole batch of 8 slots reads one 12-byte
// position group per lane, eight 12-bit fields, at 96 bytes per slot column;
// the slice's last w mod 8 slots follow in the 16-bit layout, and the slice
// starts at 128 * ppre[t] bytes.
#pragma once
#include "row_kernels.cuh"  // XDict, stage_xdict

namespace hspmv {
namespace dev {

#ifndef HSPMV_SLICE_BATCH
#define HSPMV_SLICE_BATCH 8  // slots per load batch (a multiple of 4)
#endif

struct Slices {
  const int32_t *desc;  // {prefix, first row} per task, closed by {total, m}
  const uint8_t *len;   // nonzeros per row
  const uint16_t *pos;  // dictionary positions, 64 * prefix elements per slice start
  const int32_t *ppre;  // PB = 12: the packed positions' start per task, 128-byte units
};

typedef int32_t sl_i4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t sl_u3 __attribute__((ext_vector_type(3), aligned(4)));

template <typename TV, int B>
struct SliceBatch {
  TV v[B];              // slot k0 + i of the lane's row, as stored
  uint32_t pq[B / 2];   // positions of whole 4-slot groups, two per register (PB = 12: 3 per 8 slots)
  uint32_t ps[3];       // positions of the slice's last 1-3 slots (single columns)
};

// Where the batch at slot k0 starts in the slice's streams vb / pb, and the
// vectors its groups load as: G values (16 bytes), 4 16-bit positions (u2).
template <typename TV, int PB>
struct SliceAt {
  static constexpr int G = 16 / (int)sizeof(TV);
  typedef TV tv __attribute__((ext_vector_type(G)));
  typedef uint32_t u2 __attribute__((ext_vector_type(2)));
  const gchar *vbb, *pbb;
  __device__ __forceinline__ SliceAt(const gchar *vb, const gchar *pb, int32_t k0)
      : vbb(vb + (uint64_t)(uint32_t)k0 * (kWave * sizeof(TV))),
        pbb(pb + (uint64_t)(uint32_t)k0 * (kWave * PB / 8u)) {}
};

// A whole batch: slots [k0, k0 + B) all lie in 16-byte value groups and
// 8-byte (PB = 12: 12-byte) position groups.
template <typename TV, bool NT, int B, int PB>
__device__ __forceinline__ void slice_load_full(SliceBatch<TV, B> &q, const gchar *vb, const gchar *pb,
                                                int32_t k0, int lane) {
  typedef SliceAt<TV, PB> At;
  constexpr int G = At::G;
  const At at(vb, pb, k0);
#pragma unroll
  for (int j = 0; j < B / G; ++j) {
    const typename At::tv t = ld_off<NT, typename At::tv>(at.vbb, (uint32_t)(j * kWave + lane) * 16u);
#pragma unroll
    for (int e = 0; e < G; ++e) q.v[j * G + e] = t[e];
  }
  if constexpr (PB == 12) {
    // (sizeof(sl_u3) is 16: the groups are addressed in bytes)
#pragma unroll
    for (int g = 0; g < B / 8; ++g) {
      const sl_u3 t = ld_off<NT, sl_u3>(at.pbb, (uint32_t)(g * kWave + lane) * 12u);
      q.pq[3 * g] = t[0];
      q.pq[3 * g + 1] = t[1];
      q.pq[3 * g + 2] = t[2];
    }
  } else {
#pragma unroll
    for (int g = 0; g < B / 4; ++g) {
      const typename At::u2 t = ld_off<NT, typename At::u2>(at.pbb, (uint32_t)(g * kWave + lane) * 8u);
      q.pq[2 * g] = t[0];
      q.pq[2 * g + 1] = t[1];
    }
  }
}

// The slice's last, partial batch: slots [k0, w), w - k0 < B; whole groups
// as above, the rest from the single columns.  Slots past w read as value 0
// at position 0 (and are masked like every slot past a row's end).  The
// tail's positions are 16-bit for either PB; PB sets where they start.
template <typename TV, bool NT, int B, int PB>
__device__ __forceinline__ void slice_load_tail(SliceBatch<TV, B> &q, const gchar *vb, const gchar *pb,
                                                int32_t k0, int32_t w, int lane) {
  typedef SliceAt<TV, PB> At;
  constexpr int G = At::G;
  const At at(vb, pb, k0);
#pragma unroll
  for (int i = 0; i < B; ++i) q.v[i] = TV(0);
#pragma unroll
  for (int i = 0; i < B / 2; ++i) q.pq[i] = 0u;
#pragma unroll
  for (int i = 0; i < 3; ++i) q.ps[i] = 0u;
#pragma unroll
  for (int j = 0; j < B / G; ++j) {
    if (k0 + j * G + G <= w) {  // wave-uniform
      const typename At::tv t = ld_off<NT, typename At::tv>(at.vbb, (uint32_t)(j * kWave + lane) * 16u);
#pragma unroll
      for (int e = 0; e < G; ++e) q.v[j * G + e] = t[e];
    } else {
#pragma unroll
      for (int e = 0; e < G - 1; ++e)
        if (k0 + j * G + e < w)
          q.v[j * G + e] = ld_off<NT, TV>(at.vbb, (uint32_t)((j * G + e) * kWave + lane) * (uint32_t)sizeof(TV));
    }
  }
#pragma unroll
  for (int g = 0; g < B / 4; ++g) {
    if (k0 + 4 * g + 4 <= w) {
      const typename At::u2 t = ld_off<NT, typename At::u2>(at.pbb, (uint32_t)(g * kWave + lane) * 8u);
      q.pq[2 * g] = t[0];
      q.pq[2 * g + 1] = t[1];
    } else {
#pragma unroll
      for (int r = 0; r < 3; ++r)
        if (k0 + 4 * g + r < w)
          q.ps[r] = (uint32_t)ld_off<NT, uint16_t>(at.pbb, (uint32_t)((4 * g + r) * kWave + lane) * 2u);
    }
  }
}

// Position of slot i of a whole batch.
template <int PB>
__device__ __forceinline__ uint32_t slice_pos(const uint32_t *pq, int i) {
  if constexpr (PB == 12) {
    const int d = 3 * (i / 8) + 12 * (i % 8) / 32, sh = 12 * (i % 8) % 32;
    uint32_t v = pq[d] >> sh;
    if (sh > 20) v |= pq[d + 1] << (32 - sh);
    return v & 0xfffu;
  } else {
    return (pq[i / 2] >> (16 * (i & 1))) & 0xffffu;
  }
}

// Adds the batch's slots to acc in slot order: the product rounded on its
// own (-ffp-contract=off), then the add; a slot at or past the row's end
// leaves acc as it is.  full: every position comes from pq, PB bits each
// (a tail batch's are 16-bit).  A value stored narrower than T (TV) is
// widened here, once, before its product.
template <typename T, int B, int PB, typename TV>
__device__ __forceinline__ T slice_consume(T acc, const SliceBatch<TV, B> &q, const T *xs, int32_t k0,
                                           int32_t w, int32_t len, bool full) {
  T xv[B];
#pragma unroll
  for (int i = 0; i < B; ++i) {
    const int g = i / 4, r = i % 4;
    const uint32_t p = (full || k0 + 4 * g + 4 <= w) ? slice_pos<PB>(q.pq, i) : q.ps[r < 3 ? r : 0];
    xv[i] = xs[p];
  }
#pragma unroll
  for (int i = 0; i < B; ++i) {
    const T p = (T)q.v[i] * xv[i];
    acc = (k0 + i < len) ? acc + p : acc;
  }
  return acc;
}

// What a slice kernel does with a row's sum before it is stored.  `before`
// runs ahead of the slot loop, for the lanes that own a row, and what it
// returns is handed to `after` with the sum.  A policy with kTerms (only
// SliceAxpbyDot) also has `terms`, which takes the stored value on the same
// lanes, and `reduce`, which runs on every lane of a wave that has rows with
// what `terms` left; without kTerms neither is compiled.
// hspmv_slices: the sum as it is.
template <typename T>
struct SliceStoreSum {
  static constexpr bool kTerms = false;
  struct Terms {};
  struct Old {};
  __device__ __forceinline__ Old before(const T *, int32_t) const { return Old{}; }
  __device__ __forceinline__ T after(T acc, Old) const { return acc; }
};

// Where SliceAxpby issues its load of the old y: 1 before the slot loop (the
// load's latency under the whole slice, its registers held through it), 0
// after it.
#ifndef HSPMV_SLICE_YLOAD_EARLY
#define HSPMV_SLICE_YLOAD_EARLY 1
#endif

// hspmv_slices_axpby: fl(fl(alpha s) + fl(beta y_old)), every operation
// rounded on its own (-ffp-contract=off), or fl(alpha s) alone when beta == 0
// -- a kernel-uniform branch that issues no load of y.
template <typename T>
struct SliceAxpby {
  static constexpr bool kTerms = false;
  struct Terms {};
  T alpha, beta;
  struct Old {
    const T *p;
    T v;
  };
  __device__ __forceinline__ Old before(const T *y, int32_t row) const {
    Old o{y + row, T(0)};
    if (HSPMV_SLICE_YLOAD_EARLY && beta != T(0)) o.v = *o.p;
    return o;
  }
  __device__ __forceinline__ T after(T acc, Old o) const {
    const T as = alpha * acc;
    if (beta == T(0)) return as;
    if (!HSPMV_SLICE_YLOAD_EARLY) o.v = *o.p;
    const T by = beta * o.v;
    return as + by;
  }
};

// hspmv_slices_axpby_dot: SliceAxpby's store, then the
// slice's share of w . y and y . y over the values just stored, in double
// whatever T is.  w: nullptr when w . y is not asked for (kernel-uniform, no
// load then); its load sits beside the old y's, ahead of the slot loop.  A
// lane that owns no row keeps both terms at 0.0.  One wave_sum_dpp per term
// (a fixed order), and lane 0 stores the pair to partials[t], t the logical
// slice: the sweep direction moves no partial.
typedef double sl_d2 __attribute__((ext_vector_type(2)));
template <typename T>
struct SliceAxpbyDot {
  static constexpr bool kTerms = true;
  SliceAxpby<T> ab;
  const T *w;
  uint32_t yy;  // y . y asked for
  sl_d2 *partials;
  struct Old {
    typename SliceAxpby<T>::Old o;
    T wv;
  };
  struct Terms {
    double wy = 0.0, yy = 0.0;
  };
  __device__ __forceinline__ Old before(const T *y, int32_t row) const {
    Old q{ab.before(y, row), T(0)};
    if (w) q.wv = w[row];
    return q;
  }
  __device__ __forceinline__ T after(T acc, const Old &q) const { return ab.after(acc, q.o); }
  __device__ __forceinline__ void terms(Terms &tm, T out, const Old &q) const {
    const double yd = (double)out;
    if (w) tm.wy = (double)q.wv * yd;
    if (yy) tm.yy = yd * yd;
  }
  __device__ __forceinline__ void reduce(const Terms &tm, int64_t t, int lane) const {
    const double a = wave_sum_dpp<double>(tm.wy);
    const double b = wave_sum_dpp<double>(tm.yy);
    if (lane == 0) partials[t] = sl_d2{a, b};
  }
};

// One workgroup = one dictionary block (four wave tasks, or a half block's
// two and two empty ones), staged by stage_xdict exactly as in the chunked
// kernels.  Each wave reads its slice's descriptor (one scalar load) and its
// rows' lengths before the staging; after the barrier it walks the slot
// columns in batches of B, the next batch's loads issued before the current
// one is consumed.  LDS: the dictionary alone.  Same bits as the row kernels.
// The body of the kernels below: EP is SliceStoreSum, SliceAxpby or
// SliceAxpbyDot.
template <typename T, bool NT, int B, int PB, typename TV, typename EP>
__device__ __forceinline__ void slices_body(int32_t n_slices, uint32_t blk_order, int32_t y_nt, const Slices &sl,
                                            const XDict &xd, const TV *__restrict__ val,
                                            const T *__restrict__ x, T *y, const EP &ep) {
  static_assert(B % 4 == 0 && B >= 4, "batches hold whole position groups");
  static_assert(PB == 16 || (PB == 12 && B % 8 == 0), "12-bit positions come in groups of 8 slots");
  static_assert(B % (16 / (int)sizeof(TV)) == 0, "batches hold whole 16-byte value groups");
  extern __shared__ __attribute__((aligned(16))) unsigned char xdyn[];
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t blk = sweep_block(blockIdx.x, gridDim.x, blk_order);
  const int64_t t = blk * 4 + wid;
  int32_t off = 0, poff = 0, w = 0, r0 = 0, nr = 0;
  if (t < n_slices) {  // wave-uniform
    const sl_i4 d = sload<sl_i4, 4>(sl.desc, (uint64_t)t * 8u);
    off = d[0];
    r0 = d[1];
    w = d[2] - d[0];
    nr = d[3] - d[1];
    poff = PB == 12 ? sload<int32_t>(sl.ppre, (uint64_t)t * 4u) : off;
  }
  int32_t len = 0;
  if (lane < nr) len = (int32_t)sl.len[r0 + lane];
  stage_xdict<T, 256>(reinterpret_cast<T *>(xdyn), x, xd, blk, threadIdx.x);
  if (nr <= 0) return;
  typename EP::Old old{};
  if (lane < nr) old = ep.before(y, r0 + lane);  // (the last slice's idle lanes address past row m)
  const T *xs = reinterpret_cast<const T *>(xdyn);
  const gchar *vb = uniform_ptr(val + (int64_t)off * kWave);
  const gchar *pb = uniform_ptr(sl.pos + (int64_t)poff * kWave);
  const int32_t wf = w & ~(B - 1);  // slots in whole batches
  T acc = T(0);
  SliceBatch<TV, B> cur, nxt, tail;
  int32_t k0 = 0;
  if (wf > 0) slice_load_full<TV, NT, B, PB>(cur, vb, pb, 0, lane);
  for (; k0 + 3 * B <= wf; k0 += 2 * B) {
    slice_load_full<TV, NT, B, PB>(nxt, vb, pb, k0 + B, lane);
    __builtin_amdgcn_sched_barrier(0);
    acc = slice_consume<T, B, PB>(acc, cur, xs, k0, w, len, true);
    __builtin_amdgcn_sched_barrier(0);
    slice_load_full<TV, NT, B, PB>(cur, vb, pb, k0 + 2 * B, lane);
    __builtin_amdgcn_sched_barrier(0);
    acc = slice_consume<T, B, PB>(acc, nxt, xs, k0 + B, w, len, true);
    __builtin_amdgcn_sched_barrier(0);
  }
  if (k0 + 2 * B <= wf) {
    slice_load_full<TV, NT, B, PB>(nxt, vb, pb, k0 + B, lane);
    __builtin_amdgcn_sched_barrier(0);
    acc = slice_consume<T, B, PB>(acc, cur, xs, k0, w, len, true);
    __builtin_amdgcn_sched_barrier(0);
    cur = nxt;
    k0 += B;
  }
  // cur: the last whole batch (at wf - B), not yet added
  if (w > wf) slice_load_tail<TV, NT, B, PB>(tail, vb, pb, wf, w, lane);
  __builtin_amdgcn_sched_barrier(0);
  if (wf > 0) acc = slice_consume<T, B, PB>(acc, cur, xs, wf - B, w, len, true);
  if (w > wf) acc = slice_consume<T, B, 16>(acc, tail, xs, wf, w, len, false);
  // (store_y's two stores, spelled out: they address y as y + r0 + lane and
  // y[r0 + lane], and either form alone compiles to other registers here)
  if constexpr (diag(kDiagNoStore)) {  // ablation: no y stores (kept live)
    if (lane < nr && acc == T(12345.678)) y[r0 + lane] = acc;
  } else {
    [[maybe_unused]] typename EP::Terms tm;
    if (lane < nr) {
      const T out = ep.after(acc, old);
      if (y_nt)
        __builtin_nontemporal_store(out, y + r0 + lane);
      else
        y[r0 + lane] = out;
      if constexpr (EP::kTerms) ep.terms(tm, out, old);
    }
    // every lane of the wave: the idle ones bring 0.0
    if constexpr (EP::kTerms) ep.reduce(tm, t, lane);
  }
}

// y = A x.
template <typename T, bool NT, int B, int PB, typename TV = T>
__global__ __launch_bounds__(256) void hspmv_slices(int32_t n_slices, uint32_t blk_order, int32_t y_nt,
                                                    Slices sl, XDict xd, const TV *__restrict__ val,
                                                    const T *__restrict__ x, T *__restrict__ y) {
  slices_body<T, NT, B, PB, TV>(n_slices, blk_order, y_nt, sl, xd, val, x, y, SliceStoreSum<T>{});
}

// y = alpha (A x) + beta y (hspmv_spmv_axpby's fused path): hspmv_slices with
// the epilogue between the row's sum -- the bits hspmv_slices stores -- and
// its store.  The load of the old y is predicated by lane < nr like the
// store.  (y is read and written, each row by the lane that owns it: no
// __restrict__)
template <typename T, bool NT, int B, int PB, typename TV = T>
__global__ __launch_bounds__(256) void hspmv_slices_axpby(int32_t n_slices, uint32_t blk_order, int32_t y_nt,
                                                          T alpha, T beta, Slices sl, XDict xd,
                                                          const TV *__restrict__ val, const T *__restrict__ x,
                                                          T *y) {
  slices_body<T, NT, B, PB, TV>(n_slices, blk_order, y_nt, sl, xd, val, x, y, SliceAxpby<T>{alpha, beta});
}

// hspmv_slices_axpby and, from the values it stores, the slice's pair
// {sum w[r] y[r], sum y[r]^2} in double into partials[t] (n_slices pairs;
// hspmv_spmv_axpby_dot's fused path, finished by hspmv_dot_finish).  A wave
// without rows returns before it and writes no pair.
template <typename T, bool NT, int B, int PB, typename TV = T>
__global__ __launch_bounds__(256) void hspmv_slices_axpby_dot(int32_t n_slices, uint32_t blk_order, int32_t y_nt,
                                                              T alpha, T beta, uint32_t yy, const T *w,
                                                              sl_d2 *__restrict__ partials, Slices sl, XDict xd,
                                                              const TV *__restrict__ val,
                                                              const T *__restrict__ x, T *y) {
  slices_body<T, NT, B, PB, TV>(n_slices, blk_order, y_nt, sl, xd, val, x, y,
                                SliceAxpbyDot<T>{SliceAxpby<T>{alpha, beta}, w, yy, partials});
}

}  // namespace dev
}  // namespace hspmv
