// dev_prims.cuh -- wave64 device primitives shared by every kernel unit
// (spmv_kernels.hip, the row and slice kernels, csort.hip, spmm.hip): loads,
// wave-scope synchronisation, DPP and shuffle reductions.  Device code only,
// no kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hspmv {
namespace dev {

constexpr int kWave = 64;

template <bool NT, typename T>
__device__ __forceinline__ T ldg(const T *p) {
  if constexpr (NT)
    return __builtin_nontemporal_load(p);
  else
    return *p;
}

// Loads through a wave-uniform GLOBAL (address_space 1) base pointer plus a
// 32-bit byte offset, so hipcc emits global_load ... v_off, s[base:base+1]
// (one offset VGPR per load, no 64-bit address pairs, and no flat_load,
// which would force vmcnt(0) + lgkmcnt(0) waits).
typedef __attribute__((address_space(1))) const char gchar;

template <bool NT, typename T>
__device__ __forceinline__ T ld_off(const gchar *base, uint32_t byte_off) {
  const __attribute__((address_space(1))) T *p =
      (const __attribute__((address_space(1))) T *)(base + byte_off);
  if constexpr (NT)
    return __builtin_nontemporal_load(p);
  else
    return *p;
}

template <typename T>
__device__ __forceinline__ const gchar *uniform_ptr(const T *p) {
  const uint64_t v = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (const gchar *)(((uint64_t)hi << 32) | lo);
}

// Scalar (s_load) read of an R (4, 8 or 16 bytes) at p + byte_off; p and
// byte_off must be wave-uniform.  ALIGN: what the address is known to be
// aligned to (a template argument does not carry a typedef's alignment).
template <typename R, int ALIGN = alignof(R)>
__device__ __forceinline__ R sload(const void *p, uint64_t byte_off) {
  const uint64_t v = reinterpret_cast<uint64_t>(p) + byte_off;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  typedef __attribute__((address_space(4), aligned(ALIGN))) const R cr;
  return *(cr *)(((uint64_t)hi << 32) | lo);
}

// Orders a wave's LDS writes before its other lanes' LDS reads (the
// wave-scope equivalent of a barrier; no s_barrier involved).
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Wave sum by xor shuffles (ds_bpermute): every lane holds the total.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// One DPP move of v (both dwords for 8-byte types); lanes the pattern does
// not feed read 0.
template <int CTRL, int ROW_MASK, typename T>
__device__ __forceinline__ T dpp_move(T v) {
  if constexpr (sizeof(T) == 8) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(b >> 32), CTRL, ROW_MASK, 0xf, false);
    return __builtin_bit_cast(T, ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
  } else {
    return __builtin_bit_cast(
        T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false));
  }
}

// Lane l's value of v, wave-uniform (v_readlane; l wave-uniform).
template <typename T>
__device__ __forceinline__ T lane_value(T v, int l) {
  if constexpr (sizeof(T) == 8) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)b, l);
    const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), l);
    return __builtin_bit_cast(T, ((uint64_t)hi << 32) | lo);
  } else {
    return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
  }
}

// Sums of the four 16-lane DPP rows: lane 16 q + 15 holds row q's total.
template <typename T>
__device__ __forceinline__ T row16_sum_dpp(T v) {
  v += dpp_move<0x111, 0xf>(v);
  v += dpp_move<0x112, 0xf>(v);
  v += dpp_move<0x114, 0xf>(v);
  v += dpp_move<0x118, 0xf>(v);
  return v;
}

// Wave sum by DPP (row_shr 1/2/4/8 inside each 16-lane row, then
// row_bcast 15/31 across rows: an inclusive scan whose lane 63 holds the
// total), returned wave-uniform.  No LDS round trips, unlike __shfl_xor
// (ds_bpermute): the cooperative rows' reductions are on the critical path
// of each chunk (mid-density rows, profiles/r02z*).
template <typename T>
__device__ __forceinline__ T wave_sum_dpp(T v) {
  v = row16_sum_dpp(v);
  v += dpp_move<0x142, 0xa>(v);
  v += dpp_move<0x143, 0xc>(v);
  return lane_value(v, 63);
}

// Lanes i .. 63 as a mask (0 for i >= 64).
__device__ __forceinline__ unsigned long long bits_from(int i) {
  return i >= 64 ? 0ull : (~0ull << i);
}

}  // namespace dev
}  // namespace hspmv
