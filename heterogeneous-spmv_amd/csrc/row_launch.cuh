// row_launch.cuh -- host-side launch dispatch of the row and slice kernels:
// launch_rows<T, TV> picks the instantiation a plan names.  Included by the
// instantiation units stream_f32.hip / stream_f64.hip / stream_f32v64.hip
// (one per dtype, so hipcc compiles them in parallel); host code only.
//
// The variants of one unit, per NT in {0, 1} and U in {2, 3, 4, 5, 6, 8, 16}
// (90 kernels, 36 of them with prefetch), plus the 4 slice kernels (and their
// 4 hspmv_slices_axpby and 4 hspmv_slices_axpby_dot twins, launch_slices):
//   column format   STREAM                               CSR3
//   32-bit, col16   W in {1, 2, 4} x windows on / off    W in {1, 2, 4, 8}, and
//   modes 1 and 2   x padded on / off (no padding with   W = 4 with x windows
//                   prefetch): 12, with prefetch 6       5
//   dictionary      W = 4                      1         W in {4, 8}          2
// The rules that leave the other combinations out are the `if constexpr` and
// static_flag<OFFERED> conditions below, each with its reason.
#pragma once
#include "row_kernels.cuh"
#include "slice_kernel.cuh"
#include "static_switch.h"

namespace hspmv {
namespace dev {

// The kernels' block-order argument: the XCD chunk, and the sweep direction
// of this launch in the top bit (sweep_block).
inline uint32_t block_order(const LaunchPlan &p) {
  return (uint32_t)p.xcd_chunk | (p.reverse ? kSweepReverse : 0u);
}

// ab: nullptr runs hspmv_slices (y = A x); else hspmv_slices_axpby with the
// two scalars converted to T here, once (y = alpha (A x) + beta y); with dot
// as well, hspmv_slices_axpby_dot (dot->partials: dp.sl.n pairs).
template <typename T, typename TV>
hipError_t launch_slices(const DevPlan &dp, const LaunchPlan &p, const T *x, T *y, hipStream_t st,
                         const AxpbyScalars *ab = nullptr, const DotArgs *dot = nullptr) {
  if (!dp.xd.blk || !dp.sl.len || !dp.sl.pos || !dp.sl.val || p.waves_per_block != 4 ||
      p.blocks != ((int64_t)dp.sl.n + 3) / 4 ||
      !(dp.sl.pos_bits == 16 || (dp.sl.pos_bits == 12 && dp.sl.ppre)))
    return hipErrorInvalidValue;  // the host built the slices for another block shape
  if (dot && (!ab || !dot->partials || reinterpret_cast<uintptr_t>(dot->partials) % 16 != 0))
    return hipErrorInvalidValue;
  const Slices sl{dp.sl.desc, dp.sl.len, dp.sl.pos, dp.sl.ppre};
  const XDict xd{dp.xd.blk, reinterpret_cast<const int2 *>(dp.xd.runs)};
  const unsigned dyn = (unsigned)dp.xd.lds_bytes + (unsigned)p.dyn_lds;
  const TV *val = static_cast<const TV *>(dp.sl.val);
  static_switch<12, 16>(dp.sl.pos_bits, [&](auto PB) {
    static_flag(p.nontemporal, [&](auto NT) {
      if (dot)
        hipLaunchKernelGGL((hspmv_slices_axpby_dot<T, NT, HSPMV_SLICE_BATCH, PB, TV>), dim3((unsigned)p.blocks),
                           dim3(256), dyn, st, dp.sl.n, block_order(p), (int32_t)p.y_nt, (T)ab->alpha, (T)ab->beta,
                           (uint32_t)dot->yy, static_cast<const T *>(dot->w),
                           reinterpret_cast<sl_d2 *>(dot->partials), sl, xd, val, x, y);
      else if (ab)
        hipLaunchKernelGGL((hspmv_slices_axpby<T, NT, HSPMV_SLICE_BATCH, PB, TV>), dim3((unsigned)p.blocks),
                           dim3(256), dyn, st, dp.sl.n, block_order(p), (int32_t)p.y_nt, (T)ab->alpha, (T)ab->beta,
                           sl, xd, val, x, y);
      else
        hipLaunchKernelGGL((hspmv_slices<T, NT, HSPMV_SLICE_BATCH, PB, TV>), dim3((unsigned)p.blocks), dim3(256),
                           dyn, st, dp.sl.n, block_order(p), (int32_t)p.y_nt, sl, xd, val, x, y);
    });
  });
  return hipGetLastError();
}

inline ColSrc col_src(const DevCSR &A) {
  return ColSrc{A.col_idx, A.col16, A.cbase, A.cplanes, A.n_cplanes, A.cplane_words};
}

// The launch of one (NT, U, PF, column format) choice: the workgroup shape
// W, the x windows (XW) and the padding (PAD) from the plan.
template <typename T, typename TV, bool NT, int U, bool PF, int C16, bool XD>
void launch_rows_shape(const DevCSR &A, const DevPlan &dp, const LaunchPlan &p, const T *x, T *y,
                       hipStream_t st) {
  const TV *val = static_cast<const TV *>(A.val);
  const ColSrc cs = col_src(A);
  const XDict xd{dp.xd.blk, reinterpret_cast<const int2 *>(dp.xd.runs)};
  const int2 *xw = reinterpret_cast<const int2 *>(dp.xwin);
  // dynamic LDS: the block's x dictionary (XD), or occupancy experiments (HSPMV_DYNLDS)
  const unsigned dyn = XD ? (unsigned)dp.xd.lds_bytes + (unsigned)p.dyn_lds : (unsigned)p.dyn_lds;
  const dim3 grid((unsigned)p.blocks);
  const int wpb = p.waves_per_block;
  if (p.kernel == kStream) {
    // 1, 4, or 2 waves for any other count; dictionaries are planned for 256-row blocks
    static_switch<1, 2, 4>(XD ? 4 : (wpb == 1 || wpb == 4 ? wpb : 2), [&](auto W) {
      if constexpr (!XD || W == 4) {
        // a dictionary replaces the x windows, and is sized for unpadded
        // buffers (plan_launch); padded buffers (LaunchPlan.lds_pad:
        // conflicting row lengths) have no prefetch variant: the planner
        // never pairs them
        static_flag<!XD>(xw != nullptr, [&](auto XW) {
          static_flag<!XD && !PF>(p.lds_pad, [&](auto PAD) {
            hipLaunchKernelGGL((hspmv_csr_stream<T, NT, U, PF, C16, XW, XD, W, PAD, TV>), grid, dim3(W * 64), dyn,
                               st, A.m, dp.split.long_t, dp.serial_max, block_order(p), (int32_t)p.groups,
                               (int32_t)p.y_nt, p.carry, A.row_ptr, cs, xw, xd, val, x, y);
          });
        });
      }
    });
    return;
  }
  // CSR3: 1, 2, 4, or 8 waves for any other count
  static_switch<1, 2, 4, 8>(wpb == 1 || wpb == 2 || wpb == 4 ? wpb : 8, [&](auto W) {
    // dictionaries: packed tasks only, 4 or 8 per block (launch_rows refuses the rest)
    if constexpr (!XD || W >= 4) {
      // x windows: packed tasks only (4 per block), and none under a dictionary
      static_flag<!XD && W == 4>(xw != nullptr, [&](auto XW) {
        hipLaunchKernelGGL((hspmv_csr3<T, NT, U, PF, C16, W, XW, XD, TV>), grid, dim3(W * 64), dyn, st, dp.tasks.n,
                           dp.split.long_t, dp.serial_max, block_order(p), (int32_t)p.y_nt, p.carry, dp.tasks.align,
                           dp.tasks.start, xw, xd, A.row_ptr, cs, val, x, y);
      });
    }
  });
}

// Column formats of the row kernels.  A dictionary (XD) replaces both the
// 32-bit columns and the col16 offsets: its col stream is the 16-bit xs
// positions, so it has no col16 variants.
enum { kCol32 = 0, kCol16Block = 1, kCol16Group = 2, kColDict = 3 };

// TV: the stored type of A.val / dp.sl.val (the mixed handles: float under
// T = double).
template <typename T, typename TV = T>
hipError_t launch_rows(const DevCSR &A, const DevPlan &dp, const LaunchPlan &p, const T *x, T *y,
                       hipStream_t st) {
  if (dp.sl.desc) return launch_slices<T, TV>(dp, p, x, y, st);  // row slices of a dictionary handle
  int fmt = A.col16 ? kCol16Block : kCol32;
  if (dp.xd.blk) {
    if (!A.col16 || (p.kernel == kStream && p.groups != 1) ||
        (p.kernel == kCsr3 && (!dp.tasks.start || (p.waves_per_block != 4 && p.waves_per_block != 8))))
      return hipErrorInvalidValue;  // the host built the dictionary for another block shape
    fmt = kColDict;
  } else if (A.col16 && A.c16_mode == 2) {
    if (p.kernel == kCsr3 && !dp.tasks.start)
      return hipErrorInvalidValue;  // built for the host-planned wave tasks (one base per task)
    fmt = kCol16Group;
  }
  bool known_u = false;
  static_switch<kCol32, kCol16Block, kCol16Group, kColDict>(fmt, [&](auto F) {
    constexpr bool XD = F == kColDict;
    constexpr int C16 = XD ? 0 : (int)F;
    static_flag(p.nontemporal, [&](auto NT) {
      static_flag(p.prefetch, [&](auto PF) {
        known_u = static_switch<2, 3, 4, 5, 6, 8, 16>(
            p.u, [&](auto U) { launch_rows_shape<T, TV, NT, U, PF, C16, XD>(A, dp, p, x, y, st); });
      });
    });
  });
  return known_u ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace dev
}  // namespace hspmv
