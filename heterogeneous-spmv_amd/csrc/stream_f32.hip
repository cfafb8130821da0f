// stream_f32.hip -- instantiates the STREAM / CSR3 row kernels for float
// (split from spmv_kernels.hip so hipcc compiles the dtypes in parallel).
#include "row_launch.cuh"

namespace hspmv {
hipError_t launch_rows_f32(const DevCSR &A, const DevPlan &dp, const LaunchPlan &p, const float *x,
                          float *y, hipStream_t st) {
  return dev::launch_rows<float>(A, dp, p, x, y, st);
}
hipError_t launch_slices_axpby_f32(const DevPlan &dp, const LaunchPlan &p, const AxpbyScalars &ab,
                                   const float *x, float *y, hipStream_t st) {
  return dev::launch_slices<float, float>(dp, p, x, y, st, &ab);
}
hipError_t launch_slices_axpby_dot_f32(const DevPlan &dp, const LaunchPlan &p, const AxpbyScalars &ab,
                                       const DotArgs &dot, const float *x, float *y, hipStream_t st) {
  return dev::launch_slices<float, float>(dp, p, x, y, st, &ab, &dot);
}
}  // namespace hspmv
