// stream_f32v64.hip -- instantiates the STREAM / CSR3 / row-slice kernels for
// the mixed handles: values stored and streamed as float, x, y, the products
// and the sums double (hspmv_create_mixed).  A unit of its own, like
// stream_f32.hip / stream_f64.hip, so hipcc compiles the three in parallel.
#include "row_launch.cuh"

namespace hspmv {
hipError_t launch_rows_f32v64(const DevCSR &A, const DevPlan &dp, const LaunchPlan &p, const double *x,
                              double *y, hipStream_t st) {
  return dev::launch_rows<double, float>(A, dp, p, x, y, st);
}
hipError_t launch_slices_axpby_f32v64(const DevPlan &dp, const LaunchPlan &p, const AxpbyScalars &ab,
                                      const double *x, double *y, hipStream_t st) {
  return dev::launch_slices<double, float>(dp, p, x, y, st, &ab);
}
hipError_t launch_slices_axpby_dot_f32v64(const DevPlan &dp, const LaunchPlan &p, const AxpbyScalars &ab,
                                          const DotArgs &dot, const double *x, double *y, hipStream_t st) {
  return dev::launch_slices<double, float>(dp, p, x, y, st, &ab, &dot);
}
}  // namespace hspmv
