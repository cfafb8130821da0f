// Host-side helpers shared by the host runtime units (hspmv_runtime.h) and
// the I/O units (hspmv_io.cpp, hspmv_mtx.cpp, hspmv_bandk.cpp).
#pragma once
#include <stdarg.h>
#include <stdint.h>

#include <string>

#include "hspmv.h"

namespace hspmv {

// Sets the thread-local message returned by hspmv_last_error(); returns code.
int set_error(int code, const char *fmt, ...);
void clear_error();

// Structural validation of a host CSR (row_ptr monotone from 0 to nnz,
// columns in [0, n)).  Returns HSPMV_OK or HSPMV_E_INVALID with a message.
int validate_host_csr(const hspmv_csr *A, bool check_cols);
int validate_host_maps(const hspmv_csr3_maps *maps, int64_t m);

inline size_t dtype_size(int dtype) { return dtype == HSPMV_F64 ? 8 : 4; }

// hspmv_alg_bytes for values stored in val_dtype under vectors of dtype (the
// mixed handles: 4 instead of 8 bytes per stored value).
inline double alg_bytes_of(int64_t m, int64_t x_entries, int64_t nnz, int dtype, int val_dtype, int64_t n_ssr,
                           int64_t n_sr) {
  return hspmv_alg_bytes(m, x_entries, nnz, dtype, n_ssr, n_sr) -
         (double)nnz * ((double)dtype_size(dtype) - (double)dtype_size(val_dtype));
}

}  // namespace hspmv
