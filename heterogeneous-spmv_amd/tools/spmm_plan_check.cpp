// spmm_plan_check.cpp -- host-only driver for the multi-vector operator's
// long-row table (mm_long_rows, csrc/hspmv_mm.cpp: the ids of the rows the
// wave-per-row kernel runs) and the launch shape helpers, checked against a
// direct count on a few row-length arrays -- the empty matrix, no long rows,
// all rows long, the serial bounds themselves -- and for hspmv_mm_create's
// refusals.  No device is touched.  `make asan-spmm` builds it against the
// AddressSanitizer + UBSan library and runs it.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hspmv.h"
#include "hspmv_internal.h"

#define CHECK(c)                                                                        \
  do {                                                                                  \
    if (!(c)) {                                                                         \
      fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #c, hspmv_last_error()); \
      return 1;                                                                         \
    }                                                                                   \
  } while (0)

static int check(const std::vector<int32_t> &lens, int32_t serial_max) {
  // exactly m + 1 row pointers: a read past them is the sanitizer's to find
  std::vector<int32_t> rp(lens.size() + 1, 0);
  for (size_t r = 0; r < lens.size(); ++r) rp[r + 1] = rp[r] + lens[r];
  std::vector<int32_t> rows(3, -7);  // stale content must go
  hspmv::mm_long_rows(rp.data(), (int64_t)lens.size(), serial_max, rows);
  size_t want = 0;
  for (int32_t l : lens) want += l > serial_max;
  CHECK(rows.size() == want);
  size_t j = 0;
  for (size_t r = 0; r < lens.size(); ++r)
    if (lens[r] > serial_max) {
      CHECK(j < rows.size() && rows[j] == (int32_t)r);
      ++j;
    }
  return 0;
}

int main() {
  const std::vector<std::vector<int32_t>> cases = {
      {},                                             // the empty matrix
      {0},
      {0, 0, 0},
      {1, 39, 40, 41, 56, 57, 63, 64, 65, 300, 4096, 4500, 0},
      {41, 41, 41, 41},                               // all long (fp64)
      {4500, 57, 100000},                             // all long (both)
      {40, 40, 40},                                   // none long
      std::vector<int32_t>(1000, 27),
  };
  int n = 0;
  for (const auto &lens : cases)
    for (int32_t sm : {hspmv::mm_serial_max(HSPMV_F64), hspmv::mm_serial_max(HSPMV_F32), 0, INT32_MAX}) {
      if (check(lens, sm)) return 1;
      ++n;
    }
  CHECK(hspmv::mm_serial_max(HSPMV_F64) == 40 && hspmv::mm_serial_max(HSPMV_F32) == 56);
  for (int32_t k = 1; k <= hspmv::kMmMaxRhs; ++k) {
    const int32_t kp = hspmv::mm_lanes_per_row(k);
    CHECK(kp >= k && kp < 2 * k && (kp & (kp - 1)) == 0 && 64 % kp == 0);
    for (int64_t m : {(int64_t)0, (int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)INT32_MAX - 1}) {
      const int64_t rows = 4 * (64 / kp), b = hspmv::mm_blocks(m, kp);
      CHECK(b * rows >= m && (b == 0 || (b - 1) * rows < m));
    }
  }
  // hspmv_mm_create's refusals come before any device
  const int32_t rp1[2] = {0, 0};
  hspmv_csr A = {1, 1, 0, rp1, nullptr, nullptr, HSPMV_F64};
  hspmv_mm *mm = nullptr;
  hspmv_options opt;
  memset(&opt, 0, sizeof(opt));
  opt.struct_size = sizeof(opt);
  CHECK(hspmv_mm_create(nullptr, &A, 4, &opt) == HSPMV_E_INVALID);
  CHECK(hspmv_mm_create(&mm, nullptr, 4, &opt) == HSPMV_E_INVALID && !mm);
  CHECK(hspmv_mm_create(&mm, &A, 0, &opt) == HSPMV_E_INVALID && !mm);
  CHECK(hspmv_mm_create(&mm, &A, 33, &opt) == HSPMV_E_INVALID && !mm);
  opt.flags = HSPMV_KERNEL_STREAM;
  CHECK(hspmv_mm_create(&mm, &A, 4, &opt) == HSPMV_E_INVALID && !mm);
  opt.flags = 0;
  opt.n_devices = 2;
  CHECK(hspmv_mm_create(&mm, &A, 4, &opt) == HSPMV_E_INVALID && !mm);
  opt.struct_size = 4;
  CHECK(hspmv_mm_create(&mm, &A, 4, &opt) == HSPMV_E_INVALID && !mm);
  CHECK(hspmv_mm_spmm(nullptr) == HSPMV_E_INVALID);
  hspmv_mm_destroy(nullptr);
  printf("spmm_plan_check: %d long-row tables ok\n", n);
  return 0;
}
