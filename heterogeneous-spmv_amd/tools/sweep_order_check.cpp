// sweep_order_check.cpp -- host-only driver for the row kernels' block order
// (hspmv_block_order: xcd_chunk_remap, then the sweep mirror) and the argument
// checks of hspmv_set_sweep: for every block count and XCD chunk the forward
// and the mirrored order are bijections on [0, nb) and mirror each other.
// No device is touched.  `make asan-sweep` builds it against the
// AddressSanitizer + UBSan library and runs it.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "hspmv.h"

#define CHECK(c)                                                                        \
  do {                                                                                  \
    if (!(c)) {                                                                         \
      fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #c, hspmv_last_error()); \
      return 1;                                                                         \
    }                                                                                   \
  } while (0)

static int check(int64_t nb, int32_t chunk) {
  // exactly nb entries: a write past the order's end is the sanitizer's to find
  std::vector<int32_t> fwd((size_t)nb), rev((size_t)nb);
  std::vector<char> seen((size_t)nb, 0);
  CHECK(hspmv_block_order(nb, chunk, 0, fwd.data()) == HSPMV_OK);
  CHECK(hspmv_block_order(nb, chunk, 1, rev.data()) == HSPMV_OK);
  for (int64_t b = 0; b < nb; ++b) {
    CHECK(fwd[(size_t)b] >= 0 && fwd[(size_t)b] < nb && !seen[(size_t)fwd[(size_t)b]]);
    seen[(size_t)fwd[(size_t)b]] = 1;
    CHECK(rev[(size_t)b] == nb - 1 - fwd[(size_t)b]);
  }
  return 0;
}

int main() {
  int64_t cases = 0;
  std::vector<int64_t> nbs;
  for (int64_t nb = 1; nb <= 300; ++nb) nbs.push_back(nb);
  for (int64_t nb : {3907, 7633, 40001, 1 << 20, (1 << 20) + 37}) nbs.push_back(nb);
  for (int64_t nb : nbs)
    for (int64_t chunk : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)4, (int64_t)8, (int64_t)64, nb / 8,
                          (int64_t)1 << 30}) {
      if (check(nb, (int32_t)chunk)) return 1;
      ++cases;
    }
  int32_t one = -1;
  CHECK(hspmv_block_order(0, 1, 0, nullptr) == HSPMV_OK);
  CHECK(hspmv_block_order(1, 1, 1, &one) == HSPMV_OK && one == 0);
  CHECK(hspmv_block_order(-1, 1, 0, &one) == HSPMV_E_INVALID);
  CHECK(hspmv_block_order(4, 1, 0, nullptr) == HSPMV_E_INVALID);
  CHECK(hspmv_block_order(4, -1, 0, &one) == HSPMV_E_INVALID);
  CHECK(hspmv_block_order((int64_t)1 << 31, 1, 0, &one) == HSPMV_E_INVALID);
  for (int mode : {HSPMV_SWEEP_AUTO, HSPMV_SWEEP_FORWARD, HSPMV_SWEEP_ALTERNATE, 3, -1})
    CHECK(hspmv_set_sweep(nullptr, mode) == HSPMV_E_INVALID);
  printf("sweep_order_check: %lld block orders ok\n", (long long)cases);
  return 0;
}
