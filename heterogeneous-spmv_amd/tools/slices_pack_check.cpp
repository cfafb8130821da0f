// slices_pack_check.cpp -- host-only driver for the row-slice planner and the
// position packer (hspmv_slices_plan -> build_slices, hspmv_slices_pack):
// plans random ragged matrices and fixed-run matrices through the C ABI,
// packs the positions and unpacks them again by the layout hspmv.h documents.
// No device is touched.  `make asan-slices` builds it against the
// AddressSanitizer + UBSan library and runs it.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "hspmv.h"

static size_t slot16(int32_t w, int32_t k, int i) {
  return k < w / 4 * 4 ? (size_t)(k / 4) * 256 + (size_t)i * 4 + (size_t)(k % 4) : (size_t)k * 64 + (size_t)i;
}

#define CHECK(c)                                                                        \
  do {                                                                                  \
    if (!(c)) {                                                                         \
      fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #c, hspmv_last_error()); \
      return 1;                                                                         \
    }                                                                                   \
  } while (0)

// Plans A (STREAM, dictionaries and row slices on), packs, unpacks, compares.
static int check(const std::vector<int32_t> &rp, const std::vector<int32_t> &col, int64_t n, int dtype,
                 int32_t cap, int want_bits) {
  const int64_t m = (int64_t)rp.size() - 1, nnz = rp[(size_t)m];
  std::vector<double> v64((size_t)nnz + 1, 0.5);
  std::vector<float> v32((size_t)nnz + 1, 0.5f);
  hspmv_csr A{m, n, nnz, rp.data(), col.data(),
              dtype == HSPMV_F64 ? (const void *)v64.data() : (const void *)v32.data(), dtype};
  hspmv_options o;
  memset(&o, 0, sizeof o);
  o.struct_size = sizeof o;
  o.flags = HSPMV_KERNEL_STREAM;
  o.x_dict = 1;
  o.x_dict_cap = cap;
  o.row_slices = 1;
  int64_t nd = 0, ns = 0, pe = 0;
  int32_t why = -1;
  CHECK(hspmv_slices_plan(&A, nullptr, &o, &nd, &ns, &pe, &why, nullptr, nullptr, nullptr, nullptr) == HSPMV_OK);
  CHECK(why == HSPMV_SLICES_OK);
  std::vector<int32_t> desc(2 * (size_t)(nd + 1));
  std::vector<uint8_t> len((size_t)m + 1);
  std::vector<uint16_t> pos((size_t)pe + 1);
  std::vector<char> val((size_t)(pe + 1) * 8);
  CHECK(hspmv_slices_plan(&A, nullptr, &o, &nd, &ns, &pe, &why, desc.data(), len.data(), pos.data(),
                          val.data()) == HSPMV_OK);
  CHECK(64 * (int64_t)desc[2 * (size_t)nd] == pe);
  int32_t bits = 0;
  int64_t bytes = 0;
  CHECK(hspmv_slices_pack(nd, desc.data(), pos.data(), &bits, &bytes, nullptr, nullptr) == HSPMV_OK);
  CHECK(bits == want_bits);
  std::vector<int32_t> prefix((size_t)nd + 1);
  std::vector<unsigned char> packed((size_t)bytes);  // exactly the stream: a write past it is reported
  CHECK(hspmv_slices_pack(nd, desc.data(), pos.data(), &bits, &bytes, prefix.data(), packed.data()) == HSPMV_OK);
  CHECK(bytes == 128 * (int64_t)prefix[(size_t)nd]);
  if (bits == 16) {
    CHECK(bytes == 2 * pe && memcmp(packed.data(), pos.data(), (size_t)bytes) == 0);
    return 0;
  }
  for (int64_t s = 0; s < nd; ++s) {
    const int32_t w = desc[2 * s + 2] - desc[2 * s], w8 = w / 8 * 8;
    CHECK(prefix[(size_t)s + 1] - prefix[(size_t)s] == 6 * (w / 8) + w % 8);
    const unsigned char *src = packed.data() + 128 * (size_t)prefix[(size_t)s];
    const uint16_t *want = pos.data() + 64 * (size_t)desc[2 * s];
    for (int32_t k = 0; k < w; ++k)
      for (int i = 0; i < 64; ++i) {
        uint32_t got;
        if (k < w8) {
          uint32_t d[3];
          memcpy(d, src + 768 * (size_t)(k / 8) + 12 * (size_t)i, 12);
          const int bit = 12 * (k % 8), word = bit / 32, sh = bit % 32;
          got = d[word] >> sh;
          if (sh > 20) got |= d[word + 1] << (32 - sh);
          got &= 0xfffu;
        } else {
          uint16_t t;
          memcpy(&t, src + 96 * (size_t)w8 + 2 * slot16(w - w8, k - w8, i), 2);
          got = t;
        }
        CHECK(got == want[slot16(w, k, i)]);
      }
  }
  return 0;
}

int main() {
  std::mt19937 rng(12345);
  int runs = 0;
  for (int dtype : {HSPMV_F64, HSPMV_F32}) {
    const int bound = dtype == HSPMV_F64 ? 40 : 56;
    // ragged: 64-row groups of every longest row 0 .. bound, empty rows, a short last group
    for (int rep = 0; rep < 4; ++rep) {
      std::vector<int32_t> rp{0}, col;
      const int groups = bound + 2 + rep;
      const int64_t m = 64 * (int64_t)groups - 17 * rep;
      const int stride = 1 + rep;
      for (int64_t r = 0; r < m; ++r) {
        const int w = (int)((r / 64 * 7 + rep) % (bound + 1));
        int k = (int)(rng() % (unsigned)(w + 1));
        if (r % 64 == 3) k = w;
        for (int j = 0; j < k; ++j) col.push_back((int32_t)(r * stride + (int64_t)j * (stride + 1)));
        rp.push_back((int32_t)col.size());
      }
      const int64_t n = m * stride + (int64_t)bound * (stride + 1) + 1;
      if (check(rp, col, n, dtype, 0, 12)) return 1;
      ++runs;
    }
    // one run of 256 c entries per 256-row block: largest position 256 c - 1
    for (int c : {16, 17, 20}) {
      if (dtype == HSPMV_F64 && c > 17) continue;  // over the 40960-byte cap below
      std::vector<int32_t> rp{0}, col;
      for (int r = 0; r < 512; ++r) {
        for (int j = 0; j < c; ++j) col.push_back(c * r + j);
        rp.push_back((int32_t)col.size());
      }
      if (check(rp, col, 512 * c, dtype, dtype == HSPMV_F64 ? 40960 : 0, c == 16 ? 12 : 16)) return 1;
      ++runs;
    }
  }
  printf("slices_pack_check: %d plans packed and unpacked\n", runs);
  return 0;
}
