// mixed_plan_check.cpp -- host-only driver for the mixed-precision handle's
// host side (fp32 values under fp64 vectors): hspmv_values_fit_f32,
// hspmv_create_mixed's refusals (every one comes before the first device
// call) and hspmv_slices_plan_vec on two small matrices, whose fp32 value
// stream (groups of four slots) is rebuilt here from the CSR arrays and
// compared, and whose descriptors, lengths and positions must be those of the
// widened fp64 matrix.  No device is touched.  `make asan-mixed` builds it
// against the AddressSanitizer + UBSan library and runs it.
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "hspmv.h"

#define CHECK(c)                                                                        \
  do {                                                                                  \
    if (!(c)) {                                                                         \
      fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #c, hspmv_last_error()); \
      return 1;                                                                         \
    }                                                                                   \
  } while (0)

static int fit_checks() {
  int64_t bad = -1;
  const float f[3] = {1.0f, 0.1f, -3.5f};
  CHECK(hspmv_values_fit_f32(f, 3, HSPMV_F32, &bad) == 1 && bad == -1);
  // exactly nnz elements on the heap: a read past them is the sanitizer's to find
  std::vector<double> d = {1.0, (double)0.1f, -0.0, INFINITY, -INFINITY, (double)FLT_MAX, (double)FLT_MIN};
  CHECK(hspmv_values_fit_f32(d.data(), (int64_t)d.size(), HSPMV_F64, &bad) == 1 && bad == -1);
  CHECK(hspmv_values_fit_f32(d.data(), (int64_t)d.size(), HSPMV_F64, nullptr) == 1);
  const double cases[] = {0.1, 2.0 * (double)FLT_MAX, 1e-310, ldexp(1.0 + ldexp(1.0, -20), -140)};
  for (double c : cases)
    for (size_t at : {(size_t)0, d.size() / 2, d.size()}) {
      std::vector<double> v = d;
      v.insert(v.begin() + (std::ptrdiff_t)at, c);
      bad = -1;
      CHECK(hspmv_values_fit_f32(v.data(), (int64_t)v.size(), HSPMV_F64, &bad) == 0 && bad == (int64_t)at);
      CHECK(hspmv_values_fit_f32(v.data(), (int64_t)v.size(), HSPMV_F64, nullptr) == 0);
    }
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  CHECK(hspmv_values_fit_f32(&qnan, 1, HSPMV_F64, &bad) == 1);  // the default quiet NaN round-trips
  uint64_t bits;
  memcpy(&bits, &qnan, 8);
  bits |= 1;  // a payload bit fp32 cannot hold
  double pnan;
  memcpy(&pnan, &bits, 8);
  bad = -1;
  CHECK(hspmv_values_fit_f32(&pnan, 1, HSPMV_F64, &bad) == 0 && bad == 0);
  CHECK(hspmv_values_fit_f32(nullptr, 0, HSPMV_F64, &bad) == 1);
  CHECK(hspmv_values_fit_f32(nullptr, 3, HSPMV_F64, &bad) == HSPMV_E_INVALID);
  CHECK(hspmv_values_fit_f32(d.data(), -1, HSPMV_F64, &bad) == HSPMV_E_INVALID);
  CHECK(hspmv_values_fit_f32(d.data(), 1, 7, &bad) == HSPMV_E_INVALID && hspmv_last_error()[0]);
  return 0;
}

static int refusal_checks() {
  const int32_t rp[3] = {0, 1, 2};
  const int32_t ci[2] = {0, 1};
  const float v32[2] = {1.0f, 2.0f};
  const double v64[2] = {1.0, 2.0};
  hspmv_csr A32 = {2, 2, 2, rp, ci, v32, HSPMV_F32};
  hspmv_csr A64 = {2, 2, 2, rp, ci, v64, HSPMV_F64};
  hspmv_handle *h = nullptr;
  hspmv_options opt;
  memset(&opt, 0, sizeof(opt));
  opt.struct_size = sizeof(opt);
  CHECK(hspmv_create_mixed(nullptr, &A32, nullptr, &opt, HSPMV_F64) == HSPMV_E_INVALID);
  CHECK(hspmv_create_mixed(&h, nullptr, nullptr, &opt, HSPMV_F64) == HSPMV_E_INVALID && !h);
  CHECK(hspmv_create_mixed(&h, &A64, nullptr, &opt, HSPMV_F32) == HSPMV_E_INVALID && !h && hspmv_last_error()[0]);
  CHECK(hspmv_create_mixed(&h, &A32, nullptr, &opt, 7) == HSPMV_E_INVALID && !h && hspmv_last_error()[0]);
  CHECK(hspmv_create_mixed(&h, &A32, nullptr, nullptr, -1) == HSPMV_E_INVALID && !h);
  const int devs[2] = {0, 0};
  opt.n_devices = 2;
  CHECK(hspmv_create_mixed(&h, &A32, nullptr, &opt, HSPMV_F64) == HSPMV_E_INVALID && !h);
  opt.devices = devs;
  CHECK(hspmv_create_mixed(&h, &A32, nullptr, &opt, HSPMV_F64) == HSPMV_E_INVALID && !h && hspmv_last_error()[0]);
  opt.devices = nullptr;
  opt.n_devices = 0;
  opt.flags = HSPMV_KERNEL_CSORT;
  CHECK(hspmv_create_mixed(&h, &A32, nullptr, &opt, HSPMV_F64) == HSPMV_E_INVALID && !h && hspmv_last_error()[0]);
  opt.flags = 0;
  opt.csort = 1;
  CHECK(hspmv_create_mixed(&h, &A32, nullptr, &opt, HSPMV_F64) == HSPMV_E_INVALID && !h && hspmv_last_error()[0]);
  CHECK(hspmv_get_dtypes(nullptr, nullptr, nullptr) == HSPMV_E_INVALID);
  return 0;
}

// rows of the given lengths over n columns, column (7 r + 3 k) mod n ascending
static int plan_check(const std::vector<int32_t> &lens, int32_t n, unsigned kernel, int32_t want_why) {
  std::vector<int32_t> rp(lens.size() + 1, 0);
  for (size_t r = 0; r < lens.size(); ++r) rp[r + 1] = rp[r] + lens[r];
  const int64_t m = (int64_t)lens.size(), nnz = rp[lens.size()];
  std::vector<int32_t> ci((size_t)nnz);
  std::vector<float> v32((size_t)nnz);
  std::vector<double> v64((size_t)nnz);
  for (int64_t r = 0; r < m; ++r) {
    const int32_t c0 = (int32_t)((7 * r) % (n - lens[(size_t)r] + 1));
    for (int32_t k = 0; k < lens[(size_t)r]; ++k) {
      ci[(size_t)rp[r] + k] = c0 + k;
      v32[(size_t)rp[r] + k] = 1.0f + (float)((rp[r] + k) % 251) / 256.0f;
      v64[(size_t)rp[r] + k] = (double)v32[(size_t)rp[r] + k];
    }
  }
  hspmv_csr A32 = {m, n, nnz, rp.data(), ci.data(), v32.data(), HSPMV_F32};
  hspmv_csr A64 = {m, n, nnz, rp.data(), ci.data(), v64.data(), HSPMV_F64};
  hspmv_options opt;
  memset(&opt, 0, sizeof(opt));
  opt.struct_size = sizeof(opt);
  opt.flags = kernel;
  opt.x_dict = 1;
  opt.row_slices = 1;
  int64_t nd = 0, ns = 0, pe = 0, nd64 = 0, ns64 = 0, pe64 = 0;
  int32_t why = -1, why64 = -1;
  CHECK(hspmv_slices_plan_vec(&A32, nullptr, &opt, HSPMV_F64, &nd, &ns, &pe, &why, nullptr, nullptr, nullptr,
                              nullptr) == HSPMV_OK);
  CHECK(hspmv_slices_plan(&A64, nullptr, &opt, &nd64, &ns64, &pe64, &why64, nullptr, nullptr, nullptr, nullptr) ==
        HSPMV_OK);
  CHECK(why == want_why && why64 == want_why && nd == nd64 && ns == ns64 && pe == pe64);
  int64_t r0 = 0, r1 = 0, r2 = 0;
  int32_t rw = -1;
  CHECK(hspmv_slices_plan_vec(&A64, nullptr, &opt, HSPMV_F32, &r0, &r1, &r2, &rw, nullptr, nullptr, nullptr,
                              nullptr) == HSPMV_E_INVALID);
  if (want_why != HSPMV_SLICES_OK) return 0;
  // exactly-sized outputs
  std::vector<int32_t> desc(2 * (size_t)(nd + 1)), desc64(desc.size());
  std::vector<uint8_t> len((size_t)m), len64((size_t)m);
  std::vector<uint16_t> pos((size_t)pe), pos64((size_t)pe);
  std::vector<float> val((size_t)pe, -1.0f);
  std::vector<double> val64((size_t)pe);
  CHECK(hspmv_slices_plan_vec(&A32, nullptr, &opt, HSPMV_F64, &nd, &ns, &pe, &why, desc.data(), len.data(),
                              pos.data(), val.data()) == HSPMV_OK);
  CHECK(hspmv_slices_plan(&A64, nullptr, &opt, &nd64, &ns64, &pe64, &why64, desc64.data(), len64.data(),
                          pos64.data(), val64.data()) == HSPMV_OK);
  CHECK(desc == desc64 && len == len64 && pos == pos64);
  std::vector<float> want((size_t)pe, 0.0f);
  const int G = 4;  // fp32 slots per 16-byte value group
  for (int64_t s = 0; s < nd; ++s) {
    const int32_t a = desc[2 * s + 1], b = desc[2 * s + 3], w = desc[2 * s + 2] - desc[2 * s];
    const size_t base = 64 * (size_t)desc[2 * s];
    const int32_t wg = w / G * G;
    for (int32_t r = a; r < b; ++r)
      for (int32_t k = 0; k < lens[(size_t)r]; ++k) {
        const size_t at = k < wg ? base + (size_t)(k / G) * 64 * G + (size_t)(r - a) * G + (size_t)(k % G)
                                 : base + (size_t)k * 64 + (size_t)(r - a);
        want[at] = v32[(size_t)rp[(size_t)r] + (size_t)k];
      }
  }
  CHECK(memcmp(want.data(), val.data(), 4 * (size_t)pe) == 0);
  // equal dtypes: hspmv_slices_plan itself
  int64_t a0 = 0, a1 = 0, a2 = 0, b0 = 0, b1 = 0, b2 = 0;
  int32_t wa = -1, wb = -1;
  CHECK(hspmv_slices_plan_vec(&A32, nullptr, &opt, HSPMV_F32, &a0, &a1, &a2, &wa, nullptr, nullptr, nullptr,
                              nullptr) == HSPMV_OK);
  CHECK(hspmv_slices_plan(&A32, nullptr, &opt, &b0, &b1, &b2, &wb, nullptr, nullptr, nullptr, nullptr) == HSPMV_OK);
  CHECK(a0 == b0 && a1 == b1 && a2 == b2 && wa == wb);
  return 0;
}

int main() {
  if (fit_checks()) return 1;
  if (refusal_checks()) return 1;
  // every remainder of the 4-slot value groups, an empty row, a last slice of 5 rows
  std::vector<int32_t> ragged;
  for (int r = 0; r < 197; ++r) ragged.push_back(r % 11 == 3 ? 0 : 1 + (r * 5) % 40);
  for (unsigned kernel : {HSPMV_KERNEL_STREAM, HSPMV_KERNEL_AUTO}) {
    if (plan_check(ragged, 300, kernel, HSPMV_SLICES_OK)) return 1;
    if (plan_check(std::vector<int32_t>(130, 7), 64, kernel, HSPMV_SLICES_OK)) return 1;
  }
  // a row of 41: fp64's serial bound refuses it, though fp32 alone allows 56
  std::vector<int32_t> r41(70, 5);
  r41[33] = 41;
  if (plan_check(r41, 100, HSPMV_KERNEL_STREAM, HSPMV_SLICES_LONG_ROW)) return 1;
  printf("mixed_plan_check: ok\n");
  return 0;
}
