// csort_update_check.cpp -- host-only driver for the value refresh of the
// column-sorted tables (hspmv_update_values on a handle from
// hspmv_create_updatable; csrc/refresh.hip, plan_csort's source-index table).
// Every case plans a matrix with values v0 and the source table
// (Tuning.csort_src), applies a short host restatement of the two refresh
// kernels -- the row scales from the new values, then every stream position's
// value from val[src[p]], scaled in fp64 and narrowed once -- to independent
// values v1, and asserts that the result is plan_csort(v1) byte for byte in
// the entry stream's values (rec / val64), rexp and sexp, that idx, cbase,
// every blk_* table and src do not depend on the values, that every nonzero's
// index appears exactly once in src, and that a plan without the request is
// the same tables with no src.  v1 always holds a row that becomes all zero,
// a row that was all zero, rows rescaled by 2^+-40 and a row whose values
// span more than 2^100 (fp32: its small values leave the normal range under
// the fixed-point scale, so the single rounding is exercised).  Each case
// also asserts that the branch it is there for was reached.  No device is
// touched.  `make asan-csort-update` builds it against the AddressSanitizer +
// UBSan library and runs it; `make tools` builds build/csort_update_check
// (tests/test_csort_update_plan.py).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "hspmv_runtime.h"

using namespace hspmv;

#define CHECK(c)                                                                  \
  do {                                                                            \
    if (!(c)) {                                                                   \
      fprintf(stderr, "%s:%d: [%s] %s failed\n", __FILE__, __LINE__, g_case, #c); \
      return 1;                                                                   \
    }                                                                             \
  } while (0)

static const char *g_case = "";

// ---- the matrix generators of csort_plan_check.cpp
struct Mat {
  int64_t m = 0, n = 0;
  std::vector<int32_t> rp{0}, col;
  std::vector<double> v;  // (the fp32 cases store these rounded to float)
  void row(const std::vector<int32_t> &c, const std::vector<double> &vals) {
    col.insert(col.end(), c.begin(), c.end());
    v.insert(v.end(), vals.begin(), vals.end());
    rp.push_back((int32_t)col.size());
    ++m;
  }
};

typedef std::mt19937_64 Rng;

// k distinct columns of [lo, hi), ascending
static std::vector<int32_t> pick(Rng &g, size_t k, int64_t lo, int64_t hi) {
  std::vector<int32_t> c;
  while (c.size() < k) {
    while (c.size() < k) c.push_back((int32_t)(lo + (int64_t)(g() % (uint64_t)(hi - lo))));
    std::sort(c.begin(), c.end());
    c.erase(std::unique(c.begin(), c.end()), c.end());
  }
  return c;
}

// k values in +-[0.5, 1) * 2^e, e uniform in [-span, span]
static std::vector<double> values(Rng &g, size_t k, int span = 0) {
  std::vector<double> v(k);
  for (auto &x : v) {
    const uint64_t b = g();
    x = (0.5 + (double)(b >> 12) * 0x1p-53) * ((b & 1) ? -1.0 : 1.0);
    if (span) x = std::ldexp(x, (int)(g() % (uint64_t)(2 * span + 1)) - span);
  }
  return v;
}

static Mat random_rows(uint64_t seed, int64_t m, int64_t n, int max_len) {
  Rng g(seed);
  Mat A;
  A.n = n;
  for (int64_t r = 0; r < m; ++r) {
    const size_t k = (size_t)(g() % (uint64_t)(max_len + 1));
    A.row(pick(g, std::min<size_t>(k, (size_t)n), 0, n), values(g, std::min<size_t>(k, (size_t)n)));
  }
  return A;
}

// short random rows; the rows in `at` hold `len` columns: contiguous from a
// random start (hubs), or spread over all of [0, n)
static Mat with_rows(uint64_t seed, int64_t m, int64_t n, const std::vector<int64_t> &at,
                     const std::vector<size_t> &len, bool contiguous, int span = 0) {
  Rng g(seed);
  Mat A;
  A.n = n;
  for (int64_t r = 0; r < m; ++r) {
    const auto it = std::find(at.begin(), at.end(), r);
    if (it == at.end()) {
      const size_t k = (size_t)(g() % 13);
      A.row(pick(g, k, 0, n), values(g, k, span));
      continue;
    }
    const size_t k = len[(size_t)(it - at.begin())];
    std::vector<int32_t> c;
    if (contiguous) {
      const int64_t c0 = (int64_t)(g() % (uint64_t)(n - (int64_t)k));
      for (size_t i = 0; i < k; ++i) c.push_back((int32_t)(c0 + (int64_t)i));
    } else {
      c = pick(g, k, 0, n);
    }
    A.row(c, values(g, k, span));
  }
  return A;
}

// ---- the new values: an independent draw, then the rows the issue names.
// rows_zero0: rows of v0 that the caller zeroed (filled here).
static std::vector<double> new_values(const Mat &A, uint64_t seed, int span, bool f32,
                                      const std::vector<int64_t> &rows_zero0) {
  Rng g(seed);
  std::vector<double> v = values(g, A.v.size(), span);
  std::vector<int64_t> full;  // rows with entries, apart from the ones that were zero
  for (int64_t r = 0; r < A.m; ++r)
    if (A.rp[r + 1] > A.rp[r] && std::find(rows_zero0.begin(), rows_zero0.end(), r) == rows_zero0.end())
      full.push_back(r);
  auto row_at = [&](size_t i) { return full[i * (full.size() - 1) / 6]; };
  if (full.size() >= 7) {
    for (int32_t k = A.rp[row_at(1)]; k < A.rp[row_at(1) + 1]; ++k) v[(size_t)k] = 0.0;  // becomes all zero
    for (int32_t k = A.rp[row_at(2)]; k < A.rp[row_at(2) + 1]; ++k) v[(size_t)k] = std::ldexp(v[(size_t)k], 40);
    for (int32_t k = A.rp[row_at(3)]; k < A.rp[row_at(3) + 1]; ++k) v[(size_t)k] = std::ldexp(v[(size_t)k], -40);
    // values over more than 2^100 (fp64: over 2^1060): under the fixed-point
    // scale the small ones leave the normal range with bits to round
    int64_t r = row_at(4);
    for (int64_t q : full)
      if (A.rp[q + 1] - A.rp[q] >= 4 && A.rp[q + 1] - A.rp[q] < 64) r = q;
    for (int32_t k = A.rp[r]; k < A.rp[r + 1]; ++k)
      v[(size_t)k] = std::ldexp(v[(size_t)k], (k - A.rp[r]) % 2 ? (f32 ? -80 : -560) : (f32 ? 60 : 500));
  }
  v[0] = -0.0;  // a signed zero keeps its sign
  return v;
}

// ---- the host restatement of refresh.hip

// the position, within its chunk, of the index word of the entry whose value
// is stored at pl in a wide fp64 stream (refresh.hip idx_of_val)
static int64_t idx_of_val(int64_t pl) {
  const int64_t u = (pl / 128) * 2 + pl % 2, lane = (pl % 128) / 2;
  return (u / 4) * 256 + lane * 4 + u % 4;
}

static double value_at(const void *val, bool f32, size_t k) {
  return f32 ? (double)static_cast<const float *>(val)[k] : static_cast<const double *>(val)[k];
}

// hspmv_refresh_row_scales + hspmv_refresh_long_scales
static void refresh_scales(const Mat &A, const void *val, bool f32, CsortPlan &P) {
  for (int64_t r = 0; r < A.m; ++r) {
    double mx = 0.0;
    for (int32_t k = A.rp[r]; k < A.rp[r + 1]; ++k) mx = std::fmax(mx, std::fabs(value_at(val, f32, (size_t)k)));
    const int64_t len = A.rp[r + 1] - A.rp[r];
    int e = 0;
    if (mx > 0.0) {
      int extra = 0;
      while (len <= P.long_t && ((int64_t)4096 << extra) < len) ++extra;
      e = -(std::ilogb(mx) + 1) - extra;
    }
    P.rexp[(size_t)r] = (int16_t)e;
  }
  for (size_t j = 0; j < P.long_row.size(); ++j)
    for (int32_t sl = P.long_cs[j]; sl < P.long_cs[j + 1]; ++sl) P.sexp[(size_t)sl] = P.rexp[(size_t)P.long_row[j]];
}

// hspmv_refresh_csort
static void refresh_stream(const void *val, bool f32, CsortPlan &P) {
  const int64_t C = 64 * (int64_t)P.u;
  for (int64_t b = 0; b < P.n_wg; ++b) {
    const int32_t r0 = P.blk_r[(size_t)(2 * b)], nr = P.blk_r[(size_t)(2 * b + 1)] - r0, v0 = P.blk_v[(size_t)b];
    auto scale = [&](uint32_t slot) {
      return (int32_t)slot < nr ? P.rexp[(size_t)(r0 + (int32_t)slot)]
                                : P.sexp[(size_t)P.vslice[(size_t)(v0 + (int32_t)slot - nr)]];
    };
    for (int64_t c = P.blk_c[(size_t)b]; c < P.blk_c[(size_t)b + 1]; ++c)
      for (int64_t pl = 0; pl < C; ++pl) {
        const size_t p = (size_t)(c * C + pl);
        const uint32_t k = P.src[p];
        if (f32) {
          float v = k == kCsortSrcPad ? 0.f : static_cast<const float *>(val)[k];
          if (P.fixed && k != kCsortSrcPad) v = (float)std::ldexp((double)v, scale((uint32_t)P.rec[p] >> 16));
          uint32_t bits;
          memcpy(&bits, &v, 4);
          P.rec[p] = (P.rec[p] & 0xffffffffull) | ((uint64_t)bits << 32);
        } else {
          double v = k == kCsortSrcPad ? 0.0 : static_cast<const double *>(val)[k];
          if (P.fixed && k != kCsortSrcPad)
            v = std::ldexp(v, scale(P.idx[(size_t)(c * C + (P.wide ? idx_of_val(pl) : pl))] >> 16));
          P.val64[p] = v;
        }
      }
  }
}

template <typename T>
static bool same_bytes(const std::vector<T> &a, const std::vector<T> &b) {
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

struct Want {
  bool early = false;   // chunks closed at the 65535-column span
  bool seg = false;     // segmented chunks
  bool slices = false;  // long-row slices
  bool extra = false;   // a whole long row: the `extra` term of rexp
  bool narrow = false;  // fp32 fixed point: a value scaled below the normal range, bits lost
};

static int run(const std::string &name, Mat A, int dtype, unsigned flags, Tuning tn, int cus, int span,
               const Want &want) {
  g_case = name.c_str();
  const bool f32 = dtype == HSPMV_F32;
  // v0: a zero row and an empty pattern are in the generators' hands; one more zero row here
  std::vector<int64_t> zero0;
  for (int64_t r = A.m / 3; r < A.m && zero0.empty(); ++r)
    if (A.rp[r + 1] > A.rp[r]) zero0.push_back(r);
  for (int64_t r : zero0)
    for (int32_t k = A.rp[r]; k < A.rp[r + 1]; ++k) A.v[(size_t)k] = 0.0;
  const std::vector<double> w = new_values(A, 977, span, f32, zero0);
  std::vector<float> a32(A.v.begin(), A.v.end()), b32(w.begin(), w.end());
  std::vector<double> a64 = A.v, b64 = w;
  a32.push_back(0.f), b32.push_back(0.f), a64.push_back(0.0), b64.push_back(0.0);  // (never null)
  const void *v0 = f32 ? (const void *)a32.data() : (const void *)a64.data();
  const void *v1 = f32 ? (const void *)b32.data() : (const void *)b64.data();
  const CsortLimits lim{cus, kCsortMaxLds - kCsortStaticLds};
  CsortPlan plain, P, Q;
  tn.csort_src = 0;
  CHECK(plan_csort(A.rp.data(), A.col.data(), v0, A.m, A.n, dtype, flags, tn, lim, plain));
  tn.csort_src = 1;
  CHECK(plan_csort(A.rp.data(), A.col.data(), v0, A.m, A.n, dtype, flags, tn, lim, P));
  CHECK(plan_csort(A.rp.data(), A.col.data(), v1, A.m, A.n, dtype, flags, tn, lim, Q));
  CHECK(P.fixed == (tn.deterministic == 2) && Q.fixed == P.fixed);
  const int64_t C = 64 * (int64_t)P.u, tot = P.chunks * C;
  // the request adds src and nothing else
  CHECK(plain.src.empty() && same_bytes(plain.rec, P.rec) && same_bytes(plain.val64, P.val64) &&
        plain.idx == P.idx && plain.cbase == P.cbase && plain.blk_c == P.blk_c && plain.blk_r == P.blk_r &&
        plain.blk_v == P.blk_v && plain.vslice == P.vslice && plain.rexp == P.rexp && plain.sexp == P.sexp &&
        plain.chunks == P.chunks && plain.seg_chunks == P.seg_chunks && plain.format_bytes == P.format_bytes);
  // src: one entry per stream position, every nonzero exactly once
  CHECK((int64_t)P.src.size() == std::max<int64_t>(tot, 1) && P.long_t > 0);
  std::vector<uint8_t> seen((size_t)A.rp[A.m], 0);
  for (int64_t p = 0; p < tot; ++p) {
    const uint32_t k = P.src[(size_t)p];
    if (k == kCsortSrcPad) continue;
    CHECK(k < (uint32_t)A.rp[A.m] && seen[k]++ == 0);
    // ... and it is the value stored there
    if (P.fixed) continue;
    const uint32_t stored = f32 ? (uint32_t)(P.rec[(size_t)p] >> 32) : 0;
    CHECK(f32 ? memcmp(&stored, &a32[k], 4) == 0 : memcmp(&P.val64[(size_t)p], &a64[k], 8) == 0);
  }
  for (uint8_t s : seen) CHECK(s == 1);
  // nothing but the values depends on the values
  CHECK(Q.src == P.src && Q.idx == P.idx && Q.cbase == P.cbase && Q.blk_c == P.blk_c && Q.blk_r == P.blk_r &&
        Q.blk_v == P.blk_v && Q.vslice == P.vslice && Q.long_row == P.long_row && Q.long_cs == P.long_cs &&
        Q.long_mask == P.long_mask && Q.chunks == P.chunks && Q.n_wg == P.n_wg && Q.long_t == P.long_t);
  if (f32)
    for (int64_t p = 0; p < tot; ++p) CHECK((uint32_t)Q.rec[(size_t)p] == (uint32_t)P.rec[(size_t)p]);
  // the refresh
  if (P.fixed) refresh_scales(A, v1, f32, P);
  refresh_stream(v1, f32, P);
  CHECK(same_bytes(P.rexp, Q.rexp) && same_bytes(P.sexp, Q.sexp));
  CHECK(same_bytes(P.rec, Q.rec) && same_bytes(P.val64, Q.val64));
  CHECK(!same_bytes(plain.rec, Q.rec) || !same_bytes(plain.val64, Q.val64));  // (the values did move)
  // the branch this case is for
  if (want.early) {
    int64_t n_early = 0;
    for (int64_t b = 0; b < P.n_wg; ++b)
      for (int64_t c = P.blk_c[(size_t)b]; c + 1 < P.blk_c[(size_t)b + 1]; ++c) {
        bool pad = false;
        for (int64_t pl = 0; pl < C; ++pl) pad |= P.src[(size_t)(c * C + pl)] == kCsortSrcPad;
        n_early += pad;
      }
    CHECK(n_early > 0);
  }
  if (want.seg) CHECK(P.seg_chunks > 0);
  if (want.slices) CHECK(P.n_long > 0 && P.vslice.size() > P.long_row.size());
  if (want.extra) {
    int64_t n_extra = 0;
    for (int64_t r = 0; r < A.m; ++r) n_extra += A.rp[r + 1] - A.rp[r] > 4096 && A.rp[r + 1] - A.rp[r] <= P.long_t;
    CHECK(P.fixed && n_extra > 0 && P.n_long == 0);
  }
  if (want.narrow) {  // a stored fp32 value below the normal range whose scaling lost bits
    int64_t n = 0;
    for (int64_t p = 0; p < tot; ++p) {
      const uint32_t k = P.src[(size_t)p], bits = (uint32_t)(Q.rec[(size_t)p] >> 32);
      if (k == kCsortSrcPad || (bits & 0x7f800000u) || !(bits & 0x007fffffu)) continue;
      float v;
      memcpy(&v, &bits, 4);
      int e;
      n += std::frexp((double)v, &e) != std::frexp((double)b32[k], &e);
    }
    CHECK(f32 && P.fixed && n > 0);
  }
  return 0;
}

int main() {
  const char *dn[2] = {"f32", "f64"};
  const int dts[2] = {HSPMV_F32, HSPMV_F64};
  int bad = 0, cases = 0;
  auto go = [&](const std::string &name, const Mat &A, int dtype, unsigned flags, const Tuning &tn, int cus,
                int span, const Want &w) {
    bad += run(name, A, dtype, flags, tn, cus, span, w);
    ++cases;
  };
  // random: the wide n closes chunks early at the 65535 span; H = 1, 2, 4,
  // every chunk size, wide and narrow layouts, plain and fixed-point slots
  {
    const Mat A = random_rows(1, 3000, 200000, 24);
    int i = 0;
    for (int d = 0; d < 2; ++d)
      for (int parts : {1, 2, 4})
        for (int u : {4, 8, 16})
          for (int det : {0, 2}) {
            Tuning tn;
            tn.csort_parts = parts;
            tn.csort_u = u;
            tn.csort_wide = i % 2;
            tn.deterministic = det;
            Want w;
            w.early = A.n / parts > 65535;
            w.narrow = det == 2 && d == 0;
            go(std::string("random_") + dn[d] + "_h" + std::to_string(parts) + "_u" + std::to_string(u) + "_wide" +
                   std::to_string(tn.csort_wide) + "_det" + std::to_string(det),
               A, dts[d], 0, tn, 256, d ? 300 : 30, w);
            ++i;
          }
  }
  // hub rows: ~600 contiguous columns among short rows -> segmented chunks
  {
    const Mat A = with_rows(2, 2000, 100000, {3, 500, 501, 1999}, {600, 640, 580, 610}, true);
    for (int seg : {-1, 2})
      for (int d = 0; d < 2; ++d)
        for (int det : {0, 2})
          for (int wide : {0, 1}) {
            Tuning tn;
            tn.csort_seg = seg;
            tn.deterministic = det;
            tn.csort_wide = wide;
            Want w;
            w.seg = true;
            go(std::string("hubs_") + dn[d] + "_seg" + std::to_string(seg) + "_det" + std::to_string(det) + "_wide" +
                   std::to_string(wide),
               A, dts[d], 0, tn, 64, 0, w);
          }
  }
  // long rows: two rows over 4096 nonzeros, columns in both parts: sliced, or
  // kept whole (HSPMV_FLAG_NO_SPLIT: the `extra` term of their scale)
  {
    const Mat A = with_rows(3, 500, 50000, {7, 300}, {9000, 5000}, false);
    for (int d = 0; d < 2; ++d)
      for (int det : {0, 2})
        for (int wide : {0, 1}) {
          Tuning tn;
          tn.deterministic = det;
          tn.csort_wide = wide;
          Want w;
          w.slices = true;
          const std::string tail = std::string(dn[d]) + "_det" + std::to_string(det) + "_wide" + std::to_string(wide);
          go("long_sliced_" + tail, A, dts[d], 0, tn, 32, d ? 200 : 20, w);
          Want ww;
          ww.extra = det == 2;
          go("long_whole_" + tail, A, dts[d], HSPMV_FLAG_NO_SPLIT, tn, 32, 0, ww);
        }
  }
  // empty rows and an empty-pattern tail beside values over many binades
  for (int d = 0; d < 2; ++d) {
    Mat A = with_rows(4, 400, 3000, {5, 6, 399}, {9, 0, 0}, false, d ? 300 : 30);
    for (int det : {0, 2}) {
      Tuning tn;
      tn.deterministic = det;
      go(std::string("empty_rows_") + dn[d] + "_det" + std::to_string(det), A, dts[d], 0, tn, 16, d ? 300 : 30, Want());
    }
  }
  if (bad) {
    fprintf(stderr, "csort_update_check: %d of %d cases failed\n", bad, cases);
    return 1;
  }
  printf("csort_update_check: %d cases ok\n", cases);
  return 0;
}
