// csort_plan_check.cpp -- host-only driver for the column-sorted tables
// (plan_csort, csrc/hspmv_csort_build.cpp).  Every case is planned with
// explicit CsortLimits and then
//   - decoded back into (row, column, value) triples the way csort.hip reads
//     the tables -- workgroups, chunks, lanes, through the wide layout; the
//     slot from the upper 16 bits of an index word, the column as chunk base
//     + the lower 16; a slot below the block's row count a block row, above
//     it a long-row slice (vslice, long_cs -> long_row), the last the dummy
//     -- and compared with the CSR: every nonzero once, in the workgroup of
//     its column's part and its row's block, its value (scaled by exactly
//     2^rexp[row] in fixed-point plans) intact, chunks in column order or
//     flagged segmented, spans within 16 bits, ranges monotone, lds_bytes
//     enough and within the limit, long_mask the long rows' bits;
//   - printed as one line: the scalars and an FNV-1a 64 digest of each table
//     (tests/test_csort_plan.py pins the lines).
// Each case also asserts that the branch it is there for was reached.  No
// device is touched.  `make asan-csort` builds it against the
// AddressSanitizer + UBSan library and runs it; `make tools` builds
// build/csort_plan_check.
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
static int64_t g_slices = 0;  // long-row slices of the plan decoded last

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

struct Want {
  bool plan = true;    // plan_csort's result
  bool early = false;  // chunks closed at the 65535-column span
  int seg = -1;        // segmented chunks: 0 none, 1 some, 2 all (-1: any)
  bool slices = false; // long-row slices
  bool extra = false;  // a whole long row: the `extra` term of rexp
  int fixed = -1;      // P.fixed (-1: as asked for)
};

static uint64_t fnv(const void *p, size_t bytes) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < bytes; ++i) h = (h ^ static_cast<const unsigned char *>(p)[i]) * 0x100000001b3ull;
  return h;
}
template <typename T>
static uint64_t fnv(const std::vector<T> &v) {
  return fnv(v.data(), v.size() * sizeof(T));
}

static void print_line(const char *name, const CsortPlan &P) {
  printf("%s n_wg=%d H=%d u=%d direct=%d n_long=%d nt=%d pf=%d slot32=%d part32=%d wide=%d dyn=%d fixed=%d "
         "fin_rows=%d lds=%d row_blocks=%d n_xexp=%d part=%zu spart=%zu xexp=%zu trace=%zu chunks=%lld seg=%lld "
         "pb=%lld,%lld,%lld,%lld fmt=%.0f",
         name, P.n_wg, P.H, P.u, (int)P.direct, P.n_long, (int)P.nontemporal, (int)P.prefetch, (int)P.slot32,
         (int)P.part32, (int)P.wide, (int)P.dyn, (int)P.fixed, P.fin_rows, P.lds_bytes, P.row_blocks, P.n_xexp,
         P.part_bytes, P.spart_bytes, P.xexp_part_bytes, P.trace_bytes, (long long)P.chunks,
         (long long)P.seg_chunks, (long long)P.part_begin[0], (long long)P.part_begin[1],
         (long long)P.part_begin[2], (long long)P.part_begin[3], P.format_bytes);
  const uint64_t ent = P.dtype == HSPMV_F32 ? fnv(P.rec) : fnv(P.idx);
  printf(" blk_c=%016llx blk_r=%016llx blk_v=%016llx vslice=%016llx cbase=%016llx ent=%016llx val=%016llx "
         "long_mask=%016llx long_row=%016llx long_cs=%016llx rexp=%016llx sexp=%016llx stats=%016llx\n",
         (unsigned long long)fnv(P.blk_c), (unsigned long long)fnv(P.blk_r), (unsigned long long)fnv(P.blk_v),
         (unsigned long long)fnv(P.vslice), (unsigned long long)fnv(P.cbase), (unsigned long long)ent,
         (unsigned long long)fnv(P.val64), (unsigned long long)fnv(P.long_mask),
         (unsigned long long)fnv(P.long_row), (unsigned long long)fnv(P.long_cs), (unsigned long long)fnv(P.rexp),
         (unsigned long long)fnv(P.sexp), (unsigned long long)fnv(P.wg_stats));
}

// where csort.hip reads entry q of a chunk (hspmv_csort_build.cpp `at`)
static int64_t at(bool wide, int64_t q, int per) {
  if (!wide) return q;
  const int64_t u = q / 64, lane = q % 64;
  return (u / per) * (64 * per) + lane * per + (u % per);
}

struct Dec {
  int64_t col;
  uint32_t slot;
};

// The round trip of one plan.  val: the values as the planner saw them.
static int round_trip(const Mat &A, const void *val, int dtype, int32_t long_t, const CsortLimits &lim,
                      const CsortPlan &P, const Want &want) {
  const int64_t m = A.m, n = A.n, C = 64 * (int64_t)P.u, G = P.n_wg;
  const int H = P.H;
  const bool f32 = dtype == HSPMV_F32;
  const int64_t slot_bytes = P.slot32 ? 4 : 8;
  CHECK(P.m == m && P.n == n && P.dtype == dtype && G >= 1 && H >= 1 && H <= 4 && G % H == 0);
  CHECK(P.row_blocks == G / H);
  // ranges: monotone and in bounds
  CHECK((int64_t)P.blk_c.size() == G + 1 && (int64_t)P.blk_v.size() == G + 1 && (int64_t)P.blk_r.size() == 2 * G);
  CHECK(P.blk_c[0] == 0 && P.blk_v[0] == 0);
  for (int64_t b = 0; b < G; ++b) {
    CHECK(P.blk_c[b] <= P.blk_c[b + 1] && P.blk_v[b] <= P.blk_v[b + 1]);
    CHECK(0 <= P.blk_r[2 * b] && P.blk_r[2 * b] <= P.blk_r[2 * b + 1] && P.blk_r[2 * b + 1] <= m);
  }
  CHECK(P.blk_c[G] == P.chunks && (int64_t)P.cbase.size() == std::max<int64_t>(P.chunks, 1));
  CHECK(P.blk_v[G] == (int64_t)P.vslice.size());
  CHECK((f32 ? P.rec.size() : P.idx.size()) == (size_t)(P.chunks * C));
  CHECK(f32 ? P.idx.empty() && P.val64.empty() : P.rec.empty() && P.val64.size() == P.idx.size());
  for (int h = 0; h < H; ++h) {  // each part's blocks tile [0, m) in order
    int64_t next = 0;
    for (int64_t b = h; b < G; b += H) {
      if (P.blk_r[2 * b] == m && P.blk_r[2 * b + 1] == m) continue;  // past the part's blocks
      CHECK(P.blk_r[2 * b] == next);
      next = P.blk_r[2 * b + 1];
    }
    CHECK(next == m);
  }
  for (int h = 0; h < 4; ++h) CHECK(h < H ? P.part_begin[h] >= 0 && P.part_begin[h] < n : P.part_begin[h] == 0);
  CHECK(P.part_begin[0] == 0);
  for (int h = 1; h < H; ++h) CHECK(P.part_begin[h] > P.part_begin[h - 1]);
  // long rows: the rows over long_t, their mask, slices per row
  std::vector<int32_t> longs;
  for (int64_t r = 0; r < m; ++r)
    if (A.rp[r + 1] - A.rp[r] > long_t) longs.push_back((int32_t)r);
  CHECK(P.n_long == (int32_t)longs.size() && P.long_row == longs);
  CHECK(P.direct == (H == 1 && longs.empty()));
  int64_t n_slices = 0;
  std::vector<int32_t> slice_row;
  if (longs.empty()) {
    CHECK(P.long_mask.empty() && P.long_cs.empty());
  } else {
    std::vector<uint32_t> mask((size_t)((m + 31) / 32), 0u);
    for (int32_t r : longs) mask[(size_t)r >> 5] |= 1u << (r & 31);
    CHECK(P.long_mask == mask && P.long_cs.size() == longs.size() + 1 && P.long_cs[0] == 0);
    for (size_t j = 0; j < longs.size(); ++j) {
      CHECK(P.long_cs[j] < P.long_cs[j + 1]);
      slice_row.insert(slice_row.end(), (size_t)(P.long_cs[j + 1] - P.long_cs[j]), longs[j]);
    }
    n_slices = P.long_cs.back();
  }
  CHECK((int64_t)P.vslice.size() == n_slices);
  g_slices = n_slices;
  {
    std::vector<int32_t> vs = P.vslice;  // every slice in exactly one workgroup
    std::sort(vs.begin(), vs.end());
    for (int64_t i = 0; i < n_slices; ++i) CHECK(vs[(size_t)i] == i);
  }
  CHECK(P.part_bytes == (P.direct ? 0 : (size_t)(P.part32 ? 4 : slot_bytes) * (size_t)H * (size_t)m));
  CHECK(P.spart_bytes == (P.direct ? 0 : (size_t)slot_bytes * (size_t)std::max<int64_t>(n_slices, 1)));
  // fixed-point scales
  int64_t n_extra = 0;
  if (P.fixed) {
    CHECK((int64_t)P.rexp.size() == m && (int64_t)P.sexp.size() == std::max<int64_t>(n_slices, 1));
    for (int64_t r = 0; r < m; ++r) {
      double mx = 0.0;
      for (int32_t k = A.rp[r]; k < A.rp[r + 1]; ++k)
        mx = std::max(mx, std::fabs(f32 ? (double)static_cast<const float *>(val)[k] : A.v[(size_t)k]));
      const int64_t len = A.rp[r + 1] - A.rp[r];
      int extra = 0;
      while (len <= long_t && ((int64_t)4096 << extra) < len) ++extra;
      n_extra += extra > 0;
      CHECK(P.rexp[(size_t)r] == (mx > 0.0 ? -(std::ilogb(mx) + 1) - extra : 0));
    }
    for (int64_t s = 0; s < n_slices; ++s) CHECK(P.sexp[(size_t)s] == P.rexp[(size_t)slice_row[(size_t)s]]);
    CHECK(P.n_xexp >= 1 && P.n_xexp <= kCsortXexpBlocks && P.xexp_part_bytes == 4 * (size_t)P.n_xexp);
  } else {
    CHECK(P.rexp.empty() && P.sexp.empty() && P.n_xexp == 0 && P.xexp_part_bytes == 0);
  }
  // the entries
  std::vector<uint8_t> seen((size_t)A.rp[m], 0);
  int64_t max_slots = 1, n_seg = 0, n_early = 0;
  for (int64_t b = 0; b < G; ++b) {
    const int h = (int)(b % H);
    const int64_t plo = P.part_begin[h], phi = h + 1 < H ? P.part_begin[h + 1] : n;
    const int32_t r0 = P.blk_r[2 * b], nr = P.blk_r[2 * b + 1] - r0;
    const int32_t *sl = P.vslice.data() + P.blk_v[b];
    const int32_t nsl = P.blk_v[b + 1] - P.blk_v[b];
    const uint32_t dummy = (uint32_t)(nr + nsl);
    max_slots = std::max<int64_t>(max_slots, (int64_t)dummy + 1);
    CHECK(dummy < 65536u);
    struct {
      Dec last;  // of the chunk before, in (column, slot) order
      int64_t ne, base;
    } prev = {{0, 0}, 0, 0};
    for (int64_t ch = P.blk_c[b]; ch < P.blk_c[b + 1]; ++ch) {
      const uint32_t cb = (uint32_t)P.cbase[(size_t)ch];
      const int64_t base = cb & 0x7fffffffu;
      const bool seg = cb >> 31;
      n_seg += seg;
      std::vector<Dec> e;
      bool pad = false;
      for (int64_t q = 0; q < C; ++q) {
        uint32_t ix, vb32 = 0;
        double v64 = 0.0;
        if (f32) {
          const uint64_t rec = P.rec[(size_t)(ch * C + at(P.wide, q, 2))];
          ix = (uint32_t)rec;
          vb32 = (uint32_t)(rec >> 32);
        } else {
          ix = P.idx[(size_t)(ch * C + at(P.wide, q, 4))];
          v64 = P.val64[(size_t)(ch * C + at(P.wide, q, 2))];
        }
        const uint32_t slot = ix >> 16;
        if (slot == dummy) {  // padding: 0 * x[base], and nothing after it
          uint64_t vb64;
          memcpy(&vb64, &v64, 8);
          CHECK((ix & 0xffffu) == 0 && vb32 == 0 && vb64 == 0);
          pad = true;
          continue;
        }
        CHECK(!pad && slot < dummy);
        const int64_t c = base + (ix & 0xffffu);
        CHECK(c >= plo && c < phi);  // its column's part
        int64_t r;
        if ((int32_t)slot < nr) {
          r = (int64_t)r0 + slot;  // its row's block
          CHECK(A.rp[r + 1] - A.rp[r] <= long_t);
        } else {
          r = slice_row[(size_t)sl[slot - (uint32_t)nr]];
        }
        const int32_t *rb = A.col.data() + A.rp[r], *re = A.col.data() + A.rp[r + 1];
        const int32_t *it = std::lower_bound(rb, re, (int32_t)c);
        CHECK(it != re && *it == c);
        const size_t k = (size_t)(it - A.col.data());
        CHECK(seen[k]++ == 0);
        if (f32) {
          float orig = static_cast<const float *>(val)[k];
          if (P.fixed) orig = std::ldexp(orig, P.rexp[(size_t)r]);
          CHECK(memcmp(&orig, &vb32, 4) == 0);
        } else {
          const double orig = P.fixed ? std::ldexp(A.v[k], P.rexp[(size_t)r]) : A.v[k];
          CHECK(memcmp(&orig, &v64, 8) == 0);
        }
        if (!seg && !e.empty()) CHECK(e.back().col < c || (e.back().col == c && e.back().slot <= slot));
        e.push_back({c, slot});
      }
      CHECK(!e.empty());
      // a segmented chunk holds what the column order would have put there
      if (seg) std::sort(e.begin(), e.end(), [](const Dec &x, const Dec &y) {
        return x.col != y.col ? x.col < y.col : x.slot < y.slot;
      });
      CHECK(e.front().col == base && e.back().col - base <= 65535);
      if (ch > P.blk_c[b]) {  // ... after the chunk before it, which closed early only for the span
        CHECK(prev.last.col < e.front().col ||
              (prev.last.col == e.front().col && prev.last.slot <= e.front().slot));
        if (prev.ne < C) {
          CHECK(e.front().col - prev.base > 65535);
          ++n_early;
        }
      }
      prev = {e.back(), (int64_t)e.size(), base};
    }
  }
  for (uint8_t s : seen) CHECK(s == 1);
  CHECK(n_seg == P.seg_chunks);
  CHECK(P.lds_bytes >= slot_bytes * max_slots && P.lds_bytes <= lim.lds_bytes);
  // the branch this case is for
  if (want.early) CHECK(n_early > 0);
  if (want.seg == 0) CHECK(n_seg == 0);
  if (want.seg == 1) CHECK(n_seg > 0 && n_seg < P.chunks);
  if (want.seg == 2) CHECK(n_seg == P.chunks && n_seg > 0);
  if (want.slices) CHECK(n_slices > (int64_t)longs.size() && !longs.empty());
  if (want.extra) CHECK(n_extra > 0 && n_slices == 0);
  return 0;
}

static int run(const std::string &name, const Mat &A, int dtype, unsigned flags, const Tuning &tn, int cus,
               const Want &want) {
  g_case = name.c_str();
  std::vector<float> v32(A.v.begin(), A.v.end());
  v32.push_back(0.f);  // (never null)
  std::vector<double> v64 = A.v;
  v64.push_back(0.0);
  const void *val = dtype == HSPMV_F32 ? (const void *)v32.data() : (const void *)v64.data();
  const CsortLimits lim{cus, kCsortMaxLds - kCsortStaticLds};
  CsortPlan P;
  const bool ok = plan_csort(A.rp.data(), A.col.data(), val, A.m, A.n, dtype, flags, tn, lim, P);
  CHECK(ok == want.plan);
  if (!ok) {
    printf("%s none\n", g_case);
    return 0;
  }
  CHECK(P.fixed == (want.fixed >= 0 ? want.fixed == 1 : tn.deterministic == 2));
  const int32_t long_t = (flags & HSPMV_FLAG_NO_SPLIT) ? INT32_MAX : (tn.csort_long > 0 ? tn.csort_long : kLongRow);
  if (round_trip(A, val, dtype, long_t, lim, P, want)) return 1;
  print_line(g_case, P);
  return 0;
}

int main() {
  const char *dn[2] = {"f32", "f64"};
  const int dts[2] = {HSPMV_F32, HSPMV_F64};
  int bad = 0, cases = 0;
  auto go = [&](const std::string &name, const Mat &A, int dtype, unsigned flags, const Tuning &tn, int cus,
                const Want &w) {
    bad += run(name, A, dtype, flags, tn, cus, w);
    ++cases;
  };
  // random: the wide n closes chunks early at the 65535 span (one block per
  // CU and part: a workgroup's ~140 entries lie over a part of 100 000
  // columns or more)
  {
    const Mat A = random_rows(1, 3000, 200000, 24);
    int i = 0;
    for (int d = 0; d < 2; ++d)
      for (int parts : {1, 2, 4})
        for (int u : {4, 8, 16}) {
          Tuning tn;
          tn.csort_parts = parts;
          tn.csort_u = u;
          tn.csort_balance = i % 2 ? -1 : 0;
          tn.csort_wide = i / 2 % 2;
          const int cus = i / 4 % 2 ? 8 : 256;
          Want w;
          w.early = cus == 256 && A.n / parts > 65535;  // (four parts are 50 000 columns each)
          go(std::string("random_") + dn[d] + "_h" + std::to_string(parts) + "_u" + std::to_string(u) + "_bal" +
                 std::to_string(tn.csort_balance) + "_wide" + std::to_string(tn.csort_wide) + "_cu" +
                 std::to_string(cus),
             A, dts[d], 0, tn, cus, w);
          ++i;
        }
    Tuning tn;  // the diagnostic statistics and the trace buffer's size
    tn.csort_trace = 1;
    go("random_f32_trace", A, HSPMV_F32, 0, tn, 64, Want());
  }
  // hub rows: ~600 contiguous columns among short rows -> segmented chunks
  {
    const Mat A = with_rows(2, 2000, 100000, {3, 500, 501, 1999}, {600, 640, 580, 610}, true);
    for (int seg : {-1, 0, 2})
      for (int d = 0; d < 2; ++d) {
        Tuning tn;
        tn.csort_seg = seg;
        Want w;
        w.seg = seg < 0 ? 1 : seg;
        go(std::string("hubs_") + dn[d] + "_seg" + std::to_string(seg), A, dts[d], 0, tn, 64, w);
      }
  }
  // long rows: two rows over 4096 nonzeros, columns in both parts
  {
    const Mat A = with_rows(3, 500, 50000, {7, 300}, {9000, 5000}, false);
    Tuning tn;
    Want w;
    w.slices = true;
    go("long_sliced_f64", A, HSPMV_F64, 0, tn, 32, w);
    tn.deterministic = 2;
    go("long_sliced_fixed_f32", A, HSPMV_F32, 0, tn, 32, w);
    Want ww;
    ww.extra = true;
    go("long_whole_fixed_f64", A, HSPMV_F64, HSPMV_FLAG_NO_SPLIT, tn, 32, ww);
  }
  // fixed point: values over many binades, an all-zero row, an empty row;
  // one Inf value: no fixed-point plan
  for (int d = 0; d < 2; ++d) {
    Mat A = with_rows(4, 400, 3000, {5, 6}, {9, 0}, false, d ? 300 : 30);
    for (int32_t k = A.rp[5]; k < A.rp[6]; ++k) A.v[(size_t)k] = 0.0;
    Tuning tn;
    tn.deterministic = 2;
    go(std::string("fixed_") + dn[d], A, dts[d], 0, tn, 16, Want());
    A.v[(size_t)A.rp[200]] = INFINITY;
    Want w;
    w.fixed = 0;
    go(std::string("fixed_inf_") + dn[d], A, dts[d], 0, tn, 16, w);
  }
  // degenerate shapes and the planner's exits
  {
    Mat one;
    one.n = 1;
    one.row({0}, {0.75});
    go("one_by_one", one, HSPMV_F64, 0, Tuning(), 256, Want());
    Mat n1;
    n1.n = 1;
    for (int r = 0; r < 5; ++r) {
      if (r % 2) n1.row({}, {});
      else n1.row({0}, {1.0 + r});
    }
    Tuning t4;
    t4.csort_parts = 4;  // clamped to n
    go("n1_parts4", n1, HSPMV_F32, 0, t4, 256, Want());
    Mat empty;
    empty.n = 50;
    for (int r = 0; r < 100; ++r) empty.row({}, {});
    go("empty_rows", empty, HSPMV_F64, 0, Tuning(), 256, Want());
    Tuning tc;
    tc.csort_lds_cap = 512;  // 63 slots: row_cap < 64
    Want none;
    none.plan = false;
    go("lds_cap_row_cap", random_rows(5, 300, 1000, 8), HSPMV_F64, 0, tc, 256, none);
    // 20 sliced rows and nothing else: one block per part (their in-kernel
    // weight is 0) takes the part's ~100 slices -- with room, then past a
    // cap that still leaves row_cap = 552 / 8 - 2 - (slices / 128 + 2) = 64
    std::vector<int64_t> at;
    for (int r = 0; r < 20; ++r) at.push_back(r);
    const Mat L = with_rows(6, 20, 40000, at, std::vector<size_t>(20, 20000), false);
    tc.csort_lds_cap = 2048;
    Want w;
    w.slices = true;
    go("slots_within_lds", L, HSPMV_F64, 0, tc, 256, w);
    if (552 / 8 - 2 - (g_slices / 128 + 2) < 64) {
      fprintf(stderr, "slots_over_lds: %lld slices leave row_cap < 64\n", (long long)g_slices);
      ++bad;
    }
    tc.csort_lds_cap = 552;
    go("slots_over_lds", L, HSPMV_F64, 0, tc, 256, none);
    Mat none_m;  // m == 0
    none_m.n = 4;
    go("no_rows", none_m, HSPMV_F64, 0, Tuning(), 256, none);
  }
  if (bad) {
    fprintf(stderr, "csort_plan_check: %d of %d cases failed\n", bad, cases);
    return 1;
  }
  printf("csort_plan_check: %d plans decoded\n", cases);
  return 0;
}
