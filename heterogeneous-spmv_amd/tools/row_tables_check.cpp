// row_tables_check.cpp -- host-only driver for the row kernels' host tables
// (csrc/hspmv_tables.cpp): the 16-bit columns with block bases (plan_col16)
// and group bases (plan_col16g), the x slabs (plan_xslabs), the split rows
// (plan_split_rows), the two rules median_serial_len / wants_csort and the
// bytes-saved formulas (c16_saved_of).  Every case is planned and then
// decoded back into the matrix the way the kernels read the table:
//   - block columns: col[k] = base[k >> kC16Shift] + off[k] + the plane bits
//     (bit k & 63 of planes[p * plane_words + (k >> 6)]) << (16 + p); the pad
//     base and the pad plane word exist and are 0, no bit past nnz is set;
//   - group columns: col[k] = base[g] + off[k] for every nonzero of a
//     non-split row of group g (64 rows, or the task [starts[g], starts[g+1]));
//     split rows have off 0 and do not widen a span, an empty group has base 0;
//   - slabs: a non-split row's B segments in slab order are its CSR columns
//     and value bytes, segment b's columns lie in [b W, (b + 1) W), slab b + 1
//     starts where slab b ended, split rows have B empty segments;
//   - split rows: the chunks of row r tile [rp[r], rp[r + 1]) in steps of
//     kLongChunk, long_cs is their prefix, long_nnz their sum, and no row of
//     at most split_threshold(flags) nonzeros appears.
// Each case also asserts the outcome it is there for (taken or declined, the
// planes, B).  Then one line per case: the scalars, the bytes saved for the
// launch shape the table was built for as a hex float, and an FNV-1a 64
// digest per array (tests/test_row_tables_plan.py pins the lines).
// Not reached here: the automatic ACCEPTANCE of x slabs needs >= 4 000 000
// nonzeros (2 000 000 per slab) and the exit "x within an XCD's L2" alone a
// matrix over 192 MiB; the GPU tests cover them (tests/test_planner.py: C5
// with deterministic = 1 takes slabs by itself).  No device is touched.
// `make asan-row-tables` builds this against the AddressSanitizer + UBSan
// library and runs it; `make tools` builds build/row_tables_check.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

static uint64_t fnv(const void *p, size_t bytes) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < bytes; ++i) h = (h ^ static_cast<const unsigned char *>(p)[i]) * 0x100000001b3ull;
  return h;
}
template <typename T>
static unsigned long long fnv(const std::vector<T> &v) {
  return (unsigned long long)fnv(v.data(), v.size() * sizeof(T));
}

struct Mat {
  int64_t m = 0, n = 0;
  std::vector<int32_t> rp{0}, col;
  void row(const std::vector<int32_t> &c) {
    col.insert(col.end(), c.begin(), c.end());
    rp.push_back((int32_t)col.size());
    ++m;
  }
  int64_t nnz() const { return rp.back(); }
  // the value of nonzero k: distinct bytes per k in both dtypes
  std::vector<char> values(int val_dtype) const {
    std::vector<char> v((size_t)(nnz() + 1) * dtype_size(val_dtype));  // (never empty)
    for (int64_t k = 0; k < nnz(); ++k) {
      const double d = 1.0 + (double)(k % 8191) / 8192.0 + (double)(k / 8191);
      const float f = (float)d;
      if (val_dtype == HSPMV_F64) memcpy(&v[(size_t)k * 8], &d, 8);
      else memcpy(&v[(size_t)k * 4], &f, 4);
    }
    return v;
  }
};

// Rows of 1..7 nonzeros until exactly `nnz`: row r's columns ascend from
// lo + 10 r in steps of 2, so 256 consecutive nonzeros span under 1000.
static Mat chain(int64_t nnz, int64_t n, int32_t lo = 1000000) {
  Mat A;
  A.n = n;
  for (int64_t r = 0; A.nnz() < nnz; ++r) {
    const int64_t len = std::min<int64_t>(1 + (r * 5) % 7, nnz - A.nnz());
    std::vector<int32_t> c;
    for (int64_t j = 0; j < len; ++j) c.push_back((int32_t)(lo + 10 * r + 2 * j));
    A.row(c);
  }
  return A;
}

// m rows of `len` nonzeros (rows in `empty` none), columns ascending from lo + 3 r.
static Mat rows_of(int64_t m, int64_t n, int len, int32_t lo, const std::vector<int64_t> &empty = {}) {
  Mat A;
  A.n = n;
  for (int64_t r = 0; r < m; ++r) {
    std::vector<int32_t> c;
    if (std::find(empty.begin(), empty.end(), r) == empty.end())
      for (int j = 0; j < len; ++j) c.push_back((int32_t)(lo + 3 * r + j));
    A.row(c);
  }
  return A;
}

// Row r replaced by `len` nonzeros, columns c0, c0 + step, ...
static Mat with_row(Mat A, int64_t r, int64_t len, int32_t c0, int32_t step = 1) {
  Mat B;
  B.n = A.n;
  for (int64_t i = 0; i < A.m; ++i) {
    std::vector<int32_t> c(A.col.begin() + A.rp[i], A.col.begin() + A.rp[i + 1]);
    if (i == r) {
      c.clear();
      for (int64_t j = 0; j < len; ++j) c.push_back((int32_t)(c0 + step * j));
    }
    B.row(c);
  }
  return B;
}

// The last nonzero of the row holding nonzero k moved to (its block's first
// column) + span: the block of 256 nonzeros then spans exactly `span`.
static Mat widen_block(Mat A, int64_t k, int32_t span) {
  int64_t r = 0;
  while (A.rp[r + 1] <= k) ++r;
  const int64_t last = A.rp[r + 1] - 1, k0 = (last >> kC16Shift) << kC16Shift;
  A.col[(size_t)last] = *std::min_element(A.col.begin() + k0, A.col.begin() + last) + span;
  return A;
}

static int64_t long_nnz_of(const Mat &A, unsigned flags) {
  SplitPlan L;
  plan_split_rows(A.rp.data(), A.m, flags, L);
  return L.long_nnz;
}

static SavedTerms terms(const Mat &A, int dtype, int val_dtype, unsigned flags) {
  SavedTerms t;
  t.dtype = dtype, t.val_dtype = val_dtype;
  t.m = A.m, t.nnz = A.nnz(), t.long_nnz = long_nnz_of(A, flags);
  return t;
}

struct Dt {
  int vec, val;
};
static const Dt F64{HSPMV_F64, HSPMV_F64}, F32{HSPMV_F32, HSPMV_F32}, MIX{HSPMV_F64, HSPMV_F32};
static const int64_t kWide = 60000000;  // columns of a shard no dtype keeps resident

static int print_col16(const Mat &A, Dt dt, unsigned flags, bool taken, const Col16Plan &P, int64_t groups) {
  if (!taken) {
    printf("%s col16 taken=0 span_bits=%d\n", g_case, P.span_bits);
    return 0;
  }
  SavedTerms t = terms(A, dt.vec, dt.val, flags);
  t.n_cplanes = P.n_planes, t.groups = groups;
  printf("%s col16 taken=1 mode=%d planes=%d words=%d span_bits=%d shape=%d saved=%a off=%016llx base=%016llx "
         "planes=%016llx\n",
         g_case, P.mode, P.n_planes, P.plane_words, P.span_bits, P.shape,
         c16_saved_of(P.mode == 2 ? kFmtGroup16 : kFmtBlock16, t), fnv(P.off), fnv(P.base), fnv(P.planes));
  return 0;
}

// Block columns.  planes < 0: declined, with -1 - planes the span bits reported.
static int blocks(const std::string &name, const Mat &A, Dt dt, unsigned flags, int planes) {
  g_case = name.c_str();
  Col16Plan P;
  const int64_t nnz = A.nnz();
  const bool taken = plan_col16(A.col.data(), nnz, A.m, A.n, dt.vec, dt.val, flags, P);
  CHECK(taken == (planes >= 0));
  if (!taken) {
    CHECK(P.span_bits == -1 - planes);
    return print_col16(A, dt, flags, false, P, 0);
  }
  const int64_t nb = (nnz + 255) >> kC16Shift, nw = (nnz + 63) / 64 + 1;
  CHECK(P.mode == 1 && P.shape == 0 && P.n_planes == planes && P.plane_words == nw);
  CHECK((int64_t)P.off.size() == nnz && (int64_t)P.base.size() == nb + 1 && P.base[(size_t)nb] == 0);
  CHECK((int64_t)P.planes.size() == planes * nw);
  int64_t widest = 0;
  for (int64_t k = 0; k < nnz; ++k) {
    int64_t c = (int64_t)P.base[(size_t)(k >> kC16Shift)] + P.off[(size_t)k];
    for (int p = 0; p < planes; ++p)
      c += (int64_t)((P.planes[(size_t)(p * nw + (k >> 6))] >> (k & 63)) & 1u) << (16 + p);
    CHECK(c == A.col[(size_t)k]);
    widest = std::max(widest, c - P.base[(size_t)(k >> kC16Shift)]);
  }
  for (int p = 0; p < planes; ++p) {  // the pad word, and the bits past nnz
    CHECK(P.planes[(size_t)(p * nw + nw - 1)] == 0);
    if (nnz & 63) CHECK(P.planes[(size_t)(p * nw + (nnz >> 6))] >> (nnz & 63) == 0);
  }
  CHECK(widest >> P.span_bits == 0 && (P.span_bits == 1 || widest >> (P.span_bits - 1) == 1));
  CHECK(planes == std::max(0, P.span_bits - 16));
  return print_col16(A, dt, flags, true, P, 0);
}

// Group columns over 64-row groups (starts == nullptr) or tasks.
static int groups(const std::string &name, const Mat &A, Dt dt, unsigned flags, int mode,
                  const std::vector<int32_t> *starts, bool want) {
  g_case = name.c_str();
  Tuning tn;
  tn.col16_group = mode;
  Col16Plan P;
  const bool taken = plan_col16g(A.rp.data(), A.col.data(), A.m, A.n, dt.vec, dt.val, flags, tn, starts, P);
  CHECK(taken == want);
  if (!taken) {
    CHECK(P.span_bits == 0);
    return print_col16(A, dt, flags, false, P, 0);
  }
  const int64_t ng = starts ? (int64_t)starts->size() - 1 : (A.m + 63) / 64;
  const int32_t long_t = split_threshold(flags);
  CHECK(P.mode == 2 && P.shape == (starts ? kCsr3 : kStream) && P.n_planes == 0 && P.planes.empty());
  CHECK((int64_t)P.off.size() == A.nnz() && (int64_t)P.base.size() == ng + 1 && P.base[(size_t)ng] == 0);
  int64_t widest = 0, next = 0;
  for (int64_t g = 0; g < ng; ++g) {
    const int64_t r0 = starts ? (*starts)[(size_t)g] : 64 * g;
    const int64_t r1 = starts ? (*starts)[(size_t)g + 1] : std::min<int64_t>(A.m, 64 * g + 64);
    CHECK(r0 == next && r1 >= r0);
    next = r1;
    int64_t in_kernel = 0;
    for (int64_t r = r0; r < r1; ++r) {
      const bool split = A.rp[r + 1] - A.rp[r] > long_t;
      for (int32_t k = A.rp[r]; k < A.rp[r + 1]; ++k) {
        if (split) CHECK(P.off[(size_t)k] == 0);
        else CHECK((int64_t)P.base[(size_t)g] + P.off[(size_t)k] == A.col[(size_t)k]);
        if (!split) widest = std::max<int64_t>(widest, P.off[(size_t)k]);
        in_kernel += !split;
      }
    }
    if (in_kernel == 0) CHECK(P.base[(size_t)g] == 0);
  }
  CHECK(next == A.m);
  CHECK(widest >> P.span_bits == 0 && (P.span_bits == 1 || widest >> (P.span_bits - 1) == 1));
  return print_col16(A, dt, flags, true, P, ng);
}

// x slabs.  B = 0: declined.  x_slabs: Tuning.x_slabs (-1 off, 0 auto, else forced).
static int slabs(const std::string &name, const Mat &A, Dt dt, unsigned flags, int x_slabs, int B,
                 bool with_val = true) {
  g_case = name.c_str();
  Tuning tn;
  tn.x_slabs = x_slabs;
  const std::vector<char> v = A.values(dt.val);
  const size_t sv = dtype_size(dt.val);
  XslabPlan P;
  const bool taken = plan_xslabs(A.rp.data(), A.col.data(), with_val ? v.data() : nullptr, A.m, A.n, dt.vec,
                                 dt.val, flags, tn, P);
  CHECK(taken == (B > 0));
  if (!taken) {
    printf("%s xslabs B=0\n", g_case);
    return 0;
  }
  const int64_t m = A.m, W = (A.n + B - 1) / B;
  const int32_t long_t = split_threshold(flags);
  CHECK(P.B == B && B >= 2 && B <= 32 && (int64_t)P.rp.size() == B * (m + 1));
  auto srp = [&](int b, int64_t r) { return P.rp[(size_t)b * (size_t)(m + 1) + (size_t)r]; };
  CHECK(srp(0, 0) == 0);
  for (int b = 0; b < B; ++b) {
    if (b) CHECK(srp(b, 0) == srp(b - 1, m));
    for (int64_t r = 0; r < m; ++r) CHECK(srp(b, r) <= srp(b, r + 1));
  }
  const int64_t snnz = srp(B - 1, m);
  CHECK((int64_t)P.col.size() == std::max<int64_t>(snnz, 1) && P.val.size() == P.col.size() * sv);
  int64_t in_kernel = 0;
  for (int64_t r = 0; r < m; ++r) {
    int32_t k = A.rp[r];
    const bool split = A.rp[r + 1] - k > long_t;
    for (int b = 0; b < B; ++b) {
      if (split) CHECK(srp(b, r) == srp(b, r + 1));
      for (int32_t o = srp(b, r); o < srp(b, r + 1); ++o, ++k) {
        CHECK(k < A.rp[r + 1] && P.col[(size_t)o] == A.col[(size_t)k]);
        CHECK(P.col[(size_t)o] >= b * W && P.col[(size_t)o] < (b + 1) * W);
        CHECK(memcmp(&P.val[(size_t)o * sv], &v[(size_t)k * sv], sv) == 0);
      }
    }
    if (!split) CHECK(k == A.rp[r + 1]);
    in_kernel += split ? 0 : A.rp[r + 1] - A.rp[r];
  }
  CHECK(snnz == in_kernel);
  SavedTerms t = terms(A, dt.vec, dt.val, flags);
  t.n_slabs = P.B;
  printf("%s xslabs B=%d saved=%a rp=%016llx col=%016llx val=%016llx\n", g_case, P.B, c16_saved_of(kFmtSlabs, t),
         fnv(P.rp), fnv(P.col), fnv(P.val));
  return 0;
}

// Split rows of a matrix given by its row lengths alone.
static int split(const std::string &name, const std::vector<int32_t> &lens, unsigned flags, int n_long) {
  g_case = name.c_str();
  Mat A;
  for (int32_t l : lens) A.rp.push_back(A.rp.back() + l), ++A.m;
  SplitPlan P;
  const bool taken = plan_split_rows(A.rp.data(), A.m, flags, P);
  const int32_t long_t = split_threshold(flags);
  CHECK(taken == (n_long > 0) && (int)P.long_row.size() == n_long && P.long_t == long_t);
  CHECK(P.long_cs.size() == P.long_row.size() + 1 && P.long_cs[0] == 0);
  CHECK(P.chunk_k.size() == 2 * (size_t)P.long_cs.back());
  int64_t sum = 0, j = 0;
  for (int64_t r = 0; r < A.m; ++r) {
    if (A.rp[r + 1] - A.rp[r] <= long_t) continue;
    CHECK(j < n_long && P.long_row[(size_t)j] == r);
    int32_t k = A.rp[r];
    for (int32_t c = P.long_cs[(size_t)j]; c < P.long_cs[(size_t)j + 1]; ++c) {
      CHECK(P.chunk_k[2 * (size_t)c] == k);
      k = std::min(k + kLongChunk, A.rp[r + 1]);
      CHECK(P.chunk_k[2 * (size_t)c + 1] == k);
    }
    CHECK(k == A.rp[r + 1] && P.long_cs[(size_t)j + 1] > P.long_cs[(size_t)j]);
    sum += A.rp[r + 1] - A.rp[r];
    ++j;
  }
  CHECK(j == n_long && sum == P.long_nnz);
  SavedTerms t;  // the long rows' nonzeros leave the 16-bit columns' count
  t.m = A.m, t.nnz = A.nnz(), t.long_nnz = P.long_nnz;
  printf("%s split n_long=%d n_chunks=%d long_nnz=%lld long_t=%d saved=%a long_row=%016llx long_cs=%016llx "
         "chunk_k=%016llx\n",
         g_case, n_long, P.long_cs.back(), (long long)P.long_nnz, P.long_t, c16_saved_of(kFmtBlock16, t),
         fnv(P.long_row), fnv(P.long_cs), fnv(P.chunk_k));
  return 0;
}

// The two rules of build_row_tables.
static int rules(const std::string &name, const Mat &A, Dt dt, unsigned flags, const Tuning &tn, int serial_len,
                 bool csort) {
  g_case = name.c_str();
  const int32_t med = median_serial_len(A.rp.data(), A.m);
  const bool want = wants_csort(A.rp.data(), A.col.data(), A.m, A.n, dt.vec, dt.val, flags, tn);
  CHECK(med == serial_len && want == csort);
  printf("%s rules serial_len=%d wants_csort=%d\n", g_case, med, (int)want);
  return 0;
}

int main() {
  int bad = 0, cases = 0;
#define GO(call) (bad += (call), ++cases)
  const unsigned C16 = HSPMV_FLAG_COL16, NO16 = HSPMV_FLAG_NO_COL16, NOSPLIT = HSPMV_FLAG_NO_SPLIT;
  // ---- block columns: the base-block and plane-word edges (one plane, so
  // that the plane words are there to check)
  for (int64_t nnz : {1, 65, 129, 255, 256, 257, 513}) {
    GO(blocks("blocks_nnz" + std::to_string(nnz), chain(nnz, kWide), F64, 0, 0));
    if (nnz > 1)
      GO(blocks("blocks_plane_nnz" + std::to_string(nnz), widen_block(chain(nnz, kWide), nnz / 2 + 3, 70000), F64, 0, 1));
  }
  {
    const Mat A = chain(1000, kWide);
    GO(blocks("blocks_span65535", widen_block(A, 300, 65535), F64, 0, 0));
    GO(blocks("blocks_span65536", widen_block(A, 300, 65536), F64, 0, 1));
    const Mat two = widen_block(A, 300, 200000), eight = widen_block(A, 700, (1 << 24) - 1),
              nine = widen_block(A, 700, 1 << 24);
    GO(blocks("blocks_2planes_auto", two, F64, 0, -1 - 18));
    GO(blocks("blocks_2planes_forced", two, F64, C16, 2));
    GO(blocks("blocks_8planes_forced", eight, F32, C16, 8));
    GO(blocks("blocks_9planes_forced", nine, F64, C16, -1 - 25));
    GO(blocks("blocks_no_col16", A, F64, NO16, -1 - 10));
    GO(blocks("blocks_no_col16_forced", A, F64, NO16 | C16, -1 - 10));
    Mat R = A;  // resident: declined before the scan unless forced
    R.n = 2000000;
    GO(blocks("blocks_resident_auto", R, F64, 0, -1));
    GO(blocks("blocks_resident_forced", R, F64, C16, 0));
    Mat H = A;  // 30 M columns: 120 MB of fp32 x is resident, 240 MB of fp64 x is not
    H.n = 30000000;
    GO(blocks("blocks_x120MB_f32", H, F32, 0, -1));
    GO(blocks("blocks_x240MB_mixed", H, MIX, 0, 0));
    GO(blocks("blocks_split_row", with_row(A, 40, 5000, 1000400), F64, 0, 0));
    Mat E;
    E.n = kWide;
    E.row({});
    GO(blocks("blocks_no_nonzeros", E, F64, C16, -1));
  }
  // ---- group columns
  for (int64_t m : {1, 64, 65}) {
    const Mat A = rows_of(m, 500000, 5, 1000);
    GO(groups("groups_m" + std::to_string(m), A, F64, 0, 0, nullptr, true));
  }
  {
    const Mat A = rows_of(200, 500000, 5, 1000, {64, 65, 190});
    GO(groups("groups_span65535", with_row(A, 70, 2, 1000, 65535), F64, 0, 0, nullptr, true));
    GO(groups("groups_span65536", with_row(A, 70, 2, 1000, 65536), F64, 0, 0, nullptr, false));
    const Mat S = with_row(A, 100, 4097, 400000);  // far columns: would widen group 1 past 16 bits
    GO(groups("groups_split_row", S, F32, 0, 0, nullptr, true));
    GO(groups("groups_split_row_nosplit", S, F32, NOSPLIT, 0, nullptr, false));
    std::vector<int64_t> none;
    for (int64_t r = 64; r < 128; ++r) none.push_back(r);
    const Mat G = rows_of(200, 500000, 5, 1000, none);
    GO(groups("groups_empty_group", G, F64, 0, 0, nullptr, true));
    const std::vector<int32_t> starts = {0, 3, 67, 67, 131, 200};  // a short first task, an empty one
    GO(groups("groups_tasks", A, F64, 0, 0, &starts, true));
    GO(groups("groups_tasks_split_row", S, F64, 0, 1, &starts, true));
    GO(groups("groups_mode_off", A, F64, C16, -1, nullptr, false));
    GO(groups("groups_no_col16", A, F64, NO16, 1, nullptr, false));
    Mat Wd = A;
    Wd.n = kWide;
    GO(groups("groups_wide_auto", Wd, F64, 0, 0, nullptr, false));
    GO(groups("groups_wide_mode1", Wd, F64, 0, 1, nullptr, true));
    GO(groups("groups_wide_flag", Wd, MIX, C16, 0, nullptr, true));
    Mat H = A;
    H.n = 30000000;
    GO(groups("groups_x120MB_f32", H, F32, 0, 0, nullptr, true));
    GO(groups("groups_x240MB_mixed", H, MIX, 0, 0, nullptr, false));
    const std::vector<int32_t> no_tasks = {0};
    GO(groups("groups_no_tasks", A, F64, 0, 1, &no_tasks, false));
  }
  // ---- x slabs: rows over all of [0, n)
  {
    auto spread = [](int64_t m, int64_t n, int len) {
      Mat A;
      A.n = n;
      for (int64_t r = 0; r < m; ++r) {
        std::vector<int32_t> c;
        for (int j = 0; j < len && r % 7 != 3; ++j) c.push_back((int32_t)(((r * 13) % 11 + j * (n / len)) % n));
        std::sort(c.begin(), c.end());
        c.erase(std::unique(c.begin(), c.end()), c.end());
        A.row(c);
      }
      return A;
    };
    const Mat A = spread(150, 1001, 9);  // 1001 = 7 * 11 * 13: no multiple of 2, 3 or 32
    GO(slabs("slabs_b2_f64", A, F64, 0, 2, 2));
    GO(slabs("slabs_b3_f32", A, F32, 0, 3, 3));
    GO(slabs("slabs_b3_mixed", A, MIX, 0, 3, 3));
    GO(slabs("slabs_b40_clipped", A, F64, 0, 40, 32));
    GO(slabs("slabs_b1", A, F64, 0, 1, 0));
    GO(slabs("slabs_off", A, F64, 0, -1, 0));
    GO(slabs("slabs_n_below_b", spread(20, 2, 2), F64, 0, 3, 2));
    GO(slabs("slabs_n1", spread(20, 1, 1), F64, 0, 3, 0));
    GO(slabs("slabs_m1", spread(1, 1001, 9), F64, 0, 2, 2));
    Mat none;  // m == 0
    none.n = 1001;
    GO(slabs("slabs_no_rows", none, F64, 0, 2, 0));
    GO(slabs("slabs_all_empty", rows_of(10, 1001, 0, 0), F64, 0, 2, 2));
    GO(slabs("slabs_descending", with_row(A, 50, 4, 900, -250), F64, 0, 2, 0));
    // (unsorted inside one slab is taken: the passes only need slab order)
    GO(slabs("slabs_descending_in_slab", with_row(A, 50, 4, 400, -100), F64, 0, 2, 2));
    const Mat S = with_row(spread(150, 6000, 9), 77, 4097, 100);
    GO(slabs("slabs_split_row", S, F64, 0, 2, 2));
    GO(slabs("slabs_split_row_nosplit", S, F32, NOSPLIT, 3, 3));
    GO(slabs("slabs_no_values", A, F64, 0, 2, 0, false));
    GO(slabs("slabs_vector_kernel", A, F64, HSPMV_KERNEL_VECTOR, 2, 0));
    // the automatic rule's exits a small input reaches
    GO(slabs("slabs_auto_one_slab", A, F64, 0, 0, 0));                      // x within one slab: B = 1
    GO(slabs("slabs_auto_resident", spread(150, 400000, 9), F64, 0, 0, 0));  // B = 2; resident, x within the L2
    GO(slabs("slabs_auto_extra_cost", spread(150, kWide, 9), F64, 0, 0, 0)); // not resident; 31 extra passes
  }
  // ---- split rows
  GO(split("split_4096", {3, 4096, 0, 5}, 0, 0));
  GO(split("split_4097", {3, 4097, 0, 5}, 0, 1));
  GO(split("split_8192", {8192}, 0, 1));
  GO(split("split_8193", {1, 8193, 1}, 0, 1));
  GO(split("split_several", {5000, 2, 0, 4097, 4096, 7, 12289, 9000, 1}, 0, 4));
  GO(split("split_nosplit", {5000, 2, 0, 4097, 4096, 7, 12289, 9000, 1}, NOSPLIT, 0));
  GO(split("split_no_rows", {}, 0, 0));
  // ---- the rules
  {
    Mat A;  // lengths 0, 1, 1, 3, 40, 41: the rows of 1..40 are 1, 1, 3, 40
    A.n = 60000;
    for (int len : {0, 1, 1, 3, 40, 41}) {
      std::vector<int32_t> c;
      for (int j = 0; j < len; ++j) c.push_back((int32_t)((j * 7919 + len * 104729) % 50000));
      A.row(c);
    }
    Mat scattered;  // every 64 consecutive nonzeros on 64 distinct lines of x
    scattered.n = kWide;
    for (int r = 0; r < 64; ++r) {
      std::vector<int32_t> c;
      for (int j = 0; j < 8; ++j) c.push_back((r * 8 + j) * 100000);
      scattered.row(c);
    }
    const Mat local = chain(512, kWide);
    Tuning t0, on, off, ord, ser, rep, slab;
    on.csort = 1, off.csort = -1, ord.deterministic = 1, ser.deterministic = 3, rep.deterministic = 2;
    slab.x_slabs = 2;
    GO(rules("rules_median", A, F64, 0, t0, 1, false));
    GO(rules("rules_no_serial_rows", rows_of(5, 100, 41, 0), F64, 0, t0, 0, false));
    GO(rules("rules_median_40", rows_of(5, 100, 40, 0), F64, 0, t0, 40, false));
    GO(rules("rules_kernel_csort", local, F64, HSPMV_KERNEL_CSORT, off, 4, true));
    GO(rules("rules_csort_on", local, F32, 0, on, 4, true));
    GO(rules("rules_ordered", local, F64, HSPMV_KERNEL_CSORT, ord, 4, false));
    GO(rules("rules_serial", scattered, F64, 0, ser, 8, false));
    GO(rules("rules_mixed", scattered, MIX, HSPMV_KERNEL_CSORT, on, 8, false));
    GO(rules("rules_auto_scattered", scattered, F64, 0, t0, 8, true));
    GO(rules("rules_auto_reproducible", scattered, F64, 0, rep, 8, true));
    GO(rules("rules_auto_local", local, F64, 0, t0, 4, false));
    GO(rules("rules_auto_off", scattered, F64, 0, off, 8, false));
    GO(rules("rules_auto_slabs_forced", scattered, F64, 0, slab, 8, false));
    GO(rules("rules_auto_stream_kernel", scattered, F64, HSPMV_KERNEL_STREAM, t0, 8, false));
    Mat R = scattered;  // resident, and x of 240 KB: two reasons to stay on the row kernels
    R.n = 60000;
    for (auto &c : R.col) c %= 60000;
    GO(rules("rules_auto_resident", R, F32, 0, t0, 8, false));
  }
  // ---- every bytes-saved formula on one set of terms
  {
    SavedTerms t;
    t.dtype = HSPMV_F64, t.val_dtype = HSPMV_F32;
    t.m = 100003, t.nnz = 2700011, t.long_nnz = 12289, t.x_entries = 99991;
    t.csort_format_bytes = 31234567.0;
    t.sl_padded = 43211, t.sl_pos_bytes = 4050017, t.sl_desc_n = 1563;
    t.xd_runs_n = 7001, t.xd_entries = 160001, t.blocks = 391;
    t.groups = 1563, t.n_cplanes = 3, t.n_slabs = 5;
    printf("saved_formulas csort=%a slices=%a dict=%a group16=%a block16=%a slabs=%a col32=%a\n",
           c16_saved_of(kFmtCsort, t), c16_saved_of(kFmtSlices, t), c16_saved_of(kFmtDict, t),
           c16_saved_of(kFmtGroup16, t), c16_saved_of(kFmtBlock16, t), c16_saved_of(kFmtSlabs, t),
           c16_saved_of(kFmtCol32, t));
    ++cases;
  }
  if (bad) {
    fprintf(stderr, "row_tables_check: %d of %d cases failed\n", bad, cases);
    return 1;
  }
  printf("row_tables_check: %d cases decoded\n", cases);
  return 0;
}
