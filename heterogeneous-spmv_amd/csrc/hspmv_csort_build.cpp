// hspmv_csort_build.cpp -- host build of the column-sorted row blocks (csort.hip)
// (see hspmv_runtime.h for the split of the host runtime).
#include <string.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <vector>

#include "hspmv_runtime.h"

namespace hspmv {

// Column-sorted row blocks (csort.hip; the kernel's header says why).
// Host build: rows are cut into nnz-balanced blocks of at most
// kCsortMaxSlots - (slices) rows, about one block per CU and column part;
// every workgroup (block, part) gets the block's nonzeros whose column lies
// in its part, sorted by column, plus its share of the long-row slices
// (rows > kLongRow nonzeros, cut per part into kCsortSlice-nonzero slices
// dealt round-robin over the blocks, each an extra LDS slot).  Entries are
// padded to whole chunks of 64*U, and a chunk is closed early when its
// columns would span more than 65535 (16-bit offsets from the chunk base).
// Padding entries add 0 * x[base] to a dummy slot that is never read.
// Auto: HBM-resident matrices with irregular gathers from an x beyond the
// L1 (> 256 KiB; it replaced the x-slab rule: C5 264 -> ~110 us), unless the
// handle asks for ordered sums (deterministic = 1: the slots add in atomic
// order); deterministic = 2 builds it with fixed-point (reproducible) slots;
// HSPMV_KERNEL_CSORT forces it, Tuning.csort = -1 turns auto off,
// Tuning.csort_parts = 1/2/4 sets the column parts, csort_u = 4/8/16 the
// chunk.  The row blocks are capped by the device's LDS per workgroup.
// plan_csort builds the tables on the host, one stage per function below, in
// the order they run; upload_csort puts a plan on the device; build_csort
// asks the device for its limits and runs the two.
constexpr int32_t kCsortSlice = 2048;
// a chunk whose instructions would serialise more than this many same-slot
// lanes in all is stored slot-sorted (segmented)
constexpr int64_t kCsortSegExtra = 128;
constexpr int64_t kCsortSegHeavy = 8;  // entries of one row in a chunk that make it a run
constexpr double kPartSlack = 1.25;    // widest column part / (n / H) when balancing cost
constexpr double kSweepPerRowBlock = 0.13;  // a column's sweep cost, in entries, per row block
// Row-partition weight of crowded entries (>= 8 of one row to a chunk, so
// their chunks are segmented): c5r's hub blocks ran 96-104 us against a
// part median of 85 with the same entries and 100-160 segmented chunks
// (profiles/r04/csort_trace_wg_cost_balanced.jsonl): ~1.6x per entry.
constexpr int32_t kWUnit = 16, kWCrowded = 26;
// diagnostic builds (Tuning.csort_trace): per workgroup {rows, slices,
// chunks, entries, gather quad-sectors, gather sectors, segmented chunks,
// 0} -- the cost terms the per-workgroup timelines are compared with
constexpr int kWgStats = 8;

namespace {

struct CsEnt {
  uint32_t col, slot, k;
  bool operator<(const CsEnt &o) const {
    return col != o.col ? col < o.col : (slot != o.slot ? slot < o.slot : k < o.k);
  }
};

// the shard's host CSR
struct Csr {
  const int32_t *rp, *col;
  const void *val;
  int64_t m, n;
  int dtype;
};

// What the dtype, the knobs and the device's limits fix before a table is built.
struct Shape {
  int H = 1, U = 8;   // column parts; entries per lane and chunk
  int64_t C = 0;      // entries per chunk, 64 * U
  bool slot32 = false, wide = false;
  int64_t slot_bytes = 8;
  int32_t lds_max = 0, max_slots = 0;  // the row slots' LDS on this device
  int32_t long_t = 0;                  // rows above this many nonzeros are long rows
  int64_t nb0 = 1;                     // row blocks per column part, at most
};

Shape csort_shape(const Csr &A, unsigned flags, const Tuning &tn, const CsortLimits &lim) {
  Shape S;
  S.lds_max = lim.lds_bytes;
  if (tn.csort_lds_cap > 0) S.lds_max = std::min(S.lds_max, tn.csort_lds_cap);  // A/B
  S.slot32 = A.dtype == HSPMV_F32 && tn.csort_slot32 == 1;
  S.slot_bytes = S.slot32 ? 4 : 8;
  S.max_slots = (int32_t)(S.lds_max / S.slot_bytes) - 1;
  S.H = A.n >= 2 ? 2 : 1;
  if (tn.csort_parts == 1 || tn.csort_parts == 2 || tn.csort_parts == 4)
    S.H = (int)std::min<int64_t>(tn.csort_parts, A.n);
  S.U = A.dtype == HSPMV_F32 ? 16 : 8;
  if (tn.csort_u == 4 || tn.csort_u == 8 || tn.csort_u == 16) S.U = tn.csort_u;
  const int bpc = tn.csort_blocks_per_cu > 0 ? std::min(tn.csort_blocks_per_cu, 8) : 1;
  // 16-byte entry loads: needs U a multiple of 2 (fp32 records) / 4 (fp64 indices)
  // 16-byte entry loads + the next chunk's entries loaded during this chunk's
  // gathers: fp32 C5 107 -> 103 us, RCM'd C5 192 -> 190, in four one-process
  // A/Bs (profiles/r03/ab_c5_wide_pf*.jsonl); fp64 keeps 8-byte loads
  // (unmeasured).  Neither alone moves C5 (wide 108.8 vs 108.0, PF 109.4).
  const bool wide_default = A.dtype == HSPMV_F32;
  S.wide = (tn.csort_wide >= 0 ? tn.csort_wide == 1 : wide_default) &&
           (A.dtype == HSPMV_F32 ? S.U % 2 == 0 : S.U % 4 == 0);
  S.C = 64 * S.U;
  S.long_t = tn.csort_long > 0 && !(flags & HSPMV_FLAG_NO_SPLIT) ? tn.csort_long : split_threshold(flags);
  S.nb0 = std::max<int64_t>(1, (int64_t)lim.cus * bpc / S.H);
  return S;
}

struct ColParts {
  std::vector<int64_t> pb;   // part h: columns [pb[h], pb[h+1])
  std::vector<uint8_t> tab;  // column -> part (empty for one part)
  int of(int64_t c) const { return tab.empty() ? 0 : (int)tab[(size_t)c]; }
};

// Column parts: [pb[h], pb[h+1]).  Equal widths, or (Tuning.csort_balance
// >= 0, the default) boundaries at equal shares of the parts' COST, each
// part's width kept within kPartSlack of n / H.  A workgroup's time is
// ~alpha per entry + beta per column of its part (the x sweep): from the
// per-workgroup timelines of c5r (profiles/r04c/csort_trace_wg*.jsonl),
// alpha = 2.5e-4 us, beta = 3.0-3.4e-5 us per fp32 column, so a column
// weighs kSweepPerRowBlock * (row blocks) entries (x 2 * 8 / 12 for fp64
// x and entries).  An RCM ordering concentrates a power-law matrix's
// entries in the upper columns (c5r: 59 % in the upper half): equal widths
// gave that half's workgroups 1.42x the entries (123.4 us), equal entries
// over-corrected onto the wider lower part (108.8 us, its sweep 43 % wider).
ColParts column_parts(const Csr &A, const Shape &S, const Tuning &tn) {
  const int H = S.H;
  const int64_t n = A.n;
  ColParts P;
  P.pb.assign((size_t)H + 1, 0);
  for (int h = 0; h <= H; ++h) P.pb[(size_t)h] = (n * h + H - 1) / H;  // c in part floor(c*H/n)
  if (H > 1 && tn.csort_balance >= 0) {
    std::vector<int64_t> colcnt((size_t)n + 1, 0);
    for (int64_t k = 0; k < A.rp[A.m]; ++k) ++colcnt[(size_t)A.col[k]];
    const double wsw = tn.csort_sweep_w > 0 ? tn.csort_sweep_w : kSweepPerRowBlock;
    const double wcol = wsw * (double)S.nb0 * (A.dtype == HSPMV_F64 ? 2.0 * 8.0 / 12.0 : 1.0);
    const double tot = (double)A.rp[A.m] + wcol * (double)n;
    double acc = 0.0;
    int64_t c = 0;
    for (int h = 1; h < H; ++h) {
      const double target = tot * h / H;
      while (c < n && acc + (double)colcnt[(size_t)c] + wcol <= target) acc += (double)colcnt[(size_t)c++] + wcol;
      const int64_t eq = (n * h + H - 1) / H;
      const double ps = tn.csort_slack > 1.0 ? tn.csort_slack : kPartSlack;  // A/B knob
      const int64_t slack = (int64_t)((ps - 1.0) * (double)(n / H));
      const int64_t lo = std::max(P.pb[(size_t)h - 1] + 1, eq - slack), hi = std::max(lo, eq + slack);
      P.pb[(size_t)h] = std::min(std::max(c, lo), hi);
    }
  }
  if (H > 1) {
    P.tab.assign((size_t)n, 0);
    for (int h = 0; h < H; ++h)
      std::fill(P.tab.begin() + P.pb[(size_t)h], P.tab.begin() + P.pb[(size_t)h + 1], (uint8_t)h);
  }
  return P;
}

// long rows and their slices (per part, kCsortSlice nonzeros each)
struct LongRows {
  std::vector<int32_t> row, cs{0};             // the rows; row j's slices [cs[j], cs[j+1])
  std::vector<std::vector<uint32_t>> slice_k;  // source nonzeros per slice
  std::vector<int> slice_part;
  std::vector<int32_t> slice_row;
  int64_t n_slices() const { return (int64_t)slice_k.size(); }
};

LongRows long_rows(const Csr &A, const Shape &S, const ColParts &P) {
  LongRows L;
  for (int64_t r = 0; r < A.m; ++r) {
    const int32_t k0 = A.rp[r], k1 = A.rp[r + 1];
    if (k1 - k0 <= S.long_t) continue;
    L.row.push_back((int32_t)r);
    std::vector<std::vector<uint32_t>> byp((size_t)S.H);
    for (int32_t k = k0; k < k1; ++k) byp[(size_t)P.of(A.col[k])].push_back((uint32_t)k);
    for (int h = 0; h < S.H; ++h)
      for (size_t i = 0; i < byp[(size_t)h].size(); i += kCsortSlice) {
        const size_t e = std::min(byp[(size_t)h].size(), i + kCsortSlice);
        L.slice_k.emplace_back(byp[(size_t)h].begin() + (ptrdiff_t)i, byp[(size_t)h].begin() + (ptrdiff_t)e);
        L.slice_part.push_back(h);
        L.slice_row.push_back((int32_t)r);
      }
    L.cs.push_back((int32_t)L.slice_k.size());
  }
  return L;
}

// Reproducible (fixed-point) slots (Tuning.deterministic == 2, csort.hip
// fix_q): every value of row r is stored scaled by 2^rexp[r], exactly (a
// power of two), so that the row's |v'| < 2^-extra: rexp = -(ilogb max|v| +
// 1) - extra, extra = ceil(log2 len) - 12 for a row kept whole over 4096
// nonzeros (HSPMV_FLAG_NO_SPLIT), else 0 -- every product then rounds to an
// integer below 2^kCsortFixBits and a slot of <= 4096 of them stays below
// 2^62.  A value that the scaling takes below the type's normal range loses
// bits only below the products' rounding unit (2^-kCsortFixBits of the
// row's largest).
// A matrix with an Inf or NaN value has no fixed-point scale for its row
// (the product must stay non-finite): such a handle keeps fp64 slots and
// reports csort_fixed_point = 0, deterministic = 0.
// rexp per row and sexp per slice (its row's); false, both empty, for such a matrix.
bool row_scales(const Csr &A, int32_t long_t, const LongRows &L, std::vector<int16_t> &rexp,
                std::vector<int16_t> &sexp) {
  rexp.assign((size_t)A.m, 0);
  for (int64_t r = 0; r < A.m; ++r) {
    double mx = 0.0;
    for (int32_t k = A.rp[r]; k < A.rp[r + 1]; ++k) {
      const double v = A.dtype == HSPMV_F32 ? (double)static_cast<const float *>(A.val)[k]
                                            : static_cast<const double *>(A.val)[k];
      mx = std::max(mx, std::fabs(v));
      if (!std::isfinite(v)) {
        std::vector<int16_t>().swap(rexp);
        return false;
      }
    }
    if (!(mx > 0.0)) continue;  // empty / zero rows
    const int64_t len = A.rp[r + 1] - A.rp[r];
    int extra = 0;  // (a sliced row's slots hold kCsortSlice <= 4096 products each)
    while (len <= long_t && ((int64_t)4096 << extra) < len) ++extra;
    rexp[(size_t)r] = (int16_t)(-(std::ilogb(mx) + 1) - extra);
  }
  sexp.assign((size_t)std::max<int64_t>(L.n_slices(), 1), 0);
  for (int64_t sl = 0; sl < L.n_slices(); ++sl) sexp[(size_t)sl] = rexp[(size_t)L.slice_row[(size_t)sl]];
  return true;
}

// the (scaled) value of nonzero k of row r; rexp: null unless fixed-point
struct Values {
  const void *val;
  const int16_t *rexp;
  uint32_t f32(uint32_t k, int64_t r) const {
    float v = static_cast<const float *>(val)[k];
    if (rexp) v = std::ldexp(v, rexp[r]);
    uint32_t b;
    memcpy(&b, &v, 4);
    return b;
  }
  double f64(uint32_t k, int64_t r) const {
    const double v = static_cast<const double *>(val)[k];
    return rexp ? std::ldexp(v, rexp[r]) : v;
  }
};

// [h][r]: the partition weight of row r's in-kernel nonzeros in part h
std::vector<int32_t> row_weights(const Csr &A, const Shape &S, const ColParts &P, const Tuning &tn) {
  const int H = S.H;
  const int64_t m = A.m;
  const int32_t *rp = A.rp, *col = A.col;
  std::vector<int32_t> cnt((size_t)(H * m), 0);
  parallel_ranges(m, 65536, [&](int64_t r0, int64_t r1, int) {
    for (int64_t r = r0; r < r1; ++r) {
      if (rp[r + 1] - rp[r] > S.long_t) continue;
      for (int32_t k = rp[r]; k < rp[r + 1]; ++k) ++cnt[(size_t)(P.of(col[k]) * m + r)];
    }
  });
  // a row's partition weight (int32: a row of > 2^31 / kWCrowded entries,
  // possible only unsplit, saturates)
  auto weigh = [](int64_t plain, int64_t crowded) {
    return (int32_t)std::min<int64_t>(INT32_MAX / 2, plain * kWUnit + crowded * kWCrowded);
  };
  if (tn.csort_balance < 0) {
    for (auto &v : cnt) v = weigh(v, 0);
    return cnt;
  }
  // Crowded entries: ones with >= kCsortSegHeavy entries of the same row
  // within the columns one chunk of a block covers (cspan) -- the entries
  // that make their chunks segmented.  An RCM ordering clusters a hub
  // row's columns, so the row's whole span says little: each entry's own
  // window is counted (sorted copy of the row's part, two pointers).
  std::vector<double> cspan((size_t)H, 0.0);
  for (int h = 0; h < H; ++h) {
    int64_t tot = 0;
    for (int64_t r = 0; r < m; ++r) tot += cnt[(size_t)(h * m + r)];
    cspan[(size_t)h] =
        tot ? (double)S.C * (double)(P.pb[(size_t)h + 1] - P.pb[(size_t)h]) * (double)S.nb0 / (double)tot : 0.0;
  }
  parallel_ranges(m, 65536, [&](int64_t r0, int64_t r1, int) {
    std::vector<int32_t> cs;
    std::vector<int32_t> crowded((size_t)H);
    for (int64_t r = r0; r < r1; ++r) {
      const int32_t len = rp[r + 1] - rp[r];
      if (len > S.long_t || len < kCsortSegHeavy) {
        for (int h = 0; h < H; ++h) cnt[(size_t)(h * m + r)] = weigh(cnt[(size_t)(h * m + r)], 0);
        continue;
      }
      cs.assign(col + rp[r], col + rp[r + 1]);
      std::sort(cs.begin(), cs.end());
      std::fill(crowded.begin(), crowded.end(), 0);
      for (size_t i = 0, j = 0; i < cs.size(); ++i) {  // entries i..j-1 within cspan of cs[i]
        const int h = P.of(cs[i]);
        const double lim = (double)cs[i] + cspan[(size_t)h];
        if (j < i + 1) j = i + 1;
        while (j < cs.size() && (double)cs[j] < lim && P.of(cs[j]) == h) ++j;
        if ((int64_t)(j - i) >= kCsortSegHeavy) ++crowded[(size_t)h];
      }
      for (int h = 0; h < H; ++h) {
        const size_t i = (size_t)(h * m + r);
        const int32_t cr = std::min(cnt[i], crowded[(size_t)h]);
        cnt[i] = weigh(cnt[i] - cr, cr);
      }
    }
  });
  return cnt;
}

// Greedy cuts of the m rows weighing c[r] at `target` weight or row_cap
// rows: the number of blocks, their first rows (and m) into *out.
int64_t cut_w(const int32_t *c, int64_t m, int64_t row_cap, int64_t target, std::vector<int32_t> *out) {
  int64_t start = 0, acc = 0, nblk = 1;
  if (out) out->assign(1, 0);
  for (int64_t r = 0; r < m; ++r) {
    if (r > start && (r - start >= row_cap || acc >= target)) {
      if (out) out->push_back((int32_t)r);
      ++nblk;
      start = r;
      acc = 0;
    }
    acc += c[r];
  }
  if (out) out->push_back((int32_t)m);
  return nblk;
}

// One part's row blocks: the target is the smallest that yields at most nb0
// blocks (one block more would run a second round of workgroups on one CU
// and double the launch).
void partition_rows(const int32_t *c, int64_t m, int64_t row_cap, int64_t nb0, std::vector<int32_t> &out) {
  int64_t tot_h = 0;
  for (int64_t r = 0; r < m; ++r) tot_h += c[r];
  int64_t lo = std::max<int64_t>(1, (tot_h + nb0 - 1) / nb0), hi = std::max<int64_t>(lo, tot_h + 1);
  if (cut_w(c, m, row_cap, lo, nullptr) > nb0) {
    if (cut_w(c, m, row_cap, hi, nullptr) > nb0) lo = hi;  // the row cap alone needs more blocks
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (cut_w(c, m, row_cap, mid, nullptr) <= nb0) hi = mid; else lo = mid + 1;
    }
  }
  cut_w(c, m, row_cap, lo, &out);
}

// Row blocks PER COLUMN PART.  Part h is a fixed slice of x, [pb[h],
// pb[h+1]) (above), and workgroup j works on part
// j % H: under round-robin dispatch (workgroup j on XCD j % 8;
// tools/xcd_map_probe.hip records it per box) every XCD sweeps one slice,
// which its 4 MiB L2 keeps for all its CUs.  Each part has its OWN row
// partition, balanced on the nonzeros that fall in that part and capped in
// rows (the LDS slots), so the parts' workgroups carry equal work whatever
// the ordering: with one row partition for all parts an RCM-ordered
// power-law matrix put ~90 % of a block's entries in one part (322 us vs
// 108 us on the same matrix unordered), and quantile splits per block, which
// balance the work but let every XCD sweep all of x, still took 205 us.
// [h]: the first rows of part h's blocks, and m.
std::vector<std::vector<int32_t>> row_blocks(const Csr &A, const Shape &S, const ColParts &P, const Tuning &tn,
                                             int64_t row_cap) {
  std::vector<std::vector<int32_t>> brh((size_t)S.H);
  const std::vector<int32_t> cnt = row_weights(A, S, P, tn);  // (released on return: before the entries are sorted)
  for (int h = 0; h < S.H; ++h)
    partition_rows(cnt.data() + (size_t)h * (size_t)A.m, A.m, row_cap, S.nb0, brh[(size_t)h]);
  return brh;
}

// workgroup j: part j % H, that part's block j / H (empty past its blocks)
struct WgMap {
  std::vector<int32_t> rows;             // [2j], [2j+1]: its rows
  std::vector<std::vector<int32_t>> sl;  // its long-row slices
};

WgMap deal_workgroups(const std::vector<std::vector<int32_t>> &brh, int64_t G, int64_t m, const LongRows &L) {
  const int64_t H = (int64_t)brh.size();
  WgMap W;
  W.rows.assign((size_t)(2 * G), (int32_t)m);
  for (int64_t j = 0; j < G; ++j) {
    const auto &b = brh[(size_t)(j % H)];
    const int64_t i = j / H;
    if (i + 1 < (int64_t)b.size()) {
      W.rows[(size_t)(2 * j)] = b[(size_t)i];
      W.rows[(size_t)(2 * j + 1)] = b[(size_t)i + 1];
    }
  }
  // slices dealt round-robin over the blocks of their part
  W.sl.resize((size_t)G);
  std::vector<int64_t> next((size_t)H, 0);
  for (int64_t sl = 0; sl < L.n_slices(); ++sl) {
    const int h = L.slice_part[(size_t)sl];
    const int64_t nbh = (int64_t)brh[(size_t)h].size() - 1;
    const int64_t i = next[(size_t)h]++ % nbh;
    W.sl[(size_t)(i * H + h)].push_back((int32_t)sl);
  }
  return W;
}

// chunks of C entries, closed early when the span would pass 65535:
// emit(chunk, base column, first entry, end) for each; returns their number
template <typename F>
int64_t walk_chunks(const std::vector<CsEnt> &E, int64_t C, F &&emit) {
  int64_t i = 0, cnt = 0;
  const int64_t ne = (int64_t)E.size();
  while (i < ne) {
    const uint32_t c0 = E[(size_t)i].col;
    int64_t j = i;
    while (j < ne && j - i < C && E[(size_t)j].col - c0 <= 65535u) ++j;
    emit(cnt, c0, i, j);
    ++cnt;
    i = j;
  }
  return cnt;
}

// per workgroup: sorted entries, chunks, slots (the dummy slot included)
struct WgEntries {
  std::vector<std::vector<CsEnt>> ents;
  std::vector<int64_t> nchunks;
  std::vector<int32_t> nslots;
};

// false when a workgroup's slots pass 65536 or the LDS
bool sort_entries(const Csr &A, const Shape &S, const ColParts &P, const LongRows &L, const WgMap &W,
                  WgEntries &WE) {
  const int64_t G = (int64_t)W.sl.size();
  WE.ents.resize((size_t)G);
  WE.nchunks.assign((size_t)G, 0);
  WE.nslots.assign((size_t)G, 0);
  std::atomic<bool> too_big{false};
  parallel_ranges(G, 4, [&](int64_t b0, int64_t b1, int) {
    for (int64_t b = b0; b < b1; ++b) {
      const int h = (int)(b % S.H);
      const int32_t r0 = W.rows[(size_t)(2 * b)], r1 = W.rows[(size_t)(2 * b + 1)];
      const int32_t nr = r1 - r0;
      auto &E = WE.ents[(size_t)b];
      for (int32_t r = r0; r < r1; ++r) {
        if (A.rp[r + 1] - A.rp[r] > S.long_t) continue;
        for (int32_t k = A.rp[r]; k < A.rp[r + 1]; ++k)
          if (P.of(A.col[k]) == h) E.push_back({(uint32_t)A.col[k], (uint32_t)(r - r0), (uint32_t)k});
      }
      const auto &sl = W.sl[(size_t)b];
      for (size_t v = 0; v < sl.size(); ++v)
        for (uint32_t k : L.slice_k[(size_t)sl[v]])
          E.push_back({(uint32_t)A.col[k], (uint32_t)(nr + (int32_t)v), k});
      std::sort(E.begin(), E.end());
      const int32_t ns = nr + (int32_t)sl.size() + 1;  // + the dummy slot
      WE.nslots[(size_t)b] = ns;
      if (ns > 65536 || ((int64_t)ns + 1) * S.slot_bytes > S.lds_max) too_big = true;
      WE.nchunks[(size_t)b] = walk_chunks(E, S.C, [](int64_t, uint32_t, int64_t, int64_t) {});
    }
  });
  return !too_big;
}

// blk_c, blk_v, vslice, the chunk total and the LDS of the largest
// workgroup; false when the chunks pass the kernel's index types
bool table_ranges(const Shape &S, const WgMap &W, const WgEntries &WE, CsortPlan &P) {
  const size_t G = W.sl.size();
  P.blk_c.assign(G + 1, 0);
  P.blk_v.assign(G + 1, 0);
  int64_t tot_chunks = 0;
  int32_t max_slots_used = 1;
  for (size_t b = 0; b < G; ++b) {
    P.blk_c[b] = (int32_t)tot_chunks;
    tot_chunks += WE.nchunks[b];
    P.blk_v[b] = (int32_t)P.vslice.size();
    for (int32_t sl : W.sl[b]) P.vslice.push_back(sl);
    max_slots_used = std::max(max_slots_used, WE.nslots[b]);
  }
  P.blk_c[G] = (int32_t)tot_chunks;
  P.blk_v[G] = (int32_t)P.vslice.size();
  P.chunks = tot_chunks;
  P.lds_bytes = (int32_t)(S.slot_bytes * max_slots_used);
  return tot_chunks * S.C < (int64_t)1 << 40 && tot_chunks < INT32_MAX;
}

// Same-slot lanes in one instruction serialise the LDS atomics: an RCM
// ordering puts a hub row's entries on contiguous columns, so column order
// can give one instruction 64 lanes of one row (RCM power-law: a few
// workgroups with ~100 K serialised lanes set the launch's tail, 204 vs
// 108 us).  Such chunks are stored sorted by slot instead and flagged (bit
// 31 of the base): the kernel sums each instruction's runs first (segmented
// scan).  Is the chunk e[0, ne) one of them?
bool chunk_segmented(const CsEnt *e, int64_t ne, const Tuning &tn) {
  if (tn.csort_seg == 0) return false;
  if (tn.csort_seg == 2) return true;
  uint32_t sl64[64];
  int64_t extra = 0;
  for (int64_t g = 0; g < ne; g += 64) {
    const int64_t w = std::min<int64_t>(64, ne - g);
    for (int64_t t = 0; t < w; ++t) sl64[t] = e[g + t].slot;
    std::sort(sl64, sl64 + w);
    int run = 1, mx = 1;
    for (int64_t t = 1; t < w; ++t) {
      run = sl64[t] == sl64[t - 1] ? run + 1 : 1;
      mx = std::max(mx, run);
    }
    extra += mx - 1;
  }
  return extra > (tn.csort_seg_extra > 0 ? tn.csort_seg_extra : kCsortSegExtra);
}

// The segmented order of the chunk e[0, ne) into out: the crowded rows (>=
// kCsortSegHeavy entries in this chunk; `all`: every row) first,
// slot-sorted, in column order within each: their runs are contiguous
// columns (coalesced gathers); the other entries after them, still in
// column order.
void segmented_order(const CsEnt *e, int64_t ne, bool all, std::vector<CsEnt> &out) {
  std::vector<uint32_t> slots((size_t)ne), heavy;
  for (int64_t t = 0; t < ne; ++t) slots[(size_t)t] = e[t].slot;
  std::sort(slots.begin(), slots.end());
  for (size_t t = 0; t < slots.size();) {
    size_t end = t;
    while (end < slots.size() && slots[end] == slots[t]) ++end;
    if ((int64_t)(end - t) >= kCsortSegHeavy || all) heavy.push_back(slots[t]);
    t = end;
  }
  auto is_heavy = [&](uint32_t sl) { return std::binary_search(heavy.begin(), heavy.end(), sl); };
  out.clear();
  for (int64_t t = 0; t < ne; ++t)
    if (is_heavy(e[t].slot)) out.push_back(e[t]);
  std::stable_sort(out.begin(), out.end(), [](const CsEnt &a, const CsEnt &b) { return a.slot < b.slot; });
  for (int64_t t = 0; t < ne; ++t)
    if (!is_heavy(e[t].slot)) out.push_back(e[t]);
}

// entry q of a chunk (lane q % 64, u = q / 64) is stored at q, or, for
// 16-byte loads, interleaved so that one load brings the lane entries u,
// u+1 (fp32 records, fp64 values: per = 2) or u..u+3 (fp64 indices: per = 4)
inline int64_t at(bool wide, int64_t q, int per) {
  if (!wide) return q;
  const int64_t u = q / 64, lane = q % 64;
  return (u / per) * (64 * per) + lane * per + (u % per);
}

// the gather cost terms of one chunk (w[4], w[5] of its workgroup's kWgStats)
void gather_stats(const CsEnt *src, int64_t ne, uint32_t c0, int64_t C, int sec_shift, int64_t *w) {
  for (int64_t g = 0; g < C; g += 64) {  // one gather instruction
    uint32_t sec[64];
    for (int64_t q = 0; q < 64; ++q) sec[q] = (g + q < ne ? src[g + q].col : c0) >> sec_shift;
    for (int64_t q = 0; q < 64; q += 4) {  // the L1 serves each quad on its own
      int d = 1;
      for (int t = 1; t < 4; ++t) {
        bool seen = false;
        for (int t2 = 0; t2 < t; ++t2) seen |= sec[q + t] == sec[q + t2];
        d += seen ? 0 : 1;
      }
      w[4] += d;
    }
    std::sort(sec, sec + 64);
    w[5] += (int64_t)(std::unique(sec, sec + 64) - sec);
  }
}

// the slots of one workgroup: its rows, then its slices, then the dummy
struct WgSlots {
  int32_t r0, nr;
  const int32_t *sl, *slice_row;
  uint32_t dummy;
  int64_t row_of(uint32_t slot) const {  // source row of a slot (fixed-point scale)
    return (int32_t)slot < nr ? (int64_t)r0 + slot : slice_row[sl[slot - nr]];
  }
};

// the ne entries src of chunk ch, based at column c0, into the entry stream
// (and, for an updatable handle, their CSR indices into P.src, at the
// positions of their values)
void store_chunk(int64_t ch, uint32_t c0, const CsEnt *src, int64_t ne, const Shape &S, const WgSlots &ws,
                 const Values &V, CsortPlan &P) {
  const bool f32 = P.dtype == HSPMV_F32;
  for (int64_t q = 0; q < S.C; ++q) {  // lanes >= ne: padding (gathers x[base])
    uint32_t ix = ws.dummy << 16;      // padding: 0 * x[base] into the dummy slot
    if (q < ne) ix = (src[q].slot << 16) | (src[q].col - c0);
    if (!P.src.empty()) P.src[(size_t)(ch * S.C + at(S.wide, q, 2))] = q < ne ? src[q].k : kCsortSrcPad;
    if (f32) {
      const uint32_t vb = q < ne ? V.f32(src[q].k, ws.row_of(src[q].slot)) : 0;
      P.rec[(size_t)(ch * S.C + at(S.wide, q, 2))] = ((uint64_t)vb << 32) | ix;
    } else {
      if (q < ne) P.val64[(size_t)(ch * S.C + at(S.wide, q, 2))] = V.f64(src[q].k, ws.row_of(src[q].slot));
      P.idx[(size_t)(ch * S.C + at(S.wide, q, 4))] = ix;
    }
  }
}

// Chunk encoding: cbase and the entry stream of every workgroup (blk_c and
// the chunk total are set), the segmented-chunk count and, when asked, the
// workgroups' statistics.
// Releases each workgroup's sorted entries as soon as they are stored.
void encode_chunks(const Shape &S, const Tuning &tn, const LongRows &L, const WgMap &W, const Values &V,
                   WgEntries &WE, CsortPlan &P) {
  const int64_t G = (int64_t)W.sl.size(), tot = P.chunks * S.C;
  const bool stats = tn.csort_trace == 1;
  P.cbase.assign((size_t)std::max<int64_t>(P.chunks, 1), 0);
  if (P.dtype == HSPMV_F32)
    P.rec.assign((size_t)tot, 0);
  else {
    P.idx.assign((size_t)tot, 0);
    P.val64.assign((size_t)tot, 0.0);
  }
  if (tn.csort_src == 1) P.src.assign((size_t)std::max<int64_t>(tot, 1), kCsortSrcPad);
  if (stats) P.wg_stats.assign((size_t)(kWgStats * G), 0);
  const int sec_shift = P.dtype == HSPMV_F32 ? 3 : 2;  // x entries per 32-byte sector: 8 / 4
  std::atomic<int64_t> n_seg{0};  // chunks stored slot-sorted (segmented)
  parallel_ranges(G, 4, [&](int64_t b0, int64_t b1, int) {
    std::vector<CsEnt> tmp;
    for (int64_t b = b0; b < b1; ++b) {
      auto &E = WE.ents[(size_t)b];
      const int32_t r0 = W.rows[(size_t)(2 * b)];
      const WgSlots ws{r0, W.rows[(size_t)(2 * b + 1)] - r0, W.sl[(size_t)b].data(), L.slice_row.data(),
                       (uint32_t)(WE.nslots[(size_t)b] - 1)};
      int64_t *w = stats ? P.wg_stats.data() + kWgStats * b : nullptr;
      if (w) {
        w[0] = ws.nr;
        w[1] = (int64_t)W.sl[(size_t)b].size();
      }
      walk_chunks(E, S.C, [&](int64_t ci, uint32_t c0, int64_t i, int64_t j) {
        const int64_t ch = P.blk_c[(size_t)b] + ci, ne = j - i;
        const CsEnt *src = E.data() + i;
        const bool seg = chunk_segmented(src, ne, tn);
        if (seg) {
          segmented_order(src, ne, tn.csort_seg == 2, tmp);
          src = tmp.data();
          n_seg.fetch_add(1, std::memory_order_relaxed);
        }
        P.cbase[(size_t)ch] = (int32_t)(c0 | (seg ? 0x80000000u : 0u));
        if (w) {
          w[2] += 1;
          w[3] += ne;
          w[6] += seg ? 1 : 0;
          gather_stats(src, ne, c0, S.C, sec_shift, w);
        }
        store_chunk(ch, c0, src, ne, S, ws, V, P);
      });
      std::vector<CsEnt>().swap(E);
    }
  });
  P.seg_chunks = n_seg.load();
}

// The launch's flags, the device-only arrays' sizes and the bytes moved
// (the plan's shape -- m, n, dtype, H, n_wg, n_long, fixed, chunks -- is set).
void plan_scalars(const Shape &S, const Tuning &tn, int64_t n_slices, CsortPlan &P) {
  const bool f32 = P.dtype == HSPMV_F32;
  P.u = S.U;
  P.direct = P.H == 1 && P.n_long == 0;
  P.nontemporal = true;  // the entry stream is read once; keep x in the caches
  if (tn.csort_nt >= 0) P.nontemporal = tn.csort_nt != 0;  // A/B knobs
  P.prefetch = S.wide && f32;  // see `wide` (csort_shape)
  if (tn.csort_pf >= 0) P.prefetch = tn.csort_pf != 0;
  P.slot32 = S.slot32;
  P.wide = S.wide;
  // Row partials: fp32 for fp32 data (part32, the default since r06; the
  // LDS slots stay fp64 and the finishing pass adds in fp64): half of C5's
  // 64 MB of partial traffic, C5 98.2 -> 91.9 us, c5r 99.2 -> 94.5 (t_min,
  // one process, profiles/r05q1/ab_part32.jsonl).  y then rounds twice on
  // rows with entries in both column parts (the part's sum, then y):
  // |y - y64| <= 2^-24 (sum_h |p_h| + |y64|), inside omp_spmv's own fp32
  // error (len + 2) 2^-23 sum|a x| (tests/test_gpu_parity.py).  Tuning
  // csort_part32 = 0 keeps fp64 partials (A/B).
  P.part32 = f32 && !S.slot32 && tn.csort_part32 != 0;
  // waves claim chunks from the workgroup's LDS queue: one process, 7
  // rounds (profiles/r05c/ab_csort_dyn.jsonl): C5 106.9 -> 101.9 us median,
  // c5r 107.3 -> 104.9, fp64 C5 flat (175.7 -> 174.7)
  P.dyn = tn.csort_dyn != 0;
  P.fin_rows = tn.csort_fin_rows;
  // (An in-launch combine -- write-through partials, an arrival counter per
  // row block, the last arriver adding the parts -- measured slower than
  // the finishing launch: C5 114.8 vs 107.3 us, profiles/r02s_*.)
  if (!P.direct) {
    P.part_bytes = (P.part32 ? 4 : (size_t)S.slot_bytes) * (size_t)P.H * (size_t)P.m;
    P.spart_bytes = (size_t)S.slot_bytes * (size_t)std::max<int64_t>(n_slices, 1);
  }
  if (P.fixed) {  // the x-exponent pre-pass: one block per 8192 entries of x, at most kCsortXexpBlocks
    P.n_xexp = (int32_t)std::min<int64_t>(kCsortXexpBlocks,
                                          std::max<int64_t>(1, (P.n + kCsortXexpChunk - 1) / kCsortXexpChunk));
    P.xexp_part_bytes = 4 * (size_t)P.n_xexp;
  }
  if (tn.csort_trace == 1) P.trace_bytes = 8 * kCsortTraceSlots * (size_t)P.n_wg;
  // bytes moved: the entry stream + chunk bases + the partial sums written
  // and read back + y (upload_csort adds x: the shard's distinct columns)
  const double sv = (double)dtype_size(P.dtype), tot = (double)P.chunks * (double)S.C;
  const double part_traffic =
      P.direct ? 0.0 : 2.0 * ((double)P.part_bytes + (double)S.slot_bytes * (double)n_slices);
  // (fixed-point: + the x exponent's read of x and the row scales)
  const double fix_traffic = P.fixed ? (double)P.n * sv + 2.0 * (double)P.H * (double)P.m : 0.0;
  P.format_bytes = tot * (4.0 + sv) + 4.0 * (double)P.chunks + part_traffic + sv * (double)P.m + fix_traffic;
}

}  // namespace

bool plan_csort(const int32_t *rp, const int32_t *col, const void *val, int64_t m, int64_t n, int dtype,
                unsigned flags, const Tuning &tn, const CsortLimits &lim, CsortPlan &P) {
  if (m == 0 || n == 0 || !val) return false;
  P = CsortPlan();
  P.m = m;
  P.n = n;
  P.dtype = dtype;
  const Csr A{rp, col, val, m, n, dtype};
  const Shape S = csort_shape(A, flags, tn, lim);
  P.long_t = S.long_t;
  const ColParts parts = column_parts(A, S, tn);
  const LongRows L = long_rows(A, S, parts);
  P.fixed = tn.deterministic == 2 && !S.slot32 && row_scales(A, S.long_t, L, P.rexp, P.sexp);
  const int64_t reserve = L.n_slices() / S.nb0 + 2;
  const int64_t row_cap = S.max_slots - 1 - reserve;
  if (row_cap < 64) return false;  // too many slices for the LDS: not this path
  const std::vector<std::vector<int32_t>> brh = row_blocks(A, S, parts, tn, row_cap);
  int64_t NB = 0;
  for (const auto &b : brh) NB = std::max<int64_t>(NB, (int64_t)b.size() - 1);
  const int64_t G = NB * S.H;
  if (G >= INT32_MAX) return false;
  P.n_wg = (int32_t)G;
  P.H = S.H;
  P.row_blocks = (int32_t)NB;
  const WgMap W = deal_workgroups(brh, G, m, L);
  WgEntries WE;
  if (!sort_entries(A, S, parts, L, W, WE)) return false;
  if (!table_ranges(S, W, WE, P)) return false;
  encode_chunks(S, tn, L, W, Values{val, P.fixed ? P.rexp.data() : nullptr}, WE, P);
  P.blk_r = W.rows;
  P.n_long = (int32_t)L.row.size();
  if (P.n_long) {
    P.long_mask.assign((size_t)((m + 31) / 32), 0u);
    for (int32_t r : L.row) P.long_mask[(size_t)r >> 5] |= 1u << (r & 31);
    P.long_row = L.row;
    P.long_cs = L.cs;
  }
  for (int h = 0; h < S.H; ++h) P.part_begin[h] = parts.pb[(size_t)h];
  plan_scalars(S, tn, L.n_slices(), P);
  return true;
}

int upload_csort(Shard &s, const CsortPlan &P) {
  int rc;
  // the tables go straight into the launch description (s.dev owns them)
  DevCsort &c = s.built.cs;
  c = DevCsort();
  auto up = [&](auto **d, const auto &h) -> int {
    using E = typename std::decay_t<decltype(h)>::value_type;
    if (h.empty()) return s.dev.alloc(d, sizeof(E));  // one element's room, as for a size of 1
    return s.dev.upload(d, h.data(), sizeof(E) * h.size());
  };
  if ((rc = up(&c.blk_c, P.blk_c)) || (rc = up(&c.blk_r, P.blk_r)) || (rc = up(&c.blk_v, P.blk_v)) ||
      (rc = up(&c.vslice, P.vslice)) || (rc = up(&c.cbase, P.cbase)))
    return rc;
  if (P.dtype == HSPMV_F32) {
    if ((rc = up(&c.ent, P.rec))) return rc;
  } else {
    if ((rc = up(&c.ent, P.idx)) || (rc = up(&c.val, P.val64))) return rc;
  }
  if (!P.direct && ((rc = s.dev.alloc(&c.part, P.part_bytes)) || (rc = s.dev.alloc(&c.spart, P.spart_bytes))))
    return rc;
  if (P.n_long && ((rc = up(&c.long_mask, P.long_mask)) || (rc = up(&c.long_row, P.long_row)) ||
                   (rc = up(&c.long_cs, P.long_cs))))
    return rc;
  if (P.fixed && ((rc = up(&c.rexp, P.rexp)) || (rc = up(&c.sexp, P.sexp)) ||
                  (rc = s.dev.alloc(&c.xexp_part, P.xexp_part_bytes))))
    return rc;
  if (P.trace_bytes && (rc = s.dev.alloc(&c.trace, P.trace_bytes))) return rc;
  if (!P.src.empty() && (rc = up(&c.src, P.src))) return rc;  // updatable handles: 4 B per padded entry
  c.chunks = P.chunks;
  c.n_slices = P.long_cs.empty() ? 0 : P.long_cs.back();
  c.long_t = P.long_t;
  c.n_wg = P.n_wg;
  c.H = P.H;
  c.u = P.u;
  c.direct = P.direct ? 1 : 0;
  c.n_long = P.n_long;
  c.nontemporal = P.nontemporal;
  c.prefetch = P.prefetch;
  c.slot32 = P.slot32;
  c.part32 = P.part32;
  c.wide = P.wide;
  c.dyn = P.dyn;
  c.fixed = P.fixed;
  c.fin_rows = P.fin_rows;
  c.n_xexp = P.n_xexp;
  c.n_x = P.n;
  c.m = P.m;
  c.lds_bytes = P.lds_bytes;
  c.row_blocks = P.row_blocks;
  s.csort_chunks = P.chunks;
  s.csort_seg_chunks = P.seg_chunks;
  s.csort_wg_stats = P.wg_stats;
  for (int h = 0; h < 4; ++h) s.csort_part_begin[h] = P.part_begin[h];
  s.saved.csort_format_bytes = P.format_bytes + (double)s.x_entries * (double)dtype_size(P.dtype);
  s.A.has_csort = true;
  return HSPMV_OK;
}

int build_csort(Shard &s, const int32_t *rp, const int32_t *col, const void *val, int64_t m, int64_t n,
                int dtype, unsigned flags) {
  CsortLimits lim{0, 0};
  if (hipDeviceGetAttribute(&lim.cus, hipDeviceAttributeMultiprocessorCount, s.dev.device) != hipSuccess ||
      lim.cus <= 0)
    lim.cus = 256;
  int lds_max = 0;  // the row slots must fit one workgroup's LDS on THIS device
  if (hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, s.dev.device) != hipSuccess ||
      lds_max <= 0)
    return HSPMV_OK;
  lim.lds_bytes = std::min(lds_max, kCsortMaxLds) - kCsortStaticLds;
  CsortPlan P;
  if (!plan_csort(rp, col, val, m, n, dtype, flags, s.tune, lim, P)) return HSPMV_OK;
  return upload_csort(s, P);
}

}  // namespace hspmv
