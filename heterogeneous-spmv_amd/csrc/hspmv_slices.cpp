// hspmv_slices.cpp -- row slices: the dictionary handles' matrix stored per
// 64-row wave task column-major, for the lane-per-row kernel
// (see hspmv_runtime.h for the split of the host runtime).
#include <string.h>

#include <algorithm>
#include <cstddef>
#include <vector>

#include "hspmv_runtime.h"

namespace hspmv {

// Row slices.  A handle with block x dictionaries whose in-kernel rows are
// all summed serially (<= kSerialMax / kSerialMaxF32 nonzeros) needs no
// product buffer: lane i of the wave that owns a task can walk row i itself,
// left to right, if the task's nonzeros are stored slot by slot ("sliced
// ELL").  Per wave task s (<= 64 rows, w_s = its longest row) the format holds
//   values     64 * w_s elements: slots in groups of 16 bytes per lane (2 fp64
//              / 4 fp32 consecutive slots of the lane's row, lane-major inside
//              the group: one wave load is 1 KiB contiguous), then the w_s mod
//              2 (4) last slots as single 64-lane columns; 0 past a row's end;
//   positions  the dictionary positions (plan_xdict's 16-bit positions) in
//              groups of 4 per lane (8 bytes), then the w_s mod 4 last slots
//              as single columns; 0 past a row's end;
//   lengths    one uint8 per row;
//   descriptor {prefix, first row} per task, prefix = sum of w over the
//              earlier tasks: slot k of slice s starts at element 64 * (prefix
//              + k) of both streams, so every slice is 128-byte aligned in
//              both.  A closing pair {sum of w, m} bounds the last task.
// Rows are padded to their slice's longest row only (no alignment slots), and
// the kernel masks the padding by the row length.
//
// That is the plan (build_slices, hspmv_slices_plan: the host view, in slot
// order).  The device reads the positions packed (pack_slice_pos): when every
// position of the handle is below 4096 -- every block dictionary holds at
// most 4096 entries -- the floor(w / 8) whole 8-slot groups of a slice take 12
// bytes per lane (eight 12-bit fields, little-endian in three dwords,
// lane-major inside the group: one wave load is 768 contiguous bytes), and
// the w mod 8 last slots stay 16-bit exactly as above (one 8-byte group when
// w mod 8 >= 4, then single columns).  A slice's positions then take 128 * (6
// floor(w / 8) + w mod 8) bytes, still 128-byte aligned, and start at 128 *
// pos_prefix[s] bytes: a second prefix table beside the descriptors, which
// stay as they are.  A handle with a larger dictionary, or one whose slices
// are too narrow for the packing to pay for that table, keeps the 16-bit
// stream (pos_prefix = the descriptors' prefix, not uploaded).
//
// Eligible (slices_why == HSPMV_SLICES_OK): dictionaries over the CSR3
// aligned plan's tasks or STREAM's 64-row groups, no split rows, every row
// within the vector dtype's serial bound (a mixed handle: fp64's 40), and the slice format's bytes per SpMV not
// above the CSR-order format's -- padded * (sv + 2) + m + 8 * (tasks + 1)
// against nnz * (sv + 2) + 4 * (m + 1); the rest (run records, staged x, y) is
// common; sv is the stored values' size (a mixed handle: 4).  A request for the chunked kernel's own knobs (HSPMV_U,
// HSPMV_FLAG_PREFETCH, deterministic = 3) keeps that kernel.  Auto
// (row_slices = 0) also asks for a matrix that streams from HBM, the
// dictionaries' own rule.  The two rules about speed -- the bytes and the HBM
// residence -- are auto's: row_slices = 1 takes every handle the kernel can
// run (a small matrix whose boundary rows or short last slice pad it past
// the CSR order's bytes: stencil27(21) pads 10 %), with the same y.

std::vector<int32_t> slice_starts(int kern, int64_t m, const std::vector<int32_t> &tasks) {
  if (kern == kCsr3) return tasks;
  std::vector<int32_t> st;
  for (int64_t r = 0; r < m; r += 64) st.push_back((int32_t)r);
  if (st.empty()) st.push_back(0);
  st.push_back((int32_t)m);
  return st;
}

int slices_why(const Tuning &t, unsigned flags, int kern, int W, const int32_t *rp, int64_t m,
               int64_t n, int dtype, int val_dtype, const std::vector<int32_t> &starts, SliceCounts *out) {
  SliceCounts c;
  c.n_desc = (int64_t)starts.size() - 1;
  for (int64_t s = 0; s < c.n_desc; ++s) {
    const int32_t a = starts[(size_t)s], b = starts[(size_t)s + 1];
    int32_t w = 0;
    for (int32_t r = a; r < b; ++r) w = std::max(w, rp[r + 1] - rp[r]);
    c.n_slices += b > a ? 1 : 0;
    c.max_rows = std::max<int64_t>(c.max_rows, b - a);
    c.max_len = std::max<int64_t>(c.max_len, w);
    c.padded += w;
  }
  if (out) *out = c;
  if (t.row_slices < 0) return HSPMV_SLICES_OFF;
  if (t.x_dict < 0 || (flags & HSPMV_FLAG_NO_COL16)) return HSPMV_SLICES_NO_DICT;
  if (kern == kCsr3) {
    if (t.csr3_plan == HSPMV_CSR3_PLAN_PACKED || t.csr3_plan == HSPMV_CSR3_PLAN_SSR || W != 4)
      return HSPMV_SLICES_SHAPE;
  } else if (kern != kStream || flag_groups(flags) > 1) {
    return HSPMV_SLICES_SHAPE;
  }
  if (c.max_rows > 64) return HSPMV_SLICES_SHAPE;
  if (flag_u(flags) || (flags & HSPMV_FLAG_PREFETCH) ||
      t.deterministic == HSPMV_DETERMINISTIC_SERIAL || t.serial_max > 0)
    return HSPMV_SLICES_CHUNKED;
  if (c.max_len > split_threshold(flags)) return HSPMV_SLICES_SPLIT_ROWS;
  if (c.max_len > (dtype == HSPMV_F32 ? kSerialMaxF32 : kSerialMax)) return HSPMV_SLICES_LONG_ROW;
  const double sv = (double)dtype_size(val_dtype);
  const double nnz = (double)rp[m];
  if (t.row_slices == 0 &&
      64.0 * (double)c.padded * (sv + 2.0) + (double)m + 8.0 * (double)(c.n_desc + 1) >
          nnz * (sv + 2.0) + 4.0 * (double)(m + 1))
    return HSPMV_SLICES_BYTES;
  if (t.row_slices == 0 && mall_resident(m, n, rp[m], dtype, val_dtype)) return HSPMV_SLICES_RESIDENT;
  return HSPMV_SLICES_OK;
}

// Element of slot k of lane i in a slice of width w that starts at element
// `base`; G slots per group.
static inline size_t slot_at(size_t base, int32_t w, int32_t k, int i, int G) {
  const int32_t wg = w / G * G;
  return k < wg ? base + (size_t)(k / G) * 64 * G + (size_t)i * G + (size_t)(k % G)
                : base + (size_t)k * 64 + (size_t)i;
}

void build_slices(const int32_t *rp, const uint16_t *pos, const void *val, int64_t m, int val_dtype,
                  const std::vector<int32_t> &starts, SlicePlan &P) {
  const int64_t nd = (int64_t)starts.size() - 1;
  const size_t sv = dtype_size(val_dtype);
  const int G = 16 / (int)sv;
  P.desc.assign(2 * (size_t)(nd + 1), 0);
  int64_t pre = 0;
  for (int64_t s = 0; s < nd; ++s) {
    int32_t w = 0;
    for (int32_t r = starts[(size_t)s]; r < starts[(size_t)s + 1]; ++r) w = std::max(w, rp[r + 1] - rp[r]);
    P.desc[2 * (size_t)s] = (int32_t)pre;
    P.desc[2 * (size_t)s + 1] = starts[(size_t)s];
    pre += w;
  }
  P.desc[2 * (size_t)nd] = (int32_t)pre;
  P.desc[2 * (size_t)nd + 1] = (int32_t)m;
  P.padded = pre;
  P.len.assign((size_t)std::max<int64_t>(m, 1), 0);
  for (int64_t r = 0; r < m; ++r) P.len[(size_t)r] = (uint8_t)(rp[r + 1] - rp[r]);
  P.pos.assign((size_t)std::max<int64_t>(64 * pre, 1), 0);
  P.val.assign(sv * (size_t)std::max<int64_t>(64 * pre, 1), 0);
  parallel_ranges(nd, 256, [&](int64_t s0, int64_t s1, int) {
    for (int64_t s = s0; s < s1; ++s) {
      const int32_t a = starts[(size_t)s], b = starts[(size_t)s + 1];
      const size_t base = 64 * (size_t)P.desc[2 * (size_t)s];
      const int32_t w = P.desc[2 * (size_t)s + 2] - P.desc[2 * (size_t)s];
      for (int32_t r = a; r < b; ++r)
        for (int32_t k = 0; k < rp[r + 1] - rp[r]; ++k) {
          const size_t src = (size_t)rp[r] + (size_t)k;
          P.pos[slot_at(base, w, k, r - a, 4)] = pos[src];
          memcpy(P.val.data() + sv * slot_at(base, w, k, r - a, G), (const char *)val + sv * src, sv);
        }
    }
  });
}

// 128-byte units of a slice of width w in the position stream.
static inline int64_t pos_units(int32_t w, int bits) { return bits == 12 ? 6 * (w / 8) + w % 8 : w; }

// 12 when every position of the plan fits 12 bits and the packed stream with
// its prefix table is the smaller one (slices under 8 slots wide pack nothing:
// such a handle keeps the 16-bit stream and no second table), else 16.
static int slice_pos_bits(const int32_t *desc, int64_t nd, const uint16_t *pos) {
  const int64_t n = 64 * (int64_t)desc[2 * nd];
  uint16_t top = 0;
  for (int64_t i = 0; i < n; ++i) top = std::max(top, pos[i]);
  int64_t units12 = 0;
  for (int64_t s = 0; s < nd; ++s) units12 += pos_units(desc[2 * s + 2] - desc[2 * s], 12);
  return top < 4096 && 128 * units12 + 4 * (nd + 1) < 2 * n ? 12 : 16;
}

// The device position stream of a plan (desc, pos): prefix[s] = slice s's
// start in 128-byte units (nd + 1 entries) and, when out is given, the
// stream itself, 128 * prefix[nd] bytes.
static void pack_slice_pos(const int32_t *desc, int64_t nd, const uint16_t *pos, int bits, int32_t *prefix,
                    unsigned char *out) {
  int64_t pre = 0;
  for (int64_t s = 0; s < nd; ++s) {
    prefix[s] = (int32_t)pre;
    pre += pos_units(desc[2 * s + 2] - desc[2 * s], bits);
  }
  prefix[nd] = (int32_t)pre;
  if (!out) return;
  if (bits != 12) {
    memcpy(out, pos, 128 * (size_t)pre);
    return;
  }
  parallel_ranges(nd, 256, [&](int64_t s0, int64_t s1, int) {
    for (int64_t s = s0; s < s1; ++s) {
      const size_t base = 64 * (size_t)desc[2 * s];
      const int32_t w = desc[2 * s + 2] - desc[2 * s], w8 = w / 8 * 8;
      unsigned char *dst = out + 128 * (size_t)prefix[s];
      for (int32_t g = 0; g < w / 8; ++g)
        for (int i = 0; i < 64; ++i) {
          uint64_t p[8];
          for (int e = 0; e < 8; ++e) p[e] = pos[slot_at(base, w, 8 * g + e, i, 4)];
          const uint64_t lo = p[0] | p[1] << 12 | p[2] << 24 | p[3] << 36 | p[4] << 48 | p[5] << 60;
          const uint32_t d[3] = {(uint32_t)lo, (uint32_t)(lo >> 32),
                                 (uint32_t)(p[5] >> 4 | p[6] << 8 | p[7] << 20)};
          memcpy(dst + 768 * (size_t)g + 12 * (size_t)i, d, 12);
        }
      // the w mod 8 last slots: the 16-bit layout of a slice of that width
      for (int32_t k = w8; k < w; ++k)
        for (int i = 0; i < 64; ++i) {
          const uint16_t v = pos[slot_at(base, w, k, i, 4)];
          memcpy(dst + 96 * (size_t)w8 + 2 * slot_at(0, w - w8, k - w8, i, 4), &v, 2);
        }
    }
  });
}

int upload_slices(Shard &s, const SlicePlan &P) {
  DevSlices &d = s.built.sl;
  int rc;
  const int64_t nd = (int64_t)P.desc.size() / 2 - 1;
  int32_t bits = 0;
  int64_t stream = 0;
  if ((rc = hspmv_slices_pack(nd, P.desc.data(), P.pos.data(), &bits, &stream, nullptr, nullptr))) return rc;
  size_t pos_bytes = 2 * P.pos.size(), table_bytes = 0;
  if (bits == 12) {
    std::vector<int32_t> prefix((size_t)nd + 1);
    // 16 bytes past the stream: a 12-byte load widened to 16 stays inside
    std::vector<unsigned char> packed((size_t)stream + 16, 0);
    if ((rc = hspmv_slices_pack(nd, P.desc.data(), P.pos.data(), &bits, &stream, prefix.data(), packed.data())))
      return rc;
    pos_bytes = packed.size();
    table_bytes = 4 * prefix.size();
    if ((rc = s.dev.upload(&d.pos, packed.data(), pos_bytes))) return rc;
    if ((rc = s.dev.upload(&d.ppre, prefix.data(), table_bytes))) return rc;
  } else if ((rc = s.dev.upload(&d.pos, P.pos.data(), pos_bytes))) {  // the plan's stream as it is
    return rc;
  }
  if ((rc = s.dev.upload(&d.desc, P.desc.data(), 4 * P.desc.size()))) return rc;
  if ((rc = s.dev.upload(&d.len, P.len.data(), P.len.size()))) return rc;
  if ((rc = s.dev.upload(&d.val, P.val.data(), P.val.size()))) return rc;
  d.n = (int32_t)nd;
  d.pos_bits = bits;
  s.saved.sl_desc_n = nd;
  s.saved.sl_padded = P.padded;
  s.saved.sl_pos_bytes = stream + (int64_t)table_bytes;  // the stream and ppre
  return HSPMV_OK;
}

void drop_slices(Shard &s) {
  const DevSlices &d = s.built.sl;
  for (const void *p : std::initializer_list<const void *>{d.desc, d.len, d.pos, d.ppre, d.val}) s.dev.release(p);
  s.built.sl = DevSlices();
  s.A.has_slices = false;
}

}  // namespace hspmv

using namespace hspmv;

extern "C" {

int hspmv_slices_plan(const hspmv_csr *A, const hspmv_csr3_maps *maps, const hspmv_options *opt,
                      int64_t *n_desc, int64_t *n_slices, int64_t *padded_entries, int32_t *why,
                      int32_t *desc, uint8_t *len, uint16_t *pos, void *val) {
  // (a NULL or malformed A is refused by plan_shape, whatever the dtype read here)
  return hspmv_slices_plan_vec(A, maps, opt, A ? A->dtype : HSPMV_F64, n_desc, n_slices, padded_entries, why,
                               desc, len, pos, val);
}

int hspmv_slices_plan_vec(const hspmv_csr *A, const hspmv_csr3_maps *maps, const hspmv_options *opt,
                          int vector_dtype, int64_t *n_desc, int64_t *n_slices, int64_t *padded_entries,
                          int32_t *why, int32_t *desc, uint8_t *len, uint16_t *pos, void *val) {
  clear_error();
  if (!n_desc || !n_slices || !padded_entries || !why) return set_error(HSPMV_E_INVALID, "NULL output");
  *n_desc = *n_slices = *padded_entries = 0;
  *why = HSPMV_SLICES_SHAPE;
  int rc;
  PlanShape ps;
  if ((rc = plan_shape(A, maps, opt, ps))) return rc;
  if ((rc = check_dtype_pair(A->dtype, vector_dtype))) return rc;
  const int vdt = vector_dtype;  // the dictionaries hold x entries; the slices' values stay A->dtype
  const Tuning &tune = ps.tune;
  const unsigned flags = ps.flags;
  std::vector<int32_t> &tasks = ps.tasks;
  const int W = ps.W, kern = ps.kern;
  if ((kern != kStream && kern != kCsr3) || A->m == 0) return HSPMV_OK;
  SliceCounts c;
  *why = slices_why(tune, flags, kern, W, A->row_ptr, A->m, A->n, vdt, A->dtype,
                    slice_starts(kern, A->m, tasks), &c);
  *n_desc = c.n_desc;
  *n_slices = c.n_slices;
  *padded_entries = 64 * c.padded;
  if (*why != HSPMV_SLICES_OK) return HSPMV_OK;
  XdPlan P;
  const int32_t long_t = split_threshold(flags);
  const bool fill = desc || len || pos || val;
  int64_t cut = 0;
  if (!plan_xdict_for(A->row_ptr, A->col_idx, kern, A->m, tasks, W, long_t,
                      xdict_cap_entries(vdt, tune), vdt, tune, true, fill, P, &cut)) {
    *why = HSPMV_SLICES_NO_DICT;  // some block exceeds the LDS cap
    return HSPMV_OK;
  }
  const std::vector<int32_t> starts = slice_starts(kern, A->m, tasks);  // after the occupancy cuts
  slices_why(tune, flags, kern, W, A->row_ptr, A->m, A->n, vdt, A->dtype, starts, &c);
  *n_desc = c.n_desc;
  if (!fill) return HSPMV_OK;
  SlicePlan S;
  build_slices(A->row_ptr, P.pos.data(), A->val, A->m, A->dtype, starts, S);
  if (desc) memcpy(desc, S.desc.data(), 4 * S.desc.size());
  if (len && A->m) memcpy(len, S.len.data(), (size_t)A->m);
  if (pos && S.padded) memcpy(pos, S.pos.data(), 2 * (size_t)(64 * S.padded));
  if (val && S.padded) memcpy(val, S.val.data(), dtype_size(A->dtype) * (size_t)(64 * S.padded));
  return HSPMV_OK;
}

int hspmv_slices_pack(int64_t n_desc, const int32_t *desc, const uint16_t *pos, int32_t *bits,
                      int64_t *pos_bytes, int32_t *pos_prefix, void *packed) {
  clear_error();
  if (n_desc < 0 || !desc || !pos || !bits || !pos_bytes) return set_error(HSPMV_E_INVALID, "NULL argument");
  for (int64_t s = 0; s < n_desc; ++s)
    if (desc[2 * s] < 0 || desc[2 * s + 2] < desc[2 * s]) return set_error(HSPMV_E_INVALID, "desc: prefixes decrease");
  *bits = slice_pos_bits(desc, n_desc, pos);
  std::vector<int32_t> prefix((size_t)n_desc + 1);
  pack_slice_pos(desc, n_desc, pos, *bits, prefix.data(), nullptr);
  *pos_bytes = 128 * (int64_t)prefix[(size_t)n_desc];
  if (pos_prefix) memcpy(pos_prefix, prefix.data(), 4 * prefix.size());
  if (packed) pack_slice_pos(desc, n_desc, pos, *bits, prefix.data(), (unsigned char *)packed);
  return HSPMV_OK;
}

}  // extern "C"
