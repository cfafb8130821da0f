// cli_common.h -- shared driver code of the spmv-csr / spmv-csrk executables.
//
// Reproduces the reference benchmark-driver contract:
//   argv:   <matrix file> <num_runs> [...]
//   stdout: "TimeMin: %lg" / "TimeMax: %lg" / "TimeAvg: %lg" (seconds,
//           launch + synchronize wall time, 5 warm-ups first:
//           spmv-csr/spmv.c:164-185, hip/spmv-auto-mi100.cu:200-240) and
//           "Number Wrong: %d" (|y - yhat| > 0.01 against a serial CPU SpMV,
//           cuda-spmv-csr/spmv.cu:270-284), parsed by run_scripts/run_norm.py:94-107.
// plus extra lines: KernelMin/KernelAvg (HIP-event device time), GFLOPs and
// GBps (2 nnz and algorithmic bytes / TimeMin, the wall time printed above),
// KernelGFLOPs/KernelGBps (the same / KernelMin), NumGPUs, Kernel, and
// "Check: PASS|FAIL maxrel=..." (1e-6 relative fp64 tolerance with an
// absolute floor).
//
// Options (after the positional arguments):
//   --gpus N            row-range partition over N GPUs (RCCL x-bcast / y-gather)
//   --dtype f32|f64     value type (default f64; f32 = the reference's type)
//   --vector-dtype f32|f64   type of x, y, the products and the sums (default:
//                       --dtype).  f64 with --dtype f32 is the mixed handle
//                       (hspmv_create_mixed): the file is read as fp32 and
//                       streamed as fp32, the check is the fp64 host sum of
//                       the widened values and --dump-y writes fp64; any
//                       other unequal pair prints the library's message and
//                       exits non-zero
//   --x ones|rand:SEED  input vector (default ones, as the reference)
//   --kernel auto|stream|vector[:L]|csr3|csort
//   --nt                non-temporal loads of the matrix streams
//   --plan aligned|packed|ssr   CSR-3 wave-task plan (hspmv_options.csr3_plan;
//                       ssr = one workgroup per super-super-row, the
//                       reference's cuSpMV_3 mapping)
//   --deterministic     only the ordered row kernels (omp_spmv's order; y
//                       bit-identical run to run)
//   --reproducible      y bit-identical run to run, the column-sorted kernel
//                       allowed with fixed-point row sums
//   --serial            every row summed in omp_spmv's order, one lane per
//                       row: y bit-identical to the serial check (reported
//                       as "Bitwise:")
//   --sweep forward|alternate   the row kernel's block sweep from one SpMV to
//                       the next (hspmv_set_sweep; default: the library's
//                       choice; y is the same bits either way)
//   --rhs K             spmv-csr only: Y = A X for K right-hand sides (1..32) in one
//                       pass over A (hspmv_mm_*), same protocol; column c of X
//                       is the --x generator with seed SEED + c (ones: every
//                       column ones); flops = 2 nnz K; prints "Rhs: K"; the
//                       check runs per column; --dump-y writes the row-major
//                       m x K array.  One GPU, the automatic kernel only.
//   --update-values N   the handle is created by hspmv_create_updatable; after
//                       the timed loop and its report: N rounds of
//                       hspmv_update_values on the planned handle from host
//                       memory, round k with the file's values times 1 +
//                       2^-(k+1); prints "UpdateMin:" / "UpdateAvg:" (wall
//                       seconds per call), then runs one SpMV and prints
//                       "UpdateCheck: PASS|FAIL ..." against the serial CPU
//                       sum over the last round's values (not with --rhs;
//                       a band-k order keeps its permutation: the values are
//                       those of the matrix the handle was created from)
//   --axpby ALPHA,BETA  after the timed loop, its report and the check: y0 =
//                       the --x generator with seed SEED + 1 (m entries); one
//                       hspmv_spmv_axpby(ALPHA, BETA) over it is compared byte
//                       for byte with the host model formed from the device's
//                       own s = A x ("AxpbyCheck: PASS|FAIL rows_differ=N
//                       path=fused|two_pass"); then hspmv_run_axpby is timed
//                       from y0 and printed as "AxpbyTimeMin:" / "AxpbyTimeMax:"
//                       / "AxpbyTimeAvg:" (wall) and "AxpbyKernelMin:" (not
//                       with --rhs or --gpus > 1; keep |BETA| < 1: y evolves
//                       over the timed calls)
//   --dot               after --axpby's part (ALPHA,BETA as given there, else
//                       1,0): y0 as for --axpby, w = the --x generator with
//                       seed SEED + 2; one hspmv_spmv_axpby_dot(ALPHA, BETA)
//                       asking for both dots, checked against long-double host
//                       sums over the device's own y within (m + 4) 2^-53
//                       sum |terms| ("DotCheck: PASS|FAIL wy=... yy=...
//                       path=fused|two_pass"); then hspmv_run_axpby_dot is
//                       timed from y0: "DotTimeMin:" / "DotTimeMax:" /
//                       "DotTimeAvg:" (wall), "DotKernelMin:" (not with --rhs
//                       or --gpus > 1)
//   --dump-y PATH       write y as raw binary (dtype) for external checks
//   --no-check          skip the serial CPU check
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <string>
#include <vector>

#include "hspmv.h"

namespace cli {

struct Options {
  int gpus = 1;
  int dtype = HSPMV_F64;
  int vector_dtype = -1;  // < 0: dtype
  bool x_rand = false;
  unsigned long long seed = 42;
  unsigned kernel = HSPMV_KERNEL_AUTO;
  unsigned lanes = 0;
  bool nt = false;
  int plan = HSPMV_CSR3_PLAN_AUTO;
  int deterministic = 0;  // hspmv_options.deterministic
  int sweep = HSPMV_SWEEP_AUTO;  // hspmv_set_sweep
  bool check = true;
  int rhs = 0;  // > 0: the multi-vector operator with this many right-hand sides
  int update_values = 0;  // > 0: rounds of hspmv_update_values after the timed loop
  bool axpby = false;     // --axpby ALPHA,BETA: hspmv_spmv_axpby checked, hspmv_run_axpby timed
  double alpha = 1.0, beta = 0.0;
  bool dot = false;       // --dot: hspmv_spmv_axpby_dot(ALPHA, BETA) checked, hspmv_run_axpby_dot timed
  std::string dump_y;
  std::string params = "mi355x";
  bool bandk = true;  // spmv-csrk on a .csr: band-k reorder (the reference's CSRk_Graph)
};

inline bool ends_with(const std::string &s, const char *suf) {
  const size_t n = strlen(suf);
  return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

// Parses "--opt value" style options from argv[first..].  Returns false on error.
inline bool parse_options(int argc, char **argv, int first, Options &o) {
  for (int i = first; i < argc; ++i) {
    std::string a = argv[i];
    auto need = [&](const char *name) -> const char * {
      if (i + 1 >= argc) {
        fprintf(stderr, "missing value for %s\n", name);
        return nullptr;
      }
      return argv[++i];
    };
    if (a == "--gpus") {
      const char *v = need("--gpus"); if (!v) return false;
      o.gpus = atoi(v);
    } else if (a == "--dtype") {
      const char *v = need("--dtype"); if (!v) return false;
      if (!strcmp(v, "f32")) o.dtype = HSPMV_F32;
      else if (!strcmp(v, "f64")) o.dtype = HSPMV_F64;
      else { fprintf(stderr, "bad --dtype %s\n", v); return false; }
    } else if (a == "--vector-dtype") {
      const char *v = need("--vector-dtype"); if (!v) return false;
      if (!strcmp(v, "f32")) o.vector_dtype = HSPMV_F32;
      else if (!strcmp(v, "f64")) o.vector_dtype = HSPMV_F64;
      else { fprintf(stderr, "bad --vector-dtype %s\n", v); return false; }
    } else if (a == "--x") {
      const char *v = need("--x"); if (!v) return false;
      if (!strcmp(v, "ones")) o.x_rand = false;
      else if (!strncmp(v, "rand:", 5)) { o.x_rand = true; o.seed = strtoull(v + 5, nullptr, 10); }
      else { fprintf(stderr, "bad --x %s\n", v); return false; }
    } else if (a == "--kernel") {
      const char *v = need("--kernel"); if (!v) return false;
      if (!strcmp(v, "auto")) o.kernel = HSPMV_KERNEL_AUTO;
      else if (!strcmp(v, "stream")) o.kernel = HSPMV_KERNEL_STREAM;
      else if (!strcmp(v, "csr3")) o.kernel = HSPMV_KERNEL_CSR3;
      else if (!strcmp(v, "csort")) o.kernel = HSPMV_KERNEL_CSORT;
      else if (!strncmp(v, "vector", 6)) {
        o.kernel = HSPMV_KERNEL_VECTOR;
        if (v[6] == ':') o.lanes = (unsigned)atoi(v + 7);
      } else { fprintf(stderr, "bad --kernel %s\n", v); return false; }
    } else if (a == "--nt") {
      o.nt = true;
    } else if (a == "--plan") {
      const char *v = need("--plan"); if (!v) return false;
      if (!strcmp(v, "aligned")) o.plan = HSPMV_CSR3_PLAN_ALIGNED;
      else if (!strcmp(v, "packed")) o.plan = HSPMV_CSR3_PLAN_PACKED;
      else if (!strcmp(v, "ssr")) o.plan = HSPMV_CSR3_PLAN_SSR;
      else { fprintf(stderr, "bad --plan %s\n", v); return false; }
    } else if (a == "--deterministic") {
      o.deterministic = HSPMV_DETERMINISTIC_ORDERED;
    } else if (a == "--reproducible") {
      o.deterministic = HSPMV_DETERMINISTIC_REPRODUCIBLE;
    } else if (a == "--serial") {
      o.deterministic = HSPMV_DETERMINISTIC_SERIAL;
    } else if (a == "--sweep") {
      const char *v = need("--sweep"); if (!v) return false;
      if (!strcmp(v, "forward")) o.sweep = HSPMV_SWEEP_FORWARD;
      else if (!strcmp(v, "alternate")) o.sweep = HSPMV_SWEEP_ALTERNATE;
      else { fprintf(stderr, "bad --sweep %s\n", v); return false; }
    } else if (a == "--rhs") {
      const char *v = need("--rhs"); if (!v) return false;
      o.rhs = atoi(v);
      if (o.rhs < 1 || o.rhs > 32) { fprintf(stderr, "bad --rhs %s (1..32)\n", v); return false; }
    } else if (a == "--update-values") {
      const char *v = need("--update-values"); if (!v) return false;
      o.update_values = atoi(v);
      if (o.update_values < 1) { fprintf(stderr, "bad --update-values %s (>= 1)\n", v); return false; }
    } else if (a == "--axpby") {
      const char *v = need("--axpby"); if (!v) return false;
      char *end = nullptr;
      o.alpha = strtod(v, &end);
      if (end == v || *end != ',') { fprintf(stderr, "bad --axpby %s (ALPHA,BETA)\n", v); return false; }
      const char *b = end + 1;
      o.beta = strtod(b, &end);
      if (end == b || *end != '\0') { fprintf(stderr, "bad --axpby %s (ALPHA,BETA)\n", v); return false; }
      o.axpby = true;
    } else if (a == "--dot") {
      o.dot = true;
    } else if (a == "--no-check") {
      o.check = false;
    } else if (a == "--dump-y") {
      const char *v = need("--dump-y"); if (!v) return false;
      o.dump_y = v;
    } else if (a == "--file-order") {
      o.bandk = false;
    } else if (a == "--params") {
      const char *v = need("--params"); if (!v) return false;
      o.params = v;
    } else {
      fprintf(stderr, "unknown option %s\n", a.c_str());
      return false;
    }
  }
  if (o.rhs > 0) {  // the multi-vector operator: one device, one kernel, no planner options
    if (o.gpus != 1) { fprintf(stderr, "--rhs runs on one GPU (not --gpus %d)\n", o.gpus); return false; }
    if (o.kernel != HSPMV_KERNEL_AUTO) { fprintf(stderr, "--rhs has one kernel (only --kernel auto)\n"); return false; }
    if (o.plan != HSPMV_CSR3_PLAN_AUTO || o.deterministic != 0 || o.sweep != HSPMV_SWEEP_AUTO) {
      fprintf(stderr, "--rhs takes no --plan, --deterministic, --reproducible, --serial or --sweep\n");
      return false;
    }
    if (o.update_values > 0) { fprintf(stderr, "--rhs takes no --update-values\n"); return false; }
    if (o.axpby) { fprintf(stderr, "--rhs takes no --axpby\n"); return false; }
    if (o.dot) { fprintf(stderr, "--rhs takes no --dot\n"); return false; }
  }
  if (o.axpby && o.gpus != 1) {
    fprintf(stderr, "--axpby runs on one GPU (not --gpus %d)\n", o.gpus);
    return false;
  }
  if (o.dot && o.gpus != 1) {
    fprintf(stderr, "--dot runs on one GPU (not --gpus %d)\n", o.gpus);
    return false;
  }
  return true;
}

inline unsigned flags_of(const Options &o) {
  unsigned f = o.kernel;
  if (o.kernel == HSPMV_KERNEL_VECTOR && o.lanes) f |= HSPMV_LANES(o.lanes);
  if (o.nt) f |= HSPMV_FLAG_NONTEMPORAL;
  return f;
}

// splitmix64 -> U(-1, 1); same generator as hspmv.gen.rand_x in Python.
inline void fill_x(const Options &o, int64_t n, std::vector<double> &x64) {
  x64.assign((size_t)n, 1.0);
  if (!o.x_rand) return;
  unsigned long long s = o.seed;
  for (int64_t i = 0; i < n; ++i) {
    unsigned long long z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z ^= z >> 31;
    x64[i] = (double)(z >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
  }
}

// Serial CPU check (test_spmv, spmv-csr/spmv.c:68-90) + reference count
// (|diff| > 0.01) + relative-tolerance verdict.
struct CheckResult {
  int wrong = 0;
  int64_t bit_diff = 0;  // rows whose y is not bit-identical to the serial sum
  double maxrel = 0.0;
  bool pass = true;
};

template <typename T>
CheckResult check_y(const hspmv_csr_buf &A, const T *val, const T *x, const T *y) {
  CheckResult r;
  for (int64_t row = 0; row < A.m; ++row) {
    T temp = 0;
    double mag = 0.0;
    for (int32_t k = A.row_ptr[row]; k < A.row_ptr[row + 1]; ++k) {
      temp += val[k] * x[A.col_idx[k]];
      mag += fabs((double)val[k] * (double)x[A.col_idx[k]]);
    }
    if (memcmp(&y[row], &temp, sizeof(T)) != 0) r.bit_diff++;
    const double d = (double)y[row] - (double)temp;
    if (d > .01 || d < -.01) r.wrong++;
    const double tol_rel = sizeof(T) == 8 ? 1e-6 : 1e-4;
    const double floor = (sizeof(T) == 8 ? 1e-12 : 1e-6) * mag;
    const double err = fabs(d);
    if (err > tol_rel * fabs((double)temp) + floor) r.pass = false;
    const double rel = err / (fabs((double)temp) + floor + 1e-300);
    if (rel > r.maxrel && err > 0) r.maxrel = rel;
  }
  return r;
}

inline int die(const char *what) {
  fprintf(stderr, "%s: %s\n", what, hspmv_last_error());
  return 1;
}

// --rhs K: the timed protocol through the multi-vector operator (hspmv_mm_*).
inline int run_and_report_mm(const hspmv_csr_buf &A, int num_runs, const Options &o) {
  hspmv_csr view = {A.m, A.n, A.nnz, A.row_ptr, A.col_idx, A.val, A.dtype};
  const int K = o.rhs;
  hspmv_options opt;
  memset(&opt, 0, sizeof(opt));
  opt.struct_size = sizeof(opt);
  opt.flags = flags_of(o);
  hspmv_mm *mm = nullptr;
  if (hspmv_mm_create(&mm, &view, K, &opt) != HSPMV_OK) return die("hspmv_mm_create");
  // row-major n x K: column c from the generator with seed + c
  std::vector<double> X64((size_t)A.n * (size_t)K), col;
  for (int c = 0; c < K; ++c) {
    Options oc = o;
    oc.seed = o.seed + (unsigned long long)c;
    fill_x(oc, A.n, col);
    for (int64_t i = 0; i < A.n; ++i) X64[(size_t)i * (size_t)K + (size_t)c] = col[(size_t)i];
  }
  std::vector<float> X32;
  const void *xp = X64.data();
  if (A.dtype == HSPMV_F32) {
    X32.assign(X64.begin(), X64.end());
    xp = X32.data();
  }
  if (hspmv_mm_set_x(mm, xp, K) != HSPMV_OK) return die("hspmv_mm_set_x");
  hspmv_timing t;
  if (hspmv_mm_run(mm, 5, num_runs, &t) != HSPMV_OK) return die("hspmv_mm_run");
  hspmv_mm_info info;
  if (hspmv_mm_get_info(mm, &info, sizeof(info)) != HSPMV_OK) return die("hspmv_mm_get_info");
  printf("TimeMin: %lg\n", t.wall_min);
  printf("TimeMax: %lg\n", t.wall_max);
  printf("TimeAvg: %lg\n", t.wall_avg);
  printf("KernelMin: %lg\n", t.t_min);
  printf("KernelAvg: %lg\n", t.t_avg);
  printf("GFLOPs: %lg\n", t.wall_min > 0 ? info.flops / t.wall_min * 1e-9 : 0.0);
  printf("GBps: %lg\n", t.wall_min > 0 ? info.alg_bytes / t.wall_min * 1e-9 : 0.0);
  printf("KernelGFLOPs: %lg\n", t.gflops);
  printf("KernelGBps: %lg\n", t.gbps_alg);
  printf("NumGPUs: %d\n", t.num_gpus);
  printf("Kernel: spmm lanes_per_row=%d rows_per_wave=%d waves_per_block=%d blocks=%lld long_rows=%lld\n",
         info.lanes_per_row, info.rows_per_wave, info.waves_per_block, (long long)info.blocks,
         (long long)info.long_rows);
  printf("Rhs: %d\n", K);
  const size_t sv = A.dtype == HSPMV_F64 ? 8 : 4;
  const size_t ny = (size_t)A.m * (size_t)K;
  std::vector<char> Y(sv * (ny ? ny : 1));
  if (hspmv_mm_get_y(mm, Y.data(), K) != HSPMV_OK) return die("hspmv_mm_get_y");
  if (!o.dump_y.empty()) {
    FILE *fp = fopen(o.dump_y.c_str(), "wb");
    if (!fp || fwrite(Y.data(), sv, ny, fp) != ny) {
      fprintf(stderr, "cannot write %s\n", o.dump_y.c_str());
      return 1;
    }
    fclose(fp);
  }
  int rc = 0;
  if (o.check) {  // the serial check per column; the report covers all columns
    CheckResult all;
    std::vector<double> x64((size_t)A.n), y64((size_t)A.m);
    std::vector<float> x32((size_t)A.n), y32((size_t)A.m);
    for (int c = 0; c < K; ++c) {
      CheckResult r;
      if (A.dtype == HSPMV_F64) {
        for (int64_t i = 0; i < A.n; ++i) x64[(size_t)i] = X64[(size_t)i * (size_t)K + (size_t)c];
        for (int64_t i = 0; i < A.m; ++i) y64[(size_t)i] = ((const double *)Y.data())[(size_t)i * (size_t)K + (size_t)c];
        r = check_y<double>(A, (const double *)A.val, x64.data(), y64.data());
      } else {
        for (int64_t i = 0; i < A.n; ++i) x32[(size_t)i] = X32[(size_t)i * (size_t)K + (size_t)c];
        for (int64_t i = 0; i < A.m; ++i) y32[(size_t)i] = ((const float *)Y.data())[(size_t)i * (size_t)K + (size_t)c];
        r = check_y<float>(A, (const float *)A.val, x32.data(), y32.data());
      }
      all.wrong += r.wrong;
      all.pass = all.pass && r.pass;
      if (r.maxrel > all.maxrel) all.maxrel = r.maxrel;
    }
    printf("Number Wrong: %d \n", all.wrong);
    printf("Check: %s maxrel=%.3e\n", all.pass ? "PASS" : "FAIL", all.maxrel);
    rc = all.pass ? 0 : 2;
  }
  hspmv_mm_destroy(mm);
  return rc;
}

// --axpby: s holds the device's y = A x (m entries of T, the handle's vector
// type).  One hspmv_spmv_axpby over y0 against the host model -- the two
// products and the sum each rounded to T on their own (the volatiles keep the
// host compiler from contracting them) -- byte for byte, then hspmv_run_axpby
// from y0.  Returns 0, 2 for a failed check, 1 after a library error.
template <typename T>
int run_axpby(hspmv_handle *h, int64_t m, const void *s_bytes, int num_runs, const Options &o,
              const int32_t *perm) {
  const T *s = (const T *)s_bytes;
  Options oy = o;
  oy.seed = o.seed + 1;
  std::vector<double> y64;
  fill_x(oy, m, y64);
  std::vector<T> y0((size_t)(m ? m : 1)), got(y0.size());
  for (int64_t i = 0; i < m; ++i) y0[(size_t)i] = (T)y64[(size_t)(perm ? perm[i] : i)];
  const int path = hspmv_axpby_path(h);
  if (path < 0) return die("hspmv_axpby_path");
  if (hspmv_set_y(h, y0.data()) != HSPMV_OK) return die("hspmv_set_y");
  if (hspmv_spmv_axpby(h, o.alpha, o.beta) != HSPMV_OK) return die("hspmv_spmv_axpby");
  if (hspmv_get_y(h, got.data()) != HSPMV_OK) return die("hspmv_get_y");
  const T alpha = (T)o.alpha, beta = (T)o.beta;
  long long differ = 0;
  for (int64_t i = 0; i < m; ++i) {
    volatile T want = alpha * s[i];
    if (beta != T(0)) {
      volatile T by = beta * y0[(size_t)i];
      want = want + by;
    }
    const T w = want;
    if (memcmp(&w, &got[(size_t)i], sizeof(T)) != 0) differ++;
  }
  printf("AxpbyCheck: %s rows_differ=%lld path=%s\n", differ ? "FAIL" : "PASS", differ,
         path == HSPMV_AXPBY_PATH_FUSED ? "fused" : "two_pass");
  if (hspmv_set_y(h, y0.data()) != HSPMV_OK) return die("hspmv_set_y");
  hspmv_timing t;
  if (hspmv_run_axpby(h, o.alpha, o.beta, 5, num_runs, &t) != HSPMV_OK) return die("hspmv_run_axpby");
  printf("AxpbyTimeMin: %lg\n", t.wall_min);
  printf("AxpbyTimeMax: %lg\n", t.wall_max);
  printf("AxpbyTimeAvg: %lg\n", t.wall_avg);
  printf("AxpbyKernelMin: %lg\n", t.t_min);
  return differ ? 2 : 0;
}

// --dot: one hspmv_spmv_axpby_dot(ALPHA, BETA, both dots) over y0 (as for
// --axpby) with w the --x generator at seed SEED + 2; the two results against
// long-double host sums over the device's own y, within (m + 4) 2^-53
// sum |terms| (any order of m double sums over products rounded once), then
// hspmv_run_axpby_dot from y0.  Returns 0, 2 for a failed check, 1 after a
// library error.
template <typename T>
int run_dot(hspmv_handle *h, int64_t m, int num_runs, const Options &o, const int32_t *perm) {
  Options oy = o, ow = o;
  oy.seed = o.seed + 1;
  ow.seed = o.seed + 2;
  std::vector<double> y64, w64;
  fill_x(oy, m, y64);
  fill_x(ow, m, w64);
  std::vector<T> y0((size_t)(m ? m : 1)), w(y0.size()), got(y0.size());
  for (int64_t i = 0; i < m; ++i) {
    y0[(size_t)i] = (T)y64[(size_t)(perm ? perm[i] : i)];
    w[(size_t)i] = (T)w64[(size_t)(perm ? perm[i] : i)];
  }
  const int path = hspmv_axpby_path(h);
  if (path < 0) return die("hspmv_axpby_path");
  const unsigned both = HSPMV_DOT_WY | HSPMV_DOT_YY;
  double d[2] = {0.0, 0.0};
  if (hspmv_set_y(h, y0.data()) != HSPMV_OK) return die("hspmv_set_y");
  if (hspmv_set_w(h, w.data()) != HSPMV_OK) return die("hspmv_set_w");
  if (hspmv_spmv_axpby_dot(h, o.alpha, o.beta, both) != HSPMV_OK) return die("hspmv_spmv_axpby_dot");
  if (hspmv_get_dots(h, d) != HSPMV_OK) return die("hspmv_get_dots");
  if (hspmv_get_y(h, got.data()) != HSPMV_OK) return die("hspmv_get_y");
  long double ref[2] = {0.0L, 0.0L}, mag[2] = {0.0L, 0.0L};
  for (int64_t i = 0; i < m; ++i) {
    const long double yv = (long double)got[(size_t)i];
    const long double t0 = (long double)w[(size_t)i] * yv, t1 = yv * yv;
    ref[0] += t0;
    ref[1] += t1;
    mag[0] += fabsl(t0);
    mag[1] += t1;
  }
  bool pass = true;
  for (int k = 0; k < 2; ++k) {
    const long double bound = (long double)(m + 4) * ldexpl(1.0L, -53) * mag[k];
    if (!(fabsl((long double)d[k] - ref[k]) <= bound)) pass = false;
  }
  printf("DotCheck: %s wy=%.17g yy=%.17g path=%s\n", pass ? "PASS" : "FAIL", d[0], d[1],
         path == HSPMV_AXPBY_PATH_FUSED ? "fused" : "two_pass");
  if (hspmv_set_y(h, y0.data()) != HSPMV_OK) return die("hspmv_set_y");
  hspmv_timing t;
  if (hspmv_run_axpby_dot(h, o.alpha, o.beta, both, 5, num_runs, &t) != HSPMV_OK)
    return die("hspmv_run_axpby_dot");
  printf("DotTimeMin: %lg\n", t.wall_min);
  printf("DotTimeMax: %lg\n", t.wall_max);
  printf("DotTimeAvg: %lg\n", t.wall_avg);
  printf("DotKernelMin: %lg\n", t.t_min);
  return pass ? 0 : 2;
}

// Runs the timed protocol on an already-read matrix and prints the report.
// perm (optional, m entries): A is the band-k permutation of the file's
// matrix, row i = file row perm[i]; x is generated in file order and
// permuted, and a dumped y is put back in file order.
inline int run_and_report(const hspmv_csr_buf &A, const hspmv_csr3_buf *maps, int num_runs,
                          const Options &o, const int32_t *perm = nullptr) {
  if (o.rhs > 0) {
    if ((maps && maps->n_ssr > 0) || perm) {
      fprintf(stderr, "--rhs runs plain CSR (spmv-csr), not CSR-3 maps or a band-k order\n");
      return 1;
    }
    if (o.vector_dtype >= 0 && o.vector_dtype != A.dtype) {
      fprintf(stderr, "--rhs has one dtype (no --vector-dtype other than --dtype)\n");
      return 1;
    }
    return run_and_report_mm(A, num_runs, o);
  }
  hspmv_csr view = {A.m, A.n, A.nnz, A.row_ptr, A.col_idx, A.val, A.dtype};
  hspmv_csr3_maps mv = {0, 0, nullptr, nullptr};
  if (maps && maps->n_ssr > 0) mv = {maps->n_ssr, maps->n_sr, maps->outer, maps->inner};
  hspmv_handle *h = nullptr;
  int ndev = 0;
  if (hspmv_device_count(&ndev) != HSPMV_OK) return die("hspmv_device_count");
  const int gpus = o.gpus > 0 ? o.gpus : ndev;
  std::vector<int> devs((size_t)(gpus > 0 ? gpus : 1));
  for (size_t p = 0; p < devs.size(); ++p) devs[p] = (int)p;
  hspmv_options opt;
  memset(&opt, 0, sizeof(opt));
  opt.struct_size = sizeof(opt);
  opt.flags = flags_of(o);
  opt.devices = gpus > 1 ? devs.data() : nullptr;  // row-range shards over RCCL
  opt.n_devices = gpus > 1 ? gpus : 0;
  opt.csr3_plan = o.plan;
  opt.deterministic = o.deterministic;
  // vdt: the type of x and y (the values' unless --vector-dtype gives another)
  const int vdt = o.vector_dtype >= 0 ? o.vector_dtype : A.dtype;
  if (o.update_values > 0) {  // a handle that takes new values in every plan, the column-sorted one too
    if (hspmv_create_updatable(&h, &view, mv.n_ssr > 0 ? &mv : nullptr, &opt, vdt) != HSPMV_OK)
      return die("hspmv_create_updatable");
  } else if (vdt != A.dtype) {
    if (hspmv_create_mixed(&h, &view, mv.n_ssr > 0 ? &mv : nullptr, &opt, vdt) != HSPMV_OK)
      return die("hspmv_create_mixed");
  } else if (hspmv_create_ex(&h, &view, mv.n_ssr > 0 ? &mv : nullptr, &opt) != HSPMV_OK) {
    return die("hspmv_create_ex");
  }
  if (o.sweep != HSPMV_SWEEP_AUTO && hspmv_set_sweep(h, o.sweep) != HSPMV_OK) return die("hspmv_set_sweep");
  std::vector<double> x64;
  fill_x(o, A.n, x64);
  if (perm) {
    std::vector<double> xf(x64);
    for (int64_t i = 0; i < A.n; ++i) x64[(size_t)i] = xf[(size_t)perm[i]];
  }
  std::vector<float> x32;
  const void *xp = x64.data();
  if (vdt == HSPMV_F32) {
    x32.assign(x64.begin(), x64.end());
    xp = x32.data();
  }
  if (hspmv_set_x(h, xp) != HSPMV_OK) return die("hspmv_set_x");
  hspmv_timing t;
  if (hspmv_run(h, 5, num_runs, &t) != HSPMV_OK) return die("hspmv_run");
  hspmv_info info;
  hspmv_get_info_sized(h, &info, sizeof(info));
  printf("TimeMin: %lg\n", t.wall_min);
  printf("TimeMax: %lg\n", t.wall_max);
  printf("TimeAvg: %lg\n", t.wall_avg);
  printf("KernelMin: %lg\n", t.t_min);
  printf("KernelAvg: %lg\n", t.t_avg);
  // GFLOPs / GBps from TimeMin, as a run_scripts consumer computes them
  // (run_norm.py:94-107 records TimeMin); the HIP-event rates beside them
  printf("GFLOPs: %lg\n", t.wall_min > 0 ? 2.0 * (double)A.nnz / t.wall_min * 1e-9 : 0.0);
  printf("GBps: %lg\n", t.wall_min > 0 ? info.alg_bytes / t.wall_min * 1e-9 : 0.0);
  printf("KernelGFLOPs: %lg\n", t.gflops);
  printf("KernelGBps: %lg\n", t.gbps_alg);
  printf("NumGPUs: %d\n", t.num_gpus);
  static const char *kname[] = {"auto", "vector", "stream", "csr3", "csort"};
  static const char *pname[] = {"-", "aligned", "packed", "ssr"};
  printf("Kernel: %s lanes=%d waves_per_block=%d blocks=%lld plan=%s deterministic=%d\n",
         kname[(info.kernel >= 0 && info.kernel <= 4) ? info.kernel : 0], info.lanes,
         info.waves_per_block, (long long)info.blocks,
         pname[(info.csr3_plan >= 0 && info.csr3_plan <= 3) ? info.csr3_plan : 0], info.deterministic);
  const size_t sv = vdt == HSPMV_F64 ? 8 : 4;
  std::vector<char> y(sv * (size_t)(A.m ? A.m : 1));
  if (hspmv_get_y(h, y.data()) != HSPMV_OK) return die("hspmv_get_y");
  if (!o.dump_y.empty()) {
    std::vector<char> yf(y.size());
    if (perm)  // back to the file's row order
      for (int64_t i = 0; i < A.m; ++i) memcpy(&yf[sv * (size_t)perm[i]], &y[sv * (size_t)i], sv);
    else
      yf = y;
    FILE *fp = fopen(o.dump_y.c_str(), "wb");
    if (!fp || fwrite(yf.data(), sv, (size_t)A.m, fp) != (size_t)A.m) {
      fprintf(stderr, "cannot write %s\n", o.dump_y.c_str());
      return 1;
    }
    fclose(fp);
  }
  int rc = 0;
  if (o.check) {
    CheckResult r;
    if (vdt == HSPMV_F64 && A.dtype == HSPMV_F32) {  // mixed: the fp64 sum of the widened values
      const float *v32 = (const float *)A.val;
      const std::vector<double> v64(v32, v32 + A.nnz);
      r = check_y<double>(A, v64.data(), x64.data(), (const double *)y.data());
    } else if (A.dtype == HSPMV_F64) {
      r = check_y<double>(A, (const double *)A.val, x64.data(), (const double *)y.data());
    } else {
      r = check_y<float>(A, (const float *)A.val, x32.data(), (const float *)y.data());
    }
    printf("Number Wrong: %d \n", r.wrong);
    printf("Check: %s maxrel=%.3e\n", r.pass ? "PASS" : "FAIL", r.maxrel);
    rc = r.pass ? 0 : 2;
    if (o.deterministic == HSPMV_DETERMINISTIC_SERIAL) {  // the serial order's contract
      printf("Bitwise: %lld rows differ\n", (long long)r.bit_diff);
      if (r.bit_diff) rc = 2;
    }
  }
  if (o.axpby) {
    const int arc = vdt == HSPMV_F64 ? run_axpby<double>(h, A.m, y.data(), num_runs, o, perm)
                                     : run_axpby<float>(h, A.m, y.data(), num_runs, o, perm);
    if (arc == 1) return 1;
    if (arc) rc = arc;
  }
  if (o.dot) {
    const int drc = vdt == HSPMV_F64 ? run_dot<double>(h, A.m, num_runs, o, perm)
                                     : run_dot<float>(h, A.m, num_runs, o, perm);
    if (drc == 1) return 1;
    if (drc) rc = drc;
  }
  if (o.update_values > 0) {
    // new values on the planned handle, N rounds: round k holds the file's
    // values times 1 + 2^-(k+1); then one SpMV, checked against the serial
    // sum over the last round's values
    const size_t svv = A.dtype == HSPMV_F64 ? 8 : 4;
    std::vector<char> nv(svv * (size_t)(A.nnz ? A.nnz : 1));
    double umin = 1e30, usum = 0.0;
    for (int k = 0; k < o.update_values; ++k) {
      const double f = 1.0 + ldexp(1.0, -(k + 1));
      for (int64_t i = 0; i < A.nnz; ++i) {
        if (A.dtype == HSPMV_F64)
          ((double *)nv.data())[i] = ((const double *)A.val)[i] * f;
        else
          ((float *)nv.data())[i] = (float)((double)((const float *)A.val)[i] * f);
      }
      const auto tic = std::chrono::steady_clock::now();
      if (hspmv_update_values(h, nv.data(), 0) != HSPMV_OK) return die("hspmv_update_values");
      const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - tic).count();
      umin = dt < umin ? dt : umin;
      usum += dt;
    }
    printf("UpdateMin: %lg\n", umin);
    printf("UpdateAvg: %lg\n", usum / o.update_values);
    if (hspmv_spmv(h) != HSPMV_OK) return die("hspmv_spmv");
    if (hspmv_get_y(h, y.data()) != HSPMV_OK) return die("hspmv_get_y");
    if (o.check) {
      CheckResult r;
      if (vdt == HSPMV_F64 && A.dtype == HSPMV_F32) {
        const float *v32 = (const float *)nv.data();
        const std::vector<double> v64(v32, v32 + A.nnz);
        r = check_y<double>(A, v64.data(), x64.data(), (const double *)y.data());
      } else if (A.dtype == HSPMV_F64) {
        r = check_y<double>(A, (const double *)nv.data(), x64.data(), (const double *)y.data());
      } else {
        r = check_y<float>(A, (const float *)nv.data(), x32.data(), (const float *)y.data());
      }
      printf("UpdateCheck: %s maxrel=%.3e wrong=%d\n", r.pass ? "PASS" : "FAIL", r.maxrel, r.wrong);
      if (!r.pass) rc = 2;
    }
  }
  hspmv_destroy(h);
  return rc;
}

// Reads .csr / .csr3 / .bin by extension (.csr3 and .bin may carry maps).
inline int read_matrix(const std::string &path, int dtype, hspmv_csr_buf &A, hspmv_csr3_buf &maps) {
  memset(&A, 0, sizeof(A));
  memset(&maps, 0, sizeof(maps));
  int rc;
  if (ends_with(path, ".csr3"))
    rc = hspmv_read_csr3(path.c_str(), dtype, &A, &maps);
  else if (ends_with(path, ".bin"))
    rc = hspmv_load_bin(path.c_str(), &A, &maps);
  else
    rc = hspmv_read_csr(path.c_str(), dtype, &A);
  return rc;
}

}  // namespace cli
