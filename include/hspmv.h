/*
 * hspmv.h -- C ABI of the MI355X-native CSR / CSR-3 SpMV library
 * (libhspmv.so, built from heterogeneous-spmv_amd/csrc/).
 *
 * This is the drop-in boundary for the reference's hot path.  The reference
 * has no library: its "boundary" is three things, each replaced here
 * (SURVEY.md §8b):
 *
 *  1. Kernel ABI  -- cuda_spmv (cuda-spmv-csr/spmv.cu:117-119) and
 *     cuSpMV_3 / cuSpMV_3_vec / cuSpMV_2 (cuda-spmv-csrk/hip/csrk.cuh:25-47),
 *     all taking raw device pointers.  Replaced by hspmv_spmv() on a handle
 *     that owns (or borrows, HSPMV_FLAG_DEVICE_PTRS) the device arrays.
 *  2. Host library -- CSRk_Graph(nRows, nCols, nnz, rVec, cVec, val, ...,
 *     k, supRowSizes) + putInCSRkFormat() / setX() / setY() / getY()
 *     (cuda-spmv-csrk/hip/csrk.cuh:321-353, csrk.cu:92-113, 531-641, 875-900).
 *     Replaced by hspmv_create() (+ hspmv_build_csr3_maps()), hspmv_set_x(),
 *     hspmv_get_y().
 *  3. CLI/stdout contract -- spmv-csr/spmv.c:116-225 and
 *     cuda-spmv-csrk/hip/spmv*.cu; reproduced by the spmv-csr / spmv-csrk
 *     executables built on top of this header.
 *
 * Conventions: every int-returning function returns 0 on success and a
 * negative HSPMV_E* code on failure (the reference ignores every hip* status;
 * SURVEY.md §5).  hspmv_last_error() returns a thread-local message.  No C++
 * exceptions cross this boundary.  Indices are 0-based int32 (readers accept
 * 1-based files and rebase them).  Values are fp32 or fp64 (hspmv_dtype).
 */
#ifndef HSPMV_H
#define HSPMV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history.  0.2: hspmv_options, info.deterministic.  0.3: info.rccl_version
 * / csort chunks, hspmv_xdict_plan_ex, hspmv_rccl_version, hspmv_read_mtx,
 * hspmv_rcm_reorder -- and two changes a 0.2 binary could not see
 * (hspmv_xdict_plan's 3rd argument became kernel flags; hspmv_get_info's
 * layout shrank).  1.0 declares that break: the library is libhspmv.so.1
 * (SONAME), so a binary built against 0.x fails to load instead of
 * misreading arguments; hspmv_get_info fills the whole 1.0 hspmv_info.
 * Within a major, structs only grow at the end (hspmv_options.struct_size,
 * hspmv_get_info_sized) and signatures never change. */
#define HSPMV_VERSION_MAJOR 1
#define HSPMV_VERSION_MINOR 1
/* 1.1: hspmv_options.deterministic = 2 (HSPMV_DETERMINISTIC_REPRODUCIBLE)
 * and 3 (HSPMV_DETERMINISTIC_SERIAL), hspmv_info.csort_fixed_point /
 * serial_order / csort_part_begin; hspmv_get_info frozen at the 1.0 layout
 * (HSPMV_INFO_SIZE_1_0).  Also in 1.1 (appended, nothing moved):
 * hspmv_options.row_slices, hspmv_info.row_slices, hspmv_slices_plan;
 * hspmv_set_sweep, hspmv_block_order, hspmv_info.sweep; the multi-vector
 * operator hspmv_mm_* (hspmv_mm, hspmv_mm_info); the mixed-precision handle
 * (fp32 values under fp64 vectors): hspmv_create_mixed, hspmv_get_dtypes,
 * hspmv_values_fit_f32, hspmv_slices_plan_vec; new values for a planned
 * handle or operator: hspmv_update_values, hspmv_mm_update_values,
 * HSPMV_VALUES_DEVICE, and for column-sorted handles hspmv_create_updatable,
 * hspmv_can_update_values; the general form y = alpha A x + beta y:
 * hspmv_spmv_axpby, hspmv_run_axpby, hspmv_set_y, hspmv_set_axpby_path,
 * hspmv_axpby_path; its dot products from the same pass:
 * hspmv_spmv_axpby_dot, hspmv_run_axpby_dot, hspmv_set_w,
 * hspmv_bind_w_device, hspmv_bind_dots_device, hspmv_get_dots -- functions
 * only, no struct grew. */

/* ---------------------------------------------------------------- status */
#define HSPMV_OK 0
#define HSPMV_E_INVALID (-1)   /* bad argument / malformed matrix          */
#define HSPMV_E_IO (-2)        /* file cannot be opened / parsed           */
#define HSPMV_E_NOMEM (-3)     /* host or device allocation failed         */
#define HSPMV_E_HIP (-4)       /* HIP runtime error                        */
#define HSPMV_E_RCCL (-5)      /* RCCL error                               */
#define HSPMV_E_NODEV (-6)     /* no / not enough HIP devices              */
#define HSPMV_E_STATE (-7)     /* call order violated (e.g. run before x)  */

/* ---------------------------------------------------------------- types */
typedef enum { HSPMV_F32 = 0, HSPMV_F64 = 1 } hspmv_dtype;

/* A CSR matrix.  Borrowed: hspmv_create copies host arrays (the caller may
 * free them afterwards).  With HSPMV_FLAG_DEVICE_PTRS the handle REFERENCES
 * the caller's device arrays: they must stay allocated for the handle's
 * lifetime, and row_ptr / col_idx unchanged -- the row kernels read them on
 * every SpMV, and the tables built at creation (16-bit columns, x
 * dictionaries, row slices, x slabs) are derived from the pattern.  val may
 * change: some kernels read it on every SpMV, others read a copy made at
 * creation (the row slices and the x slabs), so after writing new values into
 * it -- or to switch to another array -- call hspmv_update_values(h, NULL or
 * the new array, HSPMV_VALUES_DEVICE), which refreshes every copy; until that
 * call a changed array is used partly or not at all.  A changed pattern needs
 * a new handle. */
typedef struct {
  int64_t m, n, nnz;
  const int32_t *row_ptr; /* m+1 entries, row_ptr[0] == 0                */
  const int32_t *col_idx; /* nnz entries, 0 <= col < n                   */
  const void *val;        /* nnz entries of dtype                        */
  int32_t dtype;          /* hspmv_dtype                                 */
} hspmv_csr;

/* CSR-3 multilevel maps (A12/A13 in SURVEY.md §8a):
 * super-super-row s covers super-rows outer[s] .. outer[s+1]-1,
 * super-row r covers rows inner[r] .. inner[r+1]-1.
 * Same meaning as mapCoarseToFinerRows[2] / [1] of the reference
 * (csrk.cu:1614, .csr3 writer spmv-auto.cpp:38-62). */
typedef struct {
  int64_t n_ssr, n_sr;
  const int32_t *outer; /* n_ssr+1 */
  const int32_t *inner; /* n_sr+1  */
} hspmv_csr3_maps;

/* Owned buffers returned by the readers / builders; free with the matching
 * hspmv_free_* call. */
typedef struct {
  int64_t m, n, nnz;
  int32_t *row_ptr;
  int32_t *col_idx;
  void *val;
  int32_t dtype;
  int32_t index_base; /* base found in the file (0 or 1); arrays are 0-based */
} hspmv_csr_buf;

typedef struct {
  int64_t n_ssr, n_sr;
  int32_t *outer;
  int32_t *inner;
} hspmv_csr3_buf;

/* Timing of hspmv_run: the reference protocol (5 warm-ups, N timed runs,
 * min/max/avg; spmv-csr/spmv.c:164-185, hip/spmv-auto-mi100.cu:200-240).
 * t_* are device times from HIP events around each SpMV (max over GPUs);
 * wall_* are host steady_clock times around launch + synchronize, which is
 * what the reference measures. */
typedef struct {
  double t_min, t_max, t_avg;
  double wall_min, wall_max, wall_avg;
  double gflops;   /* 2*nnz / t_min * 1e-9                                 */
  double gbps_alg; /* hspmv_alg_bytes() / t_min * 1e-9                     */
  int32_t iters;
  int32_t num_gpus;
} hspmv_timing;

/* What a handle decided (kernel, launch shape, bytes). */
typedef struct {
  int32_t kernel;     /* HSPMV_KERNEL_* actually used                      */
  int32_t lanes;      /* lanes per row (VECTOR) / rows per wave task       */
  int32_t waves_per_block;
  int32_t num_gpus;
  int64_t blocks;     /* grid size of the launch (GPU 0)                   */
  double alg_bytes;   /* algorithmic bytes per SpMV        */
  double flops;       /* 2 * nnz                                           */
  int64_t device_bytes; /* device memory held by the handle (all GPUs)     */
  int32_t chunk_u;    /* STREAM/CSR3 elements per lane per LDS chunk        */
  int32_t n_split_rows; /* rows summed by the split-row kernels (GPU 0)     */
  int32_t xcd_remap;  /* blocks per XCD turn (1 = dispatch order)          */
  int32_t groups_per_wave; /* STREAM: 64-row groups one wave walks        */
  int64_t x_entries;  /* distinct columns referenced = x entries one SpMV
                         must read (summed over GPUs); alg_bytes uses it    */
  double format_bytes; /* bytes the device format actually moves per SpMV
                          (< alg_bytes with 16-bit column offsets)          */
  int32_t col16;      /* 0 = 32-bit columns; 1 + p = 16-bit column offsets
                         plus p high-bit planes (see HSPMV_FLAG_NO_COL16)   */
  int32_t wave_tasks; /* CSR3: wave tasks of the launch (GPU 0); 0 otherwise */
  int32_t x_windows;  /* STREAM/CSR3: 1 = row groups whose columns span
                         <= 256 entries gather from an LDS copy of that x
                         window; 0 = every gather from global x (GPU 0)     */
  int32_t x_dict;     /* 1 = block x dictionaries: each workgroup stages the
                         x runs its rows reference in LDS and the column
                         stream holds 16-bit positions in it (GPU 0)        */
  int64_t x_dict_entries; /* x entries staged per SpMV (all GPUs; 0 = none) */
  int32_t x_slabs;    /* STREAM/CSR3: 0, or the number of column slabs the
                         row kernel runs over, one pass each, so irregular
                         gathers stay in an L2-sized slice of x (GPU 0)     */
  int32_t col16_group; /* 1 = the 16-bit column offsets are relative to one
                          base per 64-row STREAM group or packed CSR3 task
                          (every one spans < 65536 columns); 0 = per
                          256-nonzero blocks or none                        */
  int32_t csort_parts; /* CSORT: column parts H of the row blocks (0 = the
                          handle does not use the column-sorted kernel)     */
  int32_t placement_trials; /* array sets timed at creation (0 = none: see
                               hspmv_options.placement_trials)             */
  int32_t placement_pick;   /* the set kept (0 = the first allocation)      */
  double placement_us[8];   /* each set's mean SpMV time at creation, us    */
  /* since 0.2 */
  int32_t deterministic;    /* 1: y is bit-identical run to run (every kernel
                               but CSORT with fp64 slots, whose LDS row sums
                               add in atomic order: fp32 y may differ in the
                               last bit where an fp64 sum sits at an fp32
                               rounding tie, fp64 y in the last bits of rows
                               it sums; CSORT with fixed-point slots is 1)  */
  int32_t csr3_plan;        /* CSR3 kernel: the HSPMV_CSR3_PLAN_* it runs;
                               0 for the other kernels                      */
  int32_t csort_slot_bytes; /* CSORT: LDS row-slot width (8 = fp64 sums)    */
  int32_t csort_row_blocks; /* CSORT: row blocks per column part (each part
                               has its own nnz-balanced row partition)     */
  /* since 0.3 */
  int32_t rccl_version;     /* ncclGetVersion() of the RCCL this process
                               resolved (librccl.so.1 is one SONAME for the
                               ROCm and the PyTorch copy: the first loaded
                               wins), e.g. 22703 = 2.27.3                   */
  int32_t reserved0;
  int64_t csort_chunks;     /* CSORT: 64*U-entry chunks of the launch       */
  int64_t csort_seg_chunks; /* CSORT: of those, chunks stored slot-sorted
                               (crowded rows summed by a segmented scan)   */
  /* since 1.0 */
  int32_t slab_kernel_rule; /* x-slab handles that have CSR-3 tasks (the
                               AUTO kernel): 1 = CSR3 tasks, since heavy
                               64-row groups (> 2048 nonzeros) hold >= 1/8
                               of the nonzeros; 2 = STREAM groups (balanced
                               groups); 0 = the rule did not apply          */
  int32_t lds_pad;          /* STREAM: 1 = bank-padded LDS product buffers
                               (the typical row of <= 40 nonzeros is a
                               multiple of 16 LDS words long)              */
  double heavy_group_frac;  /* the share of nonzeros in heavy 64-row groups
                               the rule read (0 when it did not apply)     */
  /* since 1.1 (hspmv_get_info_sized only) */
  int32_t csort_fixed_point; /* CSORT: 1 = reproducible fixed-point row sums
                                (hspmv_options.deterministic = 2)           */
  int32_t serial_order;     /* 1: every row is summed in omp_spmv's order
                                (hspmv_options.deterministic = 3): y is bit-
                                identical to spmv-csr/spmv.c:92-114's loop  */
  int64_t csort_part_begin[4]; /* CSORT (GPU 0): first column of column part
                                  h (h < csort_parts; part h ends where h + 1
                                  begins, the last at n); 0 past the parts  */
  int32_t row_slices;       /* 1: the dictionary handle's matrix is stored as
                               row slices and run by the lane-per-row kernel
                               (hspmv_options.row_slices); kernel, x_dict and
                               the other fields read as for the chunked kernel,
                               format_bytes counts the slice format          */
  int32_t slice_pos_bits;   /* bits per dictionary position in the row slices'
                               whole 8-slot groups (hspmv_slices_pack): 12 or
                               16; 0 without row slices (GPU 0)              */
  int32_t sweep;            /* 1: the row kernel changes its sweep direction
                               from one SpMV to the next (hspmv_set_sweep);
                               0: first block to last on every call (GPU 0)  */
  int32_t reserved1;
} hspmv_info;

typedef struct hspmv_handle hspmv_handle;

/* ---------------------------------------------------------------- flags */
#define HSPMV_KERNEL_AUTO 0u   /* the planner's pick by shape: STREAM or
                                  CSR3 tasks (CSR3 over maps when given),
                                  CSORT for irregular gathers; the choice
                                  is in hspmv_info.kernel                 */
#define HSPMV_KERNEL_VECTOR 1u /* L lanes (sub-wave) per row, shuffle sum  */
#define HSPMV_KERNEL_STREAM 2u /* wave per 64-row group, LDS-staged,
                                  ordered per-row sums (bit-exact vs CPU)  */
#define HSPMV_KERNEL_CSR3 3u   /* wave tasks planned from the CSR-3 maps,
                                  4 per workgroup (hspmv_options.csr3_plan:
                                  64-row aligned tasks, super-rows packed
                                  into <= 64-row tasks, or one workgroup
                                  per super-super-row)                     */
#define HSPMV_KERNEL_CSORT 4u  /* column-sorted row blocks: each workgroup
                                  walks its rows' nonzeros in column order,
                                  fp64 LDS row sums (irregular gathers).
                                  NOT bitwise vs omp_spmv and NOT bit-
                                  identical run to run: the sums add in
                                  LDS-atomic order (csort.hip,
                                  hspmv_info.deterministic) -- unless
                                  hspmv_options.deterministic = 2, which
                                  sums in fixed point (reproducible).  AUTO
                                  picks it for HBM-resident matrices whose
                                  gathers are irregular, unless
                                  hspmv_options.deterministic = 1          */
#define HSPMV_KERNEL_MASK 0xFu
/* lanes per row for VECTOR: HSPMV_LANES(L), L in {1,2,4,8,16,32,64}; 0=auto */
#define HSPMV_LANES_SHIFT 4
#define HSPMV_LANES(l) ((unsigned)(l) << HSPMV_LANES_SHIFT)
#define HSPMV_LANES_MASK (0x7Fu << HSPMV_LANES_SHIFT)
#define HSPMV_FLAG_NO_COL16 (1u << 11)    /* keep 32-bit column indices in
                                             the row kernels (see below)   */
#define HSPMV_FLAG_NONTEMPORAL (1u << 12) /* nt loads for val/col streams  */
#define HSPMV_FLAG_DEVICE_PTRS (1u << 13) /* A/maps are device pointers on
                                             the target device (borrowed for
                                             the handle's lifetime; new values:
                                             hspmv_update_values, see
                                             hspmv_csr)                     */
#define HSPMV_FLAG_NO_XCD_REMAP (1u << 14) /* keep dispatch-order blocks    */
/* Default (neither XCD flag): remap only when the matrix's bytes fit the
 * 256 MiB Infinity Cache (<= 192 MiB), where per-XCD L2 reuse of x pays;
 * HBM-resident matrices stream faster in dispatch order (profiles/r01_sweep*). */
#define HSPMV_FLAG_NO_SPLIT (1u << 15)     /* no split-row kernels: very
                                              long rows stay on one wave   */
/* STREAM/CSR3 elements per lane per LDS chunk: HSPMV_U(u), u in {2,3,4,5,6,8,16};
 * 0 = auto from the mean row length */
#define HSPMV_U_SHIFT 16
#define HSPMV_U(u) ((unsigned)(u) << HSPMV_U_SHIFT)
#define HSPMV_FLAG_PREFETCH (1u << 21) /* STREAM/CSR3: software-pipelined
                                          col/val loads one chunk ahead   */
#define HSPMV_FLAG_XCD_REMAP (1u << 22) /* force the XCD-contiguous block
                                           order whatever the size         */
#define HSPMV_FLAG_COL16 (1u << 23)     /* force 16-bit column offsets
                                           whenever p <= 8 (see below)     */
/* Explicit XCD chunk: HSPMV_XCD_CHUNK(s), s a power of two >= 1: each XCD
 * takes s consecutive blocks in turn (1 = dispatch order).  Overrides the
 * two flags above; 0 = automatic. */
#define HSPMV_XCD_CHUNK_SHIFT 24
#define HSPMV_XCD_CHUNK(s) ((unsigned)(__builtin_ctz((unsigned)(s)) + 1) << HSPMV_XCD_CHUNK_SHIFT)
/* STREAM: 64-row groups per wave, HSPMV_GROUPS(g), g in {1,2,4,8,16}; the
 * next group's row pointers are loaded while this one streams.  0 = auto. */
#define HSPMV_GROUPS_SHIFT 29
#define HSPMV_GROUPS(g) ((unsigned)(__builtin_ctz((unsigned)(g)) + 1) << HSPMV_GROUPS_SHIFT)
/* 16-bit column offsets (default when the matrix allows it): at handle
 * creation the column indices are re-encoded per 256-nonzero block as
 * col = base[k / 256] + off16[k] + (p high bits from p bit-planes), with p
 * the fewest bits that cover every block's column span (p = 0 for spans
 * < 65536, e.g. banded matrices); the STREAM and CSR3 kernels then stream
 * 2 + p/8 instead of 4 index bytes per nonzero.  Used by default when p <= 1
 * and the matrix streams from HBM (> 192 MiB); measured slower otherwise.
 * HSPMV_FLAG_COL16 forces them (any size, p <= 8).   Products and summation order are
 * unchanged, so y is bit-identical.  HSPMV_FLAG_NO_COL16 turns it off;
 * hspmv_info.col16 / format_bytes report what a handle uses. */

/* ---------------------------------------------------------------- options */
/* Explicit planner choices for hspmv_create_ex.  Zero-initialise, set
 * struct_size = sizeof(hspmv_options) (a caller built against an older,
 * shorter struct passes its own size; the fields it lacks read as 0), then
 * set what you need: every 0 means "the library's choice", which is what
 * hspmv_create / _on_device / _sharded use.  These replace the HSPMV_*
 * environment variables of earlier versions: a production handle's kernel
 * and tables depend only on the matrix, the flags and these options (only a
 * diagnostic build, `make diag-env`, reads the environment). */
#define HSPMV_CSR3_PLAN_AUTO 0    /* = ALIGNED                                */
#define HSPMV_CSR3_PLAN_ALIGNED 1 /* 64-row aligned wave tasks, 4 per
                                     workgroup (the maps bound the shards)   */
#define HSPMV_CSR3_PLAN_PACKED 2  /* whole super-rows (inner map) packed into
                                     <= 64-row wave tasks                    */
#define HSPMV_CSR3_PLAN_SSR 3     /* one workgroup per super-super-row (outer
                                     map), its super-rows split over W waves
                                     by nonzeros: the reference's cuSpMV_3
                                     mapping (csrk.cu:245-319)               */
#define HSPMV_CSR3_PLAN_ROW_GROUPS 4 /* hspmv_info only: a CSR matrix (no
                                     maps) run by the CSR3 kernel over 64-row
                                     groups with the heavy ones cut         */
#define HSPMV_DETERMINISTIC_ORDERED 1
#define HSPMV_DETERMINISTIC_REPRODUCIBLE 2
#define HSPMV_DETERMINISTIC_SERIAL 3
typedef struct {
  uint32_t struct_size;   /* sizeof(hspmv_options) of the caller            */
  uint32_t flags;         /* HSPMV_KERNEL_* | HSPMV_FLAG_* (hspmv_create)    */
  const int *devices;     /* row-range shard p on devices[p] (may repeat), as
                             hspmv_create_sharded; NULL: one shard on device */
  int32_t n_devices;
  int32_t device;         /* single-shard handle: the HIP device ...         */
  void *stream;           /* ... and its hipStream_t (NULL: library-owned)  */
  int32_t csr3_plan;      /* HSPMV_CSR3_PLAN_*                              */
  int32_t task_nnz;       /* CSR3 wave-task nonzero budget (0: 2048)        */
  int32_t x_windows;      /* -1: no LDS x windows; 0 auto                   */
  int32_t x_dict;         /* -1 off, 0 auto, 1 whenever it fits the cap     */
  int32_t x_dict_cap;     /* LDS bytes per dictionary block (0: 20 KiB)     */
  int32_t x_slabs;        /* -1 off, 0 auto, B > 0: B column slabs          */
  int32_t col16_group;    /* -1 off, 0 auto, 1 whenever every group fits    */
  int32_t csort;          /* -1 off, 0 auto, 1 whenever it can be built     */
  int32_t csort_parts;    /* column parts of the csort row blocks: 0 auto,
                             1, 2, 4                                        */
  int32_t csort_chunk_u;  /* csort entries per lane per chunk: 0, 4, 8, 16  */
  int32_t stream_waves;   /* STREAM waves per workgroup: 0 auto, 1, 2, 4    */
  int32_t deterministic;  /* HSPMV_DETERMINISTIC_*: 0 the fastest kernel
                             (CSORT's fp64 slot sums add in LDS-atomic
                             order); 1 ORDERED: only the row kernels (bit-
                             identical run to run; rows of <= 40 (fp32: 56) nonzeros
                             added in omp_spmv's order, longer ones in fixed
                             trees); 2 REPRODUCIBLE: bit-identical run to
                             run for a finite x -- CSORT then runs with
                             fixed-point (int64) row sums: each product
                             rounded once to 2^-50 of |its row's largest
                             value| * |x|max (hspmv_info.csort_fixed_point);
                             3 SERIAL: the row kernels add EVERY row left to
                             right from 0, one lane per row, as omp_spmv
                             does (spmv-csr/spmv.c:92-114): y bit-identical
                             to it for every input, at the cost of long rows
                             added one product at a time (rows over 4096
                             nonzeros: one workgroup each, or with
                             HSPMV_FLAG_NO_SPLIT their lane; VECTOR and CSORT
                             refused; a matrix the row kernels cannot
                             address fails with HSPMV_E_INVALID;
                             hspmv_info.serial_order)                      */
  int32_t placement_trials; /* array placements timed at creation (0/1
                               off, K <= 8; see hspmv_create_on_device)    */
  int32_t row_slices;     /* row slices (hspmv_slices_plan): -1 off, 0 auto
                             (eligible handles that stream from HBM and whose
                             padded format moves no more bytes), 1 whenever
                             the kernel can run the handle (the rules
                             HSPMV_SLICES_BYTES and _RESIDENT are auto's).
                             y is the same bit for bit                      */
} hspmv_options;

/* ---------------------------------------------------------------- handle */
/* hspmv_create_on_device / hspmv_create_sharded with explicit options
 * (opt == NULL: all defaults on device 0). */
int hspmv_create_ex(hspmv_handle **h, const hspmv_csr *A, const hspmv_csr3_maps *maps,
                    const hspmv_options *opt);

/* Mixed precision: the matrix values stored and streamed in A->dtype, while x,
 * y, every product and every partial sum are vector_dtype.
 *   vector_dtype == A->dtype              exactly hspmv_create_ex;
 *   A->dtype HSPMV_F32, vector HSPMV_F64  the mixed handle;
 *   anything else (fp64 values with fp32 vectors, an unknown code)
 *                                          HSPMV_E_INVALID.
 * A mixed handle reads 4 instead of 8 bytes per stored value; x given to
 * hspmv_set_x / hspmv_bind_x_device and y from hspmv_get_y / bound with
 * hspmv_bind_y_device are fp64, and with HSPMV_FLAG_DEVICE_PTRS the borrowed
 * val is fp32.  Every other entry point works on it as on any handle.
 * hspmv_info reports the mixed format: alg_bytes = nnz*(4+4) + (m+1)*4 +
 * (x_entries + m)*8 (+ the map terms of hspmv_alg_bytes), format_bytes and
 * device_bytes count 4-byte values, and hspmv_run's gbps_alg uses the same
 * alg_bytes.
 *
 * Semantics and order contract.  Each value is widened to fp64 once, before
 * its product (exact), so y is what the fp64 operator gives for the widened
 * matrix, and the handle follows fp64's rules: rows of up to 40 nonzeros
 * (not fp32's 56) are summed serially, bit-identical to omp_spmv in fp64 on
 * the widened values and to an fp64 handle with the same options on the
 * widened matrix, in every row kernel and plan; with deterministic = 3 every
 * row is; longer rows are within the fp64 tolerance.  The split-row
 * threshold, the x-dictionary LDS cap (8-byte x entries), chunk_u, the LDS
 * padding and the other launch-shape picks are fp64's, because the LDS
 * product buffers hold fp64.  The footprint rules -- the Infinity Cache
 * residence test, the row slices' byte rule, the "streams from HBM" rule of
 * the 16-bit columns and the sweep's AUTO rule -- are the same derivations
 * with 4 value bytes and 8 vector bytes: footprint = nnz*(4+4) + m*(8+4) +
 * n*8; slices: 64*padded*(4+2) + m + 8*(tasks+1) against nnz*(4+2) +
 * 4*(m+1).  For equal dtypes every rule evaluates exactly as before.
 * Kernels: STREAM, CSR3 (every plan), the row-slice kernel (value groups of
 * four fp32 slots per 16-byte load, positions unchanged), VECTOR and the
 * split-row kernels.  No column-sorted kernel: AUTO plans as under
 * deterministic = 1 (row kernels, x slabs for irregular gathers), and
 * HSPMV_KERNEL_CSORT or hspmv_options.csort = 1 returns HSPMV_E_INVALID;
 * deterministic = 2 is accepted and runs the row kernels, which are
 * reproducible.  placement_trials copies 4-byte values.
 *
 * Out of scope: multi-GPU shards (opt->n_devices > 1 returns
 * HSPMV_E_INVALID), CSORT, hspmv_mm_* with mixed types, fp64 values with fp32
 * vectors, bf16 / fp16 storage, automatic narrowing of an fp64 handle (the
 * caller decides, with hspmv_values_fit_f32), and launch-shape rules tuned
 * for the mixed kernels beyond the derivations above.
 * The argument refusals (NULL, the dtype pair, n_devices, CSORT) are made
 * before any device call. */
int hspmv_create_mixed(hspmv_handle **h, const hspmv_csr *A, const hspmv_csr3_maps *maps,
                       const hspmv_options *opt, int vector_dtype);
/* The stored values' and the vectors' hspmv_dtype of a handle (equal for every
 * handle but hspmv_create_mixed's).  Either pointer may be NULL. */
int hspmv_get_dtypes(hspmv_handle *h, int *value_dtype, int *vector_dtype);
/* Host only: 1 when every one of the nnz values of `dtype` converts to fp32
 * and back to the same bits (an fp32 array trivially; a NaN when its round
 * trip gives the same bits; -0.0 and +-inf do), so a mixed handle over the
 * narrowed values computes the fp64 operator's y bit for bit; else 0, with
 * *first_bad (may be NULL) = the first index that fails.  Negative
 * (HSPMV_E_INVALID) for a NULL array with nnz > 0, nnz < 0 or an unknown
 * dtype. */
int hspmv_values_fit_f32(const void *val, int64_t nnz, int dtype, int64_t *first_bad);

/* Upload A (and optional CSR-3 maps) to num_gpus devices (0 = all visible).
 * With num_gpus > 1 the rows are partitioned into nnz-balanced contiguous
 * ranges (on super-super-row boundaries when maps are given), x is
 * broadcast and y gathered with RCCL.  Replaces the CSRk_Graph constructor +
 * the H2D uploads of csrk.cu:580-587 / 847-865 and cuda-spmv-csr/spmv.cu:66-71. */
int hspmv_create(hspmv_handle **h, const hspmv_csr *A,
                 const hspmv_csr3_maps *maps, int num_gpus, unsigned flags);

/* The row-range partition of hspmv_create over an explicit device list:
 * shard p lives on devices[p] (n_shards >= 1; a device may repeat).  Distinct
 * devices exchange x / y through RCCL (ncclCommInitAll over the list, also
 * at n_shards = 1); a list that repeats a device exchanges by device-to-
 * device copies.  hspmv_create(num_gpus > 1) is this with devices 0..P-1. */
int hspmv_create_sharded(hspmv_handle **h, const hspmv_csr *A,
                         const hspmv_csr3_maps *maps, const int *devices,
                         int n_shards, unsigned flags);

/* Single-device handle on `device`, launching on `stream` (a hipStream_t;
 * NULL = the library creates one).  This is the entry a one-process-per-GPU
 * caller (torch.distributed, MPI) uses for its row-range shard.
 * Placement trials: for a handle that owns its arrays (no
 * HSPMV_FLAG_DEVICE_PTRS) and whose STREAM / CSR3 kernel streams from HBM,
 * the row pointers, column stream, values, x and y are copied into up to
 * three further allocations, each copy is timed over a few SpMVs and the
 * fastest placement is kept (the others are freed; y bits do not depend on
 * it).  Opt-in: hspmv_options.placement_trials = K (K <= 8 sets; default
 * off -- measured no gain); hspmv_info reports the times.  With trials
 * on, creation launches the kernel. */
int hspmv_create_on_device(hspmv_handle **h, const hspmv_csr *A,
                           const hspmv_csr3_maps *maps, int device,
                           void *stream, unsigned flags);

/* New matrix values for a planned handle, in place: the pattern is the same,
 * the numbers are not (a Newton or time step, another load case, a refinement
 * sweep).  val holds nnz values in the CSR order of the matrix the handle was
 * created from -- for a sharded handle the global matrix -- in the handle's
 * stored value dtype (hspmv_get_dtypes; fp32 for a mixed handle).  The pattern
 * (row_ptr, col_idx, the maps) is unchanged by contract; nothing re-validates
 * it.
 *
 * Contract: every later hspmv_spmv / hspmv_run gives bit for bit the y of a
 * handle newly created with the same arguments and options from the same
 * pattern with val, on every row and in every supported plan.  The plan, the
 * tables, hspmv_info (device_bytes included) and the sweep phase are untouched:
 * only the values move -- into the CSR-order array, and from there, by small
 * kernels on the handle's stream, into the row slices' and the x slabs' own
 * copies and, for a handle from hspmv_create_updatable, into the
 * column-sorted entry stream (with the fixed-point row scales restated first:
 * the device tables are then byte for byte a new handle's).
 *
 * flags = 0: val is host memory.  It is consumed before return (hspmv_set_x's
 * rule); works on single-device and sharded handles, shard p taking its range
 * of nonzeros.  A row-slice handle, which keeps no CSR-order values, stages
 * them in a device allocation of nnz values that is released before return.
 * HSPMV_VALUES_DEVICE: val is a device pointer on the handle's device;
 * single-device handles only.  Everything is enqueued on the handle's stream,
 * after the SpMVs enqueued so far and before later ones, with no host
 * synchronisation and no allocation; val must stay unchanged until that stream
 * work is done.
 * A handle over borrowed arrays (HSPMV_FLAG_DEVICE_PTRS) takes
 * HSPMV_VALUES_DEVICE only: val == NULL means "I changed my array in place,
 * refresh what you derived from it"; another pointer is the borrowed array
 * from then on.
 *
 * HSPMV_E_INVALID, the handle unchanged (every check is made, for every shard,
 * before anything is written): a NULL handle, unknown flag bits, a NULL val
 * on a handle that owns its matrix (nnz > 0), host memory for a borrowed
 * handle, HSPMV_VALUES_DEVICE on a sharded handle, a handle any shard of
 * which runs the column-sorted kernel (hspmv_info.kernel ==
 * HSPMV_KERNEL_CSORT) without having been created by hspmv_create_updatable
 * -- create it with that call, or with hspmv_options.csort = -1 or
 * deterministic = 1, to update it; hspmv_can_update_values asks beforehand --
 * and, for host memory, an Inf or NaN among the new values of a handle whose
 * column-sorted slots are fixed-point (hspmv_info.csort_fixed_point): a new
 * handle over such values keeps fp64 slots, so no update in place can equal
 * it.  nnz == 0: HSPMV_OK, nothing done.
 * Non-finite values from a device pointer are not looked at (that would take
 * a host synchronisation): keeping them out of a fixed-point column-sorted
 * handle is the caller's duty.  Indices never depend on values, so the worst
 * outcome is a non-finite or unspecified y in the rows concerned, never an
 * access out of range.
 *
 * Not covered: column-sorted handles created by any other call than
 * hspmv_create_updatable (their entries are sorted by column inside each
 * block, which only the stored source index per entry undoes); converting the
 * dtype on the way (fp64 input into a mixed handle: narrow it first); a
 * changed pattern; device pointers for sharded handles. */
#define HSPMV_VALUES_DEVICE 1u  /* val is a device pointer on the handle's device */
int hspmv_update_values(hspmv_handle *h, const void *val, unsigned flags);

/* hspmv_create_mixed -- with vector_dtype == A->dtype: hspmv_create_ex -- whose
 * handle takes hspmv_update_values in every plan, the column-sorted one
 * included: every shard that builds column-sorted tables also keeps, on the
 * device, the CSR index each entry of its (padded) entry stream came from, 4
 * bytes per stored entry (hspmv_info.csort_chunks * 64 * chunk_u entries).
 * That memory is why this is a call of its own and not the default.  The
 * planner's pick, every table the SpMV reads, y and hspmv_info are those of
 * the handle the other call creates; hspmv_info.device_bytes alone may differ.
 * Every argument, refusal and error is hspmv_create_mixed's. */
int hspmv_create_updatable(hspmv_handle **h, const hspmv_csr *A, const hspmv_csr3_maps *maps,
                           const hspmv_options *opt, int vector_dtype);
/* 1 when hspmv_update_values would not refuse the handle for its plan (the
 * rule it applies to every shard: not the column-sorted kernel, or created by
 * hspmv_create_updatable), else 0; 0 for a NULL handle.  Host only: no device
 * call, and hspmv_last_error is left alone. */
int hspmv_can_update_values(const hspmv_handle *h);

/* x (n entries of dtype) from host memory -> every GPU (setX, csrk.cu:92-102,
 * minus the x permutation: matrices are used as given). */
int hspmv_set_x(hspmv_handle *h, const void *x_host);
/* Bind caller-owned device vectors (single-device handles).  x: n entries,
 * y: m entries, on the handle's device.  NULL restores the handle's own. */
int hspmv_bind_x_device(hspmv_handle *h, const void *x_dev);
int hspmv_bind_y_device(hspmv_handle *h, void *y_dev);
/* Device pointers currently used for x / y on GPU `gpu`. */
void *hspmv_x_device(hspmv_handle *h, int gpu);
void *hspmv_y_device(hspmv_handle *h, int gpu);

/* Enqueue ONE y = A*x on the handle's stream(s).  Asynchronous; the hot path. */
int hspmv_spmv(hspmv_handle *h);
int hspmv_synchronize(hspmv_handle *h);

/* Enqueue ONE y = alpha*A*x + beta*y on the handle's stream: the general form
 * a residual (r = b - A x: alpha = -1, beta = 1 over y = b), a Newton or time
 * step and a CG-shaped loop need, without the spare vector and the separate
 * update they otherwise run after hspmv_spmv.
 *
 * Contract.  For every row r, with T the handle's vector dtype
 * (hspmv_get_dtypes; double for a mixed handle) and alpha_T, beta_T the two
 * scalars converted to T once, on the host:
 *     s    = the bits hspmv_spmv would write to y[r] for this handle, plan and x
 *     y[r] = fl( fl(alpha_T * s) + fl(beta_T * y_old[r]) )    if beta_T != 0
 *     y[r] = fl(alpha_T * s)                                  if beta_T == 0
 * Each operation is rounded on its own, no fma.  beta_T == 0 never reads
 * y_old, so a NaN or Inf there does not propagate (beta == 0 always converts
 * to 0; so does a double too small for an fp32 handle).  alpha = 1, beta = 0
 * gives hspmv_spmv's bytes.  There is no other shortcut: alpha == 0 still
 * forms s, so a NaN of A x shows.  y_old is what the handle's y holds at the
 * call: its own buffer (hspmv_set_y fills it) or the array bound by
 * hspmv_bind_y_device.  The call is enqueued with no host synchronisation and
 * advances the sweep phase exactly as hspmv_spmv does: a handle that
 * alternates its sweep keeps alternating across mixed hspmv_spmv and
 * hspmv_spmv_axpby calls.
 *
 * Two paths, the same bytes.  A handle whose plan is the row slices
 * (hspmv_info.row_slices) runs one kernel, the slice kernel with the epilogue
 * in place of its store (fused: one extra pass over m elements, the read of
 * y_old).  Every other plan runs hspmv_spmv's launches into a scratch vector
 * of m elements the handle owns, then one elementwise kernel (two-pass).  The
 * scratch is allocated by the first two-pass call (the only call that
 * allocates), freed with the handle and counted in hspmv_info.device_bytes
 * from then on.  hspmv_set_axpby_path(h, HSPMV_AXPBY_TWO_PASS) forces the
 * two-pass path (HSPMV_AXPBY_AUTO, the default: fused where it can run; other
 * modes HSPMV_E_INVALID); hspmv_axpby_path returns the path the next call
 * takes, HSPMV_AXPBY_PATH_TWO_PASS or HSPMV_AXPBY_PATH_FUSED.
 *
 * HSPMV_E_INVALID, decided before anything is launched, y untouched: a NULL
 * handle; a sharded handle (more than one shard, repeated devices included --
 * hspmv_set_y, hspmv_run_axpby and hspmv_axpby_path refuse it too); x and y
 * the same device pointer.  HSPMV_E_STATE: x not set.
 *
 * Not covered: sharded handles; hspmv_mm_*; the epilogue inside the chunked,
 * vector and column-sorted kernels (they take the two-pass path). */
#define HSPMV_AXPBY_AUTO 0
#define HSPMV_AXPBY_TWO_PASS 1
#define HSPMV_AXPBY_PATH_TWO_PASS 1
#define HSPMV_AXPBY_PATH_FUSED 2
int hspmv_spmv_axpby(hspmv_handle *h, double alpha, double beta);
int hspmv_set_axpby_path(hspmv_handle *h, int mode);
int hspmv_axpby_path(hspmv_handle *h);
/* y (m entries of the vector dtype) from host memory into the handle's y in
 * use -- its own buffer, or the array bound by hspmv_bind_y_device -- as
 * hspmv_set_x does for x: consumed before return.  Single-device handles. */
int hspmv_set_y(hspmv_handle *h, const void *y_host);

/* hspmv_spmv_axpby and, from the pass that writes y, the two dot products an
 * iterative solver takes next: p . Ap, the residual's r . r, BiCGStab's
 * r0 . Ap, t . s and t . t, the Rayleigh quotient x . A x -- without a further
 * launch and a further read of y for each.
 *
 * Contract.  y is byte for byte what hspmv_spmv_axpby(h, alpha, beta) writes:
 * the three roundings, beta_T == 0 never reads y, alpha = 1 and beta = 0 give
 * hspmv_spmv's bytes, and the sweep phase advances once per call.  With y_new
 * the values stored (in T, the vector dtype) and `which` a mask of
 * HSPMV_DOT_WY and HSPMV_DOT_YY (0 and any other bit: HSPMV_E_INVALID):
 *     dots[0] = sum over the m rows of (double)w[r] * (double)y_new[r]   HSPMV_DOT_WY
 *     dots[1] = sum over the m rows of (double)y_new[r]^2                HSPMV_DOT_YY
 * Products and sums are double for every handle (an fp32 handle's products
 * are then exact); a slot `which` does not name is written as 0.0; without
 * HSPMV_DOT_WY w is never read and need not exist.  Non-finite values
 * propagate as IEEE 754 says (a NaN of y_old under beta = 0 reaches neither y
 * nor the dots).
 *
 * Order.  The summation order is fixed per handle and path: it depends on
 * neither the sweep direction, nor the order the grid's workgroups run in,
 * nor earlier calls, and no floating-point atomic is used.  The same handle,
 * x, w and y_old give the same 16 bytes on every call.  The two paths (below)
 * sum in different orders: their dots may differ in the last bits, each
 * within (m + 4) 2^-53 sum |terms| of the exact sum.
 *
 * Where the results live.  On the device: 2 doubles {wy, yy} the handle owns,
 * or the array bound by hspmv_bind_dots_device (2 doubles on the handle's
 * device, 8-byte aligned; NULL: back to the handle's own).  The call is
 * enqueued on the handle's stream with no host synchronisation, like
 * hspmv_spmv: work that follows on that stream reads the bound array without
 * a round trip.  hspmv_get_dots synchronises the stream and copies the pair
 * the last dot call wrote.
 *
 * w.  m entries of the vector dtype: hspmv_set_w copies them from host memory
 * into a buffer the handle owns and uses that; hspmv_bind_w_device uses the
 * caller's device array (NULL: back to the handle's own).  w[r] is read only
 * by the lane or thread that owns row r.  w may be x (p . Ap; the caller
 * vouches for m entries); w the same pointer as y is HSPMV_E_INVALID: ask for
 * HSPMV_DOT_YY.
 *
 * Two paths, as for hspmv_spmv_axpby and chosen by the same rule
 * (hspmv_axpby_path, hspmv_set_axpby_path): fused, the slice kernel forms the
 * terms from the values it stores and each wave writes its slice's pair;
 * two-pass, the elementwise kernel does and each workgroup writes its pair.
 * One small kernel of a fixed launch shape then adds the pairs.
 *
 * Refusals, all before any launch, y and the dots untouched.
 * HSPMV_E_INVALID: a NULL handle; a sharded handle (the five other calls
 * below refuse it too); x and y the same device pointer; w and y the same; a
 * bad `which`.  HSPMV_E_STATE: x not set; HSPMV_DOT_WY with no w set or
 * bound; hspmv_get_dots before any dot call.
 *
 * Device memory: the handle's own w, the partial pairs and the own result are
 * allocated by the first call that needs each, counted in
 * hspmv_info.device_bytes from then on and freed with the handle; later calls
 * allocate nothing.
 *
 * Not covered: sharded handles; hspmv_mm_*; the dot epilogue inside the
 * chunked, vector and column-sorted kernels (they take the two-pass path); a
 * single-launch finish; bitwise equality of the two paths' dots. */
#define HSPMV_DOT_WY 1u
#define HSPMV_DOT_YY 2u
int hspmv_spmv_axpby_dot(hspmv_handle *h, double alpha, double beta, unsigned which);
int hspmv_set_w(hspmv_handle *h, const void *w_host);
int hspmv_bind_w_device(hspmv_handle *h, const void *w_dev);
int hspmv_bind_dots_device(hspmv_handle *h, double *dots_dev);
int hspmv_get_dots(hspmv_handle *h, double out[2]);

/* Sweep direction of the STREAM / CSR3 row kernel (the row-slice kernel
 * included) from one SpMV of this handle to the next.  A matrix larger than
 * the 256 MiB Infinity Cache that is swept first block to last on every call
 * finds none of its bytes there: each line's reuse distance is the whole
 * matrix.  With HSPMV_SWEEP_ALTERNATE every other hspmv_spmv (and every other
 * timed or warm-up iteration of hspmv_run) runs the row kernel's workgroups
 * last block to first, so a call starts on the bytes the previous call
 * touched last.  y is bit-identical in both directions: a row's sum never
 * leaves its workgroup, only the order of the workgroups changes.  Every
 * shard of a call takes the same direction; the launches of a multi-launch
 * SpMV keep their order, and the vector, column-sorted and split-row kernels
 * always run forward.  HSPMV_SWEEP_AUTO (the default) alternates where the
 * shard runs one row-kernel launch (no x slabs) over a matrix that does not
 * fit the cache, and stays forward otherwise; HSPMV_SWEEP_FORWARD is first to
 * last on every call.  Takes effect from the next call; other modes return
 * HSPMV_E_INVALID.  hspmv_info.sweep reports the outcome.  A call captured
 * into a HIP graph replays the direction it was captured with (no gain, no
 * loss against FORWARD).  As before, one handle is not to be driven from two
 * threads at once: the direction is state of the handle. */
#define HSPMV_SWEEP_AUTO 0
#define HSPMV_SWEEP_FORWARD 1
#define HSPMV_SWEEP_ALTERNATE 2
int hspmv_set_sweep(hspmv_handle *h, int mode);
/* The row kernels' block order as the host sees it: order[b] = the logical
 * block that grid index b runs among n_blocks, with xcd_chunk blocks per XCD
 * turn (hspmv_info.xcd_remap; <= 1: dispatch order) and, reverse != 0, the
 * mirrored sweep.  A bijection on [0, n_blocks); no device involved. */
int hspmv_block_order(int64_t n_blocks, int32_t xcd_chunk, int reverse, int32_t *order);

/* Reference timing protocol: warmup SpMVs, then iters timed SpMVs, each
 * bracketed by events + synchronize (hip/spmv-auto-mi100.cu:214-236). */
int hspmv_run(hspmv_handle *h, int warmup, int iters, hspmv_timing *out);
/* hspmv_run's protocol over hspmv_spmv_axpby(h, alpha, beta), with its
 * refusals.  y is not reset between iterations: it evolves from call to call
 * (y_k+1 = alpha A x + beta y_k), so the caller keeps |beta| < 1 for it to
 * stay finite over warmup + iters calls.  gflops = 2 nnz / t_min; gbps_alg
 * counts hspmv_alg_bytes plus, for beta != 0, the m elements of y_old read. */
int hspmv_run_axpby(hspmv_handle *h, double alpha, double beta, int warmup, int iters, hspmv_timing *out);
/* The same over hspmv_spmv_axpby_dot(h, alpha, beta, which), with its
 * refusals; gbps_alg adds the m elements of w under HSPMV_DOT_WY.  The dots
 * are those of the last iteration. */
int hspmv_run_axpby_dot(hspmv_handle *h, double alpha, double beta, unsigned which, int warmup, int iters,
                        hspmv_timing *out);

/* y (m entries of dtype) -> host; gathers the shards of a multi-GPU handle
 * (getY, csrk.cu:110-113). */
int hspmv_get_y(hspmv_handle *h, void *y_host);

/* Multi-GPU only: RCCL broadcast of x from GPU 0 and all-gather of y into
 * every GPU's full-length buffer, timed (seconds).  Either pointer may be NULL. */
int hspmv_exchange(hspmv_handle *h, double *bcast_x_s, double *gather_y_s);

/* Fills the 1.0 layout of hspmv_info -- exactly HSPMV_INFO_SIZE_1_0 bytes,
 * in every 1.x library, so a 1.0 binary's stack struct is never overrun
 * when a later minor grows hspmv_info (NULL -> E_INVALID).  Fields added
 * after 1.0 come only from hspmv_get_info_sized. */
#define HSPMV_INFO_SIZE_1_0 248
int hspmv_get_info(hspmv_handle *h, hspmv_info *out);
/* Fills min(out_size, sizeof(hspmv_info)) bytes: pass sizeof(hspmv_info) of
 * the header you were built against. */
int hspmv_get_info_sized(hspmv_handle *h, hspmv_info *out, uint32_t out_size);
void hspmv_destroy(hspmv_handle *h);

/* ---------------------------------------------------------------- SpMM */
/* Multi-vector product Y = A X for k right-hand sides (1 <= k <= 32) in one
 * pass over A: what block CG / block GMRES, eigensolvers with a block of
 * vectors and many-load-case solves call instead of k SpMVs, each of which
 * streams the whole matrix from HBM.  A second, small operator beside
 * hspmv_handle: it keeps A as plain CSR (a single-vector handle's formats --
 * 16-bit columns, dictionaries, row slices -- are built for one vector).
 *
 * X is ROW-MAJOR n x k with leading dimension ldx >= k (the k values of one
 * row contiguous; element (i, c) at X[i * ldx + c]), Y row-major m x k with
 * ldy >= k: a contiguous torch / numpy array of shape (n, k) binds as it is,
 * ldx = k.  Columns c >= k of a padded X are never read and those of Y never
 * written.
 *
 * Order contract: for every row of at most serial_max nonzeros (40 in fp64,
 * 56 in fp32; hspmv_mm_info.serial_max) column c of Y is bit for bit what
 * omp_spmv (spmv-csr/spmv.c:92-114) gives for x = X[:, c] -- products rounded,
 * added left to right from 0, no fma -- which is also what the ordered kernels
 * behind hspmv_spmv give on those rows.  Longer rows are summed by one wave per
 * row in a fixed order: bit-identical run to run, within the usual tolerance
 * of omp_spmv.  Rows over 4096 nonzeros stay on one wave in this version.
 *
 * From hspmv_options only struct_size, flags (HSPMV_FLAG_DEVICE_PTRS and
 * HSPMV_FLAG_NONTEMPORAL; the kernel code must be HSPMV_KERNEL_AUTO), device
 * and stream are read; every other field is ignored (n_devices > 1 is
 * refused).  NULL: defaults on device 0.
 *
 * Out of scope: multi-GPU shards, k > 32, CSR-3 maps, x dictionaries or row
 * slices for X, column-major X, alpha / beta scaling, splitting rows over
 * 4096 nonzeros across workgroups. */
typedef struct hspmv_mm hspmv_mm;
typedef struct {
  int32_t k, lanes_per_row, rows_per_wave, waves_per_block;
  int64_t blocks;          /* main-kernel grid */
  int64_t long_rows;       /* rows run by the wave-per-row kernel */
  int32_t serial_max;      /* rows up to this length carry omp_spmv's bits */
  int32_t reserved0;
  double alg_bytes;        /* nnz*(sv+4) + (m+1)*4 + (x_entries + m)*k*sv */
  double flops;            /* 2 * nnz * k */
  int64_t device_bytes;
} hspmv_mm_info;

int hspmv_mm_create(hspmv_mm **mm, const hspmv_csr *A, int32_t k, const hspmv_options *opt);
/* hspmv_update_values for the operator, which keeps plain CSR: nnz values of
 * A's dtype in CSR order, from host memory (flags = 0; consumed before return)
 * or a device pointer (HSPMV_VALUES_DEVICE; a copy on the operator's stream,
 * ordered with its SpMMs) into the operator's own values.  An operator over
 * borrowed arrays reads the caller's val on every SpMM, so it takes
 * HSPMV_VALUES_DEVICE only: NULL is accepted and does nothing, another pointer
 * is the borrowed array from then on.  HSPMV_E_INVALID: a NULL operator,
 * unknown flag bits, a NULL val on an owned operator (nnz > 0), host memory
 * for a borrowed one. */
int hspmv_mm_update_values(hspmv_mm *mm, const void *val, unsigned flags);
/* X (row-major n x k, ldx >= k) from host memory into the operator's own
 * buffer, which becomes the X in use. */
int hspmv_mm_set_x(hspmv_mm *mm, const void *X_host, int64_t ldx);
/* Y in use (own or bound) -> host, row-major m x k with ldy >= k; padding
 * columns of Y_host are left as they are.  Synchronizes the stream. */
int hspmv_mm_get_y(hspmv_mm *mm, void *Y_host, int64_t ldy);
/* Bind caller-owned device arrays on the operator's device (X: n rows of ldx
 * elements, Y: m rows of ldy).  NULL restores the operator's own buffer
 * (leading dimension k). */
int hspmv_mm_bind_x_device(hspmv_mm *mm, const void *X_dev, int64_t ldx);
int hspmv_mm_bind_y_device(hspmv_mm *mm, void *Y_dev, int64_t ldy);
/* Enqueue ONE Y = A X on the operator's stream.  Asynchronous. */
int hspmv_mm_spmm(hspmv_mm *mm);
int hspmv_mm_synchronize(hspmv_mm *mm);
/* The timing protocol of hspmv_run; gflops = 2 nnz k / t_min, gbps_alg =
 * hspmv_mm_info.alg_bytes / t_min. */
int hspmv_mm_run(hspmv_mm *mm, int warmup, int iters, hspmv_timing *out);
/* Fills min(out_size, sizeof(hspmv_mm_info)) bytes. */
int hspmv_mm_get_info(hspmv_mm *mm, hspmv_mm_info *out, uint32_t out_size);
void hspmv_mm_destroy(hspmv_mm *mm);

/* ---------------------------------------------------------------- formats */
/* Text .csr reader (spmv-csr/spmv.c:11-57 layout; index base auto-detected
 * from row_ptr[0]; values parsed correctly rounded into dtype). */
int hspmv_read_csr(const char *path, int dtype, hspmv_csr_buf *out);
/* Text .csr3 reader (reformat-csr-to-csr3/stats.c:10-79 layout). */
int hspmv_read_csr3(const char *path, int dtype, hspmv_csr_buf *A,
                    hspmv_csr3_buf *maps);
/* Matrix Market coordinate reader (the input of the reference's converter,
 * helpers/converter.m:1-50 with helpers/mmread.m): field real | integer |
 * pattern, symmetry general | symmetric | skew-symmetric (symmetric files
 * expanded as A + A.' - diag(diag(A)), mmread.m:207-209); duplicates summed,
 * exact zeros dropped, columns sorted per row (helpers/sparse2csr.m). */
int hspmv_read_mtx(const char *path, int dtype, hspmv_csr_buf *out);
/* Writers (reference text layouts: helpers/sparse2csr.m:1-7 for .csr,
 * reformat-csr-to-csr3/spmv-auto.cpp:30-65 for .csr3; values "%.6f"). */
int hspmv_write_csr(const char *path, const hspmv_csr *A);
int hspmv_write_csr3(const char *path, const hspmv_csr *A,
                     const hspmv_csr3_maps *maps);
/* Binary cache: raw little-endian arrays. */
int hspmv_save_bin(const char *path, const hspmv_csr *A,
                   const hspmv_csr3_maps *maps);
int hspmv_load_bin(const char *path, hspmv_csr_buf *A, hspmv_csr3_buf *maps);
void hspmv_free_csr(hspmv_csr_buf *A);
void hspmv_free_csr3(hspmv_csr3_buf *maps);

/* ---------------------------------------------------------------- CSR-3 */
/* Build CSR-3 maps in file order with the handCoarsen grouping rule
 * (csrk.cu:1438-1484) and level thresholds supRowSizes[i-1]*NNZ/N
 * (csrk.cu:1089-1091).  ssrs = rows->super-rows size, srs =
 * super-rows->super-super-rows size. */
int hspmv_build_csr3_maps(const hspmv_csr *A, int ssrs, int srs,
                          hspmv_csr3_buf *out);
/* The full band-k build of CSRk_Graph::putInCSRkFormat with k = 3 and HAND
 * coarsening (BAND_k::preprocessingForSpMV, csrk.cu:1035-1262; reorderA
 * :722-870): super-rows by the handCoarsen rule, RCM on the super-row graph,
 * super-super-rows over the RCM order, RCM on that graph, uncoarsening into
 * one symmetric permutation.  Outputs the permuted matrix (columns sorted
 * per row; *A_out allocated, free with hspmv_free_csr), its maps (*maps_out,
 * free with hspmv_free_csr3) and, if perm != NULL, perm[m]: new row i is row
 * perm[i] of A (so y = P^T y_out, x_out[i] = x[perm[i]]).  A must be square.
 * Replaces what reformat-csr-to-csr3 (spmv-auto.cpp:183-195) writes. */
int hspmv_build_csr3_bandk(const hspmv_csr *A, int ssrs, int srs, hspmv_csr_buf *A_out,
                           hspmv_csr3_buf *maps_out, int32_t *perm);
/* CSR-2 (one map level; spmv-csrk <file> <num_runs> <super_row_size>,
 * spmv-csrk/spmv.cpp:97-128 with CSRK_LEVEL 2, cuda-spmv-csrk/cuda/spmv.cu:130):
 * super-rows of super_row_size * NNZ / N nonzeros (handCoarsen rule), each
 * its own super-super-row (outer = identity), so every CSR-3 consumer takes
 * it unchanged.  _maps keeps the file order; _bandk also RCM-orders the
 * super-row graph and permutes A as the k = 2 band-k build does
 * (csrk.cu:1072-1096: one coarsening + RCM), outputs as
 * hspmv_build_csr3_bandk. */
int hspmv_build_csr2_maps(const hspmv_csr *A, int super_row_size, hspmv_csr3_buf *out);
int hspmv_build_csr2_bandk(const hspmv_csr *A, int super_row_size, hspmv_csr_buf *A_out,
                           hspmv_csr3_buf *maps_out, int32_t *perm);
/* Reverse Cuthill-McKee of A's symmetrised pattern: the ordering the
 * reference's converter applies before writing X.mtx.rcm.csr
 * (helpers/converter.m:14-15, Octave symrcm; tie-breaking not pinned).
 * Outputs P A P^T (columns sorted; free with hspmv_free_csr) and, if
 * perm != NULL, perm[m]: new row i is row perm[i] of A.  A must be square. */
int hspmv_rcm_reorder(const hspmv_csr *A, hspmv_csr_buf *A_out, int32_t *perm);
/* Auto parameters.  flavour 0: the .csr3 writer / Volta formula
 * (reformat-csr-to-csr3/spmv-auto.cpp:154-173); 1: the MI100 driver formula
 * (hip/spmv-auto-mi100.cu:130-158); 2: this library's MI355X choice. */
int hspmv_csr3_params(double nnz_per_row, int flavour, int *ssrs, int *srs);

/* ---------------------------------------------------------------- misc */
/* nnz-balanced contiguous row ranges: splits[0]=0 .. splits[parts]=m, with
 * row_ptr[splits[p]] ~ p*nnz/parts.  With maps != NULL splits fall on
 * super-super-row boundaries. */
int hspmv_partition_rows(int64_t m, const int32_t *row_ptr,
                         const hspmv_csr3_maps *maps, int parts,
                         int64_t *splits);
/* Algorithmic bytes of one SpMV:
 * nnz*(sv+4) + (m+1)*4 + n*sv + m*sv (+ (n_ssr+1 + n_sr+1)*4 for CSR-3),
 * where n = the x entries the SpMV reads, i.e. the number of distinct
 * columns (the matrix width when every column holds a nonzero; much less for
 * a row-range shard of a banded matrix -- hspmv_info.x_entries). */
/* Block x dictionaries (host planner; hspmv_create builds the same tables
 * when it uses them, see hspmv_info.x_dict).  The row kernel's workgroups
 * (STREAM: 256 consecutive rows; CSR3 with maps: four consecutive wave
 * tasks) each stage the x entries their rows reference -- runs of
 * consecutive columns, gaps of <= 8 bridged, <= 63 runs -- in LDS, and every
 * nonzero's column becomes a 16-bit position in that copy.  Outputs:
 * blk[n_blocks+1] record ranges; runs[2*n_records] = {x_start, lds_off} per
 * run, then a sentinel {0, entries} per block; pos[nnz] (0 for split rows,
 * > 4096 nonzeros, unless HSPMV_FLAG_NO_SPLIT).  So x[col[k]] ==
 * staged_b[pos[k]] with staged_b[lds_off + i] = x[x_start + i].  Call with
 * NULL buffers for the sizes.  *n_blocks = 0: some block needs more than
 * cap_entries (<= 0: the library's LDS cap for A's dtype), so no dictionary.
 * opt (NULL = defaults) supplies the kernel flags and the CSR-3 plan.
 * Not a reference interface: the test and diagnostic view of the format. */
int hspmv_xdict_plan_ex(const hspmv_csr *A, const hspmv_csr3_maps *maps, const hspmv_options *opt,
                        int64_t cap_entries, int64_t *n_blocks, int64_t *n_records,
                        int32_t *blk, int32_t *runs, uint16_t *pos);
/* Kernel flags instead of options (= hspmv_xdict_plan_ex with an
 * hspmv_options holding only these flags). */
int hspmv_xdict_plan(const hspmv_csr *A, const hspmv_csr3_maps *maps, unsigned flags,
                     int64_t cap_entries, int64_t *n_blocks, int64_t *n_records,
                     int32_t *blk, int32_t *runs, uint16_t *pos);
/* Row slices (host planner; hspmv_create builds the same arrays when it uses
 * them, see hspmv_info.row_slices).  A dictionary handle whose rows are all
 * short enough to be summed serially (<= 40 nonzeros, fp32 56) stores each
 * wave task of <= 64 rows column-major, padded to the task's longest row w:
 * lane i of the wave owns row i and adds its products left to right, the same
 * operations in the same order as the chunked kernel.  Slot k of the slice
 * whose descriptor is desc[2s] = prefix, desc[2s+1] = first row starts at
 * element 64 * (prefix + k) of val and of pos; w = desc[2s+2] - prefix, rows =
 * desc[2s+3] - first row (desc holds n_desc + 1 pairs).  Values: groups of 16
 * bytes per lane (2 fp64 / 4 fp32 consecutive slots; element 64 G g + G i + e
 * of the slice is slot G g + e of lane i), then the last w mod G slots as
 * single columns (element 64 k + i); positions (hspmv_xdict_plan_ex's, of the
 * same options) likewise in groups of 4.  Entries past a row's end are 0;
 * len[r] is row r's length.  *why = HSPMV_SLICES_OK when a handle with these
 * options takes the format, else the first rule that refuses it; n_slices
 * counts the tasks that have rows, padded_entries = 64 * the sum of w.  Call
 * with NULL arrays for the counts.  The test and diagnostic view of the
 * format, like hspmv_xdict_plan_ex. */
#define HSPMV_SLICES_OK 0
#define HSPMV_SLICES_OFF 1        /* hspmv_options.row_slices < 0             */
#define HSPMV_SLICES_NO_DICT 2    /* no block x dictionaries (off, or a block
                                     exceeds the LDS cap)                     */
#define HSPMV_SLICES_SHAPE 3      /* not 64-row wave tasks, four per workgroup:
                                     the packed or SSR CSR-3 plan, VECTOR,
                                     CSORT, STREAM with several groups per wave */
#define HSPMV_SLICES_CHUNKED 4    /* HSPMV_U, HSPMV_FLAG_PREFETCH or
                                     deterministic = 3 ask for the chunked kernel */
#define HSPMV_SLICES_SPLIT_ROWS 5 /* a row over 4096 nonzeros                 */
#define HSPMV_SLICES_LONG_ROW 6   /* a row over the dtype's serial bound      */
#define HSPMV_SLICES_BYTES 7      /* auto: the padded format would move more
                                     bytes per SpMV than the CSR-order format */
#define HSPMV_SLICES_RESIDENT 8   /* auto: the matrix is served from the
                                     Infinity Cache (<= 192 MiB)              */
int hspmv_slices_plan(const hspmv_csr *A, const hspmv_csr3_maps *maps, const hspmv_options *opt,
                      int64_t *n_desc, int64_t *n_slices, int64_t *padded_entries, int32_t *why,
                      int32_t *desc, uint8_t *len, uint16_t *pos, void *val);
/* hspmv_slices_plan for vectors of vector_dtype: with vector_dtype ==
 * A->dtype exactly that; with fp32 A and HSPMV_F64 what hspmv_create_mixed
 * builds -- val holds A's fp32 values in groups of four slots (G = 4), while
 * the dictionaries (8-byte x entries), the serial bound (40) and so desc, len
 * and pos are those of the widened fp64 matrix, and the byte and residence
 * rules count 4-byte values.  Other pairs: HSPMV_E_INVALID. */
int hspmv_slices_plan_vec(const hspmv_csr *A, const hspmv_csr3_maps *maps, const hspmv_options *opt,
                          int vector_dtype, int64_t *n_desc, int64_t *n_slices, int64_t *padded_entries,
                          int32_t *why, int32_t *desc, uint8_t *len, uint16_t *pos, void *val);
/* The position stream a handle uploads for the row slices {desc, pos} of
 * hspmv_slices_plan (n_desc + 1 descriptor pairs, 64 * desc[2 n_desc]
 * positions).  *bits = 12 when every position is below 4096 (every block
 * dictionary holds at most 4096 entries) and the packed stream with its
 * prefix table is smaller than pos (some slices are 8 or more slots wide),
 * else 16.  With 12, the floor(w / 8)
 * whole 8-slot groups of a slice of width w take 12 bytes per lane -- slots
 * 8 g .. 8 g + 7 of lane i as 12-bit fields, slot 8 g + e in bits 12 e .. 12 e
 * + 11 of the little-endian 96-bit word at byte 768 g + 12 i of the slice --
 * and the w mod 8 last slots follow as 16-bit positions laid out as
 * hspmv_slices_plan lays out a slice of width w mod 8.  With 16 the stream is
 * pos itself.  Slice s starts at byte 128 * pos_prefix[s]; pos_prefix (n_desc
 * + 1 entries) sums 6 floor(w / 8) + w mod 8 (16 bits: w) over the earlier
 * slices, *pos_bytes = 128 * pos_prefix[n_desc].  Call with NULL pos_prefix
 * and packed for bits and pos_bytes.  Values, lengths and descriptors are
 * hspmv_slices_plan's. */
int hspmv_slices_pack(int64_t n_desc, const int32_t *desc, const uint16_t *pos, int32_t *bits,
                      int64_t *pos_bytes, int32_t *pos_prefix, void *packed);
double hspmv_alg_bytes(int64_t m, int64_t n, int64_t nnz, int dtype,
                       int64_t n_ssr, int64_t n_sr);
int hspmv_device_count(int *count);
/* ncclGetVersion() of the RCCL this process resolved (no device needed). */
int hspmv_rccl_version(int *version);
const char *hspmv_last_error(void);
const char *hspmv_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HSPMV_H */
