/*
 * bhsparse_hip.h — C-ABI of libbhsparse_hip.so, the MI355X (gfx950) CSR SpGEMM
 * backend that sits behind the bhSPARSE `bhsparse` class API.
 *
 * This is the drop-in boundary: the C++ facade (host/bhsparse.h, same public
 * signatures as the reference's SpGEMM_cuda/bhsparse.h:17-33) and the Python
 * mirror (facade.py) call ONLY these entry points.  Plain C types, opaque
 * handle, caller-owned buffers, every function returns 0 (BHS_SUCCESS ==
 * BHSPARSE_SUCCESS, SpGEMM_cuda/common.h:26) or a negative bhs_status /
 * positive hipError_t; nothing throws or aborts.  One handle = one device =
 * one in-flight multiply; calls on a handle must be externally serialised
 * (same threading contract as the reference: single host thread, synchronous
 * calls).
 *
 * Types: index_type = int32 (SpGEMM_cuda/common.h:30), value_type = bhs_value_t: double
 * (common.h:31) or float in the f32 build.  Intermediate-product counts are int64 (the reference's int
 * overflows beyond 2^31 products, bhsparse.h:367,431).
 */
#ifndef BHSPARSE_HIP_H
#define BHSPARSE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define BHS_API __attribute__((visibility("default")))
#else
#define BHS_API
#endif

/* value_type of A, B and C: double (libbhsparse_hip.so; SpGEMM_cuda/common.h:31) or float
 * (libbhsparse_hip_f32.so, the same sources built with -DBHS_VALUE_FLOAT; the reference supports it by
 * editing the same typedef, README.md:84-86).  Callers of the f32 library define BHS_VALUE_FLOAT too. */
#ifdef BHS_VALUE_FLOAT
typedef float bhs_value_t;
#else
typedef double bhs_value_t;
#endif

typedef struct bhs_handle bhs_handle;

enum bhs_status {
    BHS_SUCCESS            = 0,
    BHS_ERR_INVALID_ARG    = -1,   /* NULL / negative size / bad state          */
    BHS_ERR_NO_DEVICE      = -2,   /* no HIP device, or not a gfx950 code object */
    BHS_ERR_ALLOC          = -3,   /* hipMalloc failed                           */
    BHS_ERR_LAUNCH         = -4,   /* kernel launch / runtime error (reference returns -1 here,
                                      bhsparse_cuda.h:251-253)                   */
    BHS_ERR_NNZ_OVERFLOW   = -5,   /* nnz(C) does not fit index_type (int32)     */
    BHS_ERR_NOT_READY      = -6,   /* get_C before spgemm, spgemm before set_data */
    BHS_ERR_INTERNAL       = -7,   /* accumulator overflow that the retry logic could not resolve */
    BHS_ERR_PEER           = -8    /* multi-GPU calls: another rank of the job failed (bhsparse_dist.h) */
};

/* ---- lifecycle -----------------------------------------------------------
 * replaces bhsparse::initPlatform -> bhsparse_cuda::initPlatform
 *   (SpGEMM_cuda/bhsparse.h:91-125, bhsparse_cuda.h:92-119: picks device 0,
 *   prints the device banner)   and freePlatform (bhsparse.h:127-149).
 * device_count must be 1 (one process per GPU; multi-GPU runs shard rows of A
 * across processes, see bhs_set_data on a row block).  device_ids may be NULL
 * (=> device 0).  Prints the reference-style device banner when verbose.      */
BHS_API int bhs_create(bhs_handle **out, int device_count, const int *device_ids);
BHS_API int bhs_destroy(bhs_handle *h);

/* verbosity: 0 silent, 1 reference-style stage prints (default 0 for the C-ABI;
 * the C++ facade sets 1 to reproduce bhsparse.h:307-336 stdout).              */
BHS_API int bhs_set_verbose(bhs_handle *h, int level);

/* ---- data ----------------------------------------------------------------
 * replaces bhsparse::initData -> bhsparse_cuda::initData
 *   (bhsparse.h:180-258, bhsparse_cuda.h:151-203: cudaMalloc + H2D of A and B).
 * Host pointers are read during the call only (copied to HBM); the reference
 * keeps borrowing them, which stays legal.  A is m x k, B is k x n, 0-based
 * CSR.  Rows of B should be column-sorted (reference precondition, SURVEY.md
 * §8b); unsorted B is detected and still multiplied correctly.               */
BHS_API int bhs_set_data(bhs_handle *h, int m, int k, int n,
                         int nnzA, const bhs_value_t *csrValA, const int *csrRowPtrA, const int *csrColIndA,
                         int nnzB, const bhs_value_t *csrValB, const int *csrRowPtrB, const int *csrColIndB);

/* Same, but the six arrays are DEVICE pointers on the handle's device (borrowed
 * until bhs_free_data; never written).  This is the entry the benchmark uses so
 * that inputs are HBM-resident when the timed region starts, and the entry a
 * multi-GPU host uses to hand each rank its row block of A with B replicated.
 * The library works on its own stream and starts reading the arrays inside this
 * call: they must be COMPLETE (producer kernels / copies on other streams
 * synchronised) before it is made, and stay unchanged until bhs_free_data.     */
BHS_API int bhs_set_data_device(bhs_handle *h, int m, int k, int n,
                                int nnzA, const bhs_value_t *d_valA, const int *d_rowPtrA, const int *d_colIndA,
                                int nnzB, const bhs_value_t *d_valB, const int *d_rowPtrB, const int *d_colIndB);

/* replaces bhsparse::free_mem -> bhsparse_cuda::free_mem (bhsparse.h:151-178,
 * bhsparse_cuda.h:121-149).  Drops A, B, C; keeps the workspace pool.         */
BHS_API int bhs_free_data(bhs_handle *h);

/* ---- compute -------------------------------------------------------------
 * replaces bhsparse::warmup (bhsparse.h:341-363, bhsparse_cuda.h:239-256:
 * re-runs the nnzCt kernel).  Here: runs the upper-bound kernel and pre-sizes
 * the workspace pool so the timed spgemm() does no hipMalloc.                 */
BHS_API int bhs_warmup(bhs_handle *h);

/* replaces bhsparse::spgemm / spgemm_cuda (bhsparse.h:260-339): the whole timed
 * region — stage 1 upper bound + row binning, stage 2 symbolic (exact nnz per
 * row), stage 3 scan + allocation of C, stage 4 numeric (C written once, in
 * place, rows column-sorted, duplicates summed, explicit zeros kept).
 *   rowPtrC_out : caller buffer of m+1 ints, filled with the exclusive-scan row
 *                 pointer (as bhsparse_cuda.h:2787-2799 does); may be NULL.
 *   nnzCt_out   : number of intermediate products (GFLOPs numerator,
 *                 bhsparse.h:287-289); may be NULL.
 *   nnzC_out    : nnz(C); may be NULL.
 *   stage_ms_out: 4 doubles, device time of the 4 stages in ms; may be NULL.
 * Synchronous: returns after C is complete in HBM.                            */
BHS_API int bhs_spgemm(bhs_handle *h, int *rowPtrC_out, int64_t *nnzCt_out, int *nnzC_out,
                       double stage_ms_out[4]);

/* The same multiply in two halves, for callers that place C themselves (the multi-GPU layer, include/bhsparse_dist.h):
 *   bhs_spgemm_symbolic  stages 1-3 of bhsparse::spgemm_cuda (bhsparse.h:297-325: compute_nnzCt, binning, and here the
 *                        exact symbolic pass + scan): afterwards nnz(C) and rowPtrC (bhs_get_C_device / bhs_get_rowptrC)
 *                        are final and the library's own C arrays are allocated;
 *   bhs_set_output_device (optional, between the halves) binds caller-owned device arrays of `capacity` entries: the
 *                        numeric half then writes colIndC / valC there (entry k of C at index k) instead of into the
 *                        library's pool -- e.g. straight into this rank's slice of the assembled global C.  Stays bound
 *                        until bhs_free_data or a call with NULL pointers;
 *   bhs_spgemm_numeric   stage 4 (bhsparse.h:327-335, compute_nnzC_Ct_* + copy) for rows [row_begin, row_end) of C,
 *                        enqueued on the handle's stream (bhs_get_stream): returns without waiting for the kernels, so
 *                        the caller can overlap the transfer of one row range with the numeric kernels of the next;
 *   bhs_spgemm_finish    waits for everything enqueued, collects errors raised on the device, reads the stage timers.
 * bhs_spgemm == symbolic + numeric(0, m) + finish.                                                              */
BHS_API int bhs_spgemm_symbolic(bhs_handle *h, int64_t *nnzCt_out, int *nnzC_out);
BHS_API int bhs_set_output_device(bhs_handle *h, int *d_colIndC, bhs_value_t *d_valC, int64_t capacity);
BHS_API int bhs_spgemm_numeric(bhs_handle *h, int row_begin, int row_end);
BHS_API int bhs_spgemm_finish(bhs_handle *h, double stage_ms_out[4]);
/* the HIP stream (hipStream_t) every kernel of this handle is enqueued on */
BHS_API int bhs_get_stream(bhs_handle *h, void **stream_out);

/* ---- masked multiply ------------------------------------------------------
 * C<M> = A·B on a pattern the caller already holds (no reference counterpart): for every entry p of row i of M,
 * valC[p] = sum over k of A(i,k) B(k, colIndM[p]); products outside M are dropped, and an entry no product lands on
 * (or whose products cancel) reads 0.  The caller's rowPtrM / colIndM are the result's rowPtrC / colIndC: no symbolic
 * stage, no scan, no sort, no column indices written (bhs_masked.hip.h).
 *   A, B     the data bound by bhs_set_data[_device], with bhs_spgemm's preconditions (a private copy sorted by "sort_b"
 *            is what is multiplied)
 *   M        m x n CSR, 0-based, int32, rows STRICTLY ascending, no values.  Checked on the device before valC is written:
 *            rowPtrM[0] != 0, a decreasing rowPtrM, rowPtrM[m] != nnzM, a column outside [0, n) or a row not strictly
 *            ascending returns BHS_ERR_INVALID_ARG with valC untouched
 *   valC     nnzM values (device: d_valC, caller-owned; host entry: copied back)
 *   nnzCt_out  products of A·B over all rows, the figure bhs_spgemm reports (GFLOP/s numerator); may be NULL
 *   ms_out   device time of the whole call, validation included; may be NULL
 * Synchronous.  BHS_ERR_NOT_READY without data, BHS_ERR_INVALID_ARG between bhs_spgemm_symbolic and bhs_spgemm_finish.
 * The call leaves the handle as it was: C of the last bhs_spgemm (bhs_get_C, bhs_get_rowptrC, the pointers of
 * bhs_get_C_device), "class_state", the speculative-launch figures and every option stay; only bhs_get_kernel_stats
 * now reports the masked call's kernel families (masked_scan, masked_short, masked_wave, masked_long, masked_hub).
 * Results are bit-exact where every partial sum is exact (integer values); otherwise the order of the additions is
 * not fixed from run to run (as with bhs_spgemm's LDS tables).  Products and sums are formed in double.  In the float
 * build (bhs_value_t float) masked_short and masked_wave round once per entry; masked_long adds every product, rounded
 * to float, to valC with a float atomic, and masked_hub adds each part's sum (double in LDS where the mask row fits
 * 2048 entries, else each product), rounded to float, with float atomics.
 *
 * Reuse workflow (FEM time steps, Newton loops, AMG with fixed coarsening): bind A and B with bhs_set_data_device, form
 * C's pattern once (bhs_spgemm, bhs_get_C_device), then rewrite the VALUES of A and B in place as often as needed and
 * call bhs_spgemm_masked_device on that pattern: the masked multiply reads valA / valB during the call and caches
 * nothing that depends on values.  The patterns of A and B must not change, and B's rows must have been ascending at
 * hand-over (bhs_get_info "b_sorted" with no private sorted copy: a copy made by "sort_b" does not see later writes).
 * Tunables ("masked_" keys of bhs_set_option): "masked_max_table_log2" (4..11, default 11) caps the LDS table: mask rows
 * beyond 2^v entries take the HBM kernel; "masked_hub_min_products" (default 131072, 0 never): rows with this many
 * products are split across workgroups.                                                                             */
BHS_API int bhs_spgemm_masked_device(bhs_handle *h, const int *d_rowPtrM, const int *d_colIndM, int nnzM,
                                     bhs_value_t *d_valC, int64_t *nnzCt_out, double *ms_out);
BHS_API int bhs_spgemm_masked(bhs_handle *h, const int *rowPtrM, const int *colIndM, int nnzM,
                              bhs_value_t *valC, int64_t *nnzCt_out, double *ms_out);   /* host arrays, copied */

/* ---- sparse add -----------------------------------------------------------
 * Z = alpha X + beta Y on CSR with the UNION of the patterns (rocSPARSE csrgeam; no reference counterpart), and the
 * multiply with an addend, C = alpha A·B + beta D (bhs_add.hip.h).  X, Y, D: 0-based int32 CSR with STRICTLY ascending
 * rows; so is the result.  The pattern never depends on values: an entry of both operands reads alpha x + beta y even
 * where that sum is 0, and alpha == 0 / beta == 0 keep their operand's entries as explicit zeros (bhs_spgemm's contract:
 * "explicit zeros kept").  Arithmetic in double, one rounding to bhs_value_t per entry; no atomics: the result does not
 * depend on scheduling.
 *
 * bhs_csr_add_symbolic_device: the pattern's row pointer.  X and Y are m x n.  Writes d_rowPtrZ (m+1 ints, caller-owned,
 *   device) and returns nnz(Z) in *nnzZ_out.  *y_inside_x_out (may be NULL) = 1 when every entry of Y is an entry of X
 *   (then rowPtrZ == rowPtrX).  Validated on the device before anything is written, as bhs_spgemm_masked validates M:
 *   rowPtr[0] != 0, a decreasing rowPtr, rowPtr[m] != nnz, a column outside [0, n) or a row not strictly ascending
 *   returns BHS_ERR_INVALID_ARG; nnz(Z) > INT32_MAX returns BHS_ERR_NNZ_OVERFLOW.  Needs no bound data (works on a handle
 *   straight after bhs_create); BHS_ERR_INVALID_ARG between bhs_spgemm_symbolic and bhs_spgemm_finish.  Synchronous.
 * bhs_csr_add_numeric_device: Z = alpha X + beta Y on the rowPtrZ of the call above: writes d_colIndZ / d_valZ
 *   (caller-owned, nnz(Z) entries, must not overlap X or Y), rows strictly ascending.  ms_out (may be NULL): device time.
 *   Synchronous.  Z may be the X of a later add.
 * bhs_spgemm_add[_device]: C = alpha A·B + beta D on the data bound by bhs_set_data[_device]; D is m x n (device arrays /
 *   host arrays, copied).  Runs the ordinary multiply (every option, path and precondition of bhs_spgemm applies), then
 *   the add.  Afterwards bhs_get_nnzC / bhs_get_C / bhs_get_rowptrC / bhs_get_C_device return THIS C (library-owned,
 *   valid until the next multiply / bhs_free_data / bhs_destroy); rowPtrC_out / nnzCt_out / nnzC_out as in bhs_spgemm
 *   (nnzCt: products of A·B; nnzC: entries of the sum).  ms_out[2] (may be NULL): device time of the multiply, of the
 *   add.  An invalid D returns BHS_ERR_INVALID_ARG before the multiply is started and leaves the handle's last C as it
 *   was.  BHS_ERR_INVALID_ARG while output arrays are bound with bhs_set_output_device (the sum's size is not known
 *   when they are bound) and between bhs_spgemm_symbolic and bhs_spgemm_finish; BHS_ERR_NOT_READY without data.
 *   Where every entry of D is an entry of A·B (A·A + A with a full diagonal, a smoothed prolongator, J·S + K with K
 *   inside the product) the add runs IN PLACE: no second C, no column rewritten; with alpha == 1 only the values D names
 *   are touched.  Otherwise the sum goes to a second set of arrays and the getters serve those; the multiply's own
 *   arrays stay where they are.  The next bhs_spgemm, bhs_spgemm_symbolic, bhs_warmup or bhs_free_data drops the sum;
 *   bhs_spgemm_masked leaves it alone.  "class_state", the speculative-launch figures and every option are what the
 *   inner bhs_spgemm leaves.
 * bhs_get_kernel_stats after any of these reports the add's kernel families (add_count, add_scan, add_bin, add_short,
 * add_wave, add_long, add_inplace) -- after bhs_spgemm_add beside the multiply's families.
 * Tunables: "add_inplace" (default 1; 0: the sum always goes to the second set of arrays).  bhs_get_info
 * "add_inplace_used": 1 / 0 for the last bhs_spgemm_add.                                                          */
BHS_API int bhs_csr_add_symbolic_device(bhs_handle *h, int m, int n,
                                        int nnzX, const int *d_rowPtrX, const int *d_colIndX,
                                        int nnzY, const int *d_rowPtrY, const int *d_colIndY,
                                        int *d_rowPtrZ, int *nnzZ_out, int *y_inside_x_out);
BHS_API int bhs_csr_add_numeric_device(bhs_handle *h, int m, int n,
                                       double alpha, int nnzX, const bhs_value_t *d_valX, const int *d_rowPtrX, const int *d_colIndX,
                                       double beta, int nnzY, const bhs_value_t *d_valY, const int *d_rowPtrY, const int *d_colIndY,
                                       const int *d_rowPtrZ, int *d_colIndZ, bhs_value_t *d_valZ, double *ms_out);
BHS_API int bhs_spgemm_add_device(bhs_handle *h, double alpha, double beta,
                                  int nnzD, const bhs_value_t *d_valD, const int *d_rowPtrD, const int *d_colIndD,
                                  int *rowPtrC_out, int64_t *nnzCt_out, int *nnzC_out, double ms_out[2]);
BHS_API int bhs_spgemm_add(bhs_handle *h, double alpha, double beta,
                           int nnzD, const bhs_value_t *valD, const int *rowPtrD, const int *colIndD,
                           int *rowPtrC_out, int64_t *nnzCt_out, int *nnzC_out, double ms_out[2]);   /* host arrays, copied */

/* ---- entry selection ------------------------------------------------------
 * Z = the entries of X that a rule keeps (no reference counterpart): by position, by magnitude and by rank within the
 * row -- tril / triu / a band, dropping explicit zeros, AMG truncation and strength of connection, threshold + top-k
 * pruning of iterated products -- and the multiply that applies the rule to its own result (bhs_select.hip.h).
 * X: m x n, 0-based int32 CSR; rows need NOT be ascending.
 *
 * The rule.  Stages apply in this order, each to what the stage before left:
 *   1. position   BHS_SEL_BAND keeps band_lo <= col - row <= band_hi (the difference in int64 arithmetic: INT64_MIN /
 *                 INT64_MAX ends are legal); BHS_SEL_DROP_DIAG drops col == row.
 *   2. ABS        keep unless |v| <= abs_tol   (abs_tol = 0 drops +0 and -0 and nothing else)
 *   3. REL        keep unless |v| <  rel_tol * rowmax
 *   4. TOPK       of what is left, the top_k entries of largest |v|
 * BHS_SEL_KEEP_DIAG: an entry with col == row that passed stage 1 passes ABS, REL and TOPK unconditionally, is not
 *   counted in top_k and does not enter the row maximum.
 * rowmax is taken over the entries stage 1 left (without the diagonal under KEEP_DIAG; 0 when there are none): it is the
 *   entry that ranks highest in the order below, so a row holding a NaN has rowmax = NaN and REL drops nothing there.
 * Magnitudes are compared as fabs((double)v) -- exact for the float build.  rel_tol * rowmax is one double product.
 * Rank order is the order of that double's bit pattern read as an unsigned 64-bit integer: NaN ranks above Inf.  The ABS
 *   and REL tests are written "keep unless", so a NaN is kept: a selection never hides a NaN.  Ties in rank go to the
 *   entry that comes first in the row.
 * The output keeps the input order of the survivors and their bits (a stable compaction): ascending rows stay
 *   ascending.  Nothing is computed on values but these comparisons; no atomics on values: the result does not depend
 *   on scheduling.
 * An invalid rule returns BHS_ERR_INVALID_ARG: DROP_DIAG together with KEEP_DIAG, top_k < 0, abs_tol or rel_tol
 *   negative, NaN or Inf, band_lo > band_hi, unknown flag bits.  Fields whose flag is not set are ignored, except that
 *   they must still be valid.
 *
 * bhs_csr_select_symbolic_device: the selection's row pointer.  Writes d_rowPtrZ (m+1 ints, caller-owned, device) and
 *   returns nnz(Z) in *nnzZ_out.  X is validated on the device before anything caller-owned is written: rowPtrX[0] != 0,
 *   a decreasing rowPtrX, rowPtrX[m] != nnzX or a column outside [0, n) returns BHS_ERR_INVALID_ARG.  d_valX may be
 *   NULL when no value flag (ABS, REL, TOPK) is set.  Needs no bound data; BHS_ERR_INVALID_ARG between
 *   bhs_spgemm_symbolic and bhs_spgemm_finish.  Synchronous.
 * bhs_csr_select_numeric_device: writes the survivors to d_colIndZ / d_valZ (caller-owned, nnz(Z) entries, must not
 *   overlap X) on the d_rowPtrZ of the call above.  d_valZ may be NULL: the pattern alone.  The rule is evaluated again:
 *   a row whose survivors are not what d_rowPtrZ says (X or the rule changed between the calls) returns
 *   BHS_ERR_INVALID_ARG; nothing is ever written outside [0, rowPtrZ[m]).  ms_out (may be NULL): device time.  Synchronous.
 * bhs_spgemm_select / bhs_spgemm_select_device: C = select(A·B) on the data bound by bhs_set_data[_device].  The rule is
 *   checked first; then the ordinary multiply runs (every option, path and precondition of bhs_spgemm applies), then the
 *   selection of its C.  Afterwards bhs_get_nnzC / bhs_get_C / bhs_get_rowptrC / bhs_get_C_device return the SELECTED C
 *   (library-owned, the second set of arrays bhs_spgemm_add uses, with the same lifetime: the next bhs_spgemm,
 *   bhs_spgemm_symbolic, bhs_warmup or bhs_free_data drops it; the multiply's own arrays never move).  Where the rule
 *   drops nothing no second set is made and the getters return what bhs_spgemm alone returns.  rowPtrC_out (may be NULL):
 *   m+1 ints, HOST memory for bhs_spgemm_select, DEVICE memory for bhs_spgemm_select_device; nnzCt_out: products of A·B;
 *   nnzC_out: entries after the selection; ms_out[2] (may be NULL): device time of the multiply, of the selection.
 *   BHS_ERR_INVALID_ARG while output arrays are bound with bhs_set_output_device and between bhs_spgemm_symbolic and
 *   bhs_spgemm_finish; BHS_ERR_NOT_READY without data.  bhs_get_info "select_dropped": entries the last call removed.
 * bhs_get_kernel_stats after any of these reports the selection's kernel families: select_count (the count pass; for
 *   the numeric call the binning), select_scan, select_short (rows of up to 32 entries), select_wave (up to 1024),
 *   select_long -- after bhs_spgemm_select beside the multiply's families.                                        */
enum {
  BHS_SEL_BAND      = 1,   /* keep band_lo <= col - row <= band_hi (int64 arithmetic) */
  BHS_SEL_DROP_DIAG = 2,   /* drop col == row */
  BHS_SEL_KEEP_DIAG = 4,   /* col == row passes ABS / REL / TOPK unconditionally, is not
                              counted in top_k and does not enter the row maximum */
  BHS_SEL_ABS       = 8,   /* keep unless |v| <= abs_tol          (abs_tol = 0 drops +-0) */
  BHS_SEL_REL       = 16,  /* keep unless |v| <  rel_tol * rowmax                          */
  BHS_SEL_TOPK      = 32   /* of what is left, the top_k entries of largest |v| */
};
typedef struct bhs_select {
  uint32_t flags; int32_t top_k; int64_t band_lo, band_hi; double abs_tol, rel_tol;
} bhs_select;
BHS_API int bhs_csr_select_symbolic_device(bhs_handle *h, int m, int n,
                                           int nnzX, const bhs_value_t *d_valX, const int *d_rowPtrX, const int *d_colIndX,
                                           const bhs_select *sel, int *d_rowPtrZ, int *nnzZ_out);
BHS_API int bhs_csr_select_numeric_device(bhs_handle *h, int m, int n,
                                          int nnzX, const bhs_value_t *d_valX, const int *d_rowPtrX, const int *d_colIndX,
                                          const bhs_select *sel, const int *d_rowPtrZ, int *d_colIndZ, bhs_value_t *d_valZ,
                                          double *ms_out);
BHS_API int bhs_spgemm_select_device(bhs_handle *h, const bhs_select *sel,
                                     int *d_rowPtrC_out, int64_t *nnzCt_out, int *nnzC_out, double ms_out[2]);
BHS_API int bhs_spgemm_select(bhs_handle *h, const bhs_select *sel,
                              int *rowPtrC_out, int64_t *nnzCt_out, int *nnzC_out, double ms_out[2]);

/* ---- transpose ------------------------------------------------------------
 * T = X^T on CSR (rocSPARSE csr2csc; no reference counterpart), with the permutation that re-values a known pattern
 * (bhs_transpose.hip.h).  What it is for: the Galerkin product P^T·A·P that ends an AMG setup, A^T·A, symmetrising a
 * graph (A + A^T: bhs_csr_add_* finishes it), handing a result to a CSC consumer -- T's arrays ARE X in CSC.
 * X: m x n, 0-based int32 CSR; rows need NOT be ascending, duplicate (row, column) pairs are legal.  T is n x m and
 * nnz(T) = nnz(X).
 *
 * T is the STABLE transpose: the entries of row j of T are the entries of X with column j, in the order of their
 * position in X's arrays.  The columns of a T row are therefore ascending -- strictly ascending when X has no duplicate
 * pair, and T is then a legal operand of bhs_csr_add_* and bhs_spgemm_masked.  Values are copied bit for bit (NaN
 * payloads and -0 included); nothing is computed on them.  The result does not depend on scheduling; in numpy it is
 *   order = argsort(colIndX, kind="stable"); colIndT = row_of_entry[order]; valT = valX[order]; perm = order;
 *   rowPtrT = cumsum of bincount(colIndX, minlength=n) with a leading 0.
 *
 * bhs_csr_transpose_device
 *   d_valX     nnzX values, or NULL: the pattern alone (d_valT must then be NULL too)
 *   d_rowPtrT  n+1 ints, d_colIndT nnzX ints, d_valT nnzX values or NULL, d_perm nnzX ints or NULL: caller-owned device
 *              arrays that must not overlap X or one another.  d_perm[q] is the position in X of entry q of T.
 *   ms_out     device time of the whole call, validation included; may be NULL
 *   X is validated on the device BEFORE anything caller-owned is written: rowPtrX[0] != 0, a decreasing rowPtrX,
 *   rowPtrX[m] != nnzX or a column outside [0, n) returns BHS_ERR_INVALID_ARG with every output untouched.
 *   m, n or nnzX may be 0; d_rowPtrT is still written (n+1 zeros when nnzX is 0).  Needs no bound data (works on a handle
 *   straight after bhs_create); BHS_ERR_INVALID_ARG between bhs_spgemm_symbolic and bhs_spgemm_finish.  Synchronous.
 * bhs_csr_transpose_values_device: valT[q] = valX[perm[q]] -- the pattern-reuse half.  Where the values of X change and
 *   its pattern does not (time steps, Newton loops, AMG with fixed coarsening: the reuse workflow of bhs_spgemm_masked)
 *   transpose once with d_perm, keep rowPtrT / colIndT, and re-value T with this call: 4 bytes of perm and the gathered
 *   value read, one value written, an entry.  A perm entry outside [0, nnzX) returns BHS_ERR_INVALID_ARG; it is not
 *   followed: nothing is read out of range (valT may have been written in part).  d_valT must not be d_valX.  Synchronous.
 * Both calls leave the handle as it was: they use counters, tile words, epoch, events and scratch of their own from the
 *   grow-only pool (8 bytes an entry of X for the keys, 8 bytes a column); C of the last multiply (every getter,
 *   bhs_get_C_device's pointers), a sum or selection the getters serve, "class_state", the speculative-launch figures
 *   and every option stay.  Only bhs_get_kernel_stats now reports the transpose's kernel families: transpose_count
 *   (validation, the columns' histogram, the T rows' bins), transpose_scan, transpose_scatter, transpose_short (T rows of
 *   up to 32 entries), transpose_wave (up to 1024), transpose_long; transpose_values after the values call.
 * Known limit: one T row is put in order by one workgroup.  A column of X with millions of entries (n = 1, a hub column)
 *   goes through a bitonic network in HBM and is slow; it is correct.                                               */
BHS_API int bhs_csr_transpose_device(bhs_handle *h, int m, int n, int nnzX,
                                     const bhs_value_t *d_valX /* may be NULL */, const int *d_rowPtrX, const int *d_colIndX,
                                     int *d_rowPtrT /* n+1 */, int *d_colIndT /* nnzX */, bhs_value_t *d_valT /* may be NULL */,
                                     int *d_perm /* may be NULL, nnzX */, double *ms_out /* may be NULL */);
BHS_API int bhs_csr_transpose_values_device(bhs_handle *h, int nnzX, const bhs_value_t *d_valX,
                                            const int *d_perm, bhs_value_t *d_valT, double *ms_out);

/* ---- assembly -------------------------------------------------------------
 * Z from triplets (MATLAB sparse(i, j, v), scipy coo_matrix.tocsr(), PETSc MatSetValuesCOO; no reference counterpart), with
 * the map that re-values a known pattern (bhs_assemble.hip.h).  What it is for: the entry into the library for whoever holds
 * triplets -- finite-element contributions, an edge list, the (lo, hi, w) of bhs_csr_spanning_forest_device -- and for a
 * CSR whose rows are unsorted or hold repeats: its output has rows strictly ascending (BHS_COO_KEEP: ascending), which
 * bhs_csr_add_*, bhs_csr_cfsplit_device, bhs_csr_interp_* and bhs_csr_ilu0_device require.
 *
 * The triplets: nnzIn of them, (rowInd[e], colInd[e], valIn[e]), in any order, repeats legal.  Z is m x n.
 *   kept      triplet e is kept when 0 <= rowInd[e] < m and 0 <= colInd[e] < n.  With BHS_COO_IGNORE_NEGATIVE a triplet with a
 *             negative row or column is dropped silently (PETSc's convention for constrained unknowns); without it a
 *             negative index is an error.  An index >= m or >= n is always an error.
 *   perm      the kept positions e sorted by (rowInd[e], colInd[e], e) -- the stable order; nkept is its length.
 *   runs      a run is a maximal stretch of perm with equal (row, column); equal columns that end one row and begin the next
 *             are never one run.  Under BHS_COO_SUM, _FIRST and _LAST each run becomes one entry of Z.  Under BHS_COO_KEEP
 *             every kept triplet stays an entry of its own: Z is sorted but has repeats, nnzZ == nkept, entryPtr[q] == q.
 *   outputs   rowPtrZ / colIndZ: Z's pattern, rows ascending.  Entry q is the run perm[entryPtr[q] .. entryPtr[q+1]);
 *             entryPtr[0] == 0, entryPtr[nnzZ] == nkept.  An empty row is an empty row of Z.
 *   values    _FIRST / _LAST (and _KEEP) copy the run's first / last value by input position, bit for bit.  _SUM:
 *             s = double(valIn[perm[a]]) -- not 0.0 + ..., a lone -0 stays -0 --, then s += double(valIn[perm[k]]) for
 *             k = a+1 .. b-1 in that order, one lane a run, and ONE rounding to the value type.  The order is fixed on
 *             purpose: the result is THE result for any input, NaN and +-Inf included.
 *   No atomic touches an output array; every output is a function of the input alone, the same bits from run to run and
 *   from handle to handle, and for values both types hold exactly in both builds.
 *
 * bhs_coo_assemble_device
 *   d_valIn    nnzIn values, or NULL: the pattern alone (d_valZ must then be NULL too)
 *   d_rowPtrZ  m+1 ints.  d_colIndZ: CAPACITY nnzIn ints, nnzZ written.  d_valZ: CAPACITY nnzIn values, nnzZ written, or
 *              NULL.  d_entryPtr: CAPACITY nnzIn+1 ints, nnzZ+1 written, or NULL.  d_perm: CAPACITY nnzIn ints, nkept
 *              written, or NULL.  Caller-owned device arrays whose footprints (the capacities) must not overlap the
 *              triplets or one another.  Nothing is written outside the capacities.
 *   flags      one of BHS_COO_SUM, _FIRST, _LAST, _KEEP, or'ed with BHS_COO_IGNORE_NEGATIVE
 *   nnzZ_out, nkept_out, ms_out (device time of the whole call, validation included): each may be NULL
 *   The triplets are validated on the device BEFORE anything caller-owned is written: an index >= m or >= n, or a negative
 *   one without the flag, returns BHS_ERR_INVALID_ARG with every output untouched.  BHS_ERR_INVALID_ARG from the host,
 *   outputs untouched as well: a NULL handle, a negative size, an unknown flag bit, NULL index arrays or NULL d_colIndZ
 *   with nnzIn > 0, NULL d_rowPtrZ, d_valZ without d_valIn, overlapping footprints.  The triplets must not change during
 *   the call: a place that no longer fits its row is not written and the call returns BHS_ERR_INTERNAL.
 *   m, n or nnzIn may be 0; d_rowPtrZ is still written (m+1 zeros when nothing is kept), and entryPtr[0].
 * bhs_coo_assemble_values_device: the pattern-reuse half -- finite-element codes re-assemble new values on an unchanged
 *   connectivity every time step or Newton iteration.  Assemble once with d_entryPtr and d_perm, keep Z's pattern, and
 *   re-value Z with this call from new valIn by the same rule (flags: BHS_COO_SUM, _FIRST or _LAST; _KEEP is refused: its
 *   values are FIRST's): the bits equal those of a full call on the same triplets.  valIn is read only at positions perm
 *   names.  The map is checked whole BEFORE d_valZ is touched and every index again ahead of its dependent read:
 *   entryPtr[0] != 0, a decreasing entryPtr, entryPtr[nnzZ] > nnzIn or a perm entry outside [0, nnzIn) returns
 *   BHS_ERR_INVALID_ARG with d_valZ untouched; a bad index is never followed.  (entryPtr[q] == entryPtr[q+1], an empty run
 *   no full call makes, gives +0.)  d_valZ must not overlap d_valIn or the map.
 * Both calls are synchronous on the handle's stream, need no bound data (they work on a handle straight after bhs_create;
 *   BHS_ERR_INVALID_ARG between bhs_spgemm_symbolic and bhs_spgemm_finish) and leave the handle as it was: counters, tile
 *   words, epoch, events and scratch of their own from the grow-only pool (12 bytes a triplet for the keys and their rows,
 *   8 bytes a row, a bit and a sixteenth of an int a triplet for the head bitmap); C of the last multiply, a sum or selection
 *   the getters serve, "class_state", the speculative-launch figures and every option stay.  Only bhs_get_kernel_stats now
 *   reports the assembly's families: assemble_count (validation, the rows' histogram and bins), assemble_scan,
 *   assemble_scatter, assemble_short (raw rows of up to 32 triplets), assemble_wave (up to 1024), assemble_long,
 *   assemble_dedupe, assemble_values; assemble_check and assemble_values after the values call.
 * Known limits: one raw row is put in order by one workgroup (a row of millions of triplets goes through a bitonic network
 *   in HBM), and one lane adds one run (a run of millions of triplets is added by one lane): both slow, both correct.      */
enum { BHS_COO_SUM = 0, BHS_COO_FIRST = 1, BHS_COO_LAST = 2, BHS_COO_KEEP = 3,   /* bits 0-1: what happens to duplicates */
       BHS_COO_IGNORE_NEGATIVE = 4 };

BHS_API int bhs_coo_assemble_device(bhs_handle *h, int m, int n, int nnzIn,
        const int *d_rowInd, const int *d_colInd,        /* nnzIn each, any order, repeats legal */
        const bhs_value_t *d_valIn                       /* may be NULL: pattern only */,
        int flags,
        int *d_rowPtrZ                                   /* out: m + 1 */,
        int *d_colIndZ                                   /* out: CAPACITY nnzIn, nnzZ written */,
        bhs_value_t *d_valZ                              /* out, may be NULL (needs d_valIn): CAPACITY nnzIn */,
        int *d_entryPtr                                  /* out, may be NULL: CAPACITY nnzIn + 1, nnzZ + 1 written */,
        int *d_perm                                      /* out, may be NULL: CAPACITY nnzIn, nkept written */,
        int *nnzZ_out, int *nkept_out, double *ms_out    /* each may be NULL */);

BHS_API int bhs_coo_assemble_values_device(bhs_handle *h, int nnzIn, const bhs_value_t *d_valIn,
        int nnzZ, const int *d_entryPtr, const int *d_perm,
        int flags /* BHS_COO_SUM, FIRST or LAST */, bhs_value_t *d_valZ /* nnzZ */, double *ms_out);

/* ---- semiring multiply ----------------------------------------------------
 * C<M> = A (+).(x) B and C = A (+).(x) B over a semiring other than plus-times (GraphBLAS mxm; no reference counterpart):
 * one relaxation step of all-pairs shortest paths (MIN_PLUS), widest / bottleneck paths (MAX_MIN, MIN_MAX), most
 * reliable paths (MAX_TIMES), reachability and BFS frontiers (OR_AND), structural triangle counting that never reads a
 * value (PLUS_PAIR).  Kernels: bhs_semiring.hip.h -- the masked multiply's, with the product and the reduction made
 * parameters.
 *
 * The rule.  For an entry (i, j) of the result, with a = A(i,k) and b = B(k,j), both converted to double, over every k
 * for which both are entries:
 *     semiring            product (x)                      reduction (+)   (+)-identity
 *     BHS_SR_PLUS_TIMES   a * b                            +               0
 *     BHS_SR_MIN_PLUS     a + b                            min             +Inf
 *     BHS_SR_MAX_PLUS     a + b                            max             -Inf
 *     BHS_SR_MAX_TIMES    a * b                            max             -Inf
 *     BHS_SR_MIN_MAX      max(a, b)                        min             +Inf
 *     BHS_SR_MAX_MIN      min(a, b)                        max             -Inf
 *     BHS_SR_OR_AND       (a != 0 and b != 0) ? 1 : 0      or              0
 *     BHS_SR_PLUS_PAIR    1 (values not read)              +               0
 *   Order of min and max, as (+) and as (x): the order of the values as numbers, with -0 below +0.
 *   NaN: a product that is NaN makes its entry NaN -- NaN propagates, it is not skipped.  That covers a NaN operand (of
 *     max(a, b) / min(a, b) too), Inf - Inf in the *_PLUS semirings and 0 * Inf in MAX_TIMES.  Which NaN comes out is not
 *     specified.
 *   OR_AND treats NaN as non-zero (NaN != 0); -0 is zero.
 *   Arithmetic: products and the reduction in double, ONE rounding to bhs_value_t per entry.  Rounding is monotone, so
 *     reducing rounded products gives the same bits: the float build's long and hub bins reduce floats in valC.
 *   PLUS_PAIR counts in integers and converts once: exact up to 2^53 in the double build, 2^24 in the float build.
 *   min, max and or do not depend on the order of their operands: unlike the plus-times kernels, results are bit for bit
 *     the same from run to run on any input, in every bin.
 *   PLUS_TIMES is accepted everywhere and forwards to the existing call (bhs_spgemm_masked[_device] / bhs_spgemm); it runs no
 *     new kernel.  A caller can hold the semiring in a variable.
 *
 * bhs_spgemm_semiring_masked[_device]: C<M> = A (+).(x) B.  The contract of bhs_spgemm_masked[_device], word for word: the
 *   preconditions on M and its validation on the device (an invalid M returns BHS_ERR_INVALID_ARG with valC untouched), the
 *   refusals (BHS_ERR_NOT_READY without data, BHS_ERR_INVALID_ARG between bhs_spgemm_symbolic and bhs_spgemm_finish), the
 *   handle left as it was, the "b_sorted" rejections, the tunables "masked_max_table_log2" and "masked_hub_min_products".
 *   Two differences: an entry of M that no product lands on reads the (+)-identity of the table above (+Inf for MIN_PLUS),
 *   and an unknown semiring returns BHS_ERR_INVALID_ARG.  bhs_get_kernel_stats then reports the families sr_scan,
 *   sr_short, sr_wave, sr_long and sr_hub.
 * bhs_spgemm_semiring: the full product.  The pattern of A (+).(x) B is the structural pattern of A·B for every semiring,
 *   and bhs_spgemm keeps computed zeros, so its C already has that pattern.  The call (1) checks the semiring before
 *   anything is started -- an unknown one returns BHS_ERR_INVALID_ARG and leaves the last C as it was --, (2) runs the
 *   ordinary bhs_spgemm (every option, path, precondition and speculative launch as ever), (3) re-values that C IN PLACE
 *   with the masked semiring kernels, M = C's own device arrays: no second set of arrays, no column rewritten, the
 *   pipeline's arrays not moved.  The plus-times values of step 2 are computed and then thrown away: a pattern-only pass
 *   through the pipeline does not exist yet.  Afterwards bhs_get_nnzC / bhs_get_C / bhs_get_rowptrC / bhs_get_C_device
 *   serve the semiring's values; rowPtrC_out / nnzCt_out / nnzC_out as in bhs_spgemm; ms_out[2] (may be NULL): device time
 *   of the multiply, of the re-valuation (the Python mirror keeps them as multiply_ms and semiring_ms).
 *   bhs_get_kernel_stats reports the sr_ families beside the multiply's.
 *   BHS_ERR_INVALID_ARG while output arrays are bound with bhs_set_output_device and between bhs_spgemm_symbolic and
 *   bhs_spgemm_finish (as bhs_spgemm_add); BHS_ERR_NOT_READY without data.                                            */
enum {
  BHS_SR_PLUS_TIMES = 0,
  BHS_SR_MIN_PLUS   = 1,
  BHS_SR_MAX_PLUS   = 2,
  BHS_SR_MAX_TIMES  = 3,
  BHS_SR_MIN_MAX    = 4,
  BHS_SR_MAX_MIN    = 5,
  BHS_SR_OR_AND     = 6,
  BHS_SR_PLUS_PAIR  = 7
};
BHS_API int bhs_spgemm_semiring_masked_device(bhs_handle *h, int semiring, const int *d_rowPtrM, const int *d_colIndM, int nnzM,
                                              bhs_value_t *d_valC, int64_t *nnzCt_out, double *ms_out);
BHS_API int bhs_spgemm_semiring_masked(bhs_handle *h, int semiring, const int *rowPtrM, const int *colIndM, int nnzM,
                                       bhs_value_t *valC, int64_t *nnzCt_out, double *ms_out);   /* host arrays, copied */
BHS_API int bhs_spgemm_semiring(bhs_handle *h, int semiring, int *rowPtrC_out, int64_t *nnzCt_out, int *nnzC_out,
                                double ms_out[2]);

/* ---- extract --------------------------------------------------------------
 * Z = X(rows, cols) on CSR: submatrix extraction and permutation (GraphBLAS extract, MATLAB's A(I, J); no reference
 * counterpart; bhs_extract.hip.h).  What it is for: the blocks A_FF, A_FC, A_CF, A_CC of a C/F splitting, an induced
 * subgraph, the column block one rank's rows reach, a symmetric reordering X(p, p) before a multiply.
 * X: m x n, 0-based int32 CSR; rows need NOT be ascending, duplicate (row, column) pairs are legal (as for the
 * transpose).  Z is mI x nJ with Z(i, j) = X(rows[i], cols[j]).
 *   rows   mI ints, each in [0, m), in any order, repeats allowed (a row may be taken twice).  NULL: all rows in order;
 *          mI must then equal m.
 *   cols   nJ ints, each in [0, n), in any order, NO repeats (a repeated column would duplicate entries: another
 *          operation, refused).  NULL: all columns in order; nJ must then equal n, no column map is built and the call
 *          is a row gather.
 * Order inside a Z row: row i of Z holds the entries q of X's row rows[i] whose column c = colIndX[q] is named by cols,
 * each relabelled to the j with cols[j] == c, in ASCENDING j; ties (duplicate pairs of X) in the order of their position
 * q in X.  Z's rows are therefore always ascending -- strictly ascending when X has no duplicate pair, and Z is then a
 * legal operand of bhs_csr_add_*, bhs_spgemm_masked and bhs_set_data_device with "b_sorted".  Values are copied bit for
 * bit (NaN payloads and -0 included); nothing is computed on them.  The result does not depend on scheduling; in numpy,
 * per Z row i with r = rows[i]:
 *   q = arange(Xp[r], Xp[r+1]); j = inv[Xj[q]] (inv[cols[t]] = t, -1 elsewhere); keep j >= 0;
 *   order = argsort(j[keep], kind="stable"); colIndZ = j[keep][order]; perm = q[keep][order]; valZ = valX[perm].
 * perm[p] is the position in X's arrays of entry p of Z: valZ = valX[perm].  Where the values of X change and its pattern
 * does not, extract once with d_perm, keep rowPtrZ / colIndZ and re-value Z with
 *   bhs_csr_transpose_values_device(h, nnzZ, d_valX, d_perm, d_valZ, ms_out)
 * -- there is no values call of its own.  That call refuses a perm entry outside [0, count) for the count it is given:
 * with count = nnzZ it serves every extraction with nnz(Z) >= nnz(X) (a permutation X(p, p), a row gather by a
 * permutation, a column permutation, rows taken more than once).  For a true sub-matrix perm may reach beyond nnzZ and
 * the values call then refuses it; re-value such a Z with the numeric call on the kept d_rowPtrZ.
 *
 * bhs_csr_extract_symbolic_device: validates, counts, writes d_rowPtrZ (mI+1 ints) and *nnzZ_out.
 * bhs_csr_extract_numeric_device: fills d_colIndZ, d_valZ (may be NULL: the pattern alone; must be NULL when d_valX is),
 *   d_perm (may be NULL), nnzZ entries each, for the d_rowPtrZ of the symbolic call (d_valX may be NULL with nnzX == 0).  ms_out (may be NULL): device time
 *   of the call, validation included.
 * Validation: on the device, BEFORE anything caller-owned is written, in both calls.  rowPtrX[0] != 0, a decreasing
 *   rowPtrX (anywhere in X), rowPtrX[m] != nnzX, a row index outside [0, m), a column index outside [0, n), a repeated
 *   column index, or a column of X outside [0, n) return BHS_ERR_INVALID_ARG with every output untouched.  Rows of X that
 *   `rows` never names are never read: X's COLUMNS are checked in the rows that are read, its row pointer everywhere.
 *   On the host: d_rows == NULL with mI != m, d_cols == NULL with nJ != n, d_valZ without d_valX, outputs that overlap
 *   inputs or one another return BHS_ERR_INVALID_ARG as well.
 *   The numeric call evaluates the rule again before it writes: if a row's survivors are not what d_rowPtrZ says, or
 *   d_rowPtrZ[mI] != nnzZ, it returns BHS_ERR_INVALID_ARG with the outputs untouched; nothing is ever written outside
 *   [0, nnzZ).
 * Sizes: nnz(Z) > INT32_MAX is possible with repeated rows and returns BHS_ERR_NNZ_OVERFLOW from the symbolic call
 *   (d_rowPtrZ untouched).  m, n, mI, nJ and nnzX may be 0; d_rowPtrZ is still written.
 * Both calls are synchronous, need no bound data (they work on a handle straight after bhs_create), return
 *   BHS_ERR_INVALID_ARG between bhs_spgemm_symbolic and bhs_spgemm_finish, and leave the handle as it was: counters,
 *   queues, tile words, epoch, events, the column map (n ints) and the keys of rows beyond the LDS (8 bytes an entry of
 *   Z, only where an X row has more than 1024 entries) are buffers of their own from the grow-only pool; C of the last
 *   multiply, a served sum or selection, "class_state", the speculative-launch figures and every option stay.  Only
 *   bhs_get_kernel_stats now reports the extraction's families: extract_map (validation of rows and cols, rowPtrX's
 *   monotonicity, the inverse column map; absent when both d_rows and d_cols are NULL), extract_count (the touched rows
 *   of X: validation, survivors, bins), extract_scan (symbolic call), extract_short (X rows of up to 32 entries),
 *   extract_wave (up to 1024), extract_long (numeric call).  bhs_get_info "extract_reordered_rows" (needs no bound data):
 *   the Z rows of the last successful numeric call whose relabelled entries were not already ascending and had to be put
 *   in order -- 0 for ascending cols on ascending X rows, a C/F split with sorted F, the row gather.
 * Known limit: one Z row is compacted and put in order by one workgroup; a single row of millions of entries is slow.  */
BHS_API int bhs_csr_extract_symbolic_device(bhs_handle *h, int m, int n,
        int nnzX, const int *d_rowPtrX, const int *d_colIndX,
        int mI, const int *d_rows /* may be NULL */, int nJ, const int *d_cols /* may be NULL */,
        int *d_rowPtrZ /* mI+1 */, int *nnzZ_out);
BHS_API int bhs_csr_extract_numeric_device(bhs_handle *h, int m, int n,
        int nnzX, const bhs_value_t *d_valX /* may be NULL */, const int *d_rowPtrX, const int *d_colIndX,
        int mI, const int *d_rows, int nJ, const int *d_cols,
        int nnzZ, const int *d_rowPtrZ, int *d_colIndZ, bhs_value_t *d_valZ /* may be NULL */,
        int *d_perm /* may be NULL */, double *ms_out /* may be NULL */);

/* ---- reduce / scale -------------------------------------------------------
 * A CSR matrix to a vector or a scalar (GraphBLAS reduce: degrees, row / column sums, diag(X), the 1-, Inf- and
 * Frobenius norms, the total of a PLUS_PAIR triangle count), and a matrix times diagonal matrices on its own pattern
 * (the diagonal case of apply: D^-1 A of a smoothed prolongator, the column normalisation of Markov clustering); no
 * reference counterpart; bhs_reduce.hip.h.
 * X: m x n, 0-based int32 CSR; rows need NOT be ascending, duplicate (row, column) pairs are legal (as for the transpose
 * and the extraction).  Both calls are synchronous, need no bound data (they work on a handle straight after
 * bhs_create), return BHS_ERR_INVALID_ARG between bhs_spgemm_symbolic and bhs_spgemm_finish, and leave the handle as it
 * was: counters, queues (2 m ints), accumulators (8 bytes an output), events and the pinned mirror are buffers of their
 * own from the grow-only pool; C of the last multiply, a served sum or selection, "class_state", the speculative-launch
 * figures and every option stay.  ms_out (may be NULL): device time of the call, validation included.
 *
 * bhs_csr_reduce_device: d_out = reduce(X) along `axis` with `op`.
 *   axis  BHS_AXIS_ROWS  d_out has m values, one per row
 *         BHS_AXIS_COLS  d_out has n values, one per column
 *         BHS_AXIS_ALL   d_out has one value
 *         BHS_AXIS_DIAG  d_out has min(m, n) values; out[i] reduces the entries with row == col == i (duplicate pairs
 *                        reduce together; with PLUS this is diag(X))
 *   op                    reduction            identity (a row, column or diagonal without an entry)
 *     BHS_RED_PLUS        sum of x             +0
 *     BHS_RED_MIN         min of x             +Inf
 *     BHS_RED_MAX         max of x             -Inf
 *     BHS_RED_ABS_PLUS    sum of |x|           +0
 *     BHS_RED_ABS_MAX     max of |x|           +0
 *     BHS_RED_SQ_PLUS     sum of x * x         +0
 *     BHS_RED_COUNT       number of entries    +0      (never reads d_valX; exact up to 2^53 in the double build and
 *                                                       2^24 in the float build, as BHS_SR_PLUS_PAIR)
 *   flags BHS_RED_OFFDIAG skips the entries with col == row; refused with BHS_AXIS_DIAG.
 *   d_valX may be NULL: every entry then counts as the value 1.
 * Arithmetic (worded as for the semirings): every entry is converted to double and reduced in double -- for float
 *   inputs |x| and x * x are exact there --, with ONE rounding to bhs_value_t per output.  min and max order values as
 *   numbers with -0 below +0.  A NaN entry makes its output NaN, under ABS_MAX too; which NaN is not specified.  A sum
 *   that is zero comes out as +0.
 * Reproducibility: MIN, MAX, ABS_MAX and COUNT are bit-for-bit functions of the input on every axis.  The sum operators
 *   (PLUS, ABS_PLUS, SQ_PLUS) on ROWS, DIAG and ALL add in an order that is a function of the input and the build alone
 *   -- two calls on the same arrays give the same bits; ALL forms one partial per workgroup, their number a function of
 *   nnzX alone, and adds the partials in a second pass of fixed order, never with atomics on one address.  The sum
 *   operators on COLS accumulate with atomics (in LDS, then in memory): their last bits may differ from run to run.
 * What is read: d_colIndX only where the call needs it -- BHS_AXIS_COLS, BHS_AXIS_DIAG (in the rows below min(m, n)) and
 *   BHS_RED_OFFDIAG --, and it is checked where it is read.  A plain row sum or total reads rowPtrX and valX only, 8 bytes
 *   an entry and not 12; COUNT on ROWS without OFFDIAG reads the row pointer alone.
 * Validation: on the device, BEFORE d_out is written (every kernel reduces into scratch; the last one, reduce_finish,
 *   rounds and stores only where nothing was refused).  rowPtrX[0] != 0, a decreasing rowPtrX, rowPtrX[m] != nnzX, or --
 *   in the calls that read columns -- a column outside [0, n) return BHS_ERR_INVALID_ARG with d_out untouched.  On the
 *   host: an unknown axis, op or flag bit, OFFDIAG with DIAG, d_out overlapping an input return BHS_ERR_INVALID_ARG.
 *   m, n and nnzX may be 0; BHS_AXIS_ALL still writes the identity.
 * bhs_get_kernel_stats then reports the families reduce_short (every row in order: the row pointer's check, the rows of
 *   up to 32 entries, 16 lanes each), reduce_wave (up to 1024 entries, a wave each), reduce_long (a workgroup each) for
 *   ROWS and DIAG; reduce_cols for COLS; reduce_all for ALL (after the three row families under OFFDIAG); reduce_finish.
 *
 * bhs_csr_scale_device: Z = alpha * Dl * X * Dr on X's pattern, Dl = diag(d_left) (m values), Dr = diag(d_right) (n
 *   values); either may be NULL (no such factor).  The pattern arrays are not copied: the caller reuses d_rowPtrX and
 *   d_colIndX for Z.  d_valZ (nnzX values) may equal d_valX (in place); any other overlap with an input is refused.
 *   flags BHS_SCALE_LEFT_DIV divides by left[i] instead of multiplying, BHS_SCALE_RIGHT_DIV the same for right[j]:
 *         D^-1 A needs no vector of reciprocals and is the correctly rounded quotient.  A DIV flag without its vector
 *         returns BHS_ERR_INVALID_ARG.
 * Arithmetic, in this order, so that numpy reproduces it bit for bit: t = double(x); with a left vector t = t * l[i]
 *   (t / l[i] under LEFT_DIV); with a right vector t = t * r[j] (t / r[j] under RIGHT_DIV); t = t * alpha; one rounding
 *   to bhs_value_t.  Only multiplications and divisions: FMA contraction cannot change a bit.  Division by zero and
 *   non-finite values follow IEEE; nothing is skipped.
 * Validation: rowPtrX is validated on the device before anything is written (BHS_ERR_INVALID_ARG, d_valZ untouched).
 *   d_colIndX is read only when d_right is given; a column outside [0, n) is never used as an index and the call returns
 *   BHS_ERR_INVALID_ARG -- scaling in place is legal, so that refusal may leave d_valZ[0, nnzX) partly written.  Nothing is
 *   ever written outside [0, nnzX).
 * Kernel-stat families: scale (no left vector: entry by entry), scale_short / scale_wave / scale_long (with a left
 *   vector: by rows, binned as the reduction's).  16 compulsory bytes an entry, 4 more with d_right.                    */
enum {
  BHS_AXIS_ROWS = 0,
  BHS_AXIS_COLS = 1,
  BHS_AXIS_ALL  = 2,
  BHS_AXIS_DIAG = 3
};
enum {
  BHS_RED_PLUS     = 0,
  BHS_RED_MIN      = 1,
  BHS_RED_MAX      = 2,
  BHS_RED_ABS_PLUS = 3,
  BHS_RED_ABS_MAX  = 4,
  BHS_RED_SQ_PLUS  = 5,
  BHS_RED_COUNT    = 6
};
enum { BHS_RED_OFFDIAG = 1 };
enum { BHS_SCALE_LEFT_DIV = 1, BHS_SCALE_RIGHT_DIV = 2 };
BHS_API int bhs_csr_reduce_device(bhs_handle *h, int m, int n, int nnzX,
        const bhs_value_t *d_valX /* may be NULL: every entry counts as 1 */,
        const int *d_rowPtrX, const int *d_colIndX,
        int axis, int op, int flags, bhs_value_t *d_out, double *ms_out /* may be NULL */);
BHS_API int bhs_csr_scale_device(bhs_handle *h, int m, int n, int nnzX,
        const bhs_value_t *d_valX, const int *d_rowPtrX, const int *d_colIndX,
        double alpha, const bhs_value_t *d_left /* m values or NULL */,
        const bhs_value_t *d_right /* n values or NULL */, int flags,
        bhs_value_t *d_valZ /* nnzX; may equal d_valX */, double *ms_out /* may be NULL */);

/* ---- CSR x dense ----------------------------------------------------------
 * A CSR matrix applied to a dense vector or to k dense vectors at once: y = alpha A x + beta y (the residual b - A x, a
 * smoother sweep, P^T r and P e of a multigrid cycle, a power-iteration step) and Y = alpha A X + beta Y; no reference
 * counterpart; bhs_spmv.hip.h.  Plus-times only; for A^T transpose first (bhs_csr_transpose_device).
 * A: m x n, 0-based int32 CSR; rows need NOT be ascending, duplicate (row, column) pairs are legal and add up (as for
 * the reductions).  m, n and nnzA may be 0.  d_valA may be NULL: every entry then counts as the value 1.
 * X is n x k, Y is m x k, both row-major with leading dimensions ldX, ldY >= k: element (i, c) sits at i * ld + c,
 * indexed in 64 bits.  bhs_csr_spmv_device is the k = 1, ld = 1 case of the same code.
 * Both calls are synchronous on the handle's stream, need no bound data (they work on a handle straight after
 * bhs_create), return BHS_ERR_INVALID_ARG between bhs_spgemm_symbolic and bhs_spgemm_finish, and leave the handle as it
 * was: counters, queues (2 m ints), events and the pinned mirror are buffers of their own from the grow-only pool; C of
 * the last multiply (whose device arrays from bhs_get_C_device may be passed straight in as A), a served sum or
 * selection, "class_state", the speculative-launch figures and every option stay.  ms_out (may be NULL): device time of
 * the call, validation included.
 * Arithmetic (worded as for the reductions): every product is double(a) * double(x); the products of a row are summed in
 *   double from +0 to s; t = alpha * s; if beta != 0, t = t + beta * double(y_old); ONE rounding to bhs_value_t.
 *   beta == 0 never reads d_y: it may hold NaN or be uninitialised.  alpha == 0 takes no shortcut: Inf and NaN in A or x
 *   propagate by IEEE.  FMA contraction is allowed; the sign of a zero result is not specified.
 * Reproducibility: the order of every sum is a function of the input arrays and the build alone -- two calls on the same
 *   arrays give the same bits.  No atomics on an output, no accumulation across workgroups.
 * Validation: on the device.  rowPtrA[0] != 0, a decreasing rowPtrA, rowPtrA[m] != nnzA, or a column outside [0, n)
 *   return BHS_ERR_INVALID_ARG.  The check comes before the dependent read: a refused row pointer is never used to
 *   address colIndA or valA, a refused column never to address x.  y is an in/out array, so a refused call may leave y
 *   partly written (as bhs_csr_scale_device in place).  Nothing is ever written outside the m x k elements of Y: not in
 *   the gaps c in [k, ldY) of a row, not past row m - 1.  X's gap columns are never read.
 *   On the host: a NULL handle, negative sizes, k < 1, ldX < k, ldY < k, a NULL d_rowPtrA, a NULL d_colIndA or d_x with
 *   nnzA > 0, a NULL d_y with m > 0, or d_y's footprint ((m - 1) ldY + k values) overlapping an input return
 *   BHS_ERR_INVALID_ARG with d_y untouched.
 * Rows are binned by length as the reductions bin them; bhs_get_kernel_stats then reports the families spmv_short (every
 *   row in order: the row pointer's check, the rows of up to 32 entries, 16 lanes each), spmv_wave (up to 1024 entries, a
 *   wave each), spmv_long (a workgroup each) for k = 1 and spmm_short, spmm_wave, spmm_long for k >= 2.  One round trip
 *   for the queues' lengths, and only when nnzA > 32.  For k >= 2 the lanes of a row lie along the columns of X first
 *   (tiles of 2, 4, .. 64 columns; a wider k loops over tiles of 64): one entry's gather is one contiguous read of X's
 *   row, and the entry is read once per tile.  Compulsory traffic: 12 bytes an entry (8 without values), 4 (m + 1), and
 *   the dense arrays.                                                                                                  */
BHS_API int bhs_csr_spmv_device(bhs_handle *h, int m, int n, int nnzA,
        const bhs_value_t *d_valA /* may be NULL: every entry counts as 1 */,
        const int *d_rowPtrA, const int *d_colIndA,
        double alpha, const bhs_value_t *d_x /* n */,
        double beta, bhs_value_t *d_y /* m, in/out */, double *ms_out /* may be NULL */);
BHS_API int bhs_csr_spmm_device(bhs_handle *h, int m, int n, int nnzA,
        const bhs_value_t *d_valA /* may be NULL */, const int *d_rowPtrA, const int *d_colIndA,
        int k, double alpha, const bhs_value_t *d_X /* n x k */, long long ldX /* >= k */,
        double beta, bhs_value_t *d_Y /* m x k, in/out */, long long ldY /* >= k */, double *ms_out /* may be NULL */);

/* ---- sampled dense-dense product -------------------------------------------
 * The product of two dense matrices evaluated only at the entries of a sparse pattern (SDDMM, the third of the usual
 * sparse-dense trio beside "CSR x dense"):
 *     Z(i, j) = alpha (X(i, :) . Y(j, :)) [M(i, j)] + beta Z_old(i, j)     for (i, j) in pattern(M)
 * -- scores on the edges of a graph (cosine similarity, attention logits that bhs_csr_spmm_device then applies), the
 * residual of a factorisation on its observed entries, the affinity of relaxed test vectors as an AMG strength of
 * connection; no reference counterpart; bhs_sddmm.hip.h.
 * M: m x n, 0-based int32 CSR; rows need NOT be ascending, duplicate (row, column) pairs are legal and every stored entry
 * gets its own value.  m, n and nnzM may be 0; k >= 1.  d_valM is read under BHS_SDDMM_TIMES_M only and may be NULL
 * without it.  X is m x k, Y is n x k, both row-major with leading dimensions ldX, ldY >= k: element (i, c) sits at
 * i * ld + c, indexed in 64 bits; the gap columns c in [k, ld) are never read.  d_X == d_Y is legal.  Z lives on M's
 * pattern: d_valZ holds nnzM values, the pattern arrays are not copied.
 * The call is synchronous on the handle's stream, needs no bound data (it works on a handle straight after bhs_create),
 * returns BHS_ERR_INVALID_ARG between bhs_spgemm_symbolic and bhs_spgemm_finish, and leaves the handle as it was:
 * counters, queues (2 m ints), events and the pinned mirror are buffers of its own from the grow-only pool; C of the last
 * multiply (whose device arrays from bhs_get_C_device may be passed straight in as M), a served sum or selection,
 * "class_state", the speculative-launch figures and every option stay.  ms_out (may be NULL): device time of the call,
 * validation included.
 * Arithmetic: all of it in double with FMA contraction OFF, so that a host loop (or numpy) restates it bit for bit.  Let
 *   T = min(64, the smallest power of two >= k).  Lane l in [0, T) holds s_l, starting from +0.  For tiles t = 0, 1, .. in
 *   ascending order lane l does s_l = s_l + double(X(i, tT + l)) * double(Y(j, tT + l)) where tT + l < k (the product is
 *   rounded, then the sum; a lane past k adds nothing).  The lanes then meet in the butterfly xor 1, 2, 4, .. T / 2, in
 *   that order: s_l = s_l + s_(l xor w), both partners the same bits.  Under BHS_SDDMM_TIMES_M s = s * double(m_ij).
 *   t = alpha * s; if beta != 0, t = t + beta * double(z_old); ONE rounding to bhs_value_t.
 *   beta == 0 never reads d_valZ: it may hold NaN or be uninitialised.  alpha == 0 takes no shortcut: Inf and NaN in X, Y
 *   or M propagate by IEEE.  In the float build the products are exact and the rule is the same.
 * Reproducibility: the bits of Z(i, j) are a function of X(i, :), Y(j, :), k, alpha, beta, m_ij and z_old alone -- not of
 *   the row's length, the entry's place in it, the kernel family that served it, the handle or the run.  No atomics.
 * Aliasing: d_valZ may be exactly d_valM (in place; under TIMES_M with beta != 0 both read the same old number).  Any
 *   other overlap of d_valZ[0, nnzM) with an input returns BHS_ERR_INVALID_ARG on the host with d_valZ untouched.
 * Validation: on the device.  rowPtrM[0] != 0, a decreasing rowPtrM, rowPtrM[m] != nnzM, or a column outside [0, n)
 *   return BHS_ERR_INVALID_ARG.  The check comes before the dependent read: a refused row pointer is never used to
 *   address colIndM, valM or valZ, a refused column never to address Y.  Z is an in/out array, so a refused call may leave
 *   d_valZ[0, nnzM) partly written; nothing is ever written outside it.
 *   On the host: a NULL handle, negative sizes, k < 1, ldX < k, ldY < k, a NULL d_rowPtrM, a NULL d_colIndM, d_X, d_Y or
 *   d_valZ with nnzM > 0, a NULL d_valM under TIMES_M with nnzM > 0, or unknown flag bits return BHS_ERR_INVALID_ARG with
 *   nothing written.
 * Rows are binned by length as the reductions bin them -- for load balance alone, no sum crosses entries --;
 *   bhs_get_kernel_stats then reports the families sddmm_short (every row in order: the row pointer's check, the rows of
 *   up to 32 entries), sddmm_wave (up to 1024 entries, a wave each) and sddmm_long (a workgroup each).  One round trip for
 *   the queues' lengths, and only when nnzM > 32.  The T lanes of an entry lie along k: one entry's gather is one
 *   contiguous read of Y's row, X's row piece stays in a register across the row's entries (k > 64 loops over tiles of 64
 *   and reads it again per tile).  Compulsory traffic: 4 bytes an entry and one value written (one more read under
 *   TIMES_M, one more where beta != 0), 4 (m + 1), X once, and a row of Y per entry wherever the cache does not hold it.  */
#define BHS_SDDMM_TIMES_M 1u
BHS_API int bhs_csr_sddmm_device(bhs_handle *h, int m, int n, int nnzM,
        const bhs_value_t *d_valM /* may be NULL without TIMES_M */,
        const int *d_rowPtrM, const int *d_colIndM,
        int k, double alpha,
        const bhs_value_t *d_X /* m x k */, long long ldX /* >= k */,
        const bhs_value_t *d_Y /* n x k */, long long ldY /* >= k */,
        double beta, bhs_value_t *d_valZ /* nnzM, in/out */,
        unsigned flags /* BHS_SDDMM_TIMES_M or 0 */, double *ms_out /* may be NULL */);

/* ---- approximate inverse --------------------------------------------------
 * The factorised sparse approximate inverse of a symmetric positive definite matrix (FSAI, Kolotilina and Yeremin): the
 * values of a lower-triangular G on a pattern the caller gives, with G A G^T ~ I and (G A G^T)_ii = 1 -- a preconditioner
 * that is applied as z = G^T (G r), two calls of bhs_csr_spmv_device, without levels, colours or any other sequential
 * dependence, and is symmetric for CG; no reference counterpart; bhs_fsai.hip.h.  G^T comes from
 * bhs_csr_transpose_device, the patterns tril(A) or a band of it from the entry selection.
 * A: n x n, 0-based int32 CSR.  Entries of A with column > row are never used: the caller may pass A or tril(A).  Of a row
 *   of A that is read, the entries up to and including the first whose column is >= the row must be strictly ascending
 *   with columns in [0, n); what lies behind that entry is not looked at.
 * The pattern of G (the caller's; n rows, nnzG entries): row i has d_i >= 1 entries J = (j_0 < .. < j_(d-1)), strictly
 *   ascending, with j_(d-1) = i and d_i <= BHS_FSAI_MAX_ROW.  It need not lie inside A's.
 * The matrix of a row, M (d x d, its lower triangle only): for q <= p, M_pq = double(the entry of A's row j_p with column
 *   j_q), +0 where row j_p holds none.
 * Arithmetic: all of it in double with FMA contraction OFF and true divisions (no reciprocal), so that a host loop (or
 *   numpy) restates it bit for bit.  This order is the contract:
 *   1. For c = 0 .. d-1: l_cc = sqrt(m_cc); l_rc = m_rc / l_cc for r > c; m_rc' = m_rc' - l_rc * l_c'c for every
 *      c < c' <= r (the product rounded, then the difference).  Every element takes its updates in ascending c.
 *   2. t = e_(d-1), the unit vector of the last position.  For q = d-1 .. 0: g_q = t_q / l_qq; t_p = t_p - l_qp * g_q for
 *      every p < q (the product rounded, then the difference).
 *   3. valG[rowPtrG[i] + p] = bhs_value_t(g_p): ONE rounding.
 *   So L^T g = e_d: row i of G is the last row of the inverse Cholesky factor of A(J, J).
 * Pivots: *bad_row_out (may be NULL) is the smallest row in which some m_cc is not > 0 or not finite when its root is
 *   taken, or -1.  The call still returns BHS_SUCCESS and the values follow IEEE, as with pivot_out of
 *   bhs_csr_ilu0_device; other rows are unaffected.
 * The call is synchronous on the handle's stream, needs no bound data (it works on a handle straight after bhs_create),
 * returns BHS_ERR_INVALID_ARG between bhs_spgemm_symbolic and bhs_spgemm_finish, and leaves the handle as it was:
 * counters, queues (2 n ints), events and the pinned mirror are buffers of its own from the grow-only pool; C of the last
 * multiply, a served sum or selection, "class_state", the speculative-launch figures and every option stay.  ms_out (may
 * be NULL): device time of the call, validation included.  n == 0 succeeds and launches nothing.
 * Reproducibility: the values are a function of the arguments -- the same bits from call to call and from handle to
 *   handle, whatever kernel family serves a row.  No atomics on an output.
 * Validation: on the device, each check ahead of the dependent read.  rowPtrG[0] != 0, a decreasing rowPtrG,
 *   rowPtrG[n] != nnzG; a row of G that is empty, longer than BHS_FSAI_MAX_ROW, not strictly ascending, with a column
 *   outside [0, i] or not ending in i; bounds of a row of A that is read outside [0, nnzA] or decreasing; an entry of the
 *   examined part of such a row that is not above its predecessor or outside [0, n): BHS_ERR_INVALID_ARG, after which
 *   d_valG[0, nnzG) is unspecified.  Nothing is ever written outside it.
 *   On the host: a NULL handle, negative sizes, flags != 0, a NULL array with n > 0, nnzG < n, or d_valG's nnzG values
 *   overlapping an input return BHS_ERR_INVALID_ARG with d_valG untouched.
 * Rows are binned by d; bhs_get_kernel_stats then reports the families fsai_short (every row in order: the validation of
 *   G, the rows of d <= 16, 16 lanes each), fsai_wave (17 <= d <= 64, a wave each) and fsai_long (65 <= d <= 128, a
 *   workgroup each); a family without rows is not launched.  One round trip for the queues' lengths, and only when
 *   nnzG > 16.  M lies packed in LDS (136, 2080 or 8256 doubles a row); grids are not capped: a row's work is bounded by
 *   its 128 unknowns.                                                                                                  */
#define BHS_FSAI_MAX_ROW 128
BHS_API int bhs_csr_fsai_device(bhs_handle *h, int n, int nnzA,
        const int *d_rowPtrA, const int *d_colIndA, const bhs_value_t *d_valA,
        int nnzG, const int *d_rowPtrG, const int *d_colIndG /* the pattern of G, the caller's */,
        bhs_value_t *d_valG /* out: nnzG values */,
        int flags /* must be 0 */, int *bad_row_out /* may be NULL */, double *ms_out /* may be NULL */);

/* ---- relaxation and fused products ----------------------------------------
 * What a multigrid cycle and a Krylov iteration do between two setups, as library calls with every array on the device
 * (no reference counterpart; bhs_relax.hip.h): `steps` sweeps of a polynomial smoother in one call -- weighted Jacobi, or
 * a Chebyshev polynomial in D^-1 A with the coefficients of bhs_chebyshev_coefficients --, and the vector product together
 * with the reductions an iteration wants of its result: r = b - A x with ||r||^2, q = A p with <p, q>.
 * A (A is n x n for the relaxation, m x n for the product): as "CSR x dense" -- 0-based int32 CSR, rows need NOT be
 *   ascending, duplicate (row, column) pairs are legal and add up, sizes may be 0, d_valA may be NULL: every entry then
 *   counts as the value 1.
 * All calls but bhs_chebyshev_coefficients are synchronous on the handle's stream, need no bound data, return
 * BHS_ERR_INVALID_ARG between bhs_spgemm_symbolic and bhs_spgemm_finish, and leave the handle as "CSR x dense" leaves it:
 * their workspaces are buffers of their own from the grow-only pool; C of the last multiply, a served sum or selection,
 * "class_state", the speculative-launch figures and every option stay.  ms_out (may be NULL): device time of the call.
 *
 * bhs_csr_relax_device.  coef holds `steps` pairs (a_s, c_s) on the HOST.  Step s, for all rows at once and reading only
 *   the x from before the step:
 *     sum_i = the products double(a) * double(x) of row i, summed in double from +0 exactly as bhs_csr_spmv_device sums
 *             them (the same bits); r = double(b_i) - sum_i; q = r / double(diag_i); dn = c_s * q; where a_s != 0,
 *             dn = dn + a_s * double(d_i); d_i <- (bhs_value_t) dn (stored when d_d is not NULL);
 *             x_i <- (bhs_value_t)(double(x_i) + dn).
 *   a_s == 0 never reads d_d.  d_diag is the divisor of every row, given by the caller (the diagonal of A, as a rule); a
 *   zero or non-finite diag_i propagates by IEEE.  c_s == 0 takes no shortcut.  The operations after the row sum round
 *   one by one (no contraction), so numpy reproduces them bit for bit from the sum.  Weighted Jacobi is a = 0, c = omega.
 *   BHS_RELAX_ZERO_GUESS: x counts as +0 in step 0 -- d_x is never read before it is written and may hold NaN -- and
 *   step 0 runs no product pass: dn = c_0 * b / diag (+ a_0 d).  A cycle's coarse levels and every application of a
 *   preconditioner start from zero: one of `steps` products saved.
 *   In place without a race: a step reads x from one array and writes another (d_x and two vectors of the workspace take
 *   turns); the result ends in d_x.
 *   Rows are binned once, in step 0, as the reductions bin them; later steps reuse the queues: one round trip for the
 *   queues' lengths (only when nnzA > 32) and one at the end, whatever `steps` is.  Kernel-stat families: relax_short,
 *   relax_wave, relax_long -- one launch per product pass each, for the bins that have rows (relax_short always) --,
 *   relax_zero (step 0 under ZERO_GUESS: the row pointer's check, the queues, the update) and relax_finish (the copy of a
 *   call whose last step may not write the caller's arrays yet: steps == 1, or steps == 2 under ZERO_GUESS).
 *   Reproducibility: the same arrays give the same bits from run to run and from handle to handle; one call of S steps
 *   gives the bits of S chained calls of one step with d_d carried between them.
 *   Validation: on the device, before the dependent read, with the refusals of "CSR x dense": rowPtrA[0] != 0, a
 *   decreasing rowPtrA, rowPtrA[n] != nnzA, a column outside [0, n) return BHS_ERR_INVALID_ARG.  Stricter than there, a
 *   refused call leaves d_x and d_d untouched: up to and including the first product pass, which reads every column, the
 *   kernels write the workspace only, and every later kernel leaves at once where the error word is raised.
 *   On the host: a NULL handle, negative sizes, steps < 1, a NULL coef or a non-finite coefficient, unknown flag bits, a
 *   NULL d_rowPtrA, a NULL d_colIndA with nnzA > 0, a NULL d_diag, d_b or d_x with n > 0, a NULL d_d with n > 0 and some
 *   a_s != 0, or d_x or d_d overlapping each other or an input return BHS_ERR_INVALID_ARG with nothing written.
 *
 * bhs_chebyshev_coefficients.  A host function without device work: the `steps` pairs for the Chebyshev iteration on the
 *   interval [lmin, lmax] of the spectrum of D^-1 A (Saad, Iterative Methods for Sparse Linear Systems, Algorithm 12.1).
 *   theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma = theta / delta; step 0: (0, 1 / theta), rho_0 = 1 / sigma;
 *   step s >= 1: rho_s = 1 / (2 sigma - rho_(s-1)), (rho_s rho_(s-1), 2 rho_s / delta).  The error after s steps is
 *   T_s((theta - lambda) / delta) / T_s(sigma) on every eigen-component lambda.  Anything but 0 < lmin < lmax, both
 *   finite, steps >= 1 and a coef that is not NULL returns BHS_ERR_INVALID_ARG.
 *
 * bhs_csr_spmv_dots_device.  z = alpha A x + beta y with the arithmetic, the single rounding, the kernels and the bits
 *   of bhs_csr_spmv_device, out of place: d_z may be exactly d_y (in place) and may overlap no other input; otherwise y is
 *   copied to z on the device first.  beta == 0 never reads d_y, which may then be NULL.  Then, of the STORED z:
 *     dots[0] = sum of double(z_i)^2;  dots[1] = sum of double(w_i) * double(z_i), left unwritten when d_w is NULL.
 *   d_w may be d_x when m == n.  Both sums run in double over 4096 consecutive elements a workgroup and then over the
 *   workgroups' partials in their order, by one workgroup: an order that is a function of m and the build alone, no atomic
 *   on a result; non-finite values propagate.  8 to 16 bytes a row beside the product's 12 bytes an entry.  dots is on the
 *   HOST and is written on success only; a refused call may leave z partly written, as y there.  Refusals: those of
 *   bhs_csr_spmv_device, a NULL dots, a NULL d_y with beta != 0 and m > 0, d_z overlapping d_w.  k = 1 only.
 *   Kernel-stat families: spmv_short, spmv_wave, spmv_long, dots_part, dots_finish.                                     */
#define BHS_RELAX_ZERO_GUESS 1u
BHS_API int bhs_csr_relax_device(bhs_handle *h, int n, int nnzA,
        const bhs_value_t *d_valA /* may be NULL: every entry counts as 1 */,
        const int *d_rowPtrA, const int *d_colIndA,
        const bhs_value_t *d_diag /* n: the divisor of row i */,
        int steps, const double *coef /* HOST: 2 * steps, (a_0, c_0), (a_1, c_1), .. */,
        const bhs_value_t *d_b /* n */, bhs_value_t *d_x /* n, in/out */,
        bhs_value_t *d_d /* n, in/out; may be NULL when every a_s == 0 */,
        unsigned flags /* BHS_RELAX_ZERO_GUESS or 0 */, double *ms_out /* may be NULL */);
BHS_API int bhs_chebyshev_coefficients(double lmin, double lmax, int steps, double *coef /* out: 2 * steps */);
BHS_API int bhs_csr_spmv_dots_device(bhs_handle *h, int m, int n, int nnzA,
        const bhs_value_t *d_valA /* may be NULL */, const int *d_rowPtrA, const int *d_colIndA,
        double alpha, const bhs_value_t *d_x /* n */,
        double beta, const bhs_value_t *d_y /* m; may be NULL when beta == 0 */,
        bhs_value_t *d_z /* m, out; may be exactly d_y */,
        const bhs_value_t *d_w /* m; may be NULL; may be d_x when m == n */,
        double *dots /* HOST: 2 */, double *ms_out /* may be NULL */);

/* ---- semiring CSR x dense -------------------------------------------------
 * One step of a graph traversal with every array on the device: y<mask> (+)= A (+).(x) x and, for k vectors (k sources)
 * at once, Y<M> (+)= A (+).(x) X over the eight semirings of "semiring multiply" (GraphBLAS mxv / mxm with a dense
 * operand; no reference counterpart; bhs_spmv_sr.hip.h): a Bellman-Ford relaxation (MIN_PLUS with BHS_MV_ACCUM), a
 * pull-direction BFS frontier (OR_AND under the complement of the visited set), bottleneck paths (MAX_MIN, MIN_MAX).
 * Row i pulls from its columns: an entry A(i, j) is an edge j -> i.
 * A, X, Y: as "CSR x dense" -- A is m x n, 0-based int32 CSR, rows need NOT be ascending, duplicate (row, column) pairs are
 *   legal and every one of them is an entry; m, n and nnzA may be 0; d_valA may be NULL: every entry then counts as the
 *   value 1.  X is n x k, M and Y are m x k, row-major with leading dimensions ldX, ldM, ldY >= k, indexed in 64 bits; the
 *   gaps c in [k, ld) are never read and never written.  bhs_csr_spmv_semiring_device is the k = 1, ld = 1 case of the
 *   same code.
 * The rule.  For element (i, c), t = (+) over the entries e of row i of a_e (x) X(col_e, c): product, reduction and
 *   identity from the table of "semiring multiply", for all eight BHS_SR_*.  Every element of X counts as an entry (a
 *   dense operand has no pattern); a row without entries gives the (+)-identity.  BHS_SR_PLUS_PAIR reads neither valA nor
 *   X and gives the number of entries of the row, duplicates counted (its columns are read and checked).  Order of min and
 *   max, -0 below +0, NaN propagation, OR_AND's notion of non-zero: word for word those of "semiring multiply".
 *   Arithmetic in double, ONE rounding to bhs_value_t per element.
 * Accumulate.  Without BHS_MV_ACCUM, Y(i,c) = round(t) and y_old is never read: it may be NaN or uninitialised.  With it,
 *   Y(i,c) = round(double(y_old) (+) t): min for the MIN_ semirings, max for MAX_, or for OR_AND (y_old != 0 counts as
 *   1), + for PLUS_.  A NaN y_old gives NaN for min and max.
 * Mask.  Element (i, c) of M is SET where its value is non-zero: NaN is set, -0 and +0 are not.  With
 *   BHS_MV_MASK_COMPLEMENT an element is selected where it is NOT set; a NULL mask selects everything; COMPLEMENT with a
 *   NULL mask is refused.  An element the mask does not select is neither read nor written, with or without ACCUM.  A row
 *   none of whose k elements is selected is not walked at all -- its columns and values are not read --, which is what
 *   makes a pull-direction BFS cheaper as the visited set grows.  Columns are therefore checked where they are read.
 * changed_out (may be NULL): the number of selected elements whose stored value differs, as a number, from what it was
 *   accumulated into: y_old with ACCUM ("has the relaxation converged"), the (+)-identity without ("how large is the next
 *   frontier").  +0 equals -0; NaN over NaN counts as unchanged, NaN against a number as changed.  The count is an exact
 *   integer: summed per workgroup, added once per workgroup to a 64-bit control word and read in the round trip the call
 *   makes anyway for its error word -- y is never copied to the host.  Integer adds commute: the same count from run to
 *   run.  Written on success only.  With a NULL changed_out the count is not taken at all (the kernels skip it).
 * Reproducibility: min, max, or and pair are bit-for-bit functions of the input.  The PLUS_TIMES sum has the guarantee of
 *   "CSR x dense": its order is a function of the input arrays and the build alone.  No atomics touch Y, nothing
 *   accumulates across workgroups into Y.  PLUS_TIMES runs the kernels of this section like the others (with a mask it
 *   could not forward to bhs_csr_spmm_device, and one path is easier to reason about than two).
 * Validation: on the device, as "CSR x dense": rowPtrA[0] != 0, a decreasing rowPtrA, rowPtrA[m] != nnzA, or a column
 *   outside [0, n) in a row that is read return BHS_ERR_INVALID_ARG.  The row pointer is checked in every row, selected
 *   or not; the check comes before the dependent read.  Y is an in/out array, so a call refused on the device may leave Y
 *   partly written (never outside its selected m x k elements).
 *   On the host, each BHS_ERR_INVALID_ARG with Y untouched: the list of "CSR x dense" (a NULL handle, negative sizes,
 *   k < 1, ldX < k, ldY < k, a NULL d_rowPtrA, a NULL d_colIndA or d_X with nnzA > 0, a NULL d_Y with m > 0), an unknown
 *   semiring, an unknown flag bit, ldM < k with a mask, COMPLEMENT without a mask, or Y's footprint overlapping A, X or M
 *   (M may overlap X: the levels of a BFS are mask and never operand, but nothing forbids it).
 * Both calls are synchronous on the handle's stream, need no bound data, return BHS_ERR_INVALID_ARG between
 *   bhs_spgemm_symbolic and bhs_spgemm_finish, and leave the handle as it was: C of the last multiply, a served sum or
 *   selection, "class_state", the speculative-launch figures and every option stay (the workspace is a buffer set of its
 *   own).  ms_out (may be NULL): device time of the call, validation included.
 * bhs_get_kernel_stats then reports srmv_short, srmv_wave, srmv_long -- the same three for every k: the bins of "CSR x
 *   dense" (up to 32 entries, up to 1024, beyond), one round trip for the queues' lengths and only when nnzA > 32; a row
 *   beyond the short bin is queued only where one of its k elements is selected.                                        */
enum { BHS_MV_ACCUM = 1, BHS_MV_MASK_COMPLEMENT = 2 };
BHS_API int bhs_csr_spmv_semiring_device(bhs_handle *h, int semiring, int m, int n, int nnzA,
        const bhs_value_t *d_valA /* may be NULL: ones */, const int *d_rowPtrA, const int *d_colIndA,
        const bhs_value_t *d_x /* n */, int flags, const bhs_value_t *d_mask /* m, or NULL */,
        bhs_value_t *d_y /* m, in/out */, long long *changed_out /* may be NULL */, double *ms_out /* may be NULL */);
BHS_API int bhs_csr_spmm_semiring_device(bhs_handle *h, int semiring, int m, int n, int nnzA,
        const bhs_value_t *d_valA /* may be NULL */, const int *d_rowPtrA, const int *d_colIndA,
        int k, const bhs_value_t *d_X /* n x k */, long long ldX /* >= k */, int flags,
        const bhs_value_t *d_M /* m x k, or NULL */, long long ldM /* >= k with a mask */,
        bhs_value_t *d_Y /* m x k, in/out */, long long ldY /* >= k */, long long *changed_out /* may be NULL */,
        double *ms_out /* may be NULL */);

/* ---- C/F splitting and interpolation ----------------------------------------
 * The other half of algebraic multigrid: classical (Ruge-Stueben) coarsening splits the vertices of an n x n pattern S of
 * strong connections into coarse (C) and fine (F) points, and the interpolation P (n x nc) has an identity row at every C
 * point and, at an F point, weights on its strong C neighbours (no reference counterpart; bhs_cfsplit.hip.h,
 * bhs_interp.hip.h).  Beside the two aggregations ("aggregation", "matching") the Galerkin operators stay sparse: P has no more entries a row than
 * S has.  amg.rs_setup_device builds the hierarchy.
 *
 * bhs_csr_cfsplit_device.  S is 0-based int32 CSR; values are NOT TAKEN, so the double and the float library run the same
 * code.
 * Neighbours and keys are the aggregation's.  N(i) is the set of columns of row i of S; the diagonal, repeated columns and
 *   the order inside a row make no difference; rows need not be sorted.  Vertex i has the key prio31(i) << 31 | i:
 *   prio31(i) = d_prio[i] >> 1 where d_prio is given, else h(i, seed) >> 1 of the aggregation's hash.  With BHS_CF_DEGREE
 *   (d_prio must be NULL, else BHS_ERR_INVALID_ARG)
 *       prio31(i) = min(rowPtrS[i+1] - rowPtrS[i], 1023) << 21 | h(i, seed) >> 11,
 *   the PMIS measure on a symmetric strength pattern: many dependants first, ties by hash, then by index.  Keys are distinct.
 * Result.  For a structurally symmetric S the C points are THE greedy maximal independent set in descending key order: a
 *   vertex is C exactly when no off-diagonal neighbour of greater key is C.  That set is unique; every F point has a C
 *   neighbour, no two C points are neighbours, an isolated vertex is C.  C points are numbered in ascending vertex order:
 *   d_cf[i] is the coarse index in [0, nc) of a C point and -1 for an F point, d_cpts (may be NULL) the C points, ascending,
 *   d_cf[d_cpts[c]] == c.  With the same d_prio or seed (no BHS_CF_DEGREE) d_cf[i] >= 0 exactly where bhs_csr_color_device
 *   gives colour 0.
 * Non-symmetric S.  The call still ends and every vertex is C or F; which one, is unspecified.
 * Rounds, synchronous over one word a vertex, state << 62 | key (undecided 1, in 2, out 0); a round reads one array of
 *   words and writes another.  For every undecided i, m is the maximum of the words over i and N(i): m's state is in: i is
 *   out; m is i's own word: i is in; else i stays undecided.  The undecided vertex of greatest key is decided in every
 *   round.  The host reads the error word and the count of undecided vertices once a round, one round trip; *rounds_out is
 *   the number of rounds until nobody is undecided, a function of the input (a path whose keys ascend with the index takes
 *   n, the worst case; grids and random patterns of a million vertices take about ten, profiles/cf_case.md).  The call returns
 *   BHS_ERR_INTERNAL when a round decides nothing or after n + 1 rounds; nothing spins on the device, no workgroup waits for
 *   another.
 * Numbering.  The C points are flagged per 64 vertices as a bitmap word, the words' counts go through the library's one-pass
 *   scan as the aggregation's roots do, a C point's number is its word's first number plus the C points below it in the word.
 *   No atomic touches a result.
 * Reproducibility.  The result is a function of (pattern, priorities or seed, flags) alone: the same bits from run to run,
 *   from handle to handle, and in the double and the float library.
 * Validation, on the device, each check ahead of the dependent read: rowPtrS[i] > rowPtrS[i+1] or either outside
 *   [0, nnzS]; a column outside [0, n).  On the host: a NULL handle, negative n or nnzS, a flag other than BHS_CF_DEGREE,
 *   BHS_CF_DEGREE with d_prio, NULL d_rowPtrS or d_cf with n > 0, NULL d_colIndS with nnzS > 0, the footprint of d_cf or
 *   d_cpts (n ints each) overlapping S, d_prio or each other, and a call between bhs_spgemm_symbolic and bhs_spgemm_finish.
 *   Each returns BHS_ERR_INVALID_ARG; the host's refusals leave the outputs untouched, after a refusal by the device they are
 *   unspecified; nothing beyond their stated sizes is ever written, nothing stays queued.
 * n == 0 succeeds with *nc_out = 0, *rounds_out = 0 and *ms_out = 0 and launches nothing.
 * Synchronous on the handle's stream, needs no bound data, leaves the handle as it was (a workspace of its own, shared with
 *   the interpolation).  ms_out (may be NULL): device time of the call, the rounds' round trips included.
 *   bhs_get_kernel_stats then reports cf_init (keys, the row pointer's validation), cf_round (the gather of a round, a row
 *   spread over 1, 4, 16 or 64 lanes by the pattern's mean row length) and cf_number (the C points counted per 64 vertices,
 *   the scan, the numbering).                                                                                        */
#define BHS_CF_DEGREE 1
BHS_API int bhs_csr_cfsplit_device(bhs_handle *h, int n, int nnzS,
        const int *d_rowPtrS, const int *d_colIndS /* n x n pattern of strong connections; values are not taken */,
        const unsigned *d_prio /* n caller priorities, or NULL: the hash */,
        unsigned seed, int flags /* 0 or BHS_CF_DEGREE */,
        int *d_cf /* out: n ints, the coarse index in [0, nc) of a C point, -1 for an F point */,
        int *d_cpts /* out, may be NULL: the C points, ascending; room for n ints */,
        int *nc_out /* may be NULL */, int *rounds_out /* may be NULL */, double *ms_out /* may be NULL */);

/* bhs_csr_interp_symbolic_device / bhs_csr_interp_numeric_device.  Direct interpolation P (n x nc) of the n x n matrix A on
 * the splitting d_cf (nc C points) and the pattern S of strong connections, as a symbolic / numeric pair with pattern reuse
 * like the add, the selection and the extraction: the pattern is a function of the patterns of A and S and of d_cf alone, so
 * the symbolic call takes no values and the numeric call may be repeated on a kept pattern with new values.
 * Input order.  Rows of A and of S are strictly ascending; checked on the device, else BHS_ERR_INVALID_ARG.
 * Interpolatory set.  C_i = { j != i : (i, j) is stored in A, j is in row i of S, d_cf[j] >= 0 } (membership in S's row: a
 *   binary search in the sorted row).
 * Pattern.  A C point's row is the single entry (d_cf[i], 1).  An F point's row has one entry d_cf[j] per j in C_i, in
 *   ascending j: P's rows are strictly ascending.  C_i may be empty on non-symmetric input; that row is empty.  An explicit
 *   zero a_ij keeps its entry, with value 0.
 * Values, in double with one rounding to the value type.  d = a_ii, or 0 where the diagonal is not stored.  An off-diagonal
 *   entry is of negative type where a_ij d < 0 and of positive type where a_ij d > 0.  N- and N+ are the sums over ALL
 *   off-diagonal entries of each type, C- and C+ the sums over C_i of each type.  d' = d, plus N+ where C+ == 0, plus N-
 *   where C- == 0, added in that order.  Then
 *       w_ij = -((N- / C-) a_ij) / d' for a negative-type j,   w_ij = -((N+ / C+) a_ij) / d' for a positive-type j,
 *   evaluated exactly in that order; an entry of neither type (a_ij d is 0 or NaN: an explicit zero, a diagonal that is not
 *   stored) carries none of either sum, w_ij = -(0 a_ij) / d'.  Where d' is 0 the IEEE results stand (a row of A without its
 *   diagonal gives NaNs).  Where A's row sums to 0 and every sign has a coarse representative, P's row sums to 1.
 *   The sums follow the SpMV's rule: a row is spread over 1, 4, 16 or 64 lanes by A's mean row length, a lane adds its
 *   entries in row order, the lanes meet in a butterfly -- the order depends on the row's length and the lanes a row alone,
 *   two calls give the same bits.
 * Symbolic.  Counts the entries of every row, scans the counts with the library's one-pass scan into d_rowPtrP (n + 1 ints)
 *   and returns *nnzP_out; one round trip for the error word and nnzP.  nnzP beyond INT_MAX: BHS_ERR_ALLOC.  After a refusal
 *   by the device d_rowPtrP is untouched.
 * Numeric.  Recomputes each row's count and compares it with rowPtrP (rowPtrP[0] == 0 and rowPtrP[n] == nnzP too); any
 *   disagreement returns BHS_ERR_INVALID_ARG with nothing written.  The fill writes entry k of row i only where
 *   k < rowPtrP[i+1] - rowPtrP[i] and rowPtrP[i] + k < nnzP: whatever the arrays hold, nothing is read or written out of
 *   bounds.  flags must be 0.
 * Validation, on the device, each check ahead of the dependent read or write: the row pointers of A, S and (numeric) P as
 *   the aggregation checks S's; a column of A or S outside [0, n); a row of A or S that does not ascend strictly; a d_cf
 *   value outside [-1, nc).  On the host: a NULL handle, negative n, nnzA, nnzS, nc or nnzP, nc > n, nnzP beyond INT_MAX,
 *   flags != 0, NULL arrays where sizes are positive (d_rowPtrA, d_rowPtrS, d_cf and d_rowPtrP with n > 0 -- d_rowPtrP of
 *   the symbolic call always --, d_colIndA and d_valA with nnzA > 0, d_colIndS with nnzS > 0, d_colIndP and d_valP with
 *   nnzP > 0), an output's footprint overlapping an input or another output, and a call between bhs_spgemm_symbolic and
 *   bhs_spgemm_finish.  Each returns BHS_ERR_INVALID_ARG; the host's refusals leave the outputs untouched.
 * n == 0: the symbolic call writes d_rowPtrP[0] = 0 and returns *nnzP_out = 0, the numeric call accepts nnzP == 0 alone; both
 *   launch no kernel.
 * Synchronous on the handle's stream, need no bound data, leave the handle as it was (the splitting's workspace).  ms_out
 *   (may be NULL): device time of the call.  bhs_get_kernel_stats then reports interp_count (validation, the rows' counts and
 *   their scan) and interp_fill (the sums, the entries).                                                             */
BHS_API int bhs_csr_interp_symbolic_device(bhs_handle *h, int n, int nnzA,
        const int *d_rowPtrA, const int *d_colIndA,
        int nnzS, const int *d_rowPtrS, const int *d_colIndS,
        const int *d_cf /* n ints in [-1, nc) */, int nc,
        int *d_rowPtrP /* out: n + 1 ints */,
        long long *nnzP_out /* may be NULL */, double *ms_out /* may be NULL */);
BHS_API int bhs_csr_interp_numeric_device(bhs_handle *h, int n, int nnzA,
        const int *d_rowPtrA, const int *d_colIndA, const bhs_value_t *d_valA,
        int nnzS, const int *d_rowPtrS, const int *d_colIndS,
        const int *d_cf /* n ints in [-1, nc) */, int nc,
        const int *d_rowPtrP /* the symbolic call's */, long long nnzP,
        int *d_colIndP /* out: nnzP ints */, bhs_value_t *d_valP /* out: nnzP values */,
        int flags /* must be 0 */, double *ms_out /* may be NULL */);

/* ---- strongly connected components ------------------------------------------
 * Which vertices of a DIRECTED graph reach one another: i and j are in one strongly connected component (SCC) where a path
 * leads from i to j and one from j to i -- irreducibility, the condensation DAG, the diagonal blocks of a block triangular
 * form, "the giant component" (no reference counterpart; bhs_scc.hip.h).  bhs_csr_components_device joins i and j whichever way
 * the entry points; this one answers the question about direction.
 * S is an n x n pattern, 0-based int32 CSR; values are NOT TAKEN, so the double and the float library run the same code and
 * give the same bits.  An entry (i, j) with j != i is a directed edge between i and j.  The SCCs of a graph and of its
 * reverse are the same, so which way the edge points does not matter: the call needs no transpose, and S and its
 * transpose give the same outputs.  Rows need not be sorted; repeated columns and self-loops change nothing.
 * Definition.  root[i] is the smallest vertex index of i's SCC.  comp[i] is the rank of root[i] among the roots, of which
 *   there are nscc: SCCs are numbered by ascending smallest vertex.  compSize[c] is the number of vertices with comp == c.
 *   d_root, d_comp, d_compSize, *nscc_out AND *rounds_out are a function of the pattern alone: the same bits from run to
 *   run, from handle to handle, and in the double and the float library.
 * Rounds (trim, forward-backward).  Per vertex: part, the colour class the previous round left it in, -1 once it is
 *   decided; a label, kept in d_root itself; a stamp and a reach flag.  An edge i -> j is valid in a round where j != i,
 *   both ends are live and part[i] == part[j].  A round runs four phases, each to ITS FIXED POINT, which is unique --
 *   that is why the rounds are a function of the pattern:
 *   1. Trim.  A live vertex with no valid out-edge or no valid in-edge is an SCC by itself.  A pass is two launches: the
 *      first stores the pass's stamp to stamp[j] over the valid edges (plain stores of one value: nothing is cleared, no
 *      atomic), the second looks for a valid out-edge in the row and for the stamp, and decides in place.  Liveness only
 *      falls.
 *   2. Forward labels.  label[v] = v on the live vertices; then passes in place over the live rows: label[j] is lowered to
 *      label[i] over the valid edges.  A word only ever falls: after the start every write is an atomic minimum, issued
 *      only where the value read is greater, the shortcut label[i] <- label[label[i]] included (once a row; sound because
 *      label[i] = u says that u reaches i inside the class).  At the fixed point label[v] is the smallest live vertex of
 *      v's class that reaches v.
 *   3. Backward reach.  The vertices with label[v] == v are reached; a pass pulls over the rows: a live i becomes reached
 *      where some valid edge i -> j has label[j] == label[i] and j reached.  Flags only rise.
 *   4. Decide.  A reached v is final with root[v] = label[v]: every member reaches the root and the root every member.
 *      Every other live v goes to the class part[v] = label[v].
 *   The smallest live vertex is always decided.  A round whose trim leaves no live vertex ends there and counts.
 *   *rounds_out is the number of rounds; a round that decides nothing, or more than n + 1 rounds, is BHS_ERR_INTERNAL.
 *   One-way rings that feed one another in ascending order take a round each; most inputs take one.
 * Passes.  The host launches 8 passes of a phase per control round trip and ends the phase after a batch whose last pass
 *   changed nothing; BHS_ERR_INTERNAL where a phase would need more than n + 1 passes.  *passes_out, the total of passes
 *   launched, DEPENDS ON TIMING -- a pass in place sees what other workgroups wrote during it; nothing else does.
 *   Nothing spins on the device, nothing waits for another workgroup.  The trim and the backward reach move one hop a
 *   synchronous pass: deep symmetric grids and long one-way chains are where this call loses (profiles/scc_case.md).
 * Outputs.  d_root: n ints.  d_comp (may be NULL): n ints in [0, nscc).  d_compSize (may be NULL, needs d_comp): CAPACITY n
 *   ints, of which nscc are written.  *nscc_out is counted as the SCCs are decided: it is written with or without d_comp.
 *   The numbering is the connected components': the root flags, the library's one-pass scan per 64 vertices, the ranks,
 *   the sizes by integer atomic adds.  The vertices sorted by SCC are the stable transpose of the n x nscc membership
 *   pattern, as there.
 * Validation, on the device, each check ahead of the dependent read: rowPtrS[i] > rowPtrS[i+1] or either outside
 *   [0, nnzS] (the row is taken as empty); a column outside [0, n) (never used as an index).  On the host: a NULL handle,
 *   negative n or nnzS, flags != 0, a NULL d_rowPtrS or d_root with n > 0, NULL d_colIndS with nnzS > 0,
 *   d_compSize without d_comp, an output's footprint overlapping S or another output, and a call between
 *   bhs_spgemm_symbolic and bhs_spgemm_finish.  Each returns BHS_ERR_INVALID_ARG.  After a refusal by the device the
 *   outputs are unspecified; nothing beyond their stated sizes is ever written, and nothing stays queued.
 * n == 0 succeeds with *nscc_out = 0, *rounds_out = 0 and *passes_out = 0 and launches nothing.
 * Synchronous on the handle's stream, needs no bound data, leaves the handle as it was (a workspace of its own).  ms_out
 *   (may be NULL): device time of the call, the round trips included.  bhs_get_kernel_stats then reports scc_trim (two
 *   launches a pass), scc_forward and scc_backward (a start and the passes, a round), scc_decide (one a round) and, where
 *   d_comp is given, scc_number; a row is spread over 1, 4, 16 or 64 lanes by the pattern's mean row length.           */
BHS_API int bhs_csr_scc_device(bhs_handle *h, int n, int nnzS,
        const int *d_rowPtrS, const int *d_colIndS /* n x n pattern; values are not taken */,
        int flags /* must be 0 */,
        int *d_root     /* out: n ints: the smallest vertex of i's SCC */,
        int *d_comp     /* out, may be NULL: n ints in [0, nscc), SCCs numbered by ascending root */,
        int *d_compSize /* out, may be NULL, needs d_comp: CAPACITY n, nscc written */,
        int *nscc_out /* may be NULL */, int *rounds_out /* may be NULL */,
        int *passes_out /* may be NULL; depends on timing */,
        double *ms_out /* may be NULL */);

/* ---- bandwidth-reducing ordering --------------------------------------------
 * The reverse Cuthill-McKee (RCM) ordering of a symmetric pattern: a permutation that makes the matrix narrow -- ahead of
 * ILU(0), of band and profile solvers, and to make SpMV on a shuffled mesh cache-friendly (symrcm, SPARSPAK's GENRCM; no
 * reference counterpart; bhs_rcm.hip.h).
 * S is an n x n pattern on the device, 0-based int32 CSR, rows STRICTLY ASCENDING, STRUCTURALLY SYMMETRIC.  Values are NOT
 * TAKEN, so the double and the float library run the same code and give the same bits.  A diagonal entry is allowed and
 * ignored.  deg(i) is the number of entries of row i with j != i; key(i) = (deg(i), i), compared lexicographically.
 * Refusals by the device, each BHS_ERR_INVALID_ARG, found by the first kernel and read before anything else runs: a falling
 *   row pointer, or nnzS != rowPtr[n]; a column outside [0, n); a row that is not strictly ascending (a repeated entry
 *   included); an entry (i, j) without (j, i), found by a binary search in row j.  After a refusal nothing stays queued,
 *   no output is promised, and nothing beyond the outputs' stated sizes is ever written.
 * Refusals by the host, each BHS_ERR_INVALID_ARG: a NULL handle, a call between bhs_spgemm_symbolic and bhs_spgemm_finish,
 *   negative n or nnzS, flags beyond BHS_RCM_PERIPHERAL | BHS_RCM_NO_REVERSE, a NULL d_rowPtrS or d_perm with n > 0, NULL
 *   d_colIndS with nnzS > 0, an output's footprint overlapping S or another output.
 * n == 0 succeeds with every count 0 and launches nothing.
 * Components.  root(i) is the smallest vertex of i's connected component, comp(i) the component's number by ascending root
 *   (the kernels of bhs_csr_components_device, under this call's own kernel record).
 * Start of a component: s0, its vertex of smallest key.  With BHS_RCM_PERIPHERAL the George-Liu refinement runs as SPARSPAK's
 *   FNROOT has it, for all components in lockstep.  A SWEEP is one breadth-first search from every component's current
 *   start at once: it gives every vertex its level, and every component e, its greatest level, and x, the vertex of
 *   smallest key on that level.  After sweep 0 every component's start moves to x.  After every later sweep a component
 *   whose new e does not exceed its old e is DONE: it keeps the start the sweep ran from and this sweep's levels; any
 *   other takes the new e, moves its start to x and sweeps again.  A done component's start no longer moves, so later
 *   sweeps give it the same levels.  Without the flag there is one sweep.  *sweeps_out is the number of sweeps (with the flag
 *   at least 2); BHS_ERR_INTERNAL after n + 1 sweeps.
 * Cuthill-McKee, level by level.  pos of a start is its component's number.  A vertex v on level l >= 1 has the parent
 *   p(v), its neighbour on level l - 1 of smallest pos.  Level l is ordered by (pos(p(v)), deg(v), v) and follows level
 *   l - 1: the FOREST ORDER.  The CM order is the forest order stably regrouped by comp: components are contiguous and ascend
 *   by root, and inside a component it is exactly the order of the serial queue algorithm in which a dequeued vertex
 *   appends its unnumbered neighbours by ascending (deg, index).
 * Outputs.  d_perm[k] is the OLD index of new row k: the CM order reversed as a whole, or the CM order itself under
 *   BHS_RCM_NO_REVERSE; it is what bhs_csr_extract_device takes as rows and cols.  d_level (may be NULL): n ints, the final
 *   sweep's levels.  d_start (may be NULL): CAPACITY n ints, d_start[c] the start of component c, ncomp written.
 *   *depth_out is the greatest number of levels of a component.  d_perm, d_level, d_start, *ncomp_out, *depth_out and
 *   *sweeps_out are a function of the pattern alone: the same bits from run to run, from handle to handle, and in the
 *   double and the float library.  Only *passes_out is exempt: the passes launched, of the components' relaxation (which
 *   DEPENDS ON TIMING) and of the sweeps, always A MULTIPLE OF THE BATCH of 8 passes a control round trip.
 * How.  rcm_check: the degrees and the refusals.  rcm_components: the components.  rcm_level: a sweep's passes -- a pull:
 *   an unvisited vertex with a neighbour on level cur takes cur + 1; a pass stores cur + 1 alone, so a racing read sees
 *   "unvisited" or cur + 1, never cur: plain stores, unique levels; a sweep ends after a batch whose last pass reached
 *   nothing.  rcm_far: per root a 64-bit atomic maximum of the level, a 64-bit atomic minimum of the key on that level,
 *   the decision; one round trip a sweep.  rcm_order: the vertices by (level, index) and levelPtr, copied to the host once
 *   (the colouring's order step; its table of depth x ceil(n / 64) counts is limited to 2^26: very deep AND very large
 *   graphs return BHS_ERR_ALLOC).  rcm_number: a launch sequence per level over that level's slice only -- the parents and
 *   their child counts, the library's one-pass scan of them, the places -- so the total work is O(nnz) with no round trip
 *   inside; the rank among siblings walks the parent's row, deg(parent) a child: quadratic in a hub's degree
 *   (profiles/rcm_case.md).  rcm_group: the regrouping by the scan of the components' sizes, and the reversal.
 *   Nothing spins on the device, nothing waits for another workgroup.  A row is spread over 1, 4, 16 or 64 lanes by the
 *   pattern's mean row length.
 * Synchronous on the handle's stream, needs no bound data, leaves the handle as it was (a workspace of its own).  ms_out
 *   (may be NULL): device time of the call, the round trips included.                                                  */
#define BHS_RCM_PERIPHERAL 1   /* the George-Liu pseudo-peripheral start of every component */
#define BHS_RCM_NO_REVERSE 2   /* the Cuthill-McKee order itself, not its reverse */
BHS_API int bhs_csr_rcm_device(bhs_handle *h, int n, int nnzS,
        const int *d_rowPtrS, const int *d_colIndS /* n x n pattern, rows ascending, symmetric; values are not taken */,
        int flags /* BHS_RCM_PERIPHERAL | BHS_RCM_NO_REVERSE */,
        int *d_perm  /* out: n ints: the old index of new row k */,
        int *d_level /* out, may be NULL: n ints: the final sweep's levels */,
        int *d_start /* out, may be NULL: CAPACITY n, ncomp written: the start of component c */,
        int *ncomp_out /* may be NULL */, int *depth_out /* may be NULL */, int *sweeps_out /* may be NULL */,
        int *passes_out /* may be NULL; a multiple of the batch, depends on timing */,
        double *ms_out /* may be NULL */);

/* ---- k-core decomposition ---------------------------------------------------
 * The core number of every vertex of a symmetric pattern by parallel peeling: the greatest k for which the vertex lies in a
 * subgraph of minimum degree k (Batagelj-Zaversnik's core numbers, networkx's core_number) -- cohesive subgraphs, the
 * degeneracy and a degeneracy ordering (no reference counterpart; bhs_kcore.hip.h).
 * S is an n x n pattern on the device, 0-based int32 CSR, rows STRICTLY ASCENDING, STRUCTURALLY SYMMETRIC.  Values are NOT
 * TAKEN, so the double and the float library run the same code and give the same bits.  A diagonal entry is allowed and
 * ignored.
 * Definition.  deg(v) = the entries of row v off the diagonal, and k_0 = 0.  In round r = 1, 2, ... let k_r = max(k_{r-1},
 *   the smallest degree among the vertices still present).  Every present vertex with deg <= k_r leaves SIMULTANEOUSLY with
 *   core = k_r and round = r; the degrees of the remaining vertices drop by the number of their neighbours that left.  The
 *   rounds end when no vertex is present.  *kmax_out is the greatest core number (the degeneracy), *rounds_out the last r.
 *   core is the usual core number; round is the synchronous peeling depth.  Sorting the vertices by (round, index) gives a
 *   degeneracy ordering: every vertex has at most core(v) <= kmax neighbours behind it.
 * Refusals by the device, each BHS_ERR_INVALID_ARG, found by the first kernel (bhs_csr_rcm_device's check, under this call's
 *   own record kcore_check): a falling row pointer, or nnzS != rowPtr[n]; a column outside [0, n); a row that is not
 *   strictly ascending (a repeated entry included); an entry (i, j) without (j, i), found by a binary search in row j.  Once
 *   the check has raised the error word every later launch leaves at once: a refused pattern is refused BEFORE d_core or
 *   d_round is written, nothing stays queued, and nothing beyond the outputs' stated sizes is ever written.
 * Refusals by the host, each BHS_ERR_INVALID_ARG: a NULL handle, a call between bhs_spgemm_symbolic and bhs_spgemm_finish,
 *   negative n or nnzS, flags other than 0, a NULL d_rowPtrS or d_core with n > 0, NULL d_colIndS with nnzS > 0, an output's
 *   footprint overlapping S or the other output.
 * n == 0 succeeds with *kmax_out = *rounds_out = 0 and launches nothing.
 * Outputs.  d_core and d_round (may be NULL), n ints each, *kmax_out and *rounds_out are a function of the pattern alone: the
 *   same bits from run to run, from handle to handle, and in the double and the float library.
 * How.  A work-efficient frontier peel, O(nnz) in all: every vertex enters one queue of n ints exactly once, and a round's
 *   vertices are a slice of it.  The order INSIDE the queue DEPENDS ON TIMING and is therefore NOT AN OUTPUT; which vertices a
 *   round holds does not.  A pass is four launches with no host decision between them.  kcore_peel: for every vertex v of
 *   the slice and every neighbour u, old = atomicSub(deg + u, 1), unconditionally; the one thread that sees old == k + 1
 *   appends u and stores core[u] = k, round[u] = r + 1 with plain stores -- the only writer these words ever have.  A
 *   present vertex has deg > k when the pass starts, so it crosses k + 1 exactly once if it ends at or below k, however
 *   many neighbours it loses; a vertex that has left only sinks.  kcore_advance: where the peel appended
 *   nothing and vertices remain, the smallest present degree by an integer atomicMin and the vertices of that degree
 *   appended and stamped -- the level jump, so empty levels cost nothing, and the call's first frontier -- then ONE thread
 *   makes the appended range the next slice.  8 passes a control round trip; the call ends after a batch whose last pass
 *   left no vertex present; the passes behind the last round leave at once.  BHS_ERR_INTERNAL when more than n + 1 passes
 *   would be needed.  Nothing spins, nothing waits for another workgroup; the atomics are integer atomics on the workspace
 *   alone, no output is written by an atomic.  A row is spread over 1, 4, 16 or 64 lanes by the pattern's mean row length,
 *   and in the peel a row of more than 32 entries a lane over a whole wave; the check gives a hub row ONE such group,
 *   and a deep graph pays four launches a round (profiles/kcore_case.md).
 * Synchronous on the handle's stream, needs no bound data, leaves the handle as it was (a workspace of its own).  ms_out
 *   (may be NULL): device time of the call, the round trips included.                                                  */
BHS_API int bhs_csr_kcore_device(bhs_handle *h, int n, int nnzS,
        const int *d_rowPtrS, const int *d_colIndS /* n x n pattern, rows ascending, symmetric; values are not taken */,
        int flags /* must be 0 */,
        int *d_core  /* out: n ints: the core number of every vertex */,
        int *d_round /* out, may be NULL: n ints: the round in which every vertex left, from 1 */,
        int *kmax_out /* may be NULL: the degeneracy */, int *rounds_out /* may be NULL */,
        double *ms_out /* may be NULL */);

/* ---- shortest paths ---------------------------------------------------------
 * Distances, and optionally predecessors, from a set of sources over weights that are not negative, by delta-stepping on a
 * queue in one device-resident call -- road networks, meshes, any graph of high diameter, where a loop of semiring calls pays
 * a host round trip a sweep; with unit weights the queue breadth-first search (no reference counterpart; bhs_sssp.hip.h).
 * Edges.  G is the n x n OUT-EDGE matrix on the device, 0-based int32 CSR: an entry G(i, j) is an edge i -> j of weight valG,
 *   the orientation of bhs_csr_push_semiring_device.  Rows need not be sorted.  Repeated entries are parallel edges.  A
 *   diagonal entry is a loop that never improves anything.  An entry of weight +Inf never relaxes.  -0 counts as 0.
 *   d_valG == NULL: every edge weighs 1.
 * Distances.  d_dist[v] is the least fixed point of d[s] = 0 for every listed source and d[v] = min over the edges (u, v) of
 *   fl(d[u] + w(u, v)), fl being ONE rounding to value_type an edge, contraction off; +Inf where v is not reached.  With
 *   several sources that is the distance to the nearest one; repeated sources are allowed.  Floating add is MONOTONE
 *   (a <= b gives fl(a + w) <= fl(b + w)) and min is EXACT, so every distance only ever takes values that are the
 *   left-to-right sum of the weights along some path, and the least fixed point does not depend on the order of the
 *   relaxations: the result is a function of the input alone -- the same bits from run to run, from handle to handle and for
 *   every delta, and in the double library the bits a textbook Dijkstra in double produces.
 * delta is the bucket width: > 0 or +Inf.  It changes the work, never the result.  +Inf is one bucket: frontier Bellman-Ford.
 *   With d_valG == NULL and delta = 1 the passes are the breadth-first levels.
 * d_parent (may be NULL).  For a reached vertex v that is no source: the SMALLEST u that has an edge (u, v) with
 *   fl(d[u] + w) == d[v] AND d[u] < d[v].  -1 for a source and for a vertex that is not reached.  -2 for a reached vertex with
 *   no such edge: one reached only over edges that gain nothing -- zero weights, or weights absorbed by rounding -- which
 *   could otherwise close a cycle.  Every parent has a STRICTLY SMALLER distance, so the parents that are not negative form a
 *   forest rooted at the sources.  One pass behind the fixed point: a push over all edges with an integer atomicMin on a
 *   workspace word, then a copy.
 * Counts.  *reached_out: the vertices with a finite distance.  *passes_out: the passes launched, the passes that had a slice
 *   (bhs_get_info "sssp_work_passes") rounded up to a multiple of 8.  bhs_get_info "sssp_buckets": the buckets that were not
 *   empty; "sssp_loose": the vertices given -2 (0 without d_parent); all three need no bound data.  reached, sssp_buckets and
 *   sssp_loose are functions of the input and delta; so are the passes, because a pass is SYNCHRONOUS: it relaxes from the
 *   distances the pass before left, which it keeps beside its slice, so which words it lowers and which vertices it appends
 *   do not depend on timing.
 * Refusals by the device, each BHS_ERR_INVALID_ARG, found by the first kernel (record sssp_check): a weight that is NaN or
 *   negative (sign bit set and not -0); a column outside [0, n); a row pointer that falls, does not start at 0 or does not end
 *   at nnzG; a source outside [0, n).  Once the check has raised the error word every later launch leaves at once: a refused
 *   input is refused BEFORE d_dist or d_parent is written, nothing stays queued, and nothing beyond the outputs' stated sizes
 *   is ever written.
 * Refusals by the host, each BHS_ERR_INVALID_ARG: a NULL handle, a call between bhs_spgemm_symbolic and bhs_spgemm_finish,
 *   negative n, nnzG or nsrc, nsrc < 1 or a NULL d_sources, d_rowPtrG or d_dist with n > 0, NULL d_colIndG with nnzG > 0,
 *   flags other than 0, a delta that is not > 0 (NaN included), an output's footprint overlapping an input or the other
 *   output.
 * n == 0 succeeds with *reached_out = *passes_out = 0 and launches nothing.
 * How.  dist is kept as the unsigned integer words of value_type's width: values that are not negative order as their words
 *   do, +Inf's word is the start value and an integer atomicMin is the relaxation.  done[v] is the distance at which v last
 *   relaxed its out-edges; v is pending while dist[v] < done[v].  A pass is four launches with no host decision between them.
 *   sssp_relax: every vertex of the slice relaxes its out-edges from its snapshot; the thread that lowers a word and leaves it
 *   below the bucket's bound claims the vertex by an atomicExch on its stamp and appends it to the next slice -- at most one
 *   append a vertex a pass; a vertex lowered to the bound or beyond stays pending.  sssp_advance: the appended vertices'
 *   snapshots; or, where nothing was appended, the smallest pending distance by an integer atomicMin, the bound
 *   (floor(min / delta) + 1) delta in double, and every pending vertex below it or EQUAL to the minimum appended -- the
 *   bucket jump, so empty buckets cost nothing and the minimum's holder is taken whatever the bound's rounding; then ONE
 *   thread swaps the slices.  8 passes a control round trip; the call ends after a batch whose last pass left no slice; the
 *   passes behind the last one leave at once.  BHS_ERR_INTERNAL when more than 2 n + 2 passes would be needed.  Nothing
 *   spins, nothing waits for another workgroup; the atomics are integer atomics on the workspace alone, and the one kernel
 *   that writes an output (sssp_finish) uses plain stores.  A row is spread over 1, 4, 16 or 64 lanes by the mean row length,
 *   and in the relax and the parents' pass a row of more than 32 entries a lane over a whole wave; the check walks the
 *   entries, not the rows (profiles/sssp_case.md).
 * Synchronous on the handle's stream, needs no bound data, leaves the handle as it was (a workspace of its own: 4 n
 *   value_type words and 3 or 4 n ints).  ms_out (may be NULL): device time of the call, the round trips included.      */
BHS_API int bhs_csr_sssp_device(bhs_handle *h, int n, int nnzG,
        const int *d_rowPtrG, const int *d_colIndG /* n x n out-edges: G(i, j) is an edge i -> j */,
        const bhs_value_t *d_valG /* the weights, not negative; NULL: every edge weighs 1 */,
        int nsrc, const int *d_sources /* nsrc vertices, repeats allowed */,
        double delta /* the bucket width: > 0 or +Inf */, int flags /* must be 0 */,
        bhs_value_t *d_dist /* out: n values; +Inf where not reached */,
        int *d_parent /* out, may be NULL: n ints; -1 a source or not reached, -2 no tight edge from a smaller distance */,
        int *reached_out /* may be NULL */, int *passes_out /* may be NULL: a multiple of 8 */,
        double *ms_out /* may be NULL */);

/* ---- betweenness centrality -------------------------------------------------
 * Which vertices the shortest paths run through: bc[u] = the sum over the listed sources s of Brandes' dependency of s on u,
 * in one device-resident call a list of sources -- all vertices for the exact centrality, a sample of pivots for an estimate
 * (no reference counterpart; bhs_bc.hip.h).  Values are not taken and every number is a double in both libraries: the double
 * and the float build run the same code and give the same bits.
 * Edges.  G is the n x n OUT-EDGE matrix on the device, 0-based int32 CSR: an entry G(i, j) is an edge i -> j.  T holds the
 *   IN-EDGES: T = G^T, row v of T lists the u with an edge u -> v; for an undirected graph T is G, the SAME arrays.  Rows need
 *   not be sorted.  Repeated entries are parallel edges: they count in sigma, each a path of its own (networkx agrees on the
 *   graph with a vertex put on every edge; on a MultiDiGraph it counts neighbours, not edges).  Loops never qualify.  T is taken as given: the call does not verify T = G^T, which would cost a sort; the result is a function of
 *   (G, T, sources) either way, and nothing is read or written out of bounds whatever T holds.
 * For each source s, in list order (a repeated source counts again):
 *   Levels.  level[s] = 0, level[v] is the breadth-first depth over G, -1 where v is not reached.
 *   Path counts.  sigma[s] = 1.  For a reached v != s, sigma[v] is the sum of sigma[u] over the entries u of ROW v OF T with
 *     level[u] == level[v] - 1.  A vertex that is not reached has sigma = 0.
 *   Dependencies.  On the deepest level delta[u] = 0.  Otherwise delta[u] = sigma[u] * S, S being the sum of
 *     (1 + delta[v]) / sigma[v] over the entries v of ROW u OF G with level[v] == level[u] + 1: a true division, contraction
 *     off.
 *   Accumulation.  bc[u] = fl(bc[u] + delta[u]) for every reached u != s with 0 < level[u] < the deepest level, one source
 *     after the other in list order.
 * Summation rule -- what makes the bits a function of the input when sigma passes 2^53 and the sums stop being exact.  Let L
 *   in {1, 4, 16, 64} be the lanes of the matrix whose row is walked: 1 up to a mean row length (nnz / n) of 4, 4 up to 16, 16
 *   up to 64, else 64.  A row of more than 32 L entries takes L_row = 64 (the wave rule of the k-core decomposition and the
 *   shortest paths), any other L_row = L.  The entry at position p in the row belongs to lane p mod L_row; each lane adds its
 *   qualifying terms in ascending p, starting from +0; the lane sums are combined by the xor butterfly
 *   t[l] = t[l] + t[l ^ off] for off = L_row / 2, ..., 1.  A non-qualifying entry contributes nothing.  IEEE semantics hold
 *   throughout: a sigma that overflows to +Inf stays +Inf, and a NaN in bc that follows from Inf * 0 or Inf / Inf is the
 *   defined result.  Every NaN is STORED as the one word 0x7FF8000000000000, in delta and in d_bc (one that the caller passes
 *   in under BHS_BC_ACCUMULATE and a dependency is added to included), so that its bits do not depend on what a processor
 *   gives an invalid operation.
 * flags.  BHS_BC_ACCUMULATE: d_bc is added to instead of zero-filled, so one call over s_1 ... s_k gives the same bits as k
 *   chained single-source calls.
 * d_level, d_sigma (may be NULL): level and sigma of the LAST source of the list.
 * Counts.  *reached_out: the sum over the sources of their reached vertices (at most 2^31 - 1 is reported).  *passes_out:
 *   the forward passes launched, a multiple of 8 per source.  bhs_get_info "bc_levels": the sum over the sources of (deepest
 *   level + 1); "bc_overflow": the sources for which some sigma is not finite; "bc_work_passes": the passes that had a slice;
 *   all three need no bound data.  All of these are functions of the input.
 * Refusals by the device, each BHS_ERR_INVALID_ARG, found by the first kernel (record bc_check), which walks entries, not
 *   rows: a row pointer of G or T that falls, does not start at 0 or does not end at its nnz; a column of either matrix
 *   outside [0, n); a source outside [0, n).  Once the check has raised the error word every later launch leaves at once: a
 *   refused call writes none of d_bc, d_level, d_sigma, and nothing stays queued.
 * Refusals by the host, each BHS_ERR_INVALID_ARG: a NULL handle, a call between bhs_spgemm_symbolic and bhs_spgemm_finish,
 *   negative n, nnzG, nnzT or nsrc, nsrc < 1 or a NULL d_sources, d_rowPtrG, d_rowPtrT or d_bc with n > 0, a NULL column
 *   array with its nnz > 0, flags other than BHS_BC_ACCUMULATE or 0, an output's footprint overlapping an input or another
 *   output.  Inputs may alias each other: the undirected case.
 * n == 0 succeeds with *reached_out = *passes_out = 0 and launches nothing.
 * How.  Per source every reached vertex enters ONE queue once; a level is a slice of it, kept in levelPtr.  bc_seed (1 launch)
 *   resets level, sigma and delta, queues the source and, on the first source of a call without BHS_BC_ACCUMULATE, zero-fills
 *   d_bc.  A forward pass is three launches with no host decision between them.  bc_expand: every vertex of the slice walks
 *   its row of G; the thread whose integer atomicCAS turns level[v] from -1 into l + 1 appends v -- the order inside the queue
 *   depends on timing and is no output.  bc_count: every vertex of the new slice pulls its sigma over its row of T by the
 *   summation rule, no atomic and ONE writer; then ONE thread stores levelPtr and makes the appended range the next slice.
 *   8 passes a control round trip; the forward half ends after a batch whose last pass left no slice; the passes behind the
 *   last level leave at once.  BHS_ERR_INTERNAL when more than n + 1 passes would be needed.  The host then knows the deepest
 *   level, and bc_back is a fixed list of max(deepest - 1, 0) launches, l = deepest - 1 down to 1, queued back to back with
 *   no round trip: each takes slice l from levelPtr on the device, computes delta by the rule and adds it to d_bc[u] with
 *   plain stores -- only u's own group of lanes ever writes bc[u].  bc_finish, once, copies d_level and d_sigma.  Nothing
 *   spins, nothing waits for another workgroup; the only atomics are integer atomics on the workspace.  Grids are capped at
 *   16 workgroups a CU with block loops.  Measured on one MI355X from one source (profiles/bc_case.md): uniform 2^20 x 8
 *   1.80 ms in 10 levels, poisson27pt 128^3 7.59 ms in 128, the R-MAT triangle 3.58 ms in 7, road-like 2^20 58.8 ms in 2063
 *   -- 1.1 to 1.36 times as many queue breadth-first calls of bhs_csr_sssp_device, and three to four orders of magnitude
 *   below networkx on a host.  It LOSES on depth: a level is four launches over grids sized for n, 28 us a level on the
 *   road-like graph; and 64 sources cost 64 times one (113 ms to 2.77 s), because several sources are not batched into one
 *   pass.
 * Synchronous on the handle's stream, needs no bound data, leaves the handle as it was (a workspace of its own: 2 n doubles
 *   and 3 n + 2 ints).  ms_out (may be NULL): device time of the call, the round trips included.                       */
#define BHS_BC_ACCUMULATE 1
BHS_API int bhs_csr_betweenness_device(bhs_handle *h, int n,
        int nnzG, const int *d_rowPtrG, const int *d_colIndG /* out-edges: G(i, j) is an edge i -> j */,
        int nnzT, const int *d_rowPtrT, const int *d_colIndT /* in-edges: T = G^T; the SAME arrays as G for an undirected graph */,
        int nsrc, const int *d_sources /* processed in this order; repeats count again */,
        int flags /* BHS_BC_ACCUMULATE or 0 */,
        double *d_bc /* out (in/out under ACCUMULATE): n doubles */,
        int *d_level, double *d_sigma /* out, may be NULL: n each, of the LAST source */,
        int *reached_out /* may be NULL */, int *passes_out /* may be NULL: a multiple of 8 per source */,
        double *ms_out /* may be NULL */);

/* ---- spanning forest --------------------------------------------------------
 * The minimum (or maximum) spanning forest of the graph that an n x n matrix A stores, by Boruvka rounds on the device: for
 * network design, as the spanning tree under a support-graph or tree preconditioner (the MAXIMUM forest of |a_ij| is the
 * strongest tree of a matrix), for single-linkage clustering (cut the heaviest forest edges, then call the components
 * below), and as a spanning tree of every component in O(log n) rounds where one traversal costs the diameter (no reference
 * counterpart; bhs_forest.hip.h).  A is n x n, 0-based int32 CSR; rows need not be sorted and A need not be symmetric.
 * Edges.  Every stored entry (i, j) with j != i whose weight is not NaN is an undirected edge {i, j}, a member of a
 *   multigraph.  Its weight w is a_ij, or |a_ij| under BHS_FOREST_ABS, or 1 where d_valA == NULL.  +-Inf, negative weights
 *   and explicit zeros are legal weights; NaN entries and the diagonal are no edges.  It makes no difference from which
 *   end, or how often, an edge is stored.
 * Key.  The tuple (k(w), lo, hi) compared lexicographically, lo = min(i, j), hi = max(i, j).  k is the reductions'
 *   order-preserving key (rd_key(x, false)): the order of the numbers with -0 below +0; in the float library the value is
 *   widened exactly, so both builds compare alike.  Under BHS_FOREST_MAXIMUM the whole order is reversed, index
 *   tie-breaks included: the complement of both words.  The order is strict over distinct (w, lo, hi); entries with equal
 *   tuples are the same edge.
 * Result.  THE spanning forest that Kruskal's algorithm builds taking edges in ascending key order: unique for ANY input,
 *   symmetric or not, repeated columns, ties everywhere.  Of a repeated {i, j} the lightest weight counts, under MAXIMUM
 *   the heaviest.  It has n - (number of weak components) edges.  The same bits come back from run to run and from handle
 *   to handle, and in the double and the float library where the weights are exactly representable in float or d_valA is
 *   NULL.
 * Rounds, synchronous: every launch either reads an array or writes the caller's own word of it, or lowers a word by an
 *   integer atomicMin whose result no order can change.  PICK: for every entry crossing two trees (label[i] != label[j])
 *   the 64-bit weight key lowers bestW[label[i]] and bestW[label[j]]; in a second launch the entries whose key equals
 *   their tree's bestW lower bestE[label] with lo << 32 | hi.  A row's own side is reduced across its L lanes first; an
 *   atomic is issued only where the value read (an agent-scope relaxed load) is greater than what it would store, so a
 *   stale read only costs an unneeded atomic.  HOOK: a root c (label[c] == c) with a pick reads the label d of the pick's
 *   far endpoint; where d picked the same tuple (a mutual pair) the smaller of c and d stays a root; every other c writes
 *   parent[c] = d, in an array of its own, not in label, and stores its pick as the edge of SLOT c (lo, hi, rd_unkey of the
 *   key).  A vertex is hooked at most once in the whole call, so a slot is written at most once; with a strict order the
 *   hook graph has no cycle but the mutual pairs.  FLATTEN: pointer jumping on parent over the round's roots --
 *   parent[c] = parent[parent[c]] in place at least doubles the distance covered in every launch, whatever the races, so
 *   ceil(log2 R) launches reach the fixed point from R roots, R known to the host from the previous round -- then
 *   label[i] = parent[label[i]] for every vertex in a launch of its own, which raises the error word where
 *   parent[parent[l]] != parent[l]: BHS_ERR_INTERNAL.  The host reads one control block a round, the error word and the
 *   trees hooked, and stops after a round that hooked nothing (or that left a single tree).  Trees with a crossing edge at
 *   least halve per round, so at most floor(log2 n) rounds hook; *rounds_out is the number of rounds that hooked at least
 *   one tree, a function of the input; BHS_ERR_INTERNAL where a 33rd round would be needed.  Nothing spins on the device,
 *   nothing waits for another workgroup, and there are no floating atomics.
 * Outputs.  d_label: n ints, label[label[i]] == label[i]; labels are equal exactly on the vertices of one tree, which is
 *   one weak component of the edges above; which vertex of the tree is the label is a function of the input, it need not
 *   be the smallest (bhs_csr_components_device gives that).  The edge list: d_edgeLo, d_edgeHi and d_edgeVal (may be
 *   NULL) have CAPACITY n, *nedges_out entries are written: the written slots in ascending slot order -- the slots are
 *   flagged per 64 vertices and the counts go through the library's one-pass scan, as the components number their roots --
 *   with lo < hi and d_edgeVal the weight as compared: a_ij, |a_ij| or 1.  The host checks the scan's total against the
 *   hooks it counted, else BHS_ERR_INTERNAL.
 * Validation, on the device, each check ahead of the dependent read: rowPtrA[i] > rowPtrA[i+1] or either outside
 *   [0, nnzA]; a column outside [0, n).  On the host, with the outputs untouched: a NULL handle, negative n or nnzA, a flag
 *   bit other than the two, a NULL d_rowPtrA, d_label, d_edgeLo or d_edgeHi with n > 0, NULL d_colIndA with nnzA > 0, an
 *   output's footprint overlapping A or another output, and a call between bhs_spgemm_symbolic and bhs_spgemm_finish.
 *   Each returns BHS_ERR_INVALID_ARG.  After a refusal by the device the outputs are unspecified; nothing beyond their
 *   stated sizes is ever written.
 * n == 0 succeeds with zero edges, zero rounds and *ms_out = 0 and launches nothing.
 * Synchronous on the handle's stream, needs no bound data, leaves the handle as it was (a workspace of its own).  ms_out
 *   (may be NULL): device time of the call, the rounds' round trips included.  bhs_get_kernel_stats then reports
 *   forest_pick (the start, and a round's clear, weight and edge launches, a row spread over 1, 4, 16 or 64 lanes by the
 *   mean row length), forest_hook (the hook, the jumps, the relabel) and forest_list (the slot flags, the scan, the
 *   write-out).  Measured: profiles/forest_case.md.                                                                  */
enum { BHS_FOREST_MAXIMUM = 1, BHS_FOREST_ABS = 2 };
BHS_API int bhs_csr_spanning_forest_device(bhs_handle *h, int n, int nnzA,
        const int *d_rowPtrA, const int *d_colIndA,
        const bhs_value_t *d_valA /* may be NULL: every weight 1 */,
        int flags /* BHS_FOREST_MAXIMUM | BHS_FOREST_ABS */,
        int *d_label          /* out: n ints */,
        int *d_edgeLo, int *d_edgeHi /* out: CAPACITY n ints each, nedges written */,
        bhs_value_t *d_edgeVal /* out, may be NULL: CAPACITY n */,
        int *nedges_out, int *rounds_out, double *ms_out /* each may be NULL */);

/* ---- connected components ---------------------------------------------------
 * Which vertices of an n x n pattern S belong together: the question asked of a graph before a traversal, an aggregation or
 * a solver setup runs (no reference counterpart; bhs_components.hip.h).  One traversal finds one component and costs the
 * graph's diameter in steps; this call finds all of them in a number of passes that grows like the diameter's logarithm.
 * S is 0-based int32 CSR; values are NOT TAKEN, so the double and the float library run the same code and give the same bits.
 * Definition.  Vertices i and j are joined where S stores (i, j) or (j, i): WEAK connectivity, S need not be symmetric.
 *   Diagonal entries, repeated columns and the order inside a row make no difference; an isolated vertex is its own
 *   component.  root[i] is the smallest vertex index in i's component.  comp[i] is the rank of root[i] among the roots, of
 *   which there are ncomp: components are numbered by ascending smallest vertex.  compSize[c] is the number of vertices
 *   with comp == c.  Everything except *passes_out is a function of the pattern: the same bits from run to run, from
 *   handle to handle, and in the double and the float library.
 * Passes.  Monotone relaxation in place on d_root, which starts as parent[i] = i.  At every instant parent[v] <= v,
 *   parent[v] lies in v's component, and a word only ever falls: every write after the start is an atomic minimum.  A pass
 *   lowers both ends of every stored entry (i, j) to the smaller of the two parents, lowers the word of i's grandparent
 *   to the row's minimum (hooking: a whole tree moves under a smaller root) and lowers parent[i] to parent[parent[i]]
 *   twice (pointer jumping).  An atomic is issued only where the value read is greater than what it would store.  A pass
 *   that lowered nothing wrote nothing and therefore read one stable array in which both ends of every entry are equal:
 *   it is constant on components, and at the component's smallest vertex that constant is the vertex itself -- the
 *   definition, however a pass's reads race with other lanes' writes.  The host launches 8 passes per control round trip
 *   and stops after a batch whose last pass lowered nothing; BHS_ERR_INTERNAL where more than n + 1 passes would be
 *   needed.  *passes_out, the passes launched, DEPENDS ON TIMING; nothing else does.  Nothing spins on the device,
 *   nothing waits for another workgroup.  A relabelled path of 32 768 vertices takes 16 passes where plain minimum-label
 *   propagation takes its diameter (profiles/components_case.md).
 * Outputs.  d_root: n ints.  d_comp (may be NULL): n ints in [0, ncomp).  d_compSize (may be NULL, needs d_comp): CAPACITY
 *   n ints, of which ncomp are written.  *ncomp_out is the number of vertices with root[i] == i, counted by the last pass:
 *   it is written with or without d_comp.  The numbering flags the roots, scans the flags per 64 vertices with the
 *   library's one-pass scan as the aggregation numbers its roots, and sets comp[i] to the rank of root[i]; the sizes are
 *   integer atomic adds, which do not depend on order.  The vertices sorted by component are NOT an output: the stable
 *   transpose of the n x ncomp membership pattern (rowPtr = 0 .. n, colInd = comp) is that list.
 * Validation, on the device, each check ahead of the dependent read: rowPtrS[i] > rowPtrS[i+1] or either outside
 *   [0, nnzS]; a column outside [0, n).  On the host: a NULL handle, negative n or nnzS, flags != 0, a NULL d_rowPtrS or
 *   d_root with n > 0, NULL d_colIndS with nnzS > 0, d_compSize without d_comp, an output's footprint overlapping S or
 *   another output, and a call between bhs_spgemm_symbolic and bhs_spgemm_finish.  Each returns BHS_ERR_INVALID_ARG.  After
 *   a refusal by the device the outputs are unspecified; nothing beyond their stated sizes is ever written.
 * n == 0 succeeds with *ncomp_out = 0 and *passes_out = 0 and launches nothing.
 * Synchronous on the handle's stream, needs no bound data, leaves the handle as it was (a workspace of its own).  ms_out
 *   (may be NULL): device time of the call, the batches' round trips included.  bhs_get_kernel_stats then reports
 *   components_pass (the relaxation, a row spread over 1, 4, 16 or 64 lanes by the pattern's mean row length) and, where
 *   d_comp is given, components_number (the root flags, the scan, the numbering and the sizes).                      */
BHS_API int bhs_csr_components_device(bhs_handle *h, int n, int nnzS,
        const int *d_rowPtrS, const int *d_colIndS /* n x n pattern; values are not taken */,
        int flags /* must be 0 */,
        int *d_root     /* out: n ints: the smallest vertex of i's component */,
        int *d_comp     /* out, may be NULL: n ints in [0, ncomp), components numbered by ascending root */,
        int *d_compSize /* out, may be NULL, needs d_comp: CAPACITY n, ncomp written */,
        int *ncomp_out /* may be NULL */, int *passes_out /* may be NULL; depends on timing */,
        double *ms_out /* may be NULL */);

/* ---- matching ---------------------------------------------------------------
 * Heavy-edge matching: every vertex of an n x n matrix A is paired with the neighbour it is most strongly coupled to, greedily
 * in descending edge key -- the coarsening step of pairwise-aggregation multigrid (Notay's AGMG) and of multilevel graph
 * partitioning, and a 1/2-approximation of the maximum-weight matching (no reference counterpart; bhs_match.hip.h).  Beside
 * the MIS(2) aggregation below, which works on a pattern and coarsens at a fixed aggressive rate, this one is driven by
 * the VALUES and halves the vertices at most: repeated on the Galerkin-coarsened matrix it gives aggregates of up to
 * 2^passes vertices that follow the strong direction (amg.pairwise_aggregate_device, amg.pa_setup_device).
 * A is 0-based int32 CSR; rows need not be sorted.
 * Edges.  An entry (i, j) of row i is an edge seen from i where j != i, its weight w = |a_ij| is greater than 0 and w is
 *   not NaN.  d_valA == NULL: every weight is 1.  +Inf is a legal weight, an explicit zero (or minus zero) is no connection.
 *   Of a repeated (i, j) the greatest weight counts.
 * Edge key.  The tuple (w, h(lo, hi), lo, hi), compared lexicographically, with lo = min(i, j), hi = max(i, j),
 *   h(lo, hi) = mix(mix(lo ^ seed) ^ hi) and mix(x): x += 0x9e3779b9; x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13;
 *   x *= 0xc2b2ae35; x ^= x >> 16 (mod 2^32; the aggregation's finaliser).  w is compared in the library's value type.
 *   Seen from one vertex, lexicographic (lo, hi) is "the greater other endpoint wins".  The hash stands in front of the
 *   indices because with index tie-breaks alone a path of equal weights needs n / 2 rounds.
 * Rounds, synchronous over d_mate (-1 undecided, i itself: finally unmatched, j: matched with j).  PROPOSE: every undecided
 *   i sets cand[i] to the undecided neighbour of greatest key over its edges, -1 without one; the lanes of a decided vertex
 *   skip its row.  ACCEPT: an undecided i with cand[i] == -1 becomes i (final: eligibility only shrinks); one with
 *   c = cand[i] and cand[c] == i becomes c.  A launch either reads mate and writes cand or reads cand and writes the vertex's
 *   own word of mate: no atomics touch a result, nothing depends on timing.  The host reads one word a round (the pairs it
 *   made, the vertices it left) and stops after a round that matched nothing -- the vertices it left become unmatched --
 *   or left nobody.  *rounds_out is the number of rounds that matched at least one pair, a function of the input;
 *   BHS_ERR_INTERNAL where more than n / 2 + 1 rounds would be needed.  Nothing spins on the device, nothing waits for
 *   another workgroup.
 * What is promised.  For ANY input the result is what these synchronous rounds give: a valid matching, mate[mate[i]] == i,
 *   and a function of the input.  Where pattern and weights are SYMMETRIC (the edge {i, j} has one weight from both ends)
 *   the edge of greatest key among the undecided is mutual in every round, and the result is THE greedy matching in
 *   descending key order: unique, maximal, independent of scheduling, the same bits from run to run and from handle to
 *   handle -- and in the double and the float library where the values are exactly representable in float or d_valA is
 *   NULL.  For other inputs the matching need not be maximal.  A path of 200 vertices with strictly increasing weights
 *   takes 100 rounds, the worst case; grids, bands and random patterns of one to two million vertices take 5 to 10
 *   (profiles/match_case.md).
 * Numbering, where d_agg is given.  leader[i] = min(i, mate[i]); the aggregates -- pairs and singletons -- are numbered by
 *   ascending leader: the leaders are flagged, the flags scanned per 64 vertices with the library's one-pass scan as the
 *   components number their roots, agg[i] is the rank of i's leader.  There are n - npairs of them; the host checks the
 *   scan's total against that, else BHS_ERR_INTERNAL.
 * Validation, on the device, each check ahead of the dependent read: rowPtrA[i] > rowPtrA[i+1] or either outside
 *   [0, nnzA]; a column outside [0, n) -- mate[j] is read only after j passed.  On the host: a NULL handle, negative n or
 *   nnzA, flags != 0, a NULL d_rowPtrA or d_mate with n > 0, NULL d_colIndA with nnzA > 0, an output's footprint
 *   overlapping A or the other output, and a call between bhs_spgemm_symbolic and bhs_spgemm_finish.  Each returns
 *   BHS_ERR_INVALID_ARG; the host's refusals leave the outputs untouched, after a refusal by the device they are
 *   unspecified; nothing beyond their stated sizes is ever written.
 * n == 0 succeeds with *npairs_out = 0, *rounds_out = 0 and *ms_out = 0 and launches nothing.
 * Synchronous on the handle's stream, needs no bound data, leaves the handle as it was (a workspace of its own).  ms_out
 *   (may be NULL): device time of the call, the rounds' round trips included.  bhs_get_kernel_stats then reports match_init
 *   (the row bounds, mate = -1), match_round (propose and accept, a row spread over 1, 4, 16 or 64 lanes by the mean row
 *   length; the closing of a round that left vertices) and, where d_agg is given, match_number (the leader flags, the scan,
 *   the numbering).                                                                                                   */
BHS_API int bhs_csr_match_device(bhs_handle *h, int n, int nnzA,
        const int *d_rowPtrA, const int *d_colIndA,
        const bhs_value_t *d_valA /* may be NULL: every weight 1 */,
        unsigned seed, int flags /* must be 0 */,
        int *d_mate /* out: n ints; mate[i] == i where i is unmatched */,
        int *d_agg  /* out, may be NULL: n ints in [0, n - npairs) */,
        int *npairs_out /* may be NULL */, int *rounds_out /* may be NULL */,
        double *ms_out /* may be NULL */);

/* ---- sparse frontier x CSR ------------------------------------------------
 * The push direction of the same traversal step: Y (+)= F (+).(x) G restricted to a LIST of rows of G (GraphBLAS vxm with a
 * sparse vector operand; no reference counterpart; bhs_push_sr.hip.h).  The pull calls above visit all m rows of A every
 * step; this call reads the listed rows of G and nothing else, so a BFS level or a Bellman-Ford round costs what its
 * frontier's out-edges cost.  What it is for: graphs of high diameter (road networks, meshes, banded matrices), whose
 * traversals are thousands of steps with small frontiers.
 * G holds OUT-edges: row j of G lists the vertices that j pushes to, an entry G(j, v) is an edge j -> v.  G is the transpose
 *   of the pull calls' A (bhs_csr_transpose_device), or A itself for a symmetric matrix.  G is m x n, 0-based int32 CSR, rows
 *   need NOT be ascending, duplicate (row, column) pairs are legal and every one of them is an entry; d_valG may be NULL:
 *   every entry then counts as the value 1.
 * d_fidx: nf rows of G, the frontier, in any order; a vertex may be listed more than once, and each listing is an operand of
 *   its own.  F is nf x k, row p belongs to d_fidx[p]; M and Y are n x k; all row-major with leading dimensions ldF, ldM,
 *   ldY >= k, indexed in 64 bits; the gaps c in [k, ld) are never read and never written.  nf, m, n and nnzG may be 0.
 * The rule.  For every list position p < nf, every entry e of row d_fidx[p] of G and every column c < k, the selected
 *   element Y(col_e, c) becomes round(double(Y(col_e, c)) (+) (g_e (x) F(p, c))).  Products, reductions, identities, the NaN
 *   rule, -0 below +0 and OR_AND's notion of non-zero (a Y that is reached counts as 1 where it is not zero, as y_old does
 *   under BHS_MV_ACCUM) are word for word those of "semiring multiply".  Every element of F counts as an entry, as X does in
 *   the pull call.  The call ALWAYS accumulates: there is no form that overwrites, and an element that no product reaches is
 *   neither read nor written.  The frontier's entries, repeats counted, number below 2^31 (else BHS_ERR_INVALID_ARG).
 * Semirings.  The seven whose (+) gives the same bits in any order: BHS_SR_MIN_PLUS, MAX_PLUS, MAX_TIMES, MIN_MAX, MAX_MIN,
 *   OR_AND and PLUS_PAIR (every PLUS_PAIR product is 1 and neither valG nor F is read, so the order of its adds cannot
 *   matter).  BHS_SR_PLUS_TIMES is refused on the host with BHS_ERR_INVALID_ARG: products that meet in an element of Y
 *   arrive through atomics in whatever order the hardware runs them, and a floating sum scattered that way would break this
 *   library's promise that a result is a bit-for-bit function of its input.  (It needs a store-then-sum-by-destination pass.)
 *   In the float build each update rounds to float; rounding is monotone, so that equals one rounding at the end for min,
 *   max and or.  PLUS_PAIR adds 1 per entry with a rounding each: exact while the count stays below 2^24 (2^53 in double).
 * The update is a compare-and-swap loop on the element's bits over the order-preserving keys of the reductions: the element
 *   is read first and nothing is written where the combined value has the same bits.  A retry happens only because another
 *   update of the same element went in; nothing waits.  The hardware's floating min / max atomics are not used (their NaN
 *   and zero ordering is not this contract's).
 * Mask.  Over Y's elements, with the set / complement rules of the pull call: M(v, c) is SET where non-zero (NaN is set, -0
 *   and +0 are not); BHS_MV_MASK_COMPLEMENT selects what is NOT set; NULL selects everything; COMPLEMENT with a NULL mask is
 *   refused.  An unselected element is neither read nor written.  BHS_MV_MASK_COMPLEMENT is the only flag.
 * changed_out (may be NULL): the number of selected elements of Y whose final value differs, as a number, from their value
 *   on entry (+0 equals -0, NaN over NaN is unchanged).  All seven (+) move an element one way only, so this is the number
 *   of elements that received at least one effective update; it is taken through a test-and-set on a workspace bit per
 *   element: an exact integer, the same from run to run.
 * d_next (may be NULL; capacity n ints) / next_count_out (may be NULL): the rows of Y with at least one changed element,
 *   ascending, each once, *next_count_out <= n of them: the next frontier.  Built by compacting a bit-per-row map with the
 *   library's scan, never appended in arrival order: the list is identical from run to run.  With d_next NULL no list is
 *   made and *next_count_out is 0; with d_next and changed_out both NULL no bitmap is touched.  Counts and the error word
 *   come back in the ONE round trip the call makes, at its end; Y is never copied to the host.
 * Validation, on the device, each check before the dependent read: a d_fidx[p] outside [0, m); for a row that is pushed,
 *   rowPtrG[j] > rowPtrG[j+1] or either of the two outside [0, nnzG]; a column outside [0, n) in a pushed row.  Each
 *   returns BHS_ERR_INVALID_ARG, and Y may be partly written, never outside its selected elements.  Rows of G that are not
 *   in the frontier are NOT READ AT ALL -- neither their row pointer nor their columns, so nothing in them is validated
 *   (rowPtrG[0] and rowPtrG[m] neither): that is the point of the call.
 *   On the host, each BHS_ERR_INVALID_ARG with Y untouched: a NULL handle, negative sizes (m, n, nnzG, nf), k < 1, ldF or
 *   ldY below k, ldM below k with a mask, NULL arrays where sizes are positive (d_rowPtrG with m > 0, d_colIndG with
 *   nnzG > 0, d_fidx or d_F with nf > 0, d_Y with n > 0), an unknown semiring or BHS_SR_PLUS_TIMES, any flag other than
 *   BHS_MV_MASK_COMPLEMENT, COMPLEMENT without a mask, the footprint of Y or of d_next overlapping G, d_fidx, F or M (or
 *   each other), and a call between bhs_spgemm_symbolic and bhs_spgemm_finish.
 * Synchronous on the handle's stream, needs no bound data, leaves the handle as it was (a workspace of its own).  ms_out
 *   (may be NULL): device time of the call.  bhs_get_kernel_stats then reports push_degrees (validation and the listed rows'
 *   lengths), push_scan (the library's one-pass scan: lengths to offsets, and the row map's counts to places), push_edges
 *   (runs of 256 consecutive (entry x column) pairs of the frontier a wave, whichever vertices they belong to: at k = 1 a
 *   hub of 10^5 entries is spread over 400 waves) and push_compact (the row map to d_next).                       */
BHS_API int bhs_csr_push_semiring_device(bhs_handle *h, int semiring,
        int m /* rows of G = vertices pushed from */, int n /* columns of G = rows of Y */, int nnzG,
        const bhs_value_t *d_valG /* may be NULL: ones */, const int *d_rowPtrG, const int *d_colIndG,
        int nf, const int *d_fidx /* nf rows of G */,
        int k, const bhs_value_t *d_F /* nf x k */, long long ldF,
        int flags /* BHS_MV_MASK_COMPLEMENT only */,
        const bhs_value_t *d_M /* n x k or NULL */, long long ldM,
        bhs_value_t *d_Y /* n x k, in/out */, long long ldY,
        int *d_next /* may be NULL; capacity n */, int *next_count_out /* may be NULL */,
        long long *changed_out /* may be NULL */, double *ms_out /* may be NULL */);

/* ---- aggregation -----------------------------------------------------------
 * MIS(2) aggregation of the vertices of an n x n pattern S of strong connections: the coarsening step of a smoothed-
 * aggregation multigrid setup, the one that produces the tentative prolongator's pattern (no reference counterpart;
 * bhs_aggregate.hip.h).  S is 0-based int32 CSR; values are NOT TAKEN, so the double and the float library run the same code.
 * Neighbours.  N(i) is the set of columns of row i of S.  The diagonal, repeated columns and the order inside a row make no
 *   difference; rows need not be sorted.
 * Keys.  Vertex i has the 64-bit key prio31(i) << 31 | i: prio31(i) = d_prio[i] >> 1 where d_prio is given, else h >> 1 of
 *   the 32-bit hash (all arithmetic mod 2^32)
 *       h = (i ^ seed) + 0x9e3779b9;  h ^= h >> 16;  h *= 0x85ebca6b;  h ^= h >> 13;  h *= 0xc2b2ae35;  h ^= h >> 16.
 *   Keys are distinct: every tie of priorities is broken by index.
 * Roots.  For a structurally symmetric S the roots are THE greedy distance-2 independent set in descending key order: a
 *   vertex is a root exactly when no vertex of greater key within two steps of it is a root.  That set is unique, so the
 *   result does not depend on how the work is scheduled.
 * Numbering.  Roots are numbered in ascending vertex order: d_agg[d_roots[a]] == a, d_roots ascending, *nagg_out of them.
 * Pass 1.  A vertex that is no root and has a root in N(i) joins the aggregate of the root of greatest key in N(i) (on a
 *   symmetric S there is at most one such root).
 * Pass 2.  Every remaining vertex joins the pass-1 aggregate of the member of N(i) of greatest key among those that pass 1
 *   or the root numbering placed.  Pass 2 reads pass 1's result and never its own: the two live in separate arrays.
 * Isolated vertices.  A vertex without off-diagonal neighbours is a root and a singleton aggregate.
 * Non-symmetric S.  The call still ends, every vertex gets an aggregate in [0, nagg) and d_agg[d_roots[a]] == a; which
 *   aggregates, is unspecified.
 * Reproducibility.  The result is a function of (pattern, priorities or seed) alone: the same bits from run to run, from
 *   handle to handle, and in the double and the float library.  No atomic touches a result.
 * The algorithm is synchronous rounds over one word a vertex, state << 62 | key (undecided 1, in 2, out 0).  A round:
 *   t1[i] = max of the words over i and N(i); then, for undecided i only, t2 = max of t1 over i and N(i) -- t2 is i's own word:
 *   i is in; t2's state is in: i is out; else i stays undecided.  The undecided vertex of greatest key is decided in every
 *   round, so the call ends within n rounds (hashed priorities: 4 to 14 at n <= 3000).  The host reads the count of
 *   undecided vertices once a round, one round trip; *rounds_out is the number of rounds.  The call returns
 *   BHS_ERR_INTERNAL when a round decides nothing or after n + 1 rounds; nothing spins on the device, nothing waits for
 *   another workgroup.
 * Validation, on the device, each check ahead of the dependent read: rowPtrS[i] > rowPtrS[i+1] or either outside
 *   [0, nnzS]; a column outside [0, n).  On the host: a NULL handle, negative n or nnzS, flags != 0, NULL d_rowPtrS or
 *   d_agg with n > 0, NULL d_colIndS with nnzS > 0, the footprint of d_agg or d_roots (n ints each) overlapping S, d_prio or
 *   each other, and a call between bhs_spgemm_symbolic and bhs_spgemm_finish.  Each returns BHS_ERR_INVALID_ARG; on refusal
 *   nothing is read or written out of bounds, the outputs' contents are unspecified, nothing stays queued.
 * n == 0 succeeds with *nagg_out = 0 and *rounds_out = 0 and launches nothing.
 * Synchronous on the handle's stream, needs no bound data, leaves the handle as it was (a workspace of its own).  ms_out
 *   (may be NULL): device time of the call, the rounds' round trips included.  bhs_get_kernel_stats then reports agg_init
 *   (keys, the row pointer's validation), agg_near and agg_decide (the two gathers of a round, a row spread over 1, 4, 16 or
 *   64 lanes by the pattern's mean row length), agg_scan (the roots counted per 64 vertices, the library's one-pass scan,
 *   the numbering) and agg_join (the two passes).                                                                   */
BHS_API int bhs_csr_aggregate_device(bhs_handle *h, int n, int nnzS,
        const int *d_rowPtrS, const int *d_colIndS /* n x n pattern of strong connections; values are not taken */,
        const unsigned *d_prio /* n caller priorities, or NULL: the hash */,
        unsigned seed, int flags /* must be 0 */,
        int *d_agg /* out: n ints, the aggregate of every vertex, in [0, nagg) */,
        int *d_roots /* out, may be NULL: the roots, ascending; room for n ints */,
        int *nagg_out /* may be NULL */, int *rounds_out /* may be NULL */, double *ms_out /* may be NULL */);

/* replaces bhsparse::get_nnzC (bhsparse.h: get_nnzC -> bhsparse_cuda::get_nnzC). */
BHS_API int bhs_get_nnzC(bhs_handle *h, int *nnzC_out);

/* replaces bhsparse::get_C -> bhsparse_cuda::get_C (bhsparse_cuda.h:3006-3020:
 * D2H of colIndC / valC; the reference also re-copies rowPtrC there — pass
 * rowPtrC_out to bhs_spgemm or use bhs_get_rowptrC).  Caller buffers hold
 * nnzC entries.                                                               */
BHS_API int bhs_get_C(bhs_handle *h, int *csrColIndC, bhs_value_t *csrValC);
BHS_API int bhs_get_rowptrC(bhs_handle *h, int *csrRowPtrC /* m+1 */);

/* Device-resident result for callers that keep C on the GPU (multi-GPU
 * all-gatherv of row blocks, chained products).  Pointers stay valid until the
 * next bhs_spgemm / bhs_free_data / bhs_destroy on this handle.               */
BHS_API int bhs_get_C_device(bhs_handle *h, const int **d_rowPtrC, const int **d_colIndC,
                             const bhs_value_t **d_valC);

/* ---- input preparation ----------------------------------------------------
 * Per-row sort of a DEVICE-resident CSR matrix by column index, in place and
 * stable: ref_spgemm::csr_sort_indices (SpGEMM_cuda/ref_spgemm.h:37-62), which
 * the reference's driver runs on the host over every Matrix Market input before
 * the multiply (main.cu:62-64).  Rows already in order are left untouched.
 * Synchronous.  (bhs_set_data / bhs_set_data_device accept unsorted rows as they
 * are; sorted rows of B let the multiply take its fastest kernels.)            */
BHS_API int bhs_csr_sort_indices_device(bhs_handle *h, int n_row, const int *d_rowPtr, int *d_colInd,
                                        bhs_value_t *d_val);

/* ---- colouring and relaxation ----------------------------------------------
 * A greedy colouring of the vertices of an n x n pattern S, and multicolour Gauss-Seidel / SOR sweeps on a vector that use
 * it: the smoother of a multigrid cycle, and a colouring for its own sake (no reference counterpart; bhs_color.hip.h,
 * bhs_gs.hip.h).
 *
 * bhs_csr_color_device.  S is 0-based int32 CSR; values are NOT TAKEN, so the double and the float library run the same
 *   code and give the same bits.
 * Keys.  The aggregation's: prio31(i) << 31 | i, prio31(i) = d_prio[i] >> 1 where d_prio is given (the lowest bit of a
 *   priority is dropped), else h >> 1 of the aggregation's hash of (i, seed).  Ties go by index.
 * Result, as a definition: THE first-fit greedy colouring in descending key order.  Going through the vertices from the
 *   greatest key down, vertex i gets the smallest colour >= 0 that no off-diagonal neighbour coloured before it holds.
 *   Diagonal entries are ignored, repeated columns and the order inside a row make no difference; an isolated vertex gets
 *   colour 0.  For a structurally symmetric S no two neighbours share a colour.
 * Rounds.  Synchronous rounds, as the aggregation's: an uncoloured vertex whose key exceeds that of every uncoloured
 *   off-diagonal neighbour takes its colour this round.  A round reads one colour array and writes another, never the one
 *   it reads, so *rounds_out is a function of the input alone.  The host reads the error word, the count of uncoloured
 *   vertices and the colours in use once a round, one round trip.  BHS_ERR_INTERNAL when a round colours nothing or after
 *   n + 1 rounds; nothing spins on the device, nothing waits for another workgroup.
 * Outputs.  d_color: n ints in [0, ncolors).  d_order: the n vertices sorted by (colour, index).  d_colorPtr: CAPACITY
 *   n + 1 ints, of which ncolors + 1 are written: colour c is d_order[d_colorPtr[c] .. d_colorPtr[c + 1]).  The order is
 *   built without atomics on results and in a number of launches that does not grow with n: the vertices per (colour, 64
 *   vertices) are counted into a colour-major table, the library's one-pass scan turns it into places.  The table holds
 *   ncolors * ceil(n / 64) ints; beyond 2^26 of them (256 MiB, and as much for the places) the call returns
 *   BHS_ERR_ALLOC -- more than 2048 colours at n = 2^21.
 * Non-symmetric S.  The call still ends and every colour is in [0, ncolors); which colouring results is unspecified.
 * Validation, on the device, each check ahead of the dependent read: rowPtrS[i] > rowPtrS[i+1] or either outside
 *   [0, nnzS]; a column outside [0, n).  On the host: a NULL handle, negative n or nnzS, flags != 0, a NULL d_rowPtrS,
 *   d_color, d_order or d_colorPtr with n > 0, NULL d_colIndS with nnzS > 0, an output's footprint overlapping S, d_prio
 *   or another output, and a call between bhs_spgemm_symbolic and bhs_spgemm_finish.  Each returns BHS_ERR_INVALID_ARG.
 * n == 0 succeeds with *ncolors_out = 0 and *rounds_out = 0 and launches nothing.
 * bhs_get_kernel_stats then reports color_round (the rounds, a row spread over 1, 4, 16 or 64 lanes by the pattern's mean
 *   row length) and color_order (the count, the scan, the numbering).
 *
 * bhs_csr_gs_device.  In place on d_x.  For every colour in turn, one launch per non-empty colour over the rows
 *   d_order[h_colorPtr[c] .. h_colorPtr[c + 1]):
 *       s = sum over the entries with j != i of double(a_ij) * double(x_j), summed in double from +0 in an order that
 *           depends on the row's length and the lanes per row alone (the SpMV's rule),
 *       t = (double(b_i) - s) / double(d_i),
 *       x_i = t where omega == 1, else x_i + omega * (t - x_i); one rounding to the value type; IEEE results where d_i is 0.
 *   d_diag (n values, required) is d_i: the diagonal entries of A are skipped, not read.  h_colorPtr is a HOST array of
 *   ncolors + 1 ints.  BHS_GS_FORWARD goes through the colours 0 .. ncolors - 1, BHS_GS_BACKWARD through them in reverse,
 *   BHS_GS_SYMMETRIC forward then backward in each of the `sweeps` sweeps.  The kernel boundary is the only synchronisation.
 * Listed rows.  Rows that are not listed are untouched; h_colorPtr[ncolors] <= n is allowed, so a caller can relax a subset.
 * Validation.  On the host: h_colorPtr starts at 0, never falls and ends <= n; ncolors in [0, n]; sweeps >= 0; a direction
 *   is given and no unknown flag; NULL arrays; d_x overlapping any input (A, d_diag, d_order, d_color, d_b); a call between
 *   bhs_spgemm_symbolic and bhs_spgemm_finish.  On the device, ahead of the dependent read: every d_order entry, row bounds,
 *   columns.  Each returns BHS_ERR_INVALID_ARG; after a refusal by the device x is unspecified.
 * BHS_GS_VERIFY needs d_color (else it may be NULL): the kernels also check color[i] == c for each listed row and
 *   color[j] != c for every off-diagonal entry read; a violation returns BHS_ERR_INVALID_ARG and leaves x unspecified.  It
 *   is a template switch: the unverified path pays nothing.  WITHOUT it an improper colouring -- two rows of one colour
 *   that share an entry -- gives values that depend on timing.
 * Repeatability.  Given a proper colouring the result is a function of the arguments: the same bits from call to call and
 *   from handle to handle.  One control round trip per call, at its end.  ms_out (may be NULL): device time of the call.
 *   bhs_get_kernel_stats then reports gs_forward and gs_backward.                                                  */
#define BHS_GS_FORWARD   1
#define BHS_GS_BACKWARD  2
#define BHS_GS_SYMMETRIC 3   /* forward then backward in each sweep */
#define BHS_GS_VERIFY    4
BHS_API int bhs_csr_color_device(bhs_handle *h, int n, int nnzS,
        const int *d_rowPtrS, const int *d_colIndS /* n x n pattern; values are not taken */,
        const unsigned *d_prio /* n caller priorities, or NULL: the hash */,
        unsigned seed, int flags /* must be 0 */,
        int *d_color /* out: n ints in [0, ncolors) */,
        int *d_order /* out: the n vertices by (colour, index) */,
        int *d_colorPtr /* out: capacity n + 1, ncolors + 1 written */,
        int *ncolors_out /* may be NULL */, int *rounds_out /* may be NULL */, double *ms_out /* may be NULL */);
BHS_API int bhs_csr_gs_device(bhs_handle *h, int n, int nnzA,
        const int *d_rowPtrA, const int *d_colIndA, const bhs_value_t *d_valA,
        const bhs_value_t *d_diag /* n values */,
        int ncolors, const int *h_colorPtr /* HOST: ncolors + 1 ints */, const int *d_order,
        const int *d_color /* may be NULL unless BHS_GS_VERIFY */,
        const bhs_value_t *d_b, bhs_value_t *d_x /* in/out */,
        double omega, int sweeps, int flags /* BHS_GS_FORWARD, _BACKWARD or _SYMMETRIC, | BHS_GS_VERIFY */,
        double *ms_out /* may be NULL */);

/* ---- measurement ----------------------------------------------------------
 * Per-kernel-family device times of the LAST bhs_spgemm (option "kernel_stats" = 1), measured with
 * hipEvents on the stream the kernels were launched on (what bench.py reports
 * as roofline.achieved; replaces the reference's never-enabled `_profiling`
 * prints, bhsparse_cuda.h:728-733).  Returns the number of records; fills up to
 * `cap` of them.  `name` points to a static string.                           */
typedef struct bhs_kernel_stat {
    const char *name;      /* e.g. "numeric_wave<256>"                        */
    int         launches;  /* launches of this family in the last spgemm      */
    double      ms;        /* summed device time of those launches            */
    int64_t     rows;      /* rows of C processed by them                     */
    int64_t     products;  /* intermediate products processed by them         */
    int64_t     nnz_out;   /* entries of C produced (numeric) / counted (symbolic) */
    int64_t     nnzA_rows; /* nnz of the A rows processed (for algorithmic bytes) */
} bhs_kernel_stat;
BHS_API int bhs_get_kernel_stats(bhs_handle *h, bhs_kernel_stat *out, int cap);

/* Tunables (tests use them to force a particular accumulator path; defaults are the measured best):
 *   "force_path"      0 auto | 1 no quarter-wave bin (tiny rows take the wave kernel) |
 *                     2 wave bins are served by the workgroup-per-row kernel
 *   "max_table_log2"  cap (6..15) on the LDS table size => forces the column-window path
 *   "no_pack32"       1: always 64-bit sort keys
 *   "sym_load_pct", "num_load_pct"  table load factor (5..75 %) that decides a row's bin
 *   "spa"             0: rows beyond the LDS tables use column windows instead of the bitmap accumulators
 *   "lds_bitmap"      0: keep the long-row bitmap in HBM even when the matrix has <= 2^20 columns
 *   "lds_bitmap_min_log2"  numeric workgroup bins with tables of at least 2^v slots go to the LDS bitmap
 *                     kernel when n <= 2^20 (default 12; 99: only rows beyond every table)
 *   "window_bitmap"   rows of thousands of entries of C column window by column window, a wave (2 k .. 8 k entries) or 256
 *                     lanes (beyond) per row, several rows per CU (bhs_row_window.hip.h): 1 (default) when the multiply has
 *                     >= 32 resp. >= 16 such rows per CU, 2 always, 0 never; needs ascending rows of B shorter than 2^16
 *                     and n <= 2^20
 *   "class_super_rows"  consecutive rows a wave of the class numeric kernel takes (0, default: a grid line of A where
 *                     "line_a" found one, else 64)
 *   "small_b"         0: always 64-bit address arithmetic for colIndB / valB (default: 32-bit byte offsets when
 *                     nnz(B) < 2^29)
 *   "lane_first"      1 (default): when every row of A has <= 12 entries and every row of B <= 64 (stencils), the
 *                     upper-bound pass and its host round trip are skipped; the lane-per-row symbolic kernel handles
 *                     every row and counts the products on the side
 *   "wave_first"      1 (default): when maxRow(A) x maxRow(B) fits a wave-per-row table and is within 4x of the average
 *                     row's product count (poisson27pt: 27 x 27), every row runs the symbolic wave kernel of that table
 *                     size straight from rowPtrA -- no upper-bound pass, host round trip or queue
 *   "direct_bins"     1 (default): a stage whose rows ALL sit in the lane bin or the quad bin (stencils) skips the
 *                     queue-fill pass; the kernel derives row q's descriptor from rowPtrA / rowPtrC
 *   "sort_b"          1 (default): rows of B that are not ascending are sorted at bhs_set_data[_device] time (device
 *                     pointers are borrowed and never written: the sort runs on a private copy); 0: multiply them as
 *                     they are (general kernels only).  Set it before bhs_set_data.
 *   "lane_rows"       lane-per-row symbolic kernel (k_row_lane: one row per lane, K-way merge of the sorted B rows in
 *                     registers) for rows with <= 12 entries and <= 144 products: 0 never, 1 (default) when EVERY row of
 *                     A has <= 12 entries (stencils), 2 for any matrix.  Needs B with strictly ascending rows.
 *   "lane_numeric"    the numeric stage of those rows goes through k_row_lane as well: 0 never, 1 always, 2 (default)
 *                     when no row of A has more than 8 entries (poisson5pt, 7pt; measured slower beyond)
 *   "compress_b"      symbolic pass on the compressed pattern of B ((column >> 5, mask) pairs; rows binned by their
 *                     pair count): 0 never, 1 (default) when the average row has more than 1536 products and the data
 *                     has <= 60 % as many pairs as entries (FEM-like inputs: keeps rows out of the workgroup-per-row
 *                     symbolic kernels), 2 always.  Only for B with ascending rows.  Set it before bhs_set_data for
 *                     mode 1 to be decided there.
 *   "kernel_stats"    1: every kernel family of a multiply is bracketed by a hipEvent pair for bhs_get_kernel_stats
 *                     (times of the families; launches / rows are always counted); 0 (default): only the four stage
 *                     timers are recorded -- the pairs cost 34 us of a 0.24 ms poisson5pt 1024^2 multiply, 0.16 ms of
 *                     the 3.3 ms power-law stand-in (many bins).  The reference's own `_profiling` prints are off by
 *                     default too (bhsparse_cuda.h:728-733).
 *   "concurrent_bins" the kernels of a stage's bins run concurrently on side streams: 0 never, 1 always,
 *                     2 (default) when the stage has >= 8 non-empty bins (power-law matrices)
 *   "spa_slots"       HBM bitmap slots (default: one per CU)
 *   "class_path"      row classes (bhs_class.hip.h): rows that repeat one another's relative pattern -- stencils, anything
 *                     assembled on a regular grid -- get their structure (sorted columns, entry count, product ->
 *                     position map) worked out once per class instead of once per row.  1 (default): tried on data
 *                     sets whose rows of A and B have at most 256 entries and, on average, at least
 *                     "class_min_products" (default 64) products per row of C and 1e7 products in all; every row is classified and verified
 *                     on the device, and a data set with rows that find no class (or a class of more than 8192
 *                     products / 512 entries per row of C) goes back to the general pipeline for good.
 *                     2: tried whatever the average; 0: never.
 *   "class_numeric"   numeric kernel of the classes whose product list fits a wave's registers (<= 64 entries per row
 *                     of A and B, <= 1024 products): 2 (default) round 5's ring kernel (bhs_class_ring.hip.h: sums in
 *                     registers, stored where an entry of C ends; B's values through a ring of slabs in LDS; 16 waves
 *                     per CU) wherever its LDS fits, 1 round 4's ring kernel (bhs_class_wg.hip.h), 0 always the
 *                     LDS-atomic kernel of round 2.  Multiplies with bigger classes (several unknowns per grid node)
 *                     run bhs_class_big.hip.h whatever this says.
 *   "class_heads"     2 (default): one pass per matrix -- the wave that finds a row differing from the row `period`
 *                     rows before it takes it through the class table itself (bhs_class_fused.hip.h; period: sampled
 *                     at bhs_set_data time, the unknowns per node); 1: rounds 3-4's three launches per matrix (list
 *                     the rows that differ, classify the list, hand the classes on); 0: every row through the table
 *   "class_tile"      1 (default): the classifier gives a row to ONE lane where rows have at most 32 entries (63 rows'
 *                     column indices as 16-byte loads through a tile in LDS, bhs_class_tile.hip.h); 0: G lanes per row
 *                     everywhere.  "class_tile_piece": rows a wave of it walks (0, default: one piece per wave slot)
 *   "spec_numeric"    1 (default): from a data set's second multiply on, the class path launches its numeric kernel on
 *                     the classes' figures of the multiply before (k_class_spec_check compares them with this multiply's
 *                     on the device; a refuted launch writes nothing and the multiply runs again); 0: always wait for
 *                     the read-back.  bhs_get_info: "spec_launches", "spec_refuted"
 *                     (round 6: a lane-first multiply -- every row through the lane kernels -- likewise, k_lane_spec_check;
 *                     "lane_from_counts" 1 (default): its numeric kernel then makes rowPtrC from the symbolic kernel's counts
 *                     and block sums, no scan kernel)
 *   "keep_columns"    1 (default, round 7): a multiply whose classes provably name the columns that the library's own
 *                     colIndC already holds sends its ring kernel out without the column stores.  Nothing is trusted: the
 *                     handle keeps the per-row classes and the classes' relative-column lists of the last multiply that
 *                     wrote every column of that array; the next multiply classifies every row anew as always, names each of
 *                     its classes by the saved class whose list is equal entry by entry (k_class_patterns), compares every
 *                     row's class with the saved one through those names (k_class_scan) and launches the short kernel on
 *                     a second go word (k_class_spec_check); a refuted launch writes nothing and the multiply runs again
 *                     and writes its columns.  Only whole multiplies of the clean class flow into the library's own arrays;
 *                     bhs_set_data*, bhs_free_data, bhs_warmup, bhs_set_output_device, any bhs_set_option, any other flow
 *                     and any error make the next multiply write every column.  colIndC as bhs_get_C_device hands it out
 *                     is const: a caller that writes there must set this to 0.  0: every multiply writes its columns.
 *                     bhs_get_info: "cols_kept" (multiplies that left colIndC as it was), "cols_refuted" (short launches
 *                     the device refuted).  "class_slot_offset" (tests): the classifiers' home slot moves by this much per
 *                     multiply, so that equal patterns get other class numbers; bhs_get_info "class_of_row0" reads one back
 *   "class_mixed"     1 (default, round 6): a row without a class -- or of a class beyond the tables, or of a class with fewer
 *                     than four rows -- goes through the general pipeline's kernels inside the same multiply while the other
 *                     rows stay on the class kernels (bhs_class_mix.hip.h; the reference bins every row for itself,
 *                     SpGEMM_cuda/bhsparse.h:483-586); 0: one such row sends the data set to the general pipeline, as until
 *                     round 5.  "class_mixed_max_pct" (default 30): more irregular rows than this share of all rows send
 *                     the data set to the general pipeline.  bhs_get_info: "class_state", "mixed_rows"
 *   "kernel_stats"    0 (default) no per-kernel timers; 1 hipEvent pairs around every kernel family (bhs_get_kernel_stats);
 *                     2 around the numeric kernels only
 *   "ring_dynamic"    the ring kernel's super-runs handed out by a counter per XCD: 0 never, 1 always, 2 (default) where other
 *                     kernels run beside it
 *   "spin_wait"       1 (default): a multiply's waits for its stream poll, with a pause between polls, for at most
 *                     "spin_wait_us" microseconds (default 0: four times the last multiply's wall time, 0.5 .. 5 ms) before
 *                     they sleep; 0: sleep at once
 *   "hub_min_products"  rows with at least this many intermediate products are split across workgroups
 *                     (bhs_hub.hip.h: items of "hub_item_products" products handed out to the whole device, one shared
 *                     bitmap slot per row); default 131072, 0 never.  "hub_item_products" (default 8192, >= 64),
 *                     "hub_slots" (rows per batch; default: as many as fit 1/16 of the device memory)
 *   "add_inplace"     1 (default): bhs_spgemm_add adds into valC in place where every entry of D is an entry of A·B; 0: the
 *                     sum always goes to a second set of arrays (tests reach both paths on the same data)
 *   "wg_per_cu"       persistent workgroups per CU of the wave kernels (default: occupancy API)
 *   "verbose"         same as bhs_set_verbose
 * Returns BHS_ERR_INVALID_ARG for unknown keys.                               */
BHS_API int bhs_set_option(bhs_handle *h, const char *key, int64_t value);

/* What the library found out about the bound data set (after bhs_set_data[_device]):
 *   "b_sorted"   1 when every row of B (as multiplied: after the optional sort) is strictly ascending
 *   "max_row_a", "max_row_b"   longest row of A / B
 *   "local_a"    1 when sampled rows of A keep their entries near the diagonal (mean |column - row| < columns / 16): the
 *                lane-per-row kernels are only chosen then
 *   "line_a"     rows per grid line of A when the places where a row's length changes repeat with a fixed period and the
 *                matrix is a whole number of such lines (a wave of the class numeric kernel then takes whole lines), else 0
 *   "compress_b_used"  1 when the symbolic pass of the general pipeline runs on B's pattern compressed to (column block,
 *                mask) pairs for this data set
 *   "class_state"  which pipeline this data set's multiplies take: 1 row classes, 2 row classes with irregular rows on the
 *                general pipeline's kernels (mixed mode), -1 the general pipeline (for good: until the next bhs_set_data)
 *   "select_dropped"  entries the last bhs_spgemm_select removed from A·B (0: no second set of arrays was made)
 *   "add_inplace_used"  1 when the last bhs_spgemm_add added into valC in place, 0 when it wrote the sum to arrays of its own
 *   "mixed_rows"   rows of the last multiply that had no class and went through the general pipeline's kernels (0: none)
 * Returns BHS_ERR_INVALID_ARG for unknown keys, BHS_ERR_NOT_READY without data.  */
BHS_API int bhs_get_info(bhs_handle *h, const char *key, int64_t *value_out);

/* Row classes of the open / last multiply, for a caller that rebuilds column indices itself instead of moving them
 * (bhs_dist's values-only all-gatherv: on a grid matrix colIndC of a row is its class's relative column list plus the
 * row number, so only valC has to cross xGMI).  No reference counterpart (the reference has no classes, no second GPU).
 *   d_classC      int32[m]: class of every row of A (= row of C); valid from bhs_spgemm_symbolic until the next multiply
 *   d_classInfo   16 bytes per class slot: int32 {entries of the A row, products, entries of the C row, representative}
 *   d_classRel    int32[slots * rel_stride]: the class's columns relative to the row, ascending
 *   usable_out    0: that multiply did not go by row classes with register-sized tables -- nothing above is valid
 * Device pointers into the handle's workspace.  BHS_ERR_NOT_READY without an open or finished multiply.            */
BHS_API int bhs_get_class_tables_device(bhs_handle *h, const int **d_classC, const void **d_classInfo,
                                        const int **d_classRel, int *slots_out, int *rel_stride_out, int *usable_out);

/* colIndC of n consecutive rows from their classes, on `stream` (a hipStream_t; NULL: the device's null stream) of the
 * CURRENT device: row i of the n rows has class d_classC[i], classInfo[class].z entries, and its entry s is column
 * d_classRel[class * rel_stride + s] + row0 + i, written at d_colIndC[d_rowPtrC[i] + s].  The tables may be another
 * handle's or another GPU's, copied over (bhs_dist).  Asynchronous.                                                  */
BHS_API int bhs_expand_class_columns_device(void *stream, int n, int row0, const int *d_classC, const void *d_classInfo,
                                            const int *d_classRel, int rel_stride, const int *d_rowPtrC, int *d_colIndC);

BHS_API const char *bhs_strerror(int status);
BHS_API const char *bhs_version(void);

/* ---- triangular solve and ILU(0) ---------------------------------------------
 * The level sets of a triangle of an n x n pattern, the sparse triangular solve on them with the triangle read IN PLACE,
 * and the incomplete factorisation A = L U on A's own pattern (no reference counterpart; bhs_trsv.hip.h, bhs_ilu0.hip.h).
 * All three read 0-based int32 CSR on the device.  A triangle is never extracted: the caller passes the whole A, or one
 * CSR that holds L and U as bhs_csr_ilu0_device leaves them.
 *
 * bhs_csr_levels_device.  Values are NOT TAKEN, so the double and the float library run the same code and give the same
 *   bits.  flags is BHS_TRI_LOWER or BHS_TRI_UPPER, exactly one and nothing else.  LOWER counts the entries with j < i,
 *   UPPER those with j > i; everything else, the diagonal included, is ignored.
 * Result, as a definition: level(i) = 0 where row i has no counted entry, else 1 + the greatest level(j) over its counted
 *   entries.  Repeated columns and the order inside a row make no difference: the result is a function of the pattern.
 * Passes.  Monotone relaxation in place: levels start at 0, a pass sets level[i] = max(level[i], 1 + max level[j]); values
 *   only rise and never pass the true level, so the fixed point is the definition however a pass's reads race with its
 *   writes.  Rows go in ascending block order for LOWER and descending for UPPER, so one pass carries a level across many
 *   rows.  The host launches 8 passes per control round trip and stops after a batch whose last pass raised nothing;
 *   BHS_ERR_INTERNAL where more than n + 1 passes would be needed.  *passes_out, the passes launched, DEPENDS ON TIMING;
 *   nothing else does.  Nothing spins on the device, nothing waits for another workgroup.
 * Outputs.  d_level: n ints in [0, nlevels).  d_order: the n rows sorted by (level, index).  d_levelPtr: CAPACITY n + 1
 *   ints, of which nlevels + 1 are written: level l is d_order[d_levelPtr[l] .. d_levelPtr[l + 1]).  The order is built as
 *   the colouring's is, through a table of nlevels * ceil(n / 64) ints; beyond 2^26 of them the call returns
 *   BHS_ERR_ALLOC -- a tridiagonal matrix of 2^20 rows is refused, and level scheduling would be pointless there.
 * Validation, on the device, each check ahead of the dependent read: rowPtrA[i] > rowPtrA[i+1] or either outside
 *   [0, nnzA]; a column outside [0, n).  On the host: a NULL handle, negative n or nnzA, flags other than one triangle, a
 *   NULL d_rowPtrA, d_level, d_order or d_levelPtr with n > 0, NULL d_colIndA with nnzA > 0, an output's footprint
 *   overlapping A or another output, and a call between bhs_spgemm_symbolic and bhs_spgemm_finish.  Each returns
 *   BHS_ERR_INVALID_ARG.  n == 0 succeeds with *nlevels_out = 0 and *passes_out = 0 and launches nothing.
 * bhs_get_kernel_stats then reports levels_pass (a row spread over 1, 4, 16 or 64 lanes by the mean row length) and
 *   levels_order (the count, the scan, the numbering).
 *
 * bhs_csr_trsv_device.  Solves T x = alpha b for the rows listed, T the LOWER or UPPER triangle of A with its diagonal.
 *   For every level in turn, ascending as h_levelPtr lists them, one launch per non-empty level over the rows
 *   d_order[h_levelPtr[l] .. h_levelPtr[l + 1]):
 *       s = sum over the triangle's off-diagonal entries of double(a_ij) * double(x_j), summed in double from +0 in an
 *           order that depends on the row's length and the lanes per row alone (the SpMV's rule),
 *       t = (alpha * double(b_i) - s) / double(a_ii); one rounding to the value type; IEEE results where a_ii is 0.
 *   a_ii is the row's own FIRST entry with j == i; a listed row without one returns BHS_ERR_INVALID_ARG (found on the
 *   device).  With BHS_TRI_UNIT_DIAG there is no division and diagonal entries are ignored.  h_levelPtr is a HOST array of
 *   nlevels + 1 ints; the caller passes UPPER levels, from an UPPER analysis, for an UPPER solve.
 * Aliasing.  d_x == d_b exactly is allowed: the solve is then in place.  Any other overlap of d_x with an input is refused.
 * Listed rows.  Rows that are not listed are untouched; h_levelPtr[nlevels] <= n is allowed.
 * Validation.  On the host: h_levelPtr starts at 0, never falls and ends <= n; nlevels in [0, n]; exactly one of
 *   BHS_TRI_LOWER and BHS_TRI_UPPER and no unknown flag; NULL arrays; the overlaps above; a call between
 *   bhs_spgemm_symbolic and bhs_spgemm_finish.  On the device, ahead of the dependent read: every d_order entry, row bounds,
 *   columns, the diagonal.  Each returns BHS_ERR_INVALID_ARG; after a refusal by the device x is unspecified.
 * Repeatability.  Given the levels of the pattern the result is a function of the arguments: the same bits from call to
 *   call and from handle to handle.  With levels that are not the pattern's -- two rows of one level of which one reads
 *   the other -- values depend on timing.  One control round trip per call, at its end.
 *   bhs_get_kernel_stats then reports trsv_level.  (A run of thin levels is NOT fused into one launch of one workgroup:
 *   measured, that was 3.4 to 4.8 times slower than a launch per level on poisson27pt 128^3 and poisson5pt 1024^2 in natural
 *   order and no faster in colour order; profiles/trsv_case.md.)
 *
 * bhs_csr_ilu0_device.  A = L U on A's pattern, IN PLACE on d_valA.  Rows must be strictly ascending and every listed row
 *   needs a diagonal entry; both are checked on the device and return BHS_ERR_INVALID_ARG.  h_levelPtr / d_order are the
 *   LOWER levels of this pattern.  On return the entries with j < i hold L, whose unit diagonal is not stored, and the
 *   entries with j >= i hold U: the two solves above, LOWER | UNIT_DIAG then UPPER, apply (L U)^-1 to a vector.
 *   Row i, in its level's launch, for each of its entries k < i in ascending order:
 *       l_ik = value_t(double(a_ik) / double(u_kk)),
 *       a_ij = value_t(double(a_ij) - double(l_ik) * double(u_kj)) for every entry j > k of row i that row k also holds.
 *   Owner computes: a row takes 1, 4, 16 or 64 lanes of one wave, every entry of the row has one lane that alone reads and
 *   writes it, rows of earlier levels are final by the kernel boundary -- the result is a function of the input.
 * Pivots.  *pivot_out (may be NULL) is the smallest listed row whose pivot u_ii is 0 or not finite, or -1; the call still
 *   returns BHS_SUCCESS and the values follow IEEE.  flags must be 0.  d_valA overlapping another argument is refused.
 *   One control round trip per call, at its end.  bhs_get_kernel_stats then reports ilu0_level.
 * ms_out (may be NULL) of all three: device time of the call.                                                        */
#define BHS_TRI_LOWER     1
#define BHS_TRI_UPPER     2
#define BHS_TRI_UNIT_DIAG 4
BHS_API int bhs_csr_levels_device(bhs_handle *h, int n, int nnzA,
        const int *d_rowPtrA, const int *d_colIndA /* n x n pattern; values are not taken */,
        int flags /* BHS_TRI_LOWER or BHS_TRI_UPPER */,
        int *d_level /* out: n ints in [0, nlevels) */,
        int *d_order /* out: the n rows by (level, index) */,
        int *d_levelPtr /* out: capacity n + 1, nlevels + 1 written */,
        int *nlevels_out /* may be NULL */, int *passes_out /* may be NULL; depends on timing */, double *ms_out /* may be NULL */);
BHS_API int bhs_csr_trsv_device(bhs_handle *h, int n, int nnzA,
        const int *d_rowPtrA, const int *d_colIndA, const bhs_value_t *d_valA,
        int nlevels, const int *h_levelPtr /* HOST: nlevels + 1 ints */, const int *d_order,
        double alpha, const bhs_value_t *d_b, bhs_value_t *d_x /* out; may be d_b itself */,
        int flags /* BHS_TRI_LOWER or BHS_TRI_UPPER, | BHS_TRI_UNIT_DIAG */, double *ms_out /* may be NULL */);
BHS_API int bhs_csr_ilu0_device(bhs_handle *h, int n, int nnzA,
        const int *d_rowPtrA, const int *d_colIndA, bhs_value_t *d_valA /* in/out */,
        int nlevels, const int *h_levelPtr /* HOST: the LOWER levels */, const int *d_order,
        int flags /* must be 0 */, int *pivot_out /* may be NULL */, double *ms_out /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* BHSPARSE_HIP_H */
