// bhsparse.h — the bhSPARSE facade class for the MI355X backend.
//
// Public interface = SpGEMM_cuda/bhsparse.h:17-33, verbatim signatures, same
// call order (main.cu:104-135), same `int` error convention (0 ==
// BHSPARSE_SUCCESS), same borrowed-pointer ownership (bhsparse.h:205-216), same
// stdout lines (stage times, "[ HIP ] SpGEMM time: T ms. Gflops = G",
// bhsparse.h:287-289).  Every method forwards to libbhsparse_hip.so through the
// C-ABI; there is no device code and no HIP header on this side.
// The OpenCL variant's trailing `use_host_mem` flag (SpGEMM_opencl/bhsparse.h:44-47)
// is accepted and ignored (MI355X is a discrete HBM part).
#ifndef BHSPARSE_AMD_BHSPARSE_H
#define BHSPARSE_AMD_BHSPARSE_H

#include <chrono>

#include "../../include/bhsparse_hip.h"
#include "common.h"

class bhsparse
{
public:
    bhsparse() : _spgemm_platform(0), _h(0), _m(0), _k(0), _n(0), _nnzCt_full(0), _nnzC(0), _h_csrRowPtrC(0) {}
    int initPlatform(bool *spgemm_platform);
    int initData(int m, int k, int n,
                 int nnzA, value_type *csrValA, index_type *csrRowPtrA, index_type *csrColIndA,
                 int nnzB, value_type *csrValB, index_type *csrRowPtrB, index_type *csrColIndB,
                 index_type *csrRowPtrC, bool use_host_mem = false);
    int spgemm();
    int warmup();

    int get_nnzC();
    int get_C(index_type *csrColIndC, value_type *csrValC);

    int freePlatform();
    int free_mem();

    // additions (not in the reference): product count and device stage times of the last spgemm()
    long long get_nnzCt() const { return _nnzCt_full; }
    const double *get_stage_ms() const { return _stage_ms; }
    // the C-ABI handle behind this object, for the multi-GPU layer (include/bhsparse_dist.h)
    bhs_handle *handle() const { return _h; }

    // EXTENSION, not part of the reference's API: the masked multiply (bhs_spgemm_masked, include/bhsparse_hip.h) on
    // the data of initData.  csrValC[p] = (A·B)(i, csrColIndM[p]) for every entry p of row i of the caller's pattern M
    // (m x n, rows strictly ascending; 0 where no product lands).  Host arrays; does not disturb get_C's result.
    int spgemm_masked(int *csrRowPtrM, int *csrColIndM, int nnzM, value_type *csrValC);

    // EXTENSION, not part of the reference's API: C = alpha A·B + beta D (bhs_spgemm_add, include/bhsparse_hip.h) on the
    // data of initData; D is m x n CSR with strictly ascending rows, host arrays.  Fills the csrRowPtrC of initData;
    // get_nnzC / get_C then return the sum.
    int spgemm_add(value_type alpha, value_type beta, int nnzD, value_type *csrValD, int *csrRowPtrD, int *csrColIndD);

    // EXTENSION, not part of the reference's API: C = select(A·B) (bhs_spgemm_select, include/bhsparse_hip.h, "entry
    // selection") on the data of initData: the multiply, then the rule `sel` applied to its result.  Fills the csrRowPtrC of
    // initData; get_nnzC / get_C then return the selected C.
    int spgemm_select(const bhs_select &sel);

    // EXTENSION, not part of the reference's API: T = X^T (bhs_csr_transpose_device, include/bhsparse_hip.h, "transpose") on
    // DEVICE arrays; X is m x n, T's arrays are the caller's (n + 1, nnzX, nnzX entries; d_valX / d_valT / d_perm may be 0).
    // Needs initPlatform only; does not disturb the data of initData or get_C's result.
    int csr_transpose_device(int m, int n, int nnzX, const value_type *d_valX, const index_type *d_rowPtrX,
                             const index_type *d_colIndX, index_type *d_rowPtrT, index_type *d_colIndT, value_type *d_valT,
                             index_type *d_perm);

    // EXTENSION, not part of the reference's API: Z = X(rows, cols) (bhs_csr_extract_{symbolic,numeric}_device,
    // include/bhsparse_hip.h, "extract") on DEVICE arrays; X is m x n, d_rows / d_cols may be 0 (all, in order), Z's arrays are
    // the caller's (mI + 1 ints, then nnzZ entries each; d_valX / d_valZ / d_perm may be 0).  Needs initPlatform only; does
    // not disturb the data of initData or get_C's result.
    int csr_extract_symbolic_device(int m, int n, int nnzX, const index_type *d_rowPtrX, const index_type *d_colIndX, int mI,
                                    const index_type *d_rows, int nJ, const index_type *d_cols, index_type *d_rowPtrZ,
                                    int *nnzZ_out);
    int csr_extract_numeric_device(int m, int n, int nnzX, const value_type *d_valX, const index_type *d_rowPtrX,
                                   const index_type *d_colIndX, int mI, const index_type *d_rows, int nJ,
                                   const index_type *d_cols, int nnzZ, const index_type *d_rowPtrZ, index_type *d_colIndZ,
                                   value_type *d_valZ, index_type *d_perm);

    // EXTENSION, not part of the reference's API: reductions and the diagonal scaling (bhs_csr_reduce_device,
    // bhs_csr_scale_device, include/bhsparse_hip.h, "reduce / scale") on DEVICE arrays; X is m x n.  axis: a BHS_AXIS_*
    // constant, op: BHS_RED_*, flags: BHS_RED_OFFDIAG / BHS_SCALE_*_DIV; d_out holds m, n, 1 or min(m, n) values, d_valZ
    // nnzX (it may be d_valX); d_left / d_right may be 0.  Needs initPlatform only; does not disturb the data of initData
    // or get_C's result.
    int csr_reduce_device(int m, int n, int nnzX, const value_type *d_valX, const index_type *d_rowPtrX,
                          const index_type *d_colIndX, int axis, int op, int flags, value_type *d_out);
    int csr_scale_device(int m, int n, int nnzX, const value_type *d_valX, const index_type *d_rowPtrX,
                         const index_type *d_colIndX, double alpha, const value_type *d_left, const value_type *d_right,
                         int flags, value_type *d_valZ);

    // EXTENSION, not part of the reference's API: CSR x dense (bhs_csr_spmv_device, bhs_csr_spmm_device,
    // include/bhsparse_hip.h, "CSR x dense") on DEVICE arrays: y = alpha A x + beta y and Y = alpha A X + beta Y; A is m x n
    // (d_valA may be 0: every entry counts as 1), X n x k and Y m x k row-major with leading dimensions ldX, ldY >= k.  Needs
    // initPlatform only; does not disturb the data of initData or get_C's result.
    int csr_spmv_device(int m, int n, int nnzA, const value_type *d_valA, const index_type *d_rowPtrA,
                        const index_type *d_colIndA, double alpha, const value_type *d_x, double beta, value_type *d_y);
    int csr_spmm_device(int m, int n, int nnzA, const value_type *d_valA, const index_type *d_rowPtrA,
                        const index_type *d_colIndA, int k, double alpha, const value_type *d_X, long long ldX, double beta,
                        value_type *d_Y, long long ldY);

    // EXTENSION, not part of the reference's API: the sampled dense-dense product (bhs_csr_sddmm_device,
    // include/bhsparse_hip.h, "sampled dense-dense product") on DEVICE arrays: Z(i, j) = alpha (X(i, :) . Y(j, :)) [M(i, j)]
    // + beta Z(i, j) on the entries of the m x n pattern M; X m x k and Y n x k row-major with leading dimensions ldX,
    // ldY >= k (d_Y may be d_X); d_valM is read under BHS_SDDMM_TIMES_M only (else it may be 0); d_valZ, nnzM values, may be
    // d_valM.  The bits of an entry are those of a host loop in the rule's order.  Needs initPlatform only; does not disturb
    // the data of initData or get_C's result.
    int csr_sddmm_device(int m, int n, int nnzM, const value_type *d_valM, const index_type *d_rowPtrM,
                         const index_type *d_colIndM, int k, double alpha, const value_type *d_X, long long ldX,
                         const value_type *d_Y, long long ldY, double beta, value_type *d_valZ, unsigned flags);

    // EXTENSION, not part of the reference's API: the factorised sparse approximate inverse (bhs_csr_fsai_device,
    // include/bhsparse_hip.h, "approximate inverse") on DEVICE arrays: the values of the lower-triangular G on the caller's
    // pattern (rows strictly ascending, ending in the diagonal, at most BHS_FSAI_MAX_ROW entries) with (G A G^T)_ii = 1 for
    // the n x n matrix A, of which the lower triangle is read; d_valG, nnzG values, overlaps no input.  *bad_row (may be 0):
    // the smallest row with a pivot that is not positive and finite, or -1.  The bits of a value are those of a host loop
    // in the rule's order.  Needs initPlatform only; does not disturb the data of initData or get_C's result.
    int csr_fsai_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA, const value_type *d_valA,
                        int nnzG, const index_type *d_rowPtrG, const index_type *d_colIndG, value_type *d_valG, int flags,
                        int *bad_row);

    // EXTENSION, not part of the reference's API: polynomial relaxation and the product with its reductions
    // (bhs_csr_relax_device, bhs_csr_spmv_dots_device, bhs_chebyshev_coefficients; include/bhsparse_hip.h, "relaxation and
    // fused products") on DEVICE arrays.  csr_relax_device: `steps` sweeps on the n x n matrix A in one call, coef a HOST
    // array of the 2 * steps numbers (a_0, c_0), (a_1, c_1), ..: d <- c (b - A x) / diag + a d, x <- x + d; d_d may be 0
    // where every a is 0; flags BHS_RELAX_ZERO_GUESS or 0.  csr_spmv_dots_device: z = alpha A x + beta y out of place (d_z
    // may be d_y; d_y may be 0 where beta == 0) with dots[0] = z.z and dots[1] = w.z (d_w may be 0) on the HOST.  Both need
    // initPlatform only.  chebyshev_coefficients fills coef for the spectrum interval [lmin, lmax]; no device work.
    int csr_relax_device(int n, int nnzA, const value_type *d_valA, const index_type *d_rowPtrA, const index_type *d_colIndA,
                         const value_type *d_diag, int steps, const double *coef, const value_type *d_b, value_type *d_x,
                         value_type *d_d, unsigned flags);
    int csr_spmv_dots_device(int m, int n, int nnzA, const value_type *d_valA, const index_type *d_rowPtrA,
                             const index_type *d_colIndA, double alpha, const value_type *d_x, double beta,
                             const value_type *d_y, value_type *d_z, const value_type *d_w, double *dots);
    static int chebyshev_coefficients(double lmin, double lmax, int steps, double *coef);

    // EXTENSION, not part of the reference's API: semiring CSR x dense with an output mask and accumulation
    // (bhs_csr_spmv_semiring_device, bhs_csr_spmm_semiring_device, include/bhsparse_hip.h, "semiring CSR x dense") on DEVICE
    // arrays: Y<M> (+)= A (+).(x) X; semiring: a BHS_SR_* constant, flags: BHS_MV_ACCUM | BHS_MV_MASK_COMPLEMENT, d_mask /
    // d_M may be 0 (everything is selected), changed_out may be 0.  One step of a BFS (OR_AND under the complement of the
    // visited set) or of Bellman-Ford (MIN_PLUS with BHS_MV_ACCUM); an entry A(i, j) is an edge j -> i.  Needs initPlatform
    // only; does not disturb the data of initData or get_C's result.
    int csr_spmv_semiring_device(int semiring, int m, int n, int nnzA, const value_type *d_valA, const index_type *d_rowPtrA,
                                 const index_type *d_colIndA, const value_type *d_x, int flags, const value_type *d_mask,
                                 value_type *d_y, long long *changed_out);
    int csr_spmm_semiring_device(int semiring, int m, int n, int nnzA, const value_type *d_valA, const index_type *d_rowPtrA,
                                 const index_type *d_colIndA, int k, const value_type *d_X, long long ldX, int flags,
                                 const value_type *d_M, long long ldM, value_type *d_Y, long long ldY, long long *changed_out);

    // EXTENSION, not part of the reference's API: the push direction of the same step (bhs_csr_push_semiring_device,
    // include/bhsparse_hip.h, "sparse frontier x CSR") on DEVICE arrays: Y<M> (+)= F (+).(x) G(fidx, :), where G holds
    // OUT-edges (row j lists the vertices j pushes to: the transpose of the pull calls' A) and d_fidx lists the nf rows of
    // the frontier; only those rows of G are read.  Any semiring but BHS_SR_PLUS_TIMES; flags: BHS_MV_MASK_COMPLEMENT or 0;
    // d_valG, d_M, d_next, next_count_out and changed_out may be 0.  d_next (n ints) receives the rows of Y that changed,
    // ascending: the next frontier.  Needs initPlatform only.
    int csr_push_semiring_device(int semiring, int m, int n, int nnzG, const value_type *d_valG, const index_type *d_rowPtrG,
                                 const index_type *d_colIndG, int nf, const index_type *d_fidx, int k, const value_type *d_F,
                                 long long ldF, int flags, const value_type *d_M, long long ldM, value_type *d_Y, long long ldY,
                                 index_type *d_next, int *next_count_out, long long *changed_out);

    // EXTENSION, not part of the reference's API: MIS(2) aggregation of an n x n pattern of strong connections on DEVICE
    // arrays (bhs_csr_aggregate_device, include/bhsparse_hip.h, "aggregation"): d_agg (n ints) receives the aggregate of
    // every vertex, d_roots (room for n ints, may be 0) the roots, ascending, *nagg_out their number and *rounds_out the
    // rounds taken.  d_prio (n priorities) may be 0: the hash of (vertex, seed); flags must be 0.  Needs initPlatform only.
    int csr_aggregate_device(int n, int nnzS, const index_type *d_rowPtrS, const index_type *d_colIndS, const unsigned *d_prio,
                             unsigned seed, int flags, index_type *d_agg, index_type *d_roots, int *nagg_out, int *rounds_out);

    // EXTENSION, not part of the reference's API: the first-fit greedy colouring in descending key order of an n x n pattern
    // on DEVICE arrays (bhs_csr_color_device, include/bhsparse_hip.h, "colouring and relaxation"): d_color (n ints) receives
    // every vertex's colour, d_order (n ints) the vertices by (colour, index), d_colorPtr (room for n + 1 ints) the
    // *ncolors_out + 1 offsets of the colours into d_order.  d_prio may be 0: the hash of (vertex, seed); flags must be 0.
    // csr_gs_device relaxes d_x in place with multicolour Gauss-Seidel / SOR sweeps on such a colouring (bhs_csr_gs_device):
    // h_colorPtr is a HOST array of ncolors + 1 ints, d_diag the diagonal of A, flags BHS_GS_FORWARD, BHS_GS_BACKWARD or
    // BHS_GS_SYMMETRIC, with BHS_GS_VERIFY (needs d_color, else it may be 0) to check the colouring.  Both need initPlatform only.
    int csr_color_device(int n, int nnzS, const index_type *d_rowPtrS, const index_type *d_colIndS, const unsigned *d_prio,
                         unsigned seed, int flags, index_type *d_color, index_type *d_order, index_type *d_colorPtr,
                         int *ncolors_out, int *rounds_out);
    int csr_gs_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA, const value_type *d_valA,
                      const value_type *d_diag, int ncolors, const index_type *h_colorPtr, const index_type *d_order,
                      const index_type *d_color, const value_type *d_b, value_type *d_x, double omega, int sweeps, int flags);

    // EXTENSION, not part of the reference's API: the level sets of a triangle, the sparse triangular solve on them and ILU(0)
    // in place, on DEVICE arrays (bhs_csr_levels_device, bhs_csr_trsv_device, bhs_csr_ilu0_device; include/bhsparse_hip.h,
    // "triangular solve and ILU(0)").  csr_levels_device: flags BHS_TRI_LOWER or BHS_TRI_UPPER; d_level (n ints) receives
    // every row's level, d_order (n ints) the rows by (level, index), d_levelPtr (room for n + 1 ints) the *nlevels_out + 1
    // offsets of the levels into d_order; *passes_out depends on timing.  csr_trsv_device solves T x = alpha b for that
    // triangle of A read in place (h_levelPtr is a HOST array of nlevels + 1 ints; flags the triangle, | BHS_TRI_UNIT_DIAG;
    // d_x may be d_b).  csr_ilu0_device factorises A = L U on A's pattern in d_valA (the LOWER levels; flags must be 0);
    // *pivot_out is the smallest row with a zero or non-finite pivot, or -1.  All need initPlatform only.
    int csr_levels_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA, int flags,
                          index_type *d_level, index_type *d_order, index_type *d_levelPtr, int *nlevels_out, int *passes_out);
    int csr_trsv_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA, const value_type *d_valA,
                        int nlevels, const index_type *h_levelPtr, const index_type *d_order, double alpha, const value_type *d_b,
                        value_type *d_x, int flags);
    int csr_ilu0_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA, value_type *d_valA,
                        int nlevels, const index_type *h_levelPtr, const index_type *d_order, int flags, int *pivot_out);

    // EXTENSION, not part of the reference's API: the connected components of an n x n pattern S on DEVICE arrays, weakly
    // (bhs_csr_components_device; include/bhsparse_hip.h, "connected components").  d_root (n ints) receives the smallest
    // vertex of every vertex's component, d_comp (n ints, may be null) the component's number by ascending root, d_compSize
    // (room for n ints, may be null, needs d_comp) the *ncomp_out sizes; *passes_out depends on timing.  flags must be 0.
    // Needs initPlatform only.
    int csr_components_device(int n, int nnzS, const index_type *d_rowPtrS, const index_type *d_colIndS, int flags,
                              index_type *d_root, index_type *d_comp, index_type *d_compSize, int *ncomp_out, int *passes_out);

    // EXTENSION, not part of the reference's API: the strongly connected components of an n x n pattern S on DEVICE arrays
    // (bhs_csr_scc_device; include/bhsparse_hip.h, "strongly connected components"); an entry (i, j) is a directed edge, and
    // which way it points does not matter.  d_root (n ints) receives the smallest vertex of every vertex's SCC, d_comp (n
    // ints, may be null) the SCC's number by ascending root, d_compSize (room for n ints, may be null, needs d_comp) the
    // *nscc_out sizes; *rounds_out is a function of the pattern, *passes_out depends on timing.  flags must be 0.  Needs
    // initPlatform only.
    int csr_scc_device(int n, int nnzS, const index_type *d_rowPtrS, const index_type *d_colIndS, int flags,
                       index_type *d_root, index_type *d_comp, index_type *d_compSize, int *nscc_out, int *rounds_out,
                       int *passes_out);

    // EXTENSION, not part of the reference's API: the reverse Cuthill-McKee ordering of an n x n pattern S on DEVICE arrays
    // (bhs_csr_rcm_device; include/bhsparse_hip.h, "bandwidth-reducing ordering").  S has strictly ascending rows and a
    // symmetric structure, checked on the device.  d_perm (n ints) receives the old index of every new row; d_level (n ints,
    // may be null) the final sweep's levels; d_start (room for n ints, may be null) the *ncomp_out starts.  *depth_out and
    // *sweeps_out are functions of the pattern, *passes_out is a multiple of the batch and depends on timing.  flags:
    // BHS_RCM_PERIPHERAL | BHS_RCM_NO_REVERSE.  Needs initPlatform only.
    int csr_rcm_device(int n, int nnzS, const index_type *d_rowPtrS, const index_type *d_colIndS, int flags,
                       index_type *d_perm, index_type *d_level, index_type *d_start, int *ncomp_out, int *depth_out,
                       int *sweeps_out, int *passes_out);

    // EXTENSION, not part of the reference's API: the k-core decomposition of an n x n pattern S on DEVICE arrays
    // (bhs_csr_kcore_device; include/bhsparse_hip.h, "k-core decomposition").  S has strictly ascending rows and a symmetric
    // structure, checked on the device; the diagonal is ignored.  d_core (n ints) receives every vertex's core number,
    // d_round (n ints, may be null) the round of the synchronous peeling in which it leaves, from 1.  *kmax_out (the
    // degeneracy) and *rounds_out are functions of the pattern.  flags must be 0.  Needs initPlatform only.
    int csr_kcore_device(int n, int nnzS, const index_type *d_rowPtrS, const index_type *d_colIndS, int flags,
                         index_type *d_core, index_type *d_round, int *kmax_out, int *rounds_out);

    // EXTENSION, not part of the reference's API: shortest paths from nsrc sources over the OUT-EDGES of an n x n matrix G on
    // DEVICE arrays by delta-stepping in one call (bhs_csr_sssp_device; include/bhsparse_hip.h, "shortest paths").  G(i, j) is
    // an edge i -> j; d_valG may be null: every weight 1; a negative or NaN weight is refused on the device.  d_dist (n values)
    // receives the distance to the nearest source, +Inf where there is none; d_parent (n ints, may be null) the smallest
    // neighbour of strictly smaller distance with a tight edge, -1 for a source or a vertex not reached, -2 where no such edge
    // exists.  delta > 0 or +Inf is the bucket width: it changes the work, never the result.  *reached_out and *passes_out (a
    // multiple of 8) are functions of the input and delta.  flags must be 0.  Needs initPlatform only.
    int csr_sssp_device(int n, int nnzG, const index_type *d_rowPtrG, const index_type *d_colIndG, const value_type *d_valG,
                        int nsrc, const index_type *d_sources, double delta, int flags, value_type *d_dist, index_type *d_parent,
                        int *reached_out, int *passes_out);

    // EXTENSION, not part of the reference's API: betweenness centrality over the OUT-EDGES G and the IN-EDGES T = G^T of an
    // n-vertex graph on DEVICE arrays, by Brandes' algorithm a source after the other in one call
    // (bhs_csr_betweenness_device; include/bhsparse_hip.h, "betweenness centrality").  For an undirected graph T is G: the same
    // arrays.  d_bc (n doubles) receives the dependencies summed over the nsrc sources in list order -- added to what it holds
    // under BHS_BC_ACCUMULATE -- every number a double whatever value_type is; d_level and d_sigma (n each, may be null) the
    // levels and the path counts of the LAST source.  Every sum has one writer and a fixed order: the bits are a function of
    // the input.  *reached_out (summed over the sources) and *passes_out (a multiple of 8 a source) are too.  Needs
    // initPlatform only.
    int csr_betweenness_device(int n, int nnzG, const index_type *d_rowPtrG, const index_type *d_colIndG, int nnzT,
                               const index_type *d_rowPtrT, const index_type *d_colIndT, int nsrc, const index_type *d_sources,
                               int flags, double *d_bc, index_type *d_level, double *d_sigma, int *reached_out, int *passes_out);

    // EXTENSION, not part of the reference's API: heavy-edge matching of the vertices of an n x n matrix A on DEVICE arrays
    // (bhs_csr_match_device; include/bhsparse_hip.h, "matching").  d_valA may be null: every weight 1.  d_mate (n ints)
    // receives every vertex's partner, the vertex itself where it is unmatched; d_agg (n ints, may be null) the number of its
    // pair or singleton by ascending smaller member, n - *npairs_out of them.  *rounds_out is a function of the input.
    // flags must be 0.  Needs initPlatform only.
    int csr_match_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA, const value_type *d_valA,
                         unsigned seed, int flags, index_type *d_mate, index_type *d_agg, int *npairs_out, int *rounds_out);

    // EXTENSION, not part of the reference's API: the minimum (flags: BHS_FOREST_MAXIMUM, BHS_FOREST_ABS) spanning forest of
    // the graph of an n x n matrix A on DEVICE arrays (bhs_csr_spanning_forest_device; include/bhsparse_hip.h, "spanning
    // forest").  d_valA may be null: every weight 1.  d_label (n ints) receives the root of every vertex's tree; d_edgeLo,
    // d_edgeHi and d_edgeVal (room for n each, d_edgeVal may be null) the *nedges_out edges, lo < hi.  *rounds_out is a function
    // of the input.  Needs initPlatform only.
    int csr_spanning_forest_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA,
                                   const value_type *d_valA, int flags, index_type *d_label, index_type *d_edgeLo,
                                   index_type *d_edgeHi, value_type *d_edgeVal, int *nedges_out, int *rounds_out);

    // EXTENSION, not part of the reference's API: Z (m x n, CSR) from nnzIn triplets on DEVICE arrays, rows ascending, duplicates
    // combined as flags says (BHS_COO_SUM, _FIRST, _LAST or _KEEP, with BHS_COO_IGNORE_NEGATIVE), and the values of a known
    // pattern from new triplet values (bhs_coo_assemble_device, bhs_coo_assemble_values_device; include/bhsparse_hip.h,
    // "assembly").  d_valIn may be null (the pattern alone), and so may d_valZ, d_entryPtr and d_perm.  d_colIndZ, d_valZ and
    // d_perm need room for nnzIn, d_entryPtr for nnzIn + 1; *nnzZ_out entries and *nkept_out map positions are written.
    // Need initPlatform only.
    int coo_assemble_device(int m, int n, int nnzIn, const index_type *d_rowInd, const index_type *d_colInd,
                            const value_type *d_valIn, int flags, index_type *d_rowPtrZ, index_type *d_colIndZ, value_type *d_valZ,
                            index_type *d_entryPtr, index_type *d_perm, int *nnzZ_out, int *nkept_out);
    int coo_assemble_values_device(int nnzIn, const value_type *d_valIn, int nnzZ, const index_type *d_entryPtr,
                                   const index_type *d_perm, int flags, value_type *d_valZ);

    // EXTENSION, not part of the reference's API: the C/F splitting of an n x n pattern S of strong connections on DEVICE
    // arrays (bhs_csr_cfsplit_device; include/bhsparse_hip.h, "C/F splitting and interpolation").  d_prio may be null: the
    // hash of (vertex, seed); flags: 0 or BHS_CF_DEGREE (not with d_prio).  d_cf (n ints) receives the coarse index of every
    // C point and -1 at an F point, d_cpts (room for n ints, may be null) the *nc_out C points, ascending.  *rounds_out is a
    // function of the input.  Needs initPlatform only.
    int csr_cfsplit_device(int n, int nnzS, const index_type *d_rowPtrS, const index_type *d_colIndS, const unsigned *d_prio,
                           unsigned seed, int flags, index_type *d_cf, index_type *d_cpts, int *nc_out, int *rounds_out);

    // EXTENSION, not part of the reference's API: the direct interpolation P (n x nc) of A on the splitting d_cf and the
    // pattern S, a symbolic / numeric pair on DEVICE arrays (bhs_csr_interp_symbolic_device, bhs_csr_interp_numeric_device;
    // same heading).  Rows of A and S strictly ascending.  The symbolic call fills d_rowPtrP (n + 1 ints) and *nnzP_out; the
    // numeric call d_colIndP and d_valP (nnzP each) and may be repeated with new values of A.  Need initPlatform only.
    int csr_interp_symbolic_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA, int nnzS,
                                   const index_type *d_rowPtrS, const index_type *d_colIndS, const index_type *d_cf, int nc,
                                   index_type *d_rowPtrP, long long *nnzP_out);
    int csr_interp_numeric_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA, const value_type *d_valA,
                                  int nnzS, const index_type *d_rowPtrS, const index_type *d_colIndS, const index_type *d_cf, int nc,
                                  const index_type *d_rowPtrP, long long nnzP, index_type *d_colIndP, value_type *d_valP);

    // EXTENSION, not part of the reference's API: the multiply over a semiring (bhs_spgemm_semiring*, include/bhsparse_hip.h,
    // "semiring multiply"; semiring: a BHS_SR_* constant) on the data of initData.  spgemm_semiring is the full product: it
    // fills the csrRowPtrC of initData, and get_nnzC / get_C then return A (+).(x) B on the pattern of A·B.
    // spgemm_semiring_masked is spgemm_masked over the semiring: an entry of M no product lands on reads the (+)-identity.
    int spgemm_semiring(int semiring);
    int spgemm_semiring_masked(int semiring, int *csrRowPtrM, int *csrColIndM, int nnzM, value_type *csrValC);

private:
    bool       *_spgemm_platform;
    bhs_handle *_h;
    int         _m, _k, _n;
    long long   _nnzCt_full;      // size_t in the reference (bhsparse.h:57)
    int         _nnzC;
    index_type *_h_csrRowPtrC;    // caller-owned, filled by spgemm()
    double      _stage_ms[4];
};

inline int bhsparse::initPlatform(bool *spgemm_platform)
{
    _spgemm_platform = spgemm_platform;
    if (!spgemm_platform) return BHS_ERR_INVALID_ARG;
    if (!(spgemm_platform[BHSPARSE_HIP] || spgemm_platform[BHSPARSE_CUDA] || spgemm_platform[BHSPARSE_OPENCL]))
        return BHS_ERR_INVALID_ARG;
    int dev = 0;                                  // the reference hard-codes device 0 (bhsparse_cuda.h:100-101)
    if (const char *e = getenv("BHSPARSE_DEVICE")) dev = atoi(e);
    int err = bhs_create(&_h, 1, &dev);
    if (err != BHSPARSE_SUCCESS) return err;
    return bhs_set_verbose(_h, 1);                // device banner + stage lines, as the reference prints
}

inline int bhsparse::initData(int m, int k, int n,
                              int nnzA, value_type *csrValA, index_type *csrRowPtrA, index_type *csrColIndA,
                              int nnzB, value_type *csrValB, index_type *csrRowPtrB, index_type *csrColIndB,
                              index_type *csrRowPtrC, bool /*use_host_mem*/)
{
    if (!_h) return BHS_ERR_NOT_READY;
    _m = m; _k = k; _n = n;
    _nnzC = 0;
    _h_csrRowPtrC = csrRowPtrC;
    return bhs_set_data(_h, m, k, n, nnzA, csrValA, csrRowPtrA, csrColIndA, nnzB, csrValB, csrRowPtrB, csrColIndB);
}

inline int bhsparse::warmup()
{
    if (!_h) return BHS_ERR_NOT_READY;
    int err = bhs_set_verbose(_h, 0);             // warm-ups are silent in the reference too
    if (err == BHSPARSE_SUCCESS) err = bhs_warmup(_h);
    bhs_set_verbose(_h, 1);
    if (err != BHSPARSE_SUCCESS) std::cout << "warmup error = " << err << std::endl;
    return err;
}

inline int bhsparse::spgemm()
{
    if (!_h) return BHS_ERR_NOT_READY;
    const auto t0 = std::chrono::steady_clock::now();
    int64_t nnzCt = 0;
    int err = bhs_spgemm(_h, _h_csrRowPtrC, &nnzCt, &_nnzC, _stage_ms);
    const double time = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (err != BHSPARSE_SUCCESS) { std::cout << "spgemm error = " << err << std::endl; return err; }
    _nnzCt_full = nnzCt;
    std::cout << "[ HIP ] SpGEMM time: " << time << " ms. Gflops = "
              << 2.0 * (double)_nnzCt_full / (time * 1.0e+6) << std::endl;
    return err;
}

inline int bhsparse::spgemm_masked(int *csrRowPtrM, int *csrColIndM, int nnzM, value_type *csrValC)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_spgemm_masked(_h, csrRowPtrM, csrColIndM, nnzM, csrValC, 0, 0);
}

inline int bhsparse::spgemm_add(value_type alpha, value_type beta, int nnzD, value_type *csrValD, int *csrRowPtrD, int *csrColIndD)
{
    if (!_h) return BHS_ERR_NOT_READY;
    int64_t nnzCt = 0;
    int err = bhs_spgemm_add(_h, alpha, beta, nnzD, csrValD, csrRowPtrD, csrColIndD, _h_csrRowPtrC, &nnzCt, &_nnzC, 0);
    if (err == BHSPARSE_SUCCESS) _nnzCt_full = nnzCt;
    return err;
}

inline int bhsparse::spgemm_select(const bhs_select &sel)
{
    if (!_h) return BHS_ERR_NOT_READY;
    int64_t nnzCt = 0;
    int err = bhs_spgemm_select(_h, &sel, _h_csrRowPtrC, &nnzCt, &_nnzC, 0);
    if (err == BHSPARSE_SUCCESS) _nnzCt_full = nnzCt;
    return err;
}

inline int bhsparse::spgemm_semiring(int semiring)
{
    if (!_h) return BHS_ERR_NOT_READY;
    int64_t nnzCt = 0;
    int err = bhs_spgemm_semiring(_h, semiring, _h_csrRowPtrC, &nnzCt, &_nnzC, 0);
    if (err == BHSPARSE_SUCCESS) _nnzCt_full = nnzCt;
    return err;
}

inline int bhsparse::spgemm_semiring_masked(int semiring, int *csrRowPtrM, int *csrColIndM, int nnzM, value_type *csrValC)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_spgemm_semiring_masked(_h, semiring, csrRowPtrM, csrColIndM, nnzM, csrValC, 0, 0);
}

inline int bhsparse::csr_transpose_device(int m, int n, int nnzX, const value_type *d_valX, const index_type *d_rowPtrX,
                                          const index_type *d_colIndX, index_type *d_rowPtrT, index_type *d_colIndT,
                                          value_type *d_valT, index_type *d_perm)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_transpose_device(_h, m, n, nnzX, d_valX, d_rowPtrX, d_colIndX, d_rowPtrT, d_colIndT, d_valT, d_perm, 0);
}

inline int bhsparse::csr_extract_symbolic_device(int m, int n, int nnzX, const index_type *d_rowPtrX, const index_type *d_colIndX,
                                                 int mI, const index_type *d_rows, int nJ, const index_type *d_cols,
                                                 index_type *d_rowPtrZ, int *nnzZ_out)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_extract_symbolic_device(_h, m, n, nnzX, d_rowPtrX, d_colIndX, mI, d_rows, nJ, d_cols, d_rowPtrZ, nnzZ_out);
}

inline int bhsparse::csr_extract_numeric_device(int m, int n, int nnzX, const value_type *d_valX, const index_type *d_rowPtrX,
                                                const index_type *d_colIndX, int mI, const index_type *d_rows, int nJ,
                                                const index_type *d_cols, int nnzZ, const index_type *d_rowPtrZ,
                                                index_type *d_colIndZ, value_type *d_valZ, index_type *d_perm)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_extract_numeric_device(_h, m, n, nnzX, d_valX, d_rowPtrX, d_colIndX, mI, d_rows, nJ, d_cols, nnzZ, d_rowPtrZ,
                                          d_colIndZ, d_valZ, d_perm, 0);
}

inline int bhsparse::csr_reduce_device(int m, int n, int nnzX, const value_type *d_valX, const index_type *d_rowPtrX,
                                       const index_type *d_colIndX, int axis, int op, int flags, value_type *d_out)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_reduce_device(_h, m, n, nnzX, d_valX, d_rowPtrX, d_colIndX, axis, op, flags, d_out, 0);
}

inline int bhsparse::csr_scale_device(int m, int n, int nnzX, const value_type *d_valX, const index_type *d_rowPtrX,
                                      const index_type *d_colIndX, double alpha, const value_type *d_left,
                                      const value_type *d_right, int flags, value_type *d_valZ)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_scale_device(_h, m, n, nnzX, d_valX, d_rowPtrX, d_colIndX, alpha, d_left, d_right, flags, d_valZ, 0);
}

inline int bhsparse::csr_spmv_device(int m, int n, int nnzA, const value_type *d_valA, const index_type *d_rowPtrA,
                                     const index_type *d_colIndA, double alpha, const value_type *d_x, double beta,
                                     value_type *d_y)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_spmv_device(_h, m, n, nnzA, d_valA, d_rowPtrA, d_colIndA, alpha, d_x, beta, d_y, 0);
}

inline int bhsparse::csr_spmm_device(int m, int n, int nnzA, const value_type *d_valA, const index_type *d_rowPtrA,
                                     const index_type *d_colIndA, int k, double alpha, const value_type *d_X, long long ldX,
                                     double beta, value_type *d_Y, long long ldY)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_spmm_device(_h, m, n, nnzA, d_valA, d_rowPtrA, d_colIndA, k, alpha, d_X, ldX, beta, d_Y, ldY, 0);
}

inline int bhsparse::csr_sddmm_device(int m, int n, int nnzM, const value_type *d_valM, const index_type *d_rowPtrM,
                                      const index_type *d_colIndM, int k, double alpha, const value_type *d_X, long long ldX,
                                      const value_type *d_Y, long long ldY, double beta, value_type *d_valZ, unsigned flags)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_sddmm_device(_h, m, n, nnzM, d_valM, d_rowPtrM, d_colIndM, k, alpha, d_X, ldX, d_Y, ldY, beta, d_valZ, flags, 0);
}

inline int bhsparse::csr_fsai_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA,
                                     const value_type *d_valA, int nnzG, const index_type *d_rowPtrG,
                                     const index_type *d_colIndG, value_type *d_valG, int flags, int *bad_row)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_fsai_device(_h, n, nnzA, d_rowPtrA, d_colIndA, d_valA, nnzG, d_rowPtrG, d_colIndG, d_valG, flags, bad_row, 0);
}

inline int bhsparse::csr_relax_device(int n, int nnzA, const value_type *d_valA, const index_type *d_rowPtrA,
                                      const index_type *d_colIndA, const value_type *d_diag, int steps, const double *coef,
                                      const value_type *d_b, value_type *d_x, value_type *d_d, unsigned flags)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_relax_device(_h, n, nnzA, d_valA, d_rowPtrA, d_colIndA, d_diag, steps, coef, d_b, d_x, d_d, flags, 0);
}

inline int bhsparse::csr_spmv_dots_device(int m, int n, int nnzA, const value_type *d_valA, const index_type *d_rowPtrA,
                                          const index_type *d_colIndA, double alpha, const value_type *d_x, double beta,
                                          const value_type *d_y, value_type *d_z, const value_type *d_w, double *dots)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_spmv_dots_device(_h, m, n, nnzA, d_valA, d_rowPtrA, d_colIndA, alpha, d_x, beta, d_y, d_z, d_w, dots, 0);
}

inline int bhsparse::chebyshev_coefficients(double lmin, double lmax, int steps, double *coef)
{
    return bhs_chebyshev_coefficients(lmin, lmax, steps, coef);
}

inline int bhsparse::csr_spmv_semiring_device(int semiring, int m, int n, int nnzA, const value_type *d_valA,
                                              const index_type *d_rowPtrA, const index_type *d_colIndA, const value_type *d_x,
                                              int flags, const value_type *d_mask, value_type *d_y, long long *changed_out)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_spmv_semiring_device(_h, semiring, m, n, nnzA, d_valA, d_rowPtrA, d_colIndA, d_x, flags, d_mask, d_y,
                                        changed_out, 0);
}

inline int bhsparse::csr_spmm_semiring_device(int semiring, int m, int n, int nnzA, const value_type *d_valA,
                                              const index_type *d_rowPtrA, const index_type *d_colIndA, int k,
                                              const value_type *d_X, long long ldX, int flags, const value_type *d_M,
                                              long long ldM, value_type *d_Y, long long ldY, long long *changed_out)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_spmm_semiring_device(_h, semiring, m, n, nnzA, d_valA, d_rowPtrA, d_colIndA, k, d_X, ldX, flags, d_M, ldM,
                                        d_Y, ldY, changed_out, 0);
}

inline int bhsparse::csr_push_semiring_device(int semiring, int m, int n, int nnzG, const value_type *d_valG,
                                              const index_type *d_rowPtrG, const index_type *d_colIndG, int nf,
                                              const index_type *d_fidx, int k, const value_type *d_F, long long ldF, int flags,
                                              const value_type *d_M, long long ldM, value_type *d_Y, long long ldY,
                                              index_type *d_next, int *next_count_out, long long *changed_out)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_push_semiring_device(_h, semiring, m, n, nnzG, d_valG, d_rowPtrG, d_colIndG, nf, d_fidx, k, d_F, ldF, flags,
                                        d_M, ldM, d_Y, ldY, d_next, next_count_out, changed_out, 0);
}

inline int bhsparse::csr_aggregate_device(int n, int nnzS, const index_type *d_rowPtrS, const index_type *d_colIndS,
                                          const unsigned *d_prio, unsigned seed, int flags, index_type *d_agg,
                                          index_type *d_roots, int *nagg_out, int *rounds_out)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_aggregate_device(_h, n, nnzS, d_rowPtrS, d_colIndS, d_prio, seed, flags, d_agg, d_roots, nagg_out, rounds_out, 0);
}

inline int bhsparse::csr_color_device(int n, int nnzS, const index_type *d_rowPtrS, const index_type *d_colIndS,
                                      const unsigned *d_prio, unsigned seed, int flags, index_type *d_color,
                                      index_type *d_order, index_type *d_colorPtr, int *ncolors_out, int *rounds_out)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_color_device(_h, n, nnzS, d_rowPtrS, d_colIndS, d_prio, seed, flags, d_color, d_order, d_colorPtr, ncolors_out,
                                rounds_out, 0);
}

inline int bhsparse::csr_gs_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA,
                                   const value_type *d_valA, const value_type *d_diag, int ncolors, const index_type *h_colorPtr,
                                   const index_type *d_order, const index_type *d_color, const value_type *d_b, value_type *d_x,
                                   double omega, int sweeps, int flags)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_gs_device(_h, n, nnzA, d_rowPtrA, d_colIndA, d_valA, d_diag, ncolors, h_colorPtr, d_order, d_color, d_b, d_x,
                             omega, sweeps, flags, 0);
}

inline int bhsparse::csr_levels_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA, int flags,
                                       index_type *d_level, index_type *d_order, index_type *d_levelPtr, int *nlevels_out,
                                       int *passes_out)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_levels_device(_h, n, nnzA, d_rowPtrA, d_colIndA, flags, d_level, d_order, d_levelPtr, nlevels_out, passes_out, 0);
}

inline int bhsparse::csr_trsv_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA,
                                     const value_type *d_valA, int nlevels, const index_type *h_levelPtr,
                                     const index_type *d_order, double alpha, const value_type *d_b, value_type *d_x, int flags)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_trsv_device(_h, n, nnzA, d_rowPtrA, d_colIndA, d_valA, nlevels, h_levelPtr, d_order, alpha, d_b, d_x, flags, 0);
}

inline int bhsparse::csr_ilu0_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA, value_type *d_valA,
                                     int nlevels, const index_type *h_levelPtr, const index_type *d_order, int flags,
                                     int *pivot_out)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_ilu0_device(_h, n, nnzA, d_rowPtrA, d_colIndA, d_valA, nlevels, h_levelPtr, d_order, flags, pivot_out, 0);
}

inline int bhsparse::csr_components_device(int n, int nnzS, const index_type *d_rowPtrS, const index_type *d_colIndS, int flags,
                                           index_type *d_root, index_type *d_comp, index_type *d_compSize, int *ncomp_out,
                                           int *passes_out)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_components_device(_h, n, nnzS, d_rowPtrS, d_colIndS, flags, d_root, d_comp, d_compSize, ncomp_out, passes_out, 0);
}

inline int bhsparse::csr_scc_device(int n, int nnzS, const index_type *d_rowPtrS, const index_type *d_colIndS, int flags,
                                    index_type *d_root, index_type *d_comp, index_type *d_compSize, int *nscc_out, int *rounds_out,
                                    int *passes_out)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_scc_device(_h, n, nnzS, d_rowPtrS, d_colIndS, flags, d_root, d_comp, d_compSize, nscc_out, rounds_out, passes_out, 0);
}

inline int bhsparse::csr_rcm_device(int n, int nnzS, const index_type *d_rowPtrS, const index_type *d_colIndS, int flags,
                                    index_type *d_perm, index_type *d_level, index_type *d_start, int *ncomp_out, int *depth_out,
                                    int *sweeps_out, int *passes_out)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_rcm_device(_h, n, nnzS, d_rowPtrS, d_colIndS, flags, d_perm, d_level, d_start, ncomp_out, depth_out, sweeps_out,
                              passes_out, 0);
}

inline int bhsparse::csr_kcore_device(int n, int nnzS, const index_type *d_rowPtrS, const index_type *d_colIndS, int flags,
                                      index_type *d_core, index_type *d_round, int *kmax_out, int *rounds_out)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_kcore_device(_h, n, nnzS, d_rowPtrS, d_colIndS, flags, d_core, d_round, kmax_out, rounds_out, 0);
}

inline int bhsparse::csr_sssp_device(int n, int nnzG, const index_type *d_rowPtrG, const index_type *d_colIndG,
                                     const value_type *d_valG, int nsrc, const index_type *d_sources, double delta, int flags,
                                     value_type *d_dist, index_type *d_parent, int *reached_out, int *passes_out)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_sssp_device(_h, n, nnzG, d_rowPtrG, d_colIndG, d_valG, nsrc, d_sources, delta, flags, d_dist, d_parent, reached_out,
                               passes_out, 0);
}

inline int bhsparse::csr_betweenness_device(int n, int nnzG, const index_type *d_rowPtrG, const index_type *d_colIndG, int nnzT,
                                            const index_type *d_rowPtrT, const index_type *d_colIndT, int nsrc,
                                            const index_type *d_sources, int flags, double *d_bc, index_type *d_level,
                                            double *d_sigma, int *reached_out, int *passes_out)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_betweenness_device(_h, n, nnzG, d_rowPtrG, d_colIndG, nnzT, d_rowPtrT, d_colIndT, nsrc, d_sources, flags, d_bc,
                                      d_level, d_sigma, reached_out, passes_out, 0);
}

inline int bhsparse::csr_match_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA,
                                      const value_type *d_valA, unsigned seed, int flags, index_type *d_mate, index_type *d_agg,
                                      int *npairs_out, int *rounds_out)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_match_device(_h, n, nnzA, d_rowPtrA, d_colIndA, d_valA, seed, flags, d_mate, d_agg, npairs_out, rounds_out, 0);
}

inline int bhsparse::csr_spanning_forest_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA,
                                                const value_type *d_valA, int flags, index_type *d_label, index_type *d_edgeLo,
                                                index_type *d_edgeHi, value_type *d_edgeVal, int *nedges_out, int *rounds_out)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_spanning_forest_device(_h, n, nnzA, d_rowPtrA, d_colIndA, d_valA, flags, d_label, d_edgeLo, d_edgeHi, d_edgeVal,
                                          nedges_out, rounds_out, 0);
}

inline int bhsparse::coo_assemble_device(int m, int n, int nnzIn, const index_type *d_rowInd, const index_type *d_colInd,
                                         const value_type *d_valIn, int flags, index_type *d_rowPtrZ, index_type *d_colIndZ,
                                         value_type *d_valZ, index_type *d_entryPtr, index_type *d_perm, int *nnzZ_out, int *nkept_out)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_coo_assemble_device(_h, m, n, nnzIn, d_rowInd, d_colInd, d_valIn, flags, d_rowPtrZ, d_colIndZ, d_valZ, d_entryPtr, d_perm,
                                   nnzZ_out, nkept_out, 0);
}

inline int bhsparse::coo_assemble_values_device(int nnzIn, const value_type *d_valIn, int nnzZ, const index_type *d_entryPtr,
                                                const index_type *d_perm, int flags, value_type *d_valZ)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_coo_assemble_values_device(_h, nnzIn, d_valIn, nnzZ, d_entryPtr, d_perm, flags, d_valZ, 0);
}

inline int bhsparse::csr_cfsplit_device(int n, int nnzS, const index_type *d_rowPtrS, const index_type *d_colIndS,
                                        const unsigned *d_prio, unsigned seed, int flags, index_type *d_cf, index_type *d_cpts,
                                        int *nc_out, int *rounds_out)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_cfsplit_device(_h, n, nnzS, d_rowPtrS, d_colIndS, d_prio, seed, flags, d_cf, d_cpts, nc_out, rounds_out, 0);
}

inline int bhsparse::csr_interp_symbolic_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA, int nnzS,
                                                const index_type *d_rowPtrS, const index_type *d_colIndS, const index_type *d_cf,
                                                int nc, index_type *d_rowPtrP, long long *nnzP_out)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_interp_symbolic_device(_h, n, nnzA, d_rowPtrA, d_colIndA, nnzS, d_rowPtrS, d_colIndS, d_cf, nc, d_rowPtrP, nnzP_out, 0);
}

inline int bhsparse::csr_interp_numeric_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA,
                                               const value_type *d_valA, int nnzS, const index_type *d_rowPtrS,
                                               const index_type *d_colIndS, const index_type *d_cf, int nc,
                                               const index_type *d_rowPtrP, long long nnzP, index_type *d_colIndP,
                                               value_type *d_valP)
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_csr_interp_numeric_device(_h, n, nnzA, d_rowPtrA, d_colIndA, d_valA, nnzS, d_rowPtrS, d_colIndS, d_cf, nc, d_rowPtrP,
                                         nnzP, d_colIndP, d_valP, 0, 0);
}

inline int bhsparse::get_nnzC()
{
    int v = 0;
    if (!_h || bhs_get_nnzC(_h, &v) != BHSPARSE_SUCCESS) return 0;
    return v;
}

inline int bhsparse::get_C(index_type *csrColIndC, value_type *csrValC)
{
    if (!_h) return BHS_ERR_NOT_READY;
    int err = bhs_get_C(_h, csrColIndC, csrValC);
    if (err == BHSPARSE_SUCCESS && _h_csrRowPtrC) err = bhs_get_rowptrC(_h, _h_csrRowPtrC);   // bhsparse_cuda.h:3016
    return err;
}

inline int bhsparse::free_mem()
{
    if (!_h) return BHS_ERR_NOT_READY;
    return bhs_free_data(_h);
}

inline int bhsparse::freePlatform()
{
    if (!_h) return BHSPARSE_SUCCESS;
    int err = bhs_destroy(_h);
    _h = 0;
    return err;
}

#endif
