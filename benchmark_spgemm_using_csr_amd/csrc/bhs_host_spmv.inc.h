// bhs_host_spmv.inc.h -- CSR x dense (bhs_csr_spmv_device, bhs_csr_spmm_device; kernels in bhs_spmv.hip.h)
// (A part of bhsparse_hip.hip's translation unit: included there after the selection.  The bins, the control words and the
// queues are the reductions' -- the kernels' header brings bhs_reduce.hip.h with it.)
//
// Like the reductions both calls work beside the pipeline: their workspace (h->mvWs: counters, the queues of the rows
// beyond the short bin, events, the pinned mirror; set up and read by bhs_host_side.inc.h) is a buffer of its own from the
// grow-only pool.  They bind nothing and serve nothing through the getters: the output array is the caller's.  The vector
// product is the k = 1, ld = 1 case of the one body here.
//
// The kernels' header is included here, not among the translation unit's kernel headers (as bhs_host_reduce.inc.h does).
#include "bhs_spmv.hip.h"

namespace {

struct MvIn {
    MvDims d;
    const int* Ap; const int* Aj; const value_t* Ax;
    const value_t* X; value_t* Y;
};

// the three kernels of one column tile
struct MvKernels {
    void (*rowsShort)(MvDims, const int*, const int*, const value_t*, const value_t*, value_t*, int*, int*);
    void (*rowsWave)(int, const int*, MvDims, const int*, const int*, const value_t*, const value_t*, value_t*, int*);
    void (*rowsLong)(int, const int*, MvDims, const int*, const int*, const value_t*, const value_t*, value_t*, int*);
};

template <int T> MvKernels mv_tile() { return {k_mv_short<T>, k_mv_wave<T>, k_mv_long<T>}; }

// the narrowest tile that holds k columns; the widest beyond it (the kernels loop over its tiles)
MvKernels mv_kernels(int k)
{
    if (k <= 1) return mv_tile<1>();
    if (k <= 2) return mv_tile<2>();
    if (k <= 4) return mv_tile<4>();
    if (k <= 8) return mv_tile<8>();
    if (k <= 16) return mv_tile<16>();
    if (k <= 32) return mv_tile<32>();
    return mv_tile<64>();
}

int mv_run(bhs_handle* h, const MvIn& in, double* ms_out)
{
    const MvDims& d = in.d;
    SideWs& ws = h->mvWs;
    BHS_TRY(side_open(h, ws, RD_INTS, sizeof(int) * 2 * (size_t)std::max(d.m, 1), 0));
    BHS_TRY(side_start(h, ws));
    int* ctl = (int*)ws.ctl.p;
    int* queue = (int*)ws.queue.p;
    const MvKernels kern = mv_kernels(d.k);
    const bool vec = d.k == 1;
    const unsigned gShort = (unsigned)std::max<long long>(1, ((long long)d.m + kRdRows - 1) / kRdRows);
    BHS_TRY(timed(h, vec ? "spmv_short" : "spmm_short", d.m, [&] {
        hipLaunchKernelGGL(kern.rowsShort, dim3(gShort), dim3(256), 0, h->stream, d, in.Ap, in.Aj, in.Ax, in.X, in.Y, ctl, queue);
        return 1;
    }));
    if (d.nnzA > kRdShortL) {                                        // (else no row can be longer)
        BHS_TRY(side_read_ctl(h, ws, RD_INTS));
        if (ws.host[RD_ERR]) return BHS_ERR_INVALID_ARG;
        if (const int nq = ws.host[RD_CNT_WAVE]) {
            BHS_TRY(timed(h, vec ? "spmv_wave" : "spmm_wave", nq, [&] {
                hipLaunchKernelGGL(kern.rowsWave, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, h->stream, nq,
                                   queue + (size_t)RD_CNT_WAVE * d.m, d, in.Ap, in.Aj, in.Ax, in.X, in.Y, ctl);
                return 1;
            }));
        }
        if (const int nq = ws.host[RD_CNT_LONG]) {
            BHS_TRY(timed(h, vec ? "spmv_long" : "spmm_long", nq, [&] {
                hipLaunchKernelGGL(kern.rowsLong, dim3((unsigned)std::min<long long>(nq, (long long)h->numCU * 8)), dim3(256), 0,
                                   h->stream, nq, queue + (size_t)RD_CNT_LONG * d.m, d, in.Ap, in.Aj, in.Ax, in.X, in.Y, ctl);
                return 1;
            }));
        }
    }
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, RD_INTS));
    BHS_TRY(side_close(h, ws, ms_out));
    return ws.host[RD_ERR] ? (int)BHS_ERR_INVALID_ARG : (int)BHS_SUCCESS;
}

// bytes of a rows x k row-major array of leading dimension ld: up to its last element
size_t mv_bytes(int rows, int k, long long ld)
{
    return rows > 0 ? sizeof(value_t) * ((size_t)(rows - 1) * (size_t)ld + (size_t)k) : 0;
}

int mv_call(bhs_handle* h, int m, int n, int nnzA, const bhs_value_t* d_valA, const int* d_rowPtrA, const int* d_colIndA, int k,
            double alpha, const bhs_value_t* d_X, long long ldX, double beta, bhs_value_t* d_Y, long long ldY, double* ms_out)
{
    if (!h || h->ps.open || m < 0 || n < 0 || nnzA < 0 || !d_rowPtrA) return BHS_ERR_INVALID_ARG;
    if (k < 1 || ldX < k || ldY < k) return BHS_ERR_INVALID_ARG;
    if (nnzA > 0 && (!d_colIndA || !d_X)) return BHS_ERR_INVALID_ARG;
    if (m > 0 && !d_Y) return BHS_ERR_INVALID_ARG;
    const size_t yBytes = mv_bytes(m, k, ldY);
    if (side_aliased({{d_Y, yBytes}}, {{d_rowPtrA, sizeof(int) * ((size_t)m + 1)}, {d_colIndA, sizeof(int) * (size_t)nnzA},
                                       {d_valA, sizeof(value_t) * (size_t)nnzA}, {d_X, mv_bytes(n, k, ldX)}}))
        return BHS_ERR_INVALID_ARG;
    MvIn in;
    in.d.m = m; in.d.n = n; in.d.nnzA = nnzA; in.d.k = k; in.d.ldX = ldX; in.d.ldY = ldY; in.d.alpha = alpha; in.d.beta = beta;
    in.Ap = d_rowPtrA; in.Aj = d_colIndA; in.Ax = (const value_t*)d_valA; in.X = (const value_t*)d_X; in.Y = (value_t*)d_Y;
    return guarded(h, [&] { return mv_run(h, in, ms_out); });
}

}  // namespace

extern "C" {

int bhs_csr_spmv_device(bhs_handle* h, int m, int n, int nnzA, const bhs_value_t* d_valA, const int* d_rowPtrA,
                        const int* d_colIndA, double alpha, const bhs_value_t* d_x, double beta, bhs_value_t* d_y, double* ms_out)
{
    return mv_call(h, m, n, nnzA, d_valA, d_rowPtrA, d_colIndA, 1, alpha, d_x, 1, beta, d_y, 1, ms_out);
}

int bhs_csr_spmm_device(bhs_handle* h, int m, int n, int nnzA, const bhs_value_t* d_valA, const int* d_rowPtrA,
                        const int* d_colIndA, int k, double alpha, const bhs_value_t* d_X, long long ldX, double beta,
                        bhs_value_t* d_Y, long long ldY, double* ms_out)
{
    return mv_call(h, m, n, nnzA, d_valA, d_rowPtrA, d_colIndA, k, alpha, d_X, ldX, beta, d_Y, ldY, ms_out);
}

}  // extern "C"
