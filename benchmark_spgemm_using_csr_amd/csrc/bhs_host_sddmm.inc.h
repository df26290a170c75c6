// bhs_host_sddmm.inc.h -- the sampled dense-dense product (bhs_csr_sddmm_device; kernels in bhs_sddmm.hip.h)
// (A part of bhsparse_hip.hip's translation unit: included there after the relaxation; mv_bytes is bhs_host_spmv.inc.h's.
// The bins, the control words and the queues are the reductions' -- the kernels' header brings bhs_reduce.hip.h with it.)
//
// Like CSR x dense the call works beside the pipeline: its workspace (h->sdWs: counters, the queues of the rows beyond the
// short bin, events, the pinned mirror; set up and read by bhs_host_side.inc.h) is a buffer of its own from the grow-only
// pool.  It binds nothing and serves nothing through the getters: the output array is the caller's.  One round trip for the
// queues' lengths, where a row can be longer than the short bin, and the one that ends the call.
//
// The kernels' header is included here, not among the translation unit's kernel headers (as bhs_host_spmv.inc.h does).
#include "bhs_sddmm.hip.h"

namespace {

struct SdIn {
    SdDims d;
    const int* Mp; const int* Mj; const value_t* Mx;
    const value_t* X; const value_t* Y; value_t* Zx;
};

// the three kernels of one tile
struct SdKernels {
    void (*rowsShort)(SdDims, const int*, const int*, const value_t*, const value_t*, const value_t*, value_t*, int*, int*);
    void (*rowsWave)(int, const int*, SdDims, const int*, const int*, const value_t*, const value_t*, const value_t*, value_t*, int*);
    void (*rowsLong)(int, const int*, SdDims, const int*, const int*, const value_t*, const value_t*, const value_t*, value_t*, int*);
};

template <int T> SdKernels sd_tile() { return {k_sd_short<T>, k_sd_wave<T>, k_sd_long<T>}; }

// T = min(64, the smallest power of two >= k): the contract's tile, not a tuning choice (it fixes the order of the sums)
SdKernels sd_kernels(int k)
{
    if (k <= 1) return sd_tile<1>();
    if (k <= 2) return sd_tile<2>();
    if (k <= 4) return sd_tile<4>();
    if (k <= 8) return sd_tile<8>();
    if (k <= 16) return sd_tile<16>();
    if (k <= 32) return sd_tile<32>();
    return sd_tile<64>();
}

int sd_run(bhs_handle* h, const SdIn& in, double* ms_out)
{
    const SdDims& d = in.d;
    SideWs& ws = h->sdWs;
    BHS_TRY(side_open(h, ws, RD_INTS, sizeof(int) * 2 * (size_t)std::max(d.m, 1), 0));
    BHS_TRY(side_start(h, ws));
    int* ctl = (int*)ws.ctl.p;
    int* queue = (int*)ws.queue.p;
    const SdKernels kern = sd_kernels(d.k);
    const unsigned gShort = (unsigned)std::max<long long>(1, ((long long)d.m + kRdRows - 1) / kRdRows);
    BHS_TRY(timed(h, "sddmm_short", d.m, [&] {
        hipLaunchKernelGGL(kern.rowsShort, dim3(gShort), dim3(256), 0, h->stream, d, in.Mp, in.Mj, in.Mx, in.X, in.Y, in.Zx, ctl, queue);
        return 1;
    }));
    if (d.nnzM > kRdShortL) {                                        // (else no row can be longer)
        BHS_TRY(side_read_ctl(h, ws, RD_INTS));
        if (ws.host[RD_ERR]) return BHS_ERR_INVALID_ARG;
        if (const int nq = ws.host[RD_CNT_WAVE]) {
            BHS_TRY(timed(h, "sddmm_wave", nq, [&] {
                hipLaunchKernelGGL(kern.rowsWave, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, h->stream, nq,
                                   queue + (size_t)RD_CNT_WAVE * d.m, d, in.Mp, in.Mj, in.Mx, in.X, in.Y, in.Zx, ctl);
                return 1;
            }));
        }
        if (const int nq = ws.host[RD_CNT_LONG]) {
            BHS_TRY(timed(h, "sddmm_long", nq, [&] {
                hipLaunchKernelGGL(kern.rowsLong, dim3((unsigned)std::min<long long>(nq, (long long)h->numCU * 8)), dim3(256), 0,
                                   h->stream, nq, queue + (size_t)RD_CNT_LONG * d.m, d, in.Mp, in.Mj, in.Mx, in.X, in.Y, in.Zx, ctl);
                return 1;
            }));
        }
    }
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, RD_INTS));
    BHS_TRY(side_close(h, ws, ms_out));
    return ws.host[RD_ERR] ? (int)BHS_ERR_INVALID_ARG : (int)BHS_SUCCESS;
}

}  // namespace

extern "C" {

int bhs_csr_sddmm_device(bhs_handle* h, int m, int n, int nnzM, const bhs_value_t* d_valM, const int* d_rowPtrM,
                         const int* d_colIndM, int k, double alpha, const bhs_value_t* d_X, long long ldX, const bhs_value_t* d_Y,
                         long long ldY, double beta, bhs_value_t* d_valZ, unsigned flags, double* ms_out)
{
    if (!h || h->ps.open || m < 0 || n < 0 || nnzM < 0 || !d_rowPtrM) return BHS_ERR_INVALID_ARG;
    if (k < 1 || ldX < k || ldY < k || (flags & ~BHS_SDDMM_TIMES_M)) return BHS_ERR_INVALID_ARG;
    const bool timesM = (flags & BHS_SDDMM_TIMES_M) != 0;
    if (nnzM > 0 && (!d_colIndM || !d_X || !d_Y || !d_valZ || (timesM && !d_valM))) return BHS_ERR_INVALID_ARG;
    const size_t zBytes = sizeof(value_t) * (size_t)nnzM;
    const void* valM = (const void*)d_valZ == (const void*)d_valM ? nullptr : d_valM;   // (in place on valM exactly, or apart from every input)
    if (side_aliased({{d_valZ, zBytes}}, {{d_rowPtrM, sizeof(int) * ((size_t)m + 1)}, {d_colIndM, sizeof(int) * (size_t)nnzM},
                                          {valM, zBytes}, {d_X, mv_bytes(m, k, ldX)}, {d_Y, mv_bytes(n, k, ldY)}}))
        return BHS_ERR_INVALID_ARG;
    SdIn in;
    in.d.m = m; in.d.n = n; in.d.nnzM = nnzM; in.d.k = k; in.d.ldX = ldX; in.d.ldY = ldY; in.d.alpha = alpha; in.d.beta = beta;
    in.d.timesM = timesM ? 1 : 0;
    in.Mp = d_rowPtrM; in.Mj = d_colIndM; in.Mx = timesM ? (const value_t*)d_valM : nullptr;
    in.X = (const value_t*)d_X; in.Y = (const value_t*)d_Y; in.Zx = (value_t*)d_valZ;
    return guarded(h, [&] { return sd_run(h, in, ms_out); });
}

}  // extern "C"
