// bhs_host_fsai.inc.h -- the factorised sparse approximate inverse (bhs_csr_fsai_device; kernels in bhs_fsai.hip.h)
// (A part of bhsparse_hip.hip's translation unit: included there after the sampled product.  The control words and the
// error flag are the reductions'; the bins -- 16, 64 and 128 unknowns a row -- and the queues' filling are the kernels'
// own.)
//
// Like the sampled product the call works beside the pipeline: its workspace (h->fsWs: counters, the queues of the rows
// beyond the short bin, events, the pinned mirror; set up and read by bhs_host_side.inc.h) is a buffer of its own from the
// grow-only pool.  It binds nothing and serves nothing through the getters: the output array is the caller's.  One round
// trip for the queues' lengths, where a row can be longer than the short bin, and the one that ends the call.  A row's work
// is bounded by its 128 unknowns, so no grid is capped and no kernel loops over blocks: a workgroup per 16 rows, per 4 rows
// and per row.
//
// The kernels' header is included here, not among the translation unit's kernel headers (as bhs_host_sddmm.inc.h does).
#include "bhs_fsai.hip.h"

namespace {

struct FsIn {
    FsDims d;
    const int* Ap; const int* Aj; const value_t* Ax;
    const int* Gp; const int* Gj; value_t* Gx;
};

int fs_run(bhs_handle* h, const FsIn& in, int* bad_row_out, double* ms_out)
{
    const FsDims& d = in.d;
    SideWs& ws = h->fsWs;
    BHS_TRY(side_open(h, ws, FS_INTS, sizeof(int) * 2 * (size_t)d.n, 0));
    int* ctl = (int*)ws.ctl.p;
    int* queue = (int*)ws.queue.p;
    BHS_HIP(hipMemsetD32Async((hipDeviceptr_t)(ctl + FS_BAD_ROW), 0x7fffffff, 1, h->stream));
    BHS_TRY(side_start(h, ws));
    BHS_TRY(timed(h, "fsai_short", d.n, [&] {
        hipLaunchKernelGGL(k_fsai_short, dim3((unsigned)(((long long)d.n + kFsRows - 1) / kFsRows)), dim3(256), 0, h->stream, d, in.Ap,
                           in.Aj, in.Ax, in.Gp, in.Gj, in.Gx, ctl, queue);
        return 1;
    }));
    if (d.nnzG > kFsShortD) {                                        // (else no row can be longer)
        BHS_TRY(side_read_ctl(h, ws, FS_INTS));
        if (ws.host[RD_ERR]) return BHS_ERR_INVALID_ARG;
        if (const int nq = ws.host[RD_CNT_WAVE]) {
            BHS_TRY(timed(h, "fsai_wave", nq, [&] {
                hipLaunchKernelGGL(k_fsai_wave, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, h->stream, nq,
                                   queue + (size_t)RD_CNT_WAVE * d.n, d, in.Ap, in.Aj, in.Ax, in.Gp, in.Gj, in.Gx, ctl);
                return 1;
            }));
        }
        if (const int nq = ws.host[RD_CNT_LONG]) {
            BHS_TRY(timed(h, "fsai_long", nq, [&] {
                hipLaunchKernelGGL(k_fsai_long, dim3((unsigned)nq), dim3(256), 0, h->stream, nq, queue + (size_t)RD_CNT_LONG * d.n, d,
                                   in.Ap, in.Aj, in.Ax, in.Gp, in.Gj, in.Gx, ctl);
                return 1;
            }));
        }
    }
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, FS_INTS));
    BHS_TRY(side_close(h, ws, ms_out));
    if (ws.host[RD_ERR]) return BHS_ERR_INVALID_ARG;
    if (bad_row_out) *bad_row_out = ws.host[FS_BAD_ROW] == 0x7fffffff ? -1 : ws.host[FS_BAD_ROW];
    return BHS_SUCCESS;
}

}  // namespace

extern "C" {

int bhs_csr_fsai_device(bhs_handle* h, int n, int nnzA, const int* d_rowPtrA, const int* d_colIndA, const bhs_value_t* d_valA,
                        int nnzG, const int* d_rowPtrG, const int* d_colIndG, bhs_value_t* d_valG, int flags, int* bad_row_out,
                        double* ms_out)
{
    if (!h || h->ps.open || n < 0 || nnzA < 0 || nnzG < 0 || flags != 0 || nnzG < n) return BHS_ERR_INVALID_ARG;
    if (n > 0 && (!d_rowPtrA || !d_colIndA || !d_valA || !d_rowPtrG || !d_colIndG || !d_valG)) return BHS_ERR_INVALID_ARG;
    const size_t rp = sizeof(int) * ((size_t)n + 1);
    if (side_aliased({{d_valG, sizeof(value_t) * (size_t)nnzG}},
                     {{d_rowPtrA, rp}, {d_colIndA, sizeof(int) * (size_t)nnzA}, {d_valA, sizeof(value_t) * (size_t)nnzA},
                      {d_rowPtrG, rp}, {d_colIndG, sizeof(int) * (size_t)nnzG}}))
        return BHS_ERR_INVALID_ARG;
    if (n == 0) {                                                    // nothing to do, nothing launched
        if (bad_row_out) *bad_row_out = -1;
        return side_nothing(nullptr, nullptr, ms_out);
    }
    FsIn in;
    in.d.n = n; in.d.nnzA = nnzA; in.d.nnzG = nnzG;
    in.Ap = d_rowPtrA; in.Aj = d_colIndA; in.Ax = (const value_t*)d_valA;
    in.Gp = d_rowPtrG; in.Gj = d_colIndG; in.Gx = (value_t*)d_valG;
    return guarded(h, [&] { return fs_run(h, in, bad_row_out, ms_out); });
}

}  // extern "C"
