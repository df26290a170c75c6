// bhs_host_semiring.inc.h -- the multiply over a semiring (bhs_spgemm_semiring[_masked[_device]], kernels in bhs_semiring.hip.h)
// (A part of bhsparse_hip.hip's translation unit: included there last.)
//
// The masked calls are bhs_spgemm_masked[_device] with another product and another reduction: the same driver (mask_drive), validation and
// binning pass (k_masked_scan), the same workspace and staging copies (the masked multiply's own: h->maskWs, h->maskM),
// the same bins and launch shapes -- so they leave the handle as the masked multiply does.  bhs_spgemm_semiring runs the
// ordinary multiply and then re-values its C in place, with M = C's own device arrays.
//
// The kernels' header is included here, not among the translation unit's kernel headers: it comes after every other piece
// of device and host code, so that nothing before it moves.
#include "bhs_semiring.hip.h"

namespace {

inline bool sr_known(int semiring) { return semiring >= BHS_SR_PLUS_TIMES && semiring <= BHS_SR_PLUS_PAIR; }

// The kernel set of a semiring S for mask_drive (bhs_host_masked.inc.h): the masked multiply's driver, bins and launch
// shapes.  In the long and the hub bin valC is handed over as cells (bhs_semiring.hip.h).
template <typename S>
struct SrKernels {
    static const char* family(int f)
    {
        static const char* const names[] = {"sr_scan", "sr_short", "sr_wave", "sr_long", "sr_hub"};
        return names[f];
    }
    template <int G, int CAP, int BLOCK>
    static void lds(const MaskLaunch& a, unsigned grid)
    {
        hipLaunchKernelGGL((k_sr_lds<S, G, CAP, BLOCK>), dim3(grid), dim3(BLOCK), 0, a.st, a.nq, a.q, a.Mp, a.Mj, a.Ap, a.Aj, a.Ax,
                           a.Bp, a.Bj, a.Bx, a.bSorted, a.valC);
    }
    static void long_rows(const MaskLaunch& a)
    {
        hipLaunchKernelGGL(k_sr_long<S>, dim3((unsigned)a.nq), dim3(256), 0, a.st, a.nq, a.q, a.Mp, a.Mj, a.Ap, a.Aj, a.Ax, a.Bp,
                           a.Bj, a.Bx, a.bSorted, (cell_t*)a.valC);
    }
    static int hub(const MaskLaunch& a, int parts, unsigned gy, int ldsCap)    // identity, products, decode
    {
        cell_t* cells = (cell_t*)a.valC;
        hipLaunchKernelGGL(k_sr_init<S>, dim3(gy), dim3(256), 0, a.st, a.nq, a.q, a.Mp, cells);
        hipLaunchKernelGGL(k_sr_hub<S>, dim3((unsigned)parts, gy), dim3(256), 0, a.st, a.nq, a.q, a.Mp, a.Mj, a.Ap, a.Aj, a.Ax,
                           a.Bp, a.Bj, a.Bx, a.bSorted, ldsCap, cells);
        hipLaunchKernelGGL(k_sr_decode<S>, dim3(gy), dim3(256), 0, a.st, a.nq, a.q, a.Mp, cells);
        return 3;
    }
};

template <typename S>
int sr_run(bhs_handle* h, const int* dMp, const int* dMj, int nnzM, value_t* dValC, bool keepStats, int64_t* nnzCt_out, double* ms_out)
{
    return mask_drive<SrKernels<S>>(h, dMp, dMj, nnzM, dValC, keepStats, nnzCt_out, ms_out);
}

int sr_dispatch(bhs_handle* h, int semiring, const int* dMp, const int* dMj, int nnzM, value_t* dValC, bool keepStats,
                int64_t* nnzCt_out, double* ms_out)
{
    switch (semiring) {
    case BHS_SR_MIN_PLUS: return sr_run<SrMinPlus>(h, dMp, dMj, nnzM, dValC, keepStats, nnzCt_out, ms_out);
    case BHS_SR_MAX_PLUS: return sr_run<SrMaxPlus>(h, dMp, dMj, nnzM, dValC, keepStats, nnzCt_out, ms_out);
    case BHS_SR_MAX_TIMES: return sr_run<SrMaxTimes>(h, dMp, dMj, nnzM, dValC, keepStats, nnzCt_out, ms_out);
    case BHS_SR_MIN_MAX: return sr_run<SrMinMaxS>(h, dMp, dMj, nnzM, dValC, keepStats, nnzCt_out, ms_out);
    case BHS_SR_MAX_MIN: return sr_run<SrMaxMin>(h, dMp, dMj, nnzM, dValC, keepStats, nnzCt_out, ms_out);
    case BHS_SR_OR_AND: return sr_run<SrOrAnd>(h, dMp, dMj, nnzM, dValC, keepStats, nnzCt_out, ms_out);
    case BHS_SR_PLUS_PAIR: return sr_run<SrPlusPair>(h, dMp, dMj, nnzM, dValC, keepStats, nnzCt_out, ms_out);
    default: return BHS_ERR_INVALID_ARG;
    }
}

}  // namespace

extern "C" {

int bhs_spgemm_semiring_masked_device(bhs_handle* h, int semiring, const int* d_rowPtrM, const int* d_colIndM, int nnzM,
                                      bhs_value_t* d_valC, int64_t* nnzCt_out, double* ms_out)
{
    BHS_TRY(masked_check(h, nnzM));
    if (!sr_known(semiring)) return BHS_ERR_INVALID_ARG;
    if (semiring == BHS_SR_PLUS_TIMES) return bhs_spgemm_masked_device(h, d_rowPtrM, d_colIndM, nnzM, d_valC, nnzCt_out, ms_out);
    if (!d_rowPtrM || (nnzM > 0 && (!d_colIndM || !d_valC))) return BHS_ERR_INVALID_ARG;
    return guarded(h, [&] { return sr_dispatch(h, semiring, d_rowPtrM, d_colIndM, nnzM, (value_t*)d_valC, false, nnzCt_out, ms_out); });
}

int bhs_spgemm_semiring_masked(bhs_handle* h, int semiring, const int* rowPtrM, const int* colIndM, int nnzM, bhs_value_t* valC,
                               int64_t* nnzCt_out, double* ms_out)
{
    BHS_TRY(masked_check(h, nnzM));
    if (!sr_known(semiring)) return BHS_ERR_INVALID_ARG;
    if (semiring == BHS_SR_PLUS_TIMES) return bhs_spgemm_masked(h, rowPtrM, colIndM, nnzM, valC, nnzCt_out, ms_out);
    if (!rowPtrM || (nnzM > 0 && (!colIndM || !valC))) return BHS_ERR_INVALID_ARG;
    return guarded(h, [&] {
        return mask_staged(h, rowPtrM, colIndM, nnzM, valC, [&](const int* dMp, const int* dMj, value_t* dValC) {
            return sr_dispatch(h, semiring, dMp, dMj, nnzM, dValC, false, nnzCt_out, ms_out);
        });
    });
}

int bhs_spgemm_semiring(bhs_handle* h, int semiring, int* rowPtrC_out, int64_t* nnzCt_out, int* nnzC_out, double ms_out[2])
{
    if (!h) return BHS_ERR_INVALID_ARG;
    if (!sr_known(semiring)) return BHS_ERR_INVALID_ARG;             // (before anything is started: the last C stands)
    if (!h->hasData) return BHS_ERR_NOT_READY;
    if (h->ps.open || h->extCj) return BHS_ERR_INVALID_ARG;          // (as bhs_spgemm_add: a split multiply owns the stream; bound output arrays are the caller's)
    return guarded(h, [&]() -> int {
        double stage[4] = {0, 0, 0, 0};
        BHS_TRY(bhs_spgemm(h, rowPtrC_out, nnzCt_out, nnzC_out, stage));
        double srMs = 0;
        if (semiring != BHS_SR_PLUS_TIMES && h->nnzC > 0) {
            const int rc = sr_dispatch(h, semiring, (const int*)h->Cp.p, (const int*)h->Cj.p, (int)h->nnzC, (value_t*)h->Cx.p, true,
                                       nullptr, &srMs);
            if (rc) return rc == BHS_ERR_INVALID_ARG ? (int)BHS_ERR_INTERNAL : rc;   // (C's own pattern did not pass the mask's validation)
        }
        if (ms_out) { ms_out[0] = stage[0] + stage[1] + stage[2] + stage[3]; ms_out[1] = srMs; }
        return BHS_SUCCESS;
    });
}

}  // extern "C"
