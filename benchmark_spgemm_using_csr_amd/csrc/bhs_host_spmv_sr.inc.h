// bhs_host_spmv_sr.inc.h -- semiring CSR x dense with mask and accumulate (bhs_csr_spmv_semiring_device,
// bhs_csr_spmm_semiring_device; kernels in bhs_spmv_sr.hip.h)
// (A part of bhsparse_hip.hip's translation unit: included there directly after bhs_host_spmv.inc.h, whose mv_bytes it uses.
// It comes ahead of the semiring multiply's host part and uses nothing of bhs_semiring.hip.h: the rule of the eight
// semirings is restated below as (what combines, what multiplies, the identity).)
//
// The body is mv_run's with a workspace of its own (h->srmvWs: its control block is longer by the 64-bit count of changed
// elements, and a workspace's pinned mirror is sized once) and one more thing read in the final round trip: that count.
// The vector call is the k = 1, ld = 1 case.
#include "bhs_spmv_sr.hip.h"

namespace {

struct SmvIn {
    SmvDims d;
    int kind;
    const int* Ap; const int* Aj; const value_t* Ax;
    const value_t* X; const value_t* M; value_t* Y;
};

// the three kernels of one way to combine and one column tile
struct SmvKernels {
    void (*rowsShort)(SmvDims, const int*, const int*, const value_t*, const value_t*, const value_t*, value_t*, int*, int*);
    void (*rowsWave)(int, const int*, SmvDims, const int*, const int*, const value_t*, const value_t*, const value_t*, value_t*, int*);
    void (*rowsLong)(int, const int*, SmvDims, const int*, const int*, const value_t*, const value_t*, const value_t*, value_t*, int*);
};

template <int KIND, int T> SmvKernels smv_tile() { return {k_smv_short<KIND, T>, k_smv_wave<KIND, T>, k_smv_long<KIND, T>}; }

// the narrowest tile that holds k columns; the widest beyond it (the kernels loop over its tiles)
template <int KIND> SmvKernels smv_tiles(int k)
{
    if (k <= 1) return smv_tile<KIND, 1>();
    if (k <= 2) return smv_tile<KIND, 2>();
    if (k <= 4) return smv_tile<KIND, 4>();
    if (k <= 8) return smv_tile<KIND, 8>();
    if (k <= 16) return smv_tile<KIND, 16>();
    if (k <= 32) return smv_tile<KIND, 32>();
    return smv_tile<KIND, 64>();
}

SmvKernels smv_kernels(int kind, int k)
{
    return kind == kRdSum ? smv_tiles<kRdSum>(k) : kind == kRdMin ? smv_tiles<kRdMin>(k) : smv_tiles<kRdMax>(k);
}

// the table of include/bhsparse_hip.h, "semiring multiply": false for an unknown semiring
bool smv_rule(int semiring, int& kind, int& mult, rd_u64& id)
{
    const double inf = __builtin_inf();
    switch (semiring) {
    case BHS_SR_PLUS_TIMES: kind = kRdSum; mult = kSmvTimes; id = rd_bits(0.0); return true;
    case BHS_SR_MIN_PLUS:   kind = kRdMin; mult = kSmvPlus;  id = rd_key(inf, false); return true;
    case BHS_SR_MAX_PLUS:   kind = kRdMax; mult = kSmvPlus;  id = rd_key(-inf, true); return true;
    case BHS_SR_MAX_TIMES:  kind = kRdMax; mult = kSmvTimes; id = rd_key(-inf, true); return true;
    case BHS_SR_MIN_MAX:    kind = kRdMin; mult = kSmvMax;   id = rd_key(inf, false); return true;
    case BHS_SR_MAX_MIN:    kind = kRdMax; mult = kSmvMin;   id = rd_key(-inf, true); return true;
    case BHS_SR_OR_AND:     kind = kRdMax; mult = kSmvAnd;   id = rd_key(0.0, true); return true;    // or: max over {0, 1}
    case BHS_SR_PLUS_PAIR:  kind = kRdSum; mult = kSmvPair;  id = rd_bits(0.0); return true;
    }
    return false;
}

int smv_run(bhs_handle* h, const SmvIn& in, long long* changed_out, double* ms_out)
{
    const SmvDims& d = in.d;
    SideWs& ws = h->srmvWs;
    BHS_TRY(side_open(h, ws, SMV_INTS, sizeof(int) * 2 * (size_t)std::max(d.m, 1), 0));
    BHS_TRY(side_start(h, ws));
    int* ctl = (int*)ws.ctl.p;
    int* queue = (int*)ws.queue.p;
    const SmvKernels kern = smv_kernels(in.kind, d.k);
    const unsigned gShort = (unsigned)std::max<long long>(1, ((long long)d.m + kRdRows - 1) / kRdRows);
    BHS_TRY(timed(h, "srmv_short", d.m, [&] {
        hipLaunchKernelGGL(kern.rowsShort, dim3(gShort), dim3(256), 0, h->stream, d, in.Ap, in.Aj, in.Ax, in.X, in.M, in.Y, ctl, queue);
        return 1;
    }));
    if (d.nnzA > kRdShortL) {                                        // (else no row can be longer)
        BHS_TRY(side_read_ctl(h, ws, RD_INTS));
        if (ws.host[RD_ERR]) return BHS_ERR_INVALID_ARG;
        if (const int nq = ws.host[RD_CNT_WAVE]) {
            BHS_TRY(timed(h, "srmv_wave", nq, [&] {
                hipLaunchKernelGGL(kern.rowsWave, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, h->stream, nq,
                                   queue + (size_t)RD_CNT_WAVE * d.m, d, in.Ap, in.Aj, in.Ax, in.X, in.M, in.Y, ctl);
                return 1;
            }));
        }
        if (const int nq = ws.host[RD_CNT_LONG]) {
            BHS_TRY(timed(h, "srmv_long", nq, [&] {
                hipLaunchKernelGGL(kern.rowsLong, dim3((unsigned)std::min<long long>(nq, (long long)h->numCU * 8)), dim3(256), 0,
                                   h->stream, nq, queue + (size_t)RD_CNT_LONG * d.m, d, in.Ap, in.Aj, in.Ax, in.X, in.M, in.Y, ctl);
                return 1;
            }));
        }
    }
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, SMV_INTS));                          // the error word and the count, one round trip
    BHS_TRY(side_close(h, ws, ms_out));
    if (ws.host[RD_ERR]) return BHS_ERR_INVALID_ARG;
    if (changed_out) memcpy(changed_out, ws.host + SMV_CHANGED, sizeof(long long));
    return BHS_SUCCESS;
}

int smv_call(bhs_handle* h, int semiring, int m, int n, int nnzA, const bhs_value_t* d_valA, const int* d_rowPtrA,
             const int* d_colIndA, int k, const bhs_value_t* d_X, long long ldX, int flags, const bhs_value_t* d_M, long long ldM,
             bhs_value_t* d_Y, long long ldY, long long* changed_out, double* ms_out)
{
    if (!h || h->ps.open || m < 0 || n < 0 || nnzA < 0 || !d_rowPtrA) return BHS_ERR_INVALID_ARG;
    if (k < 1 || ldX < k || ldY < k) return BHS_ERR_INVALID_ARG;
    if (nnzA > 0 && (!d_colIndA || !d_X)) return BHS_ERR_INVALID_ARG;
    if (m > 0 && !d_Y) return BHS_ERR_INVALID_ARG;
    SmvIn in;
    if (!smv_rule(semiring, in.kind, in.d.mult, in.d.id)) return BHS_ERR_INVALID_ARG;
    if (flags & ~(BHS_MV_ACCUM | BHS_MV_MASK_COMPLEMENT)) return BHS_ERR_INVALID_ARG;
    if (d_M ? ldM < k : (flags & BHS_MV_MASK_COMPLEMENT) != 0) return BHS_ERR_INVALID_ARG;
    const size_t yBytes = mv_bytes(m, k, ldY);
    if (side_aliased({{d_Y, yBytes}}, {{d_rowPtrA, sizeof(int) * ((size_t)m + 1)}, {d_colIndA, sizeof(int) * (size_t)nnzA},
                                       {d_valA, sizeof(value_t) * (size_t)nnzA}, {d_X, mv_bytes(n, k, ldX)},
                                       {d_M, d_M ? mv_bytes(m, k, ldM) : 0}}))
        return BHS_ERR_INVALID_ARG;                                  // (M may overlap X: both are inputs)
    in.d.m = m; in.d.n = n; in.d.nnzA = nnzA; in.d.k = k; in.d.ldX = ldX; in.d.ldM = d_M ? ldM : 0; in.d.ldY = ldY;
    in.d.flags = flags | (changed_out ? kSmvCount : 0);              // (no count where nobody reads it)
    in.Ap = d_rowPtrA; in.Aj = d_colIndA; in.Ax = (const value_t*)d_valA; in.X = (const value_t*)d_X;
    in.M = (const value_t*)d_M; in.Y = (value_t*)d_Y;
    return guarded(h, [&] { return smv_run(h, in, changed_out, ms_out); });
}

}  // namespace

extern "C" {

int bhs_csr_spmv_semiring_device(bhs_handle* h, int semiring, int m, int n, int nnzA, const bhs_value_t* d_valA,
                                 const int* d_rowPtrA, const int* d_colIndA, const bhs_value_t* d_x, int flags,
                                 const bhs_value_t* d_mask, bhs_value_t* d_y, long long* changed_out, double* ms_out)
{
    return smv_call(h, semiring, m, n, nnzA, d_valA, d_rowPtrA, d_colIndA, 1, d_x, 1, flags, d_mask, 1, d_y, 1, changed_out, ms_out);
}

int bhs_csr_spmm_semiring_device(bhs_handle* h, int semiring, int m, int n, int nnzA, const bhs_value_t* d_valA,
                                 const int* d_rowPtrA, const int* d_colIndA, int k, const bhs_value_t* d_X, long long ldX,
                                 int flags, const bhs_value_t* d_M, long long ldM, bhs_value_t* d_Y, long long ldY,
                                 long long* changed_out, double* ms_out)
{
    return smv_call(h, semiring, m, n, nnzA, d_valA, d_rowPtrA, d_colIndA, k, d_X, ldX, flags, d_M, ldM, d_Y, ldY, changed_out,
                    ms_out);
}

}  // extern "C"
