// bhs_host_push_sr.inc.h -- sparse frontier x CSR over a semiring, the push direction (bhs_csr_push_semiring_device;
// kernels in bhs_push_sr.hip.h)
// (A part of bhsparse_hip.hip's translation unit: included there directly after bhs_host_spmv_sr.inc.h, whose smv_rule and
// whose mv_bytes it uses.)
//
// A workspace of its own (h->pushWs): the control block of bhs_push_sr.hip.h, the two bitmaps in its queue buffer (the row
// map, 64 rows a word, then the changed elements' bits), the counts of its two scans -- the frontier's degrees, then the row
// map's words -- in its count buffer, one after the other; the scanned offsets go to h->pushOff.  The call makes ONE round
// trip, at its end, for the error word and the two counts: the edge pass takes the number of entries from the control block
// on the device, and its grid is sized from what the host knows (nnzG, nf) -- a run loop, so any grid is a correct one.

#include "bhs_push_sr.hip.h"

namespace {

struct PuIn {
    PuDims d;
    int kind;
    const int* Gp; const int* Gj; const value_t* Gx;
    const int* fidx;
    const value_t* F; const value_t* M; value_t* Y;
    int* next;
};

constexpr SideScanWords kPuScanDeg = {PU_TICKET_A, PU_TOTAL_A, PU_BINS_A, PU_MAXCNT_A};
constexpr SideScanWords kPuScanRows = {PU_TICKET_B, PU_TOTAL_B, PU_BINS_B, PU_MAXCNT_B};

int pu_run(bhs_handle* h, const PuIn& in, int* next_count_out, long long* changed_out, double* ms_out)
{
    const PuDims& d = in.d;
    SideWs& ws = h->pushWs;
    const size_t nWords = ((size_t)d.n + 63) / 64;                    // of the row map
    const size_t rowBytes = in.next ? sizeof(rd_u64) * nWords : 0;
    const size_t bitBytes = changed_out ? sizeof(unsigned) * (((size_t)d.n * (size_t)d.k + 31) / 32) : 0;
    const size_t scanned = std::max<size_t>((size_t)d.nf, in.next ? nWords : 0) + 1;
    BHS_TRY(side_open(h, ws, PU_INTS, rowBytes + bitBytes, scanned));
    BHS_TRY(ensure(h, h->pushOff, sizeof(int) * scanned));
    int* ctl = (int*)ws.ctl.p;
    int* cnt = (int*)ws.cnt.p;
    int* off = (int*)h->pushOff.p;
    rd_u64* rows = (rd_u64*)ws.queue.p;
    unsigned* bits = (unsigned*)((char*)ws.queue.p + rowBytes);
    if (rowBytes + bitBytes) BHS_HIP(hipMemsetAsync(ws.queue.p, 0, rowBytes + bitBytes, h->stream));
    BHS_TRY(side_start(h, ws));
    if (d.nf > 0) {
        BHS_TRY(timed(h, "push_degrees", d.nf, [&] {
            hipLaunchKernelGGL(k_push_degrees, dim3((unsigned)(((long long)d.nf + 255) / 256)), dim3(256), 0, h->stream, d, in.fidx,
                               in.Gp, cnt, ctl);
            return 1;
        }));
        BHS_TRY(side_scan(h, ws, "push_scan", kPuScanDeg, d.nf, off, off));
        // what the host knows of the number of runs: nnzG entries for a list without repeats, kPuRun / T of them a run, four
        // runs a workgroup; no more than 256 workgroups a listed vertex (a single hub still has every CU)
        const long long reps = d.m > 0 ? ((long long)d.nf + d.m - 1) / d.m : 1;
        const long long perWg = 4 * (kPuRun / d.tile);
        const long long est = ((long long)d.nnzG * reps + perWg - 1) / perWg;
        const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>(std::min<long long>(est, (long long)d.nf * 256),
                                                                                    (long long)h->numCU * 8));
        const auto kern = in.kind == kRdSum ? k_push_edges<kRdSum> : in.kind == kRdMin ? k_push_edges<kRdMin> : k_push_edges<kRdMax>;
        BHS_TRY(timed(h, "push_edges", d.nf, [&] {
            hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, h->stream, d, in.fidx, (const int*)off, in.Gp, in.Gj, in.Gx, in.F,
                               in.M, in.Y, bits, rows, ctl);
            return 1;
        }));
    }
    if (in.next && nWords) {
        const unsigned grid = (unsigned)((nWords + 255) / 256);
        BHS_TRY(timed(h, "push_compact", (int64_t)nWords, [&] {
            hipLaunchKernelGGL(k_push_count, dim3(grid), dim3(256), 0, h->stream, (int)nWords, (const rd_u64*)rows, cnt);
            return 1;
        }));
        BHS_TRY(side_scan(h, ws, "push_scan", kPuScanRows, (int)nWords, off, off));
        BHS_TRY(timed(h, "push_compact", 0, [&] {
            hipLaunchKernelGGL(k_push_compact, dim3(grid), dim3(256), 0, h->stream, (int)nWords, (const rd_u64*)rows, (const int*)off,
                               in.next);
            return 1;
        }));
    }
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, PU_INTS));                           // the error word and the two counts, one round trip
    BHS_TRY(side_close(h, ws, ms_out));
    if (ws.host[RD_ERR]) return BHS_ERR_INVALID_ARG;
    if (changed_out) memcpy(changed_out, ws.host + PU_CHANGED, sizeof(long long));
    if (next_count_out) {
        long long cntNext = 0;
        if (in.next) memcpy(&cntNext, ws.host + PU_TOTAL_B, sizeof(long long));
        *next_count_out = (int)cntNext;
    }
    return BHS_SUCCESS;
}

}  // namespace

extern "C" {

int bhs_csr_push_semiring_device(bhs_handle* h, int semiring, int m, int n, int nnzG, const bhs_value_t* d_valG,
                                 const int* d_rowPtrG, const int* d_colIndG, int nf, const int* d_fidx, int k,
                                 const bhs_value_t* d_F, long long ldF, int flags, const bhs_value_t* d_M, long long ldM,
                                 bhs_value_t* d_Y, long long ldY, int* d_next, int* next_count_out, long long* changed_out,
                                 double* ms_out)
{
    if (!h || h->ps.open || m < 0 || n < 0 || nnzG < 0 || nf < 0) return BHS_ERR_INVALID_ARG;
    if (k < 1 || ldF < k || ldY < k) return BHS_ERR_INVALID_ARG;
    if ((m > 0 && !d_rowPtrG) || (nnzG > 0 && !d_colIndG) || (nf > 0 && (!d_fidx || !d_F)) || (n > 0 && !d_Y))
        return BHS_ERR_INVALID_ARG;
    PuIn in;
    rd_u64 id;
    if (!smv_rule(semiring, in.kind, in.d.mult, id) || semiring == BHS_SR_PLUS_TIMES) return BHS_ERR_INVALID_ARG;   // (a scattered sum has no fixed order)
    if (flags & ~BHS_MV_MASK_COMPLEMENT) return BHS_ERR_INVALID_ARG;
    if (d_M ? ldM < k : (flags & BHS_MV_MASK_COMPLEMENT) != 0) return BHS_ERR_INVALID_ARG;
    const size_t yBytes = mv_bytes(n, k, ldY), nextBytes = d_next ? sizeof(int) * (size_t)n : 0;
    if (side_aliased({{d_Y, yBytes}, {d_next, nextBytes}},
                     {{d_rowPtrG, sizeof(int) * ((size_t)m + 1)}, {d_colIndG, sizeof(int) * (size_t)nnzG}, {d_valG, sizeof(value_t) * (size_t)nnzG},
                      {d_fidx, sizeof(int) * (size_t)nf}, {d_F, mv_bytes(nf, k, ldF)}, {d_M, d_M ? mv_bytes(n, k, ldM) : 0}}))
        return BHS_ERR_INVALID_ARG;
    int T = 1;
    while (T < k && T < 64) T *= 2;
    in.d.m = m; in.d.n = n; in.d.nnzG = nnzG; in.d.nf = nf; in.d.k = k; in.d.ldF = ldF; in.d.ldM = d_M ? ldM : 0; in.d.ldY = ldY;
    in.d.flags = flags | (changed_out ? kSmvCount : 0) | (d_next ? kPuRowMap : 0);   // (no bitmap where nobody reads it)
    in.d.tile = T;
    in.Gp = d_rowPtrG; in.Gj = d_colIndG; in.Gx = (const value_t*)d_valG; in.fidx = d_fidx; in.F = (const value_t*)d_F;
    in.M = (const value_t*)d_M; in.Y = (value_t*)d_Y; in.next = d_next;
    return guarded(h, [&] { return pu_run(h, in, next_count_out, changed_out, ms_out); });
}

}  // extern "C"
