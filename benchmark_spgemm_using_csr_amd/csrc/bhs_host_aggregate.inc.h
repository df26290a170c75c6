// bhs_host_aggregate.inc.h -- MIS(2) aggregation of a pattern of strong connections (bhs_csr_aggregate_device; kernels in
// bhs_aggregate.hip.h)
// (A part of bhsparse_hip.hip's translation unit, on the shared pieces of bhs_host_side.inc.h.)
//
// A workspace of its own (h->aggWs): the control block of bhs_aggregate.hip.h; in its queue buffer the vertices' words, the
// first gather's result (8 bytes a vertex each), the root bitmap (a word per 64 vertices) and pass 1's aggregates (an int a
// vertex); in its count buffer the roots per bitmap word, scanned in place, the scanned offsets copied to h->aggOff.
// A round is two launches and ONE round trip, for the error word and the count of undecided vertices (side_rounds: the loop
// ends when the count is zero, and with BHS_ERR_INTERNAL when a round decides nothing or after n + 1 rounds); the call's
// close is one more, for the number of roots.

#include "bhs_aggregate.hip.h"

namespace {

struct AgIn {
    AgDims d;
    const int* Sp; const int* Sj;
    const unsigned* prio;
    int* agg; int* roots;
};

template <int L>
int ag_rounds(bhs_handle* h, const AgIn& in, rd_u64* w, rd_u64* t1, int* ctl, int* rounds_out)
{
    const AgDims& d = in.d;
    const unsigned grid = (unsigned)(((long long)d.n + 256 / L - 1) / (256 / L));
    const unsigned gridDecide = std::min<unsigned>(grid, (unsigned)h->numCU * 16);   // (a block loop: one add to the count a workgroup)
    return side_rounds(h, h->aggWs, d.n, AG_INTS, rounds_out, [&](long long, long long left) {
        BHS_TRY(timed(h, "agg_near", d.n, [&] {
            hipLaunchKernelGGL(k_agg_near<L>, dim3(grid), dim3(256), 0, h->stream, d, in.Sp, in.Sj, (const rd_u64*)w, t1, ctl);
            return 1;
        }));
        return timed(h, "agg_decide", left, [&] {
            hipLaunchKernelGGL(k_agg_decide<L>, dim3(gridDecide), dim3(256), 0, h->stream, d, in.Sp, in.Sj, (const rd_u64*)t1, w, ctl);
            return 1;
        });
    });
}

template <int L>
int ag_join(bhs_handle* h, const AgIn& in, const rd_u64* w, int* agg1, int* ctl)
{
    const AgDims& d = in.d;
    const unsigned grid = (unsigned)(((long long)d.n + 256 / L - 1) / (256 / L));
    BHS_TRY(timed(h, "agg_join", d.n, [&] {
        hipLaunchKernelGGL((k_agg_join<L, 1>), dim3(grid), dim3(256), 0, h->stream, d, in.Sp, in.Sj, w, (const int*)agg1, agg1, ctl);
        hipLaunchKernelGGL((k_agg_join<L, 2>), dim3(grid), dim3(256), 0, h->stream, d, in.Sp, in.Sj, w, (const int*)agg1, in.agg, ctl);
        return 2;
    }));
    return BHS_SUCCESS;
}

int ag_run(bhs_handle* h, const AgIn& in, int* nagg_out, int* rounds_out, double* ms_out)
{
    const AgDims& d = in.d;
    SideWs& ws = h->aggWs;
    const size_t n = (size_t)d.n, nWords = (n + 63) / 64;
    BHS_TRY(side_open(h, ws, AG_INTS, sizeof(rd_u64) * (2 * n + nWords) + sizeof(int) * n, nWords + 1));
    BHS_TRY(ensure(h, h->aggOff, sizeof(int) * (nWords + 1)));
    BHS_TRY(side_start(h, ws));
    int* ctl = (int*)ws.ctl.p;
    int* cnt = (int*)ws.cnt.p;
    int* off = (int*)h->aggOff.p;
    rd_u64* w = (rd_u64*)ws.queue.p;
    rd_u64* t1 = w + n;
    rd_u64* map = t1 + n;
    int* agg1 = (int*)(map + nWords);
    const unsigned gridN = (unsigned)((n + 255) / 256);
    BHS_TRY(timed(h, "agg_init", d.n, [&] {
        hipLaunchKernelGGL(k_agg_init, dim3(gridN), dim3(256), 0, h->stream, d, in.Sp, in.prio, w, ctl);
        return 1;
    }));
    const int L = side_lanes(d.n, d.nnzS);
    int rounds = 0;
    BHS_TRY(with_lanes(L, [&](auto l) { return ag_rounds<l.value>(h, in, w, t1, ctl, &rounds); }));
    BHS_TRY(timed(h, "agg_scan", d.n, [&] {
        hipLaunchKernelGGL(k_agg_count, dim3(gridN), dim3(256), 0, h->stream, d.n, (const rd_u64*)w, map, cnt);
        return 1;
    }));
    BHS_TRY(side_scan(h, ws, "agg_scan", kAgScan, (int)nWords, off, off));
    BHS_TRY(timed(h, "agg_scan", 0, [&] {
        hipLaunchKernelGGL(k_agg_number, dim3((unsigned)((nWords + 255) / 256)), dim3(256), 0, h->stream, (int)nWords,
                           (const rd_u64*)map, (const int*)off, agg1, in.roots);
        return 1;
    }));
    BHS_TRY(with_lanes(L, [&](auto l) { return ag_join<l.value>(h, in, w, agg1, ctl); }));
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, AG_INTS));                           // the number of roots
    BHS_TRY(side_close(h, ws, ms_out));
    if (ws.host[RD_ERR]) return BHS_ERR_INVALID_ARG;
    long long nagg = 0;
    memcpy(&nagg, ws.host + AG_TOTAL, sizeof(nagg));
    if (nagg < 1 || nagg > (long long)d.n) return BHS_ERR_INTERNAL;
    if (nagg_out) *nagg_out = (int)nagg;
    if (rounds_out) *rounds_out = rounds;
    return BHS_SUCCESS;
}

}  // namespace

extern "C" {

int bhs_csr_aggregate_device(bhs_handle* h, int n, int nnzS, const int* d_rowPtrS, const int* d_colIndS, const unsigned* d_prio,
                             unsigned seed, int flags, int* d_agg, int* d_roots, int* nagg_out, int* rounds_out, double* ms_out)
{
    if (!h || h->ps.open || n < 0 || nnzS < 0 || flags != 0) return BHS_ERR_INVALID_ARG;
    if ((n > 0 && (!d_rowPtrS || !d_agg)) || (nnzS > 0 && !d_colIndS)) return BHS_ERR_INVALID_ARG;
    const size_t outBytes = sizeof(int) * (size_t)n;
    if (side_aliased({{d_agg, outBytes}, {d_roots, outBytes}},
                     {{d_rowPtrS, sizeof(int) * ((size_t)n + 1)}, {d_colIndS, sizeof(int) * (size_t)nnzS}, {d_prio, sizeof(unsigned) * (size_t)n}}))
        return BHS_ERR_INVALID_ARG;
    if (n == 0) return side_nothing(nagg_out, rounds_out, ms_out);     // nothing to aggregate, nothing launched
    AgIn in;
    in.d.n = n; in.d.nnzS = nnzS; in.d.seed = seed; in.d.hasPrio = d_prio ? 1 : 0;
    in.Sp = d_rowPtrS; in.Sj = d_colIndS; in.prio = d_prio; in.agg = d_agg; in.roots = d_roots;
    return guarded(h, [&] { return ag_run(h, in, nagg_out, rounds_out, ms_out); });
}

}  // extern "C"
