// bhs_host_match.inc.h -- heavy-edge matching of a matrix's vertices (bhs_csr_match_device; kernels in bhs_match.hip.h)
// (A part of bhsparse_hip.hip's translation unit, on the shared pieces of bhs_host_side.inc.h.)
//
// A workspace of its own (h->mtWs): the control block of bhs_match.hip.h; in its queue buffer the leader bitmap (a word per 64
// vertices) and the scanned offsets behind it, where the aggregates are numbered, and the rounds' candidates (an int a
// vertex); in its count buffer the leaders per bitmap word, scanned in place.  The mates are the caller's d_mate itself.
// A round is two launches and ONE round trip, for the error word, the pairs the round made and the vertices it left
// undecided; the loop ends after a round that matched nothing (the vertices it left become unmatched: k_mt_finish) or left
// nobody, and with BHS_ERR_INTERNAL when more than n / 2 + 1 rounds would be needed (a verdict of its own: the loop is here,
// not side_rounds).  The numbering adds three launches, the scan among them; the call's close is one more round trip,
// whatever n.

#include "bhs_match.hip.h"

namespace {

struct MtIn {
    AgDims d;                            // (hasPrio: are there values)
    const int* Ap; const int* Aj; const value_t* Ax;
    int* mate; int* agg;
};

template <int L>
int mt_rounds(bhs_handle* h, const MtIn& in, int* cand, int* ctl, long long* npairs_out, int* rounds_out)
{
    const AgDims& d = in.d;
    SideWs& ws = h->mtWs;
    const unsigned grid = (unsigned)(((long long)d.n + 256 / L - 1) / (256 / L));
    const unsigned gridN = (unsigned)(((long long)d.n + 255) / 256);
    const unsigned gridAccept = std::min<unsigned>(gridN, (unsigned)h->numCU * 16);   // (a block loop: one add to the count a workgroup)
    long long left = d.n, npairs = 0;
    int rounds = 0;
    for (long long round = 1;; ++round) {
        if (round > (long long)d.n / 2 + 1) return BHS_ERR_INTERNAL;  // (a productive round makes a pair: n / 2 of them, one more finds nothing)
        BHS_HIP(hipMemsetAsync(ctl + AG_UNDEC, 0, sizeof(rd_u64), h->stream));
        BHS_TRY(timed(h, "match_round", left, [&] {
            hipLaunchKernelGGL(k_mt_propose<L>, dim3(grid), dim3(256), 0, h->stream, d, in.Ap, in.Aj, in.Ax, (const int*)in.mate, cand, ctl);
            hipLaunchKernelGGL(k_mt_accept, dim3(gridAccept), dim3(256), 0, h->stream, d.n, (const int*)cand, in.mate, ctl);
            return 2;
        }));
        BHS_TRY(side_read_ctl(h, ws, MT_INTS));                       // the error word and the counts: the round's one round trip
        if (ws.host[RD_ERR]) return BHS_ERR_INVALID_ARG;
        rd_u64 count = 0;
        memcpy(&count, ws.host + AG_UNDEC, sizeof(count));
        const long long made = (long long)(count & 0xffffffffull), now = (long long)(count >> 32);
        if (2 * made + now > left) return BHS_ERR_INTERNAL;
        if (made == 0) {
            if (now > 0)                                             // (only where pattern or weights are not symmetric)
                BHS_TRY(timed(h, "match_round", now, [&] {
                    hipLaunchKernelGGL(k_mt_finish, dim3(gridN), dim3(256), 0, h->stream, d.n, in.mate);
                    return 1;
                }));
            break;
        }
        ++rounds;
        npairs += made;
        left = now;
        if (now == 0) break;
    }
    *npairs_out = npairs;
    *rounds_out = rounds;
    return BHS_SUCCESS;
}

int mt_run(bhs_handle* h, const MtIn& in, int* npairs_out, int* rounds_out, double* ms_out)
{
    const AgDims& d = in.d;
    SideWs& ws = h->mtWs;
    const size_t n = (size_t)d.n, nWords = (n + 63) / 64;
    const bool number = in.agg != nullptr;
    BHS_TRY(side_open(h, ws, MT_INTS, sizeof(rd_u64) * nWords + sizeof(int) * (nWords + 1 + n), number ? nWords + 1 : 0));
    int* ctl = (int*)ws.ctl.p;
    rd_u64* map = (rd_u64*)ws.queue.p;
    int* off = (int*)(map + nWords);
    int* cand = off + nWords + 1;
    BHS_TRY(side_start(h, ws));
    const unsigned gridN = (unsigned)((n + 255) / 256);
    BHS_TRY(timed(h, "match_init", d.n, [&] {
        hipLaunchKernelGGL(k_mt_init, dim3(gridN), dim3(256), 0, h->stream, d, in.Ap, in.mate, ctl);
        return 1;
    }));
    const int L = side_lanes(d.n, d.nnzS);
    long long npairs = 0;
    int rounds = 0;
    BHS_TRY(with_lanes(L, [&](auto l) { return mt_rounds<l.value>(h, in, cand, ctl, &npairs, &rounds); }));
    if (2 * npairs > (long long)d.n) return BHS_ERR_INTERNAL;
    if (number) {
        int* cnt = (int*)ws.cnt.p;
        BHS_TRY(timed(h, "match_number", d.n, [&] {
            hipLaunchKernelGGL(k_mt_flag, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)in.mate, map, cnt);
            return 1;
        }));
        BHS_TRY(side_scan(h, ws, "match_number", kAgScan, (int)nWords, off, off));
        BHS_TRY(timed(h, "match_number", 0, [&] {
            hipLaunchKernelGGL(k_mt_number, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)in.mate, (const rd_u64*)map,
                               (const int*)off, in.agg, ctl);
            return 1;
        }));
    }
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, MT_INTS));                           // the numbering's error word and total (the span's end in any case)
    BHS_TRY(side_close(h, ws, ms_out));
    if (number) {
        long long total = 0;
        memcpy(&total, ws.host + AG_TOTAL, sizeof(total));
        if (ws.host[RD_ERR] || total != (long long)d.n - npairs) return BHS_ERR_INTERNAL;   // (the mates were this call's own)
    }
    if (npairs_out) *npairs_out = (int)npairs;
    if (rounds_out) *rounds_out = rounds;
    return BHS_SUCCESS;
}

}  // namespace

extern "C" {

int bhs_csr_match_device(bhs_handle* h, int n, int nnzA, const int* d_rowPtrA, const int* d_colIndA, const bhs_value_t* d_valA,
                         unsigned seed, int flags, int* d_mate, int* d_agg, int* npairs_out, int* rounds_out, double* ms_out)
{
    if (!h || h->ps.open || n < 0 || nnzA < 0 || flags != 0) return BHS_ERR_INVALID_ARG;
    if ((n > 0 && (!d_rowPtrA || !d_mate)) || (nnzA > 0 && !d_colIndA)) return BHS_ERR_INVALID_ARG;
    const size_t outBytes = sizeof(int) * (size_t)n;
    if (side_aliased({{d_mate, outBytes}, {d_agg, outBytes}},
                     {{d_rowPtrA, sizeof(int) * ((size_t)n + 1)}, {d_colIndA, sizeof(int) * (size_t)nnzA}, {d_valA, sizeof(value_t) * (size_t)nnzA}}))
        return BHS_ERR_INVALID_ARG;
    if (n == 0) return side_nothing(npairs_out, rounds_out, ms_out);   // no vertex, no pair, nothing launched
    MtIn in;
    in.d.n = n; in.d.nnzS = nnzA; in.d.seed = seed; in.d.hasPrio = d_valA ? 1 : 0;
    in.Ap = d_rowPtrA; in.Aj = d_colIndA; in.Ax = (const value_t*)d_valA; in.mate = d_mate; in.agg = d_agg;
    return guarded(h, [&] { return mt_run(h, in, npairs_out, rounds_out, ms_out); });
}

}  // extern "C"
