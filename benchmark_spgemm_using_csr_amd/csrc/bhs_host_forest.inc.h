// bhs_host_forest.inc.h -- the minimum or maximum spanning forest of a matrix's graph (bhs_csr_spanning_forest_device; kernels
// in bhs_forest.hip.h)
// (A part of bhsparse_hip.hip's translation unit, on the shared pieces of bhs_host_side.inc.h.)
//
// A workspace of its own (h->sfWs): the control block of bhs_forest.hip.h; in its queue buffer the trees' picks (bestW and
// bestE, a 64-bit word a vertex each), the slot bitmap (a word per 64 vertices), the slots' weights, then the ints: parent,
// the slots' two ends (lo == -1: an empty slot) and the scanned offsets; in its count buffer the written slots per bitmap
// word, scanned in place.  The labels are the caller's d_label itself.
// A round is 5 launches and ceil(log2 R) pointer jumps from R roots, R known from the round before, and ONE round trip: the
// error words and the trees the round hooked.  The loop ends after a round that hooked nothing, or that left one tree, and
// with BHS_ERR_INTERNAL where a 33rd hooking round would be needed (trees with a crossing edge at least halve a round): a
// verdict of its own, so the loop is here, not side_rounds.  The edge list adds three launches, the scan among them; the
// call's close is one more round trip, whatever n.

#include "bhs_forest.hip.h"

namespace {

constexpr int kSfMaxRounds = 32;    // floor(log2 n) rounds hook at most, n < 2^31

struct SfIn {
    AgDims d;                            // (hasPrio: are there values; seed: the flags)
    const int* Ap; const int* Aj; const value_t* Ax;
    int* label; int* edgeLo; int* edgeHi; value_t* edgeVal;
};

struct SfWork {
    rd_u64* bestW; rd_u64* bestE; rd_u64* map;
    value_t* slotVal;
    int* parent; int* slotLo; int* slotHi; int* off;
};

// ceil(log2 r): the launches of k_sf_jump that flatten any hook forest over r roots
int sf_jumps(long long r)
{
    int k = 0;
    while ((1ll << k) < r) ++k;
    return k;
}

template <int L>
int sf_rounds(bhs_handle* h, const SfIn& in, const SfWork& w, int* ctl, long long* hooks_out, int* rounds_out)
{
    const AgDims& d = in.d;
    SideWs& ws = h->sfWs;
    const unsigned rows = (unsigned)(((long long)d.n + 256 / L - 1) / (256 / L));
    const unsigned gridN = (unsigned)(((long long)d.n + 255) / 256);
    const unsigned gridRows = std::min<unsigned>(rows, (unsigned)h->numCU * 16);   // (block loops)
    const unsigned gridHook = std::min<unsigned>(gridN, (unsigned)h->numCU * 16);  // (one add to the count a workgroup)
    long long roots = d.n, hooks = 0;
    int rounds = 0;
    for (;;) {
        BHS_HIP(hipMemsetAsync(ctl + AG_UNDEC, 0, sizeof(rd_u64), h->stream));
        BHS_TRY(timed(h, "forest_pick", roots, [&] {
            hipLaunchKernelGGL(k_sf_clear, dim3(gridN), dim3(256), 0, h->stream, d.n, w.bestW, w.bestE);
            hipLaunchKernelGGL(k_sf_weight<L>, dim3(gridRows), dim3(256), 0, h->stream, d, in.Ap, in.Aj, in.Ax, (const int*)in.label,
                               w.bestW, ctl);
            hipLaunchKernelGGL(k_sf_edge<L>, dim3(gridRows), dim3(256), 0, h->stream, d, in.Ap, in.Aj, in.Ax, (const int*)in.label,
                               (const rd_u64*)w.bestW, w.bestE);
            return 3;
        }));
        const int jumps = sf_jumps(roots);
        BHS_TRY(timed(h, "forest_hook", roots, [&] {
            hipLaunchKernelGGL(k_sf_hook, dim3(gridHook), dim3(256), 0, h->stream, d, (const int*)in.label, (const rd_u64*)w.bestW,
                               (const rd_u64*)w.bestE, w.parent, w.slotLo, w.slotHi, w.slotVal, ctl);
            for (int s = 0; s < jumps; ++s)
                hipLaunchKernelGGL(k_sf_jump, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)in.label, w.parent);
            hipLaunchKernelGGL(k_sf_relabel, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)w.parent, in.label, ctl);
            return jumps + 2;
        }));
        BHS_TRY(side_read_ctl(h, ws, SF_INTS));                       // the error words and the trees hooked: the round's one round trip
        if (ws.host[RD_ERR]) return BHS_ERR_INVALID_ARG;
        if (ws.host[SF_BROKEN]) return BHS_ERR_INTERNAL;
        long long hooked = 0;
        memcpy(&hooked, ws.host + AG_UNDEC, sizeof(hooked));
        if (hooked < 0 || hooked >= roots) return BHS_ERR_INTERNAL;   // (a root stays in every tree)
        if (hooked == 0) break;
        if (rounds == kSfMaxRounds) return BHS_ERR_INTERNAL;
        ++rounds;
        hooks += hooked;
        roots -= hooked;
        if (roots == 1) break;                                        // one tree: no entry crosses
    }
    *hooks_out = hooks;
    *rounds_out = rounds;
    return BHS_SUCCESS;
}

int sf_run(bhs_handle* h, const SfIn& in, int* nedges_out, int* rounds_out, double* ms_out)
{
    const AgDims& d = in.d;
    SideWs& ws = h->sfWs;
    const size_t n = (size_t)d.n, nWords = (n + 63) / 64;
    BHS_TRY(side_open(h, ws, SF_INTS, sizeof(rd_u64) * (2 * n + nWords) + sizeof(value_t) * n + sizeof(int) * (3 * n + nWords + 1),
                         nWords + 1));
    int* ctl = (int*)ws.ctl.p;
    SfWork w;
    w.bestW = (rd_u64*)ws.queue.p;
    w.bestE = w.bestW + n;
    w.map = w.bestE + n;
    w.slotVal = (value_t*)(w.map + nWords);
    w.parent = (int*)(w.slotVal + n);
    w.slotLo = w.parent + n;
    w.slotHi = w.slotLo + n;
    w.off = w.slotHi + n;
    BHS_TRY(side_start(h, ws));
    const unsigned gridN = (unsigned)((n + 255) / 256);
    BHS_TRY(timed(h, "forest_pick", 0, [&] {
        hipLaunchKernelGGL(k_sf_init, dim3(gridN), dim3(256), 0, h->stream, d, in.Ap, in.label, w.parent, w.slotLo, ctl);
        return 1;
    }));
    const int L = side_lanes(d.n, d.nnzS);
    long long hooks = 0;
    int rounds = 0;
    BHS_TRY(with_lanes(L, [&](auto l) { return sf_rounds<l.value>(h, in, w, ctl, &hooks, &rounds); }));
    int* cnt = (int*)ws.cnt.p;
    BHS_TRY(timed(h, "forest_list", d.n, [&] {
        hipLaunchKernelGGL(k_sf_flag, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)w.slotLo, w.map, cnt);
        return 1;
    }));
    BHS_TRY(side_scan(h, ws, "forest_list", kAgScan, (int)nWords, w.off, w.off));
    BHS_TRY(timed(h, "forest_list", hooks, [&] {
        hipLaunchKernelGGL(k_sf_write, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)w.slotLo, (const int*)w.slotHi,
                           (const value_t*)w.slotVal, (const rd_u64*)w.map, (const int*)w.off, in.edgeLo, in.edgeHi, in.edgeVal, ctl);
        return 1;
    }));
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, SF_INTS));                           // the write-out's error word and the scan's total
    BHS_TRY(side_close(h, ws, ms_out));
    long long total = 0;
    memcpy(&total, ws.host + AG_TOTAL, sizeof(total));
    if (ws.host[RD_ERR] || ws.host[SF_BROKEN] || total != hooks) return BHS_ERR_INTERNAL;   // (the slots were this call's own)
    if (nedges_out) *nedges_out = (int)hooks;
    if (rounds_out) *rounds_out = rounds;
    return BHS_SUCCESS;
}

}  // namespace

extern "C" {

int bhs_csr_spanning_forest_device(bhs_handle* h, int n, int nnzA, const int* d_rowPtrA, const int* d_colIndA,
                                   const bhs_value_t* d_valA, int flags, int* d_label, int* d_edgeLo, int* d_edgeHi,
                                   bhs_value_t* d_edgeVal, int* nedges_out, int* rounds_out, double* ms_out)
{
    if (!h || h->ps.open || n < 0 || nnzA < 0 || (flags & ~(BHS_FOREST_MAXIMUM | BHS_FOREST_ABS))) return BHS_ERR_INVALID_ARG;
    if ((n > 0 && (!d_rowPtrA || !d_label || !d_edgeLo || !d_edgeHi)) || (nnzA > 0 && !d_colIndA)) return BHS_ERR_INVALID_ARG;
    if (side_aliased({{d_label, sizeof(int) * (size_t)n}, {d_edgeLo, sizeof(int) * (size_t)n}, {d_edgeHi, sizeof(int) * (size_t)n},
                      {d_edgeVal, sizeof(value_t) * (size_t)n}},
                     {{d_rowPtrA, sizeof(int) * ((size_t)n + 1)}, {d_colIndA, sizeof(int) * (size_t)nnzA}, {d_valA, sizeof(value_t) * (size_t)nnzA}}))
        return BHS_ERR_INVALID_ARG;
    if (n == 0) return side_nothing(nedges_out, rounds_out, ms_out);   // no vertex, no edge, nothing launched
    SfIn in;
    in.d.n = n; in.d.nnzS = nnzA; in.d.seed = (unsigned)flags; in.d.hasPrio = d_valA ? 1 : 0;
    in.Ap = d_rowPtrA; in.Aj = d_colIndA; in.Ax = (const value_t*)d_valA; in.label = d_label;
    in.edgeLo = d_edgeLo; in.edgeHi = d_edgeHi; in.edgeVal = (value_t*)d_edgeVal;
    static_assert(BHS_FOREST_MAXIMUM == kSfMaximum && BHS_FOREST_ABS == kSfAbs, "flags");
    return guarded(h, [&] { return sf_run(h, in, nedges_out, rounds_out, ms_out); });
}

}  // extern "C"
