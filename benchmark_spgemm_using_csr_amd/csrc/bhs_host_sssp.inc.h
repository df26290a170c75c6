// bhs_host_sssp.inc.h -- shortest paths by delta-stepping (bhs_csr_sssp_device; kernels in bhs_sssp.hip.h)
// (A part of bhsparse_hip.hip's translation unit, on the shared pieces of bhs_host_side.inc.h.)
//
// A workspace of its own (h->ssspWs): the control block of bhs_sssp.hip.h; in its queue buffer four arrays of n distance
// words (dist, done and the two slices' snapshots) and behind them three or four of n ints (stamp, the two slices, and the
// parents' words where parents are asked for).  The loop is side_passes_within's: kSsspBatch passes of four launches a
// control round trip, the count being the next slice's length, which the last launch of a pass writes; it ends after a batch
// whose last pass left no slice, and with BHS_ERR_INTERNAL when more than 2 n + 2 passes would be needed (a bucket that
// settles n_k vertices takes at most n_k + 1 passes, and no more than n buckets hold a vertex).  There is no round trip
// behind the check: once it has raised the error word every later launch leaves at once, so a refused input has written no
// output when the first batch's read finds the word.  The passes behind the last one leave at once.  The call's close is one
// more round trip, whatever n.

#include "bhs_sssp.hip.h"

namespace {

constexpr int kSsspBatch = 8;       // passes between two reads of the control words

struct SsspIn {
    SsDims d;
    const int* Gp; const int* Gj; const value_t* Gx; const int* src;
    value_t* outDist; int* outPar;
    ss_word* dist; ss_word* done;
    unsigned* stamp; int* par;
    SsSlices sl;
};

template <int L>
int sssp_passes(bhs_handle* h, const SsspIn& in, int* ctl, int* passes_out)
{
    const SsDims& d = in.d;
    SideWs& ws = h->ssspWs;
    const unsigned cap = (unsigned)h->numCU * 16;                     // (block loops)
    const unsigned gridL = std::min<unsigned>((unsigned)(((long long)d.n + 256 / L - 1) / (256 / L)), cap);
    const unsigned gridN = std::min<unsigned>((unsigned)(((long long)d.n + 255) / 256), cap);
    return side_passes_within(h, ws, 2 * (long long)d.n + 2, kSsspBatch, 2, SSSP_INTS, passes_out, [&] {
        BHS_TRY(timed(h, "sssp_relax", d.n, [&] {
            hipLaunchKernelGGL(k_sssp_relax<L>, dim3(gridL), dim3(256), 0, h->stream, d, in.Gp, in.Gj, in.Gx, in.dist, in.done, in.stamp, in.sl, ctl);
            return 1;
        }));
        return timed(h, "sssp_advance", d.n, [&] {
            hipLaunchKernelGGL(k_sssp_min, dim3(gridN), dim3(256), 0, h->stream, d, (const ss_word*)in.dist, (const ss_word*)in.done, in.sl, ctl);
            hipLaunchKernelGGL(k_sssp_gather, dim3(gridN), dim3(256), 0, h->stream, d, (const ss_word*)in.dist, (const ss_word*)in.done, in.sl, ctl);
            hipLaunchKernelGGL(k_sssp_advance, dim3(1), dim3(64), 0, h->stream, d, ctl);
            return 3;
        });
    });
}

int sssp_run(bhs_handle* h, SsspIn& in, int* reached_out, int* passes_out, double* ms_out)
{
    const SsDims& d = in.d;
    SideWs& ws = h->ssspWs;
    const size_t n = (size_t)d.n;
    BHS_TRY(side_open(h, ws, SSSP_INTS, sizeof(ss_word) * 4 * n + sizeof(int) * (in.outPar ? 4 : 3) * n, 0));
    in.dist = (ss_word*)ws.queue.p;
    in.done = in.dist + n;
    in.sl.sv[0] = in.done + n;
    in.sl.sv[1] = in.sl.sv[0] + n;
    in.stamp = (unsigned*)(in.sl.sv[1] + n);
    in.sl.q[0] = (int*)in.stamp + n;
    in.sl.q[1] = in.sl.q[0] + n;
    in.par = in.outPar ? in.sl.q[1] + n : nullptr;
    BHS_TRY(side_start(h, ws));
    int* ctl = (int*)ws.ctl.p;
    const int L = side_lanes(d.n, d.nnzG);
    const unsigned cap = (unsigned)h->numCU * 16;
    const unsigned gridN = std::min<unsigned>((unsigned)(((long long)d.n + 255) / 256), cap);
    const unsigned gridS = std::min<unsigned>((unsigned)(((long long)d.nsrc + 255) / 256), cap);
    BHS_TRY(timed(h, "sssp_check", d.n, [&] {
        const unsigned grid = std::min<unsigned>((unsigned)((std::max<long long>(d.n, d.nnzG) + 255) / 256), cap);   // (rows, then entries)
        hipLaunchKernelGGL(k_sssp_check, dim3(grid), dim3(256), 0, h->stream, d, in.Gp, in.Gj, in.Gx, in.src, in.dist, in.done, in.stamp,
                           in.par, ctl);
        return 1;
    }));
    BHS_TRY(timed(h, "sssp_seed", d.nsrc, [&] {
        hipLaunchKernelGGL(k_sssp_seed, dim3(gridS), dim3(256), 0, h->stream, d, in.src, in.dist, in.stamp, in.sl, ctl);
        return 1;
    }));
    int passes = 0;
    BHS_TRY(with_lanes(L, [&](auto l) { return sssp_passes<l.value>(h, in, ctl, &passes); }));
    if (in.outPar)
        BHS_TRY(with_lanes(L, [&](auto l) {
            return timed(h, "sssp_parents", d.n, [&] {
                const unsigned grid = std::min<unsigned>((unsigned)(((long long)d.n + 256 / l.value - 1) / (256 / l.value)), cap);
                hipLaunchKernelGGL(k_sssp_parents<l.value>, dim3(grid), dim3(256), 0, h->stream, d, in.Gp, in.Gj, in.Gx, (const ss_word*)in.dist,
                                   in.par, ctl);
                hipLaunchKernelGGL(k_sssp_roots, dim3(gridS), dim3(256), 0, h->stream, d, in.src, in.par, ctl);
                return 2;
            });
        }));
    BHS_TRY(timed(h, "sssp_finish", d.n, [&] {
        hipLaunchKernelGGL(k_sssp_finish, dim3(gridN), dim3(256), 0, h->stream, d, (const ss_word*)in.dist, (const int*)in.par, in.outDist,
                           in.outPar, ctl);
        return 1;
    }));
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, SSSP_INTS));                         // the counts of the finish, the buckets, the passes that had a slice
    BHS_TRY(side_close(h, ws, ms_out));
    const long long reached = ws.host[SSSP_REACHED], loose = ws.host[SSSP_LOOSE], buckets = ws.host[SSSP_BUCKETS];
    const long long work = ws.host[SSSP_PASS];
    if (ws.host[RD_ERR] || ws.host[SSSP_DONE] != 1) return BHS_ERR_INTERNAL;   // (the check accepted the input)
    if (reached < 1 || reached > (long long)d.n || loose < 0 || loose >= reached || buckets < 1 || buckets > work || work > (long long)passes)
        return BHS_ERR_INTERNAL;
    h->ssspBuckets = buckets;
    h->ssspLoose = loose;
    h->ssspWork = work;
    if (reached_out) *reached_out = (int)reached;
    if (passes_out) *passes_out = passes;
    return BHS_SUCCESS;
}

}  // namespace

extern "C" {

int bhs_csr_sssp_device(bhs_handle* h, int n, int nnzG, const int* d_rowPtrG, const int* d_colIndG, const bhs_value_t* d_valG, int nsrc,
                        const int* d_sources, double delta, int flags, bhs_value_t* d_dist, int* d_parent, int* reached_out, int* passes_out,
                        double* ms_out)
{
    if (!h || h->ps.open || n < 0 || nnzG < 0 || nsrc < 0 || flags != 0 || !(delta > 0.0)) return BHS_ERR_INVALID_ARG;
    if (n > 0 && (nsrc < 1 || !d_sources || !d_rowPtrG || !d_dist)) return BHS_ERR_INVALID_ARG;
    if (nnzG > 0 && !d_colIndG) return BHS_ERR_INVALID_ARG;
    if (side_aliased({{d_dist, sizeof(value_t) * (size_t)n}, {d_parent, sizeof(int) * (size_t)n}},
                     {{d_rowPtrG, sizeof(int) * ((size_t)n + 1)}, {d_colIndG, sizeof(int) * (size_t)nnzG},
                      {d_valG, sizeof(value_t) * (size_t)nnzG}, {d_sources, sizeof(int) * (size_t)nsrc}}))
        return BHS_ERR_INVALID_ARG;
    if (n == 0) {                                                     // no vertex: nothing launched
        h->ssspBuckets = h->ssspLoose = h->ssspWork = 0;
        return side_nothing(reached_out, passes_out, ms_out);
    }
    SsspIn in;
    memset(&in, 0, sizeof(in));
    in.d.n = n; in.d.nnzG = nnzG; in.d.hasVal = d_valG ? 1 : 0; in.d.nsrc = nsrc; in.d.delta = delta;
    in.Gp = d_rowPtrG; in.Gj = d_colIndG; in.Gx = (const value_t*)d_valG; in.src = d_sources;
    in.outDist = (value_t*)d_dist; in.outPar = d_parent;
    return guarded(h, [&] { return sssp_run(h, in, reached_out, passes_out, ms_out); });
}

}  // extern "C"
