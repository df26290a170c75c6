// bhs_host_bc.inc.h -- betweenness centrality (bhs_csr_betweenness_device; kernels in bhs_bc.hip.h)
// (A part of bhsparse_hip.hip's translation unit, on the shared pieces of bhs_host_side.inc.h.)
//
// A workspace of its own (h->bcWs): the control block of bhs_bc.hip.h; in its queue buffer sigma and delta as n doubles each
// and behind them level, the queue (n ints each) and levelPtr (n + 2 ints).  The sources are taken one after the other.  A
// source is one seed launch, then side_passes_within's loop: kBcBatch passes of three launches a control round trip, the count
// being the next slice's length, which the last launch of a pass writes; it ends after a batch whose last pass left no slice
// (at most n passes have one, so n + 1 bounds them), and its last read tells the host the deepest level.  The backward sweep
// is then a fixed list of launches, one a level from deepest - 1 down to 1, queued back to back with no round trip.  There is
// no round trip behind the check: once it has raised the error word every later launch leaves at once, so a refused input has
// written no output when the first batch's read finds the word.  The call's close is one more round trip, whatever n.

#include "bhs_bc.hip.h"

namespace {

constexpr int kBcBatch = 8;         // passes between two reads of the control words

struct BcIn {
    BcDims d;
    const int* Gp; const int* Gj; const int* Tp; const int* Tj; const int* src;
    int accumulate;
    double* bc; int* outLevel; double* outSigma;
    BcWork w;
};

unsigned bc_grid(bhs_handle* h, long long n, int L)
{
    return std::min<unsigned>((unsigned)((n + 256 / L - 1) / (256 / L)), (unsigned)h->numCU * 16);   // (block loops)
}

template <int LG, int LT>
int bc_source(bhs_handle* h, const BcIn& in, int si, int* ctl, long long* passes, long long* backs)
{
    const BcDims& d = in.d;
    SideWs& ws = h->bcWs;
    const unsigned gridN = bc_grid(h, d.n, 1), gridG = bc_grid(h, d.n, LG), gridT = bc_grid(h, d.n, LT);
    BHS_TRY(timed(h, "bc_seed", d.n, [&] {
        hipLaunchKernelGGL(k_bc_seed, dim3(gridN), dim3(256), 0, h->stream, d, in.src, si, si == 0 && !in.accumulate ? 1 : 0, in.w, in.bc, ctl);
        return 1;
    }));
    int launched = 0;
    BHS_TRY(side_passes_within(h, ws, (long long)d.n + 1, kBcBatch, 2, BC_INTS, &launched, [&] {
        BHS_TRY(timed(h, "bc_expand", d.n, [&] {
            hipLaunchKernelGGL(k_bc_expand<LG>, dim3(gridG), dim3(256), 0, h->stream, d, in.Gp, in.Gj, in.w, ctl);
            return 1;
        }));
        return timed(h, "bc_count", d.n, [&] {
            hipLaunchKernelGGL(k_bc_count<LT>, dim3(gridT), dim3(256), 0, h->stream, d, in.Tp, in.Tj, in.w, ctl);
            hipLaunchKernelGGL(k_bc_advance, dim3(1), dim3(64), 0, h->stream, d, in.w, ctl);
            return 2;
        });
    }));
    *passes += launched;
    const int deepest = ws.host[BC_DEEPEST];                          // (the loop's last read)
    if (ws.host[BC_DONE] != 1 || deepest < 0 || deepest >= d.n) return BHS_ERR_INTERNAL;
    for (int lev = deepest - 1; lev >= 1; --lev) {                    // no host decision inside: every launch takes its slice on the device
        BHS_TRY(timed(h, "bc_back", d.n, [&] {
            hipLaunchKernelGGL(k_bc_back<LG>, dim3(gridG), dim3(256), 0, h->stream, d, in.Gp, in.Gj, lev, in.w, in.bc, ctl);
            return 1;
        }));
        *backs += 1;
    }
    return BHS_SUCCESS;
}

int bc_run(bhs_handle* h, BcIn& in, int* reached_out, int* passes_out, double* ms_out)
{
    const BcDims& d = in.d;
    SideWs& ws = h->bcWs;
    const size_t n = (size_t)d.n;
    BHS_TRY(side_open(h, ws, BC_INTS, sizeof(double) * 2 * n + sizeof(int) * (3 * n + 2), 0));
    in.w.sigma = (double*)ws.queue.p;
    in.w.delta = in.w.sigma + n;
    in.w.level = (int*)(in.w.delta + n);
    in.w.queue = in.w.level + n;
    in.w.levelPtr = in.w.queue + n;
    BHS_TRY(side_start(h, ws));
    int* ctl = (int*)ws.ctl.p;
    const int LG = side_lanes(d.n, d.nnzG), LT = side_lanes(d.n, d.nnzT);
    BHS_TRY(timed(h, "bc_check", d.n, [&] {
        const long long most = std::max<long long>(std::max<long long>(d.n, d.nsrc), std::max<long long>(d.nnzG, d.nnzT));
        hipLaunchKernelGGL(k_bc_check, dim3(bc_grid(h, most, 1)), dim3(256), 0, h->stream, d, in.Gp, in.Gj, in.Tp, in.Tj, in.src, ctl);
        return 1;
    }));
    long long passes = 0, backs = 0;
    for (int si = 0; si < d.nsrc; ++si)
        BHS_TRY(with_lanes(LG, [&](auto lg) {
            return with_lanes(LT, [&](auto lt) { return bc_source<decltype(lg)::value, decltype(lt)::value>(h, in, si, ctl, &passes, &backs); });
        }));
    BHS_TRY(timed(h, "bc_finish", d.n, [&] {
        hipLaunchKernelGGL(k_bc_finish, dim3(bc_grid(h, d.n, 1)), dim3(256), 0, h->stream, d, in.w, in.outLevel, in.outSigma, ctl);
        return 1;
    }));
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, BC_INTS));                           // the counts over the sources
    BHS_TRY(side_close(h, ws, ms_out));
    long long reached = 0, levels = 0, overflow = 0, work = 0;
    memcpy(&reached, ws.host + BC_REACHED, sizeof(reached));
    memcpy(&levels, ws.host + BC_LEVELS, sizeof(levels));
    memcpy(&overflow, ws.host + BC_OVERFLOW, sizeof(overflow));
    memcpy(&work, ws.host + BC_WORK, sizeof(work));
    if (ws.host[RD_ERR] || ws.host[BC_FINISHED] != 1) return BHS_ERR_INTERNAL;   // (the check accepted the input)
    if (reached < d.nsrc || reached > (long long)d.nsrc * d.n || levels < d.nsrc || levels > reached || work != levels || work > passes ||
        overflow < 0 || overflow > d.nsrc || backs > levels)
        return BHS_ERR_INTERNAL;
    h->bcLevels = levels;
    h->bcOverflow = overflow;
    h->bcWork = work;
    if (reached_out) *reached_out = (int)std::min<long long>(reached, 0x7fffffff);
    if (passes_out) *passes_out = (int)std::min<long long>(passes, 0x7fffffff);
    return BHS_SUCCESS;
}

}  // namespace

extern "C" {

int bhs_csr_betweenness_device(bhs_handle* h, int n, int nnzG, const int* d_rowPtrG, const int* d_colIndG, int nnzT, const int* d_rowPtrT,
                               const int* d_colIndT, int nsrc, const int* d_sources, int flags, double* d_bc, int* d_level, double* d_sigma,
                               int* reached_out, int* passes_out, double* ms_out)
{
    if (!h || h->ps.open || n < 0 || nnzG < 0 || nnzT < 0 || nsrc < 0 || (flags & ~BHS_BC_ACCUMULATE)) return BHS_ERR_INVALID_ARG;
    if (n > 0 && (nsrc < 1 || !d_sources || !d_rowPtrG || !d_rowPtrT || !d_bc)) return BHS_ERR_INVALID_ARG;
    if ((nnzG > 0 && !d_colIndG) || (nnzT > 0 && !d_colIndT)) return BHS_ERR_INVALID_ARG;
    if (side_aliased({{d_bc, sizeof(double) * (size_t)n}, {d_level, sizeof(int) * (size_t)n}, {d_sigma, sizeof(double) * (size_t)n}},
                     {{d_rowPtrG, sizeof(int) * ((size_t)n + 1)}, {d_colIndG, sizeof(int) * (size_t)nnzG},
                      {d_rowPtrT, sizeof(int) * ((size_t)n + 1)}, {d_colIndT, sizeof(int) * (size_t)nnzT},
                      {d_sources, sizeof(int) * (size_t)nsrc}}))
        return BHS_ERR_INVALID_ARG;
    if (n == 0) {                                                     // no vertex: nothing launched
        h->bcLevels = h->bcOverflow = h->bcWork = 0;
        return side_nothing(reached_out, passes_out, ms_out);
    }
    BcIn in;
    memset(&in, 0, sizeof(in));
    in.d.n = n; in.d.nnzG = nnzG; in.d.nnzT = nnzT; in.d.nsrc = nsrc;
    in.Gp = d_rowPtrG; in.Gj = d_colIndG; in.Tp = d_rowPtrT; in.Tj = d_colIndT; in.src = d_sources;
    in.accumulate = (flags & BHS_BC_ACCUMULATE) ? 1 : 0;
    in.bc = d_bc; in.outLevel = d_level; in.outSigma = d_sigma;
    return guarded(h, [&] { return bc_run(h, in, reached_out, passes_out, ms_out); });
}

}  // extern "C"
