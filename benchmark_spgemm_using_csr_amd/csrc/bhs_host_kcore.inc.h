// bhs_host_kcore.inc.h -- the k-core decomposition of a pattern (bhs_csr_kcore_device; kernels in bhs_kcore.hip.h)
// (A part of bhsparse_hip.hip's translation unit, on the shared pieces of bhs_host_side.inc.h; the check is
// bhs_rcm.hip.h's, launched under this call's own record.)
//
// A workspace of its own (h->coreWs): the control block of bhs_kcore.hip.h; in its queue buffer the degrees and the queue,
// n ints each.  The loop is side_passes': kCoreBatch passes of four launches a control round trip, the count being the
// vertices still present, which the last launch of a pass writes; it ends after a batch whose last pass left none, and with
// BHS_ERR_INTERNAL when more than n + 1 passes would be needed (a pass removes a vertex while one is present).  There is no
// round trip behind the check: once it has raised the error word every later launch leaves at once, so a refused pattern
// has written no output when the first batch's read finds the word.  The passes behind the last round are no-ops that leave
// at once.  The call's close is one more round trip, whatever n.

#include "bhs_kcore.hip.h"

namespace {

constexpr int kCoreBatch = 8;       // passes between two reads of the control words

struct CoreIn {
    AgDims d;
    const int* Sp; const int* Sj;
    int* core; int* round;
    int* deg; int* queue;
};

template <int L>
int core_passes(bhs_handle* h, const CoreIn& in, int* ctl, int* passes_out)
{
    const AgDims& d = in.d;
    SideWs& ws = h->coreWs;
    const unsigned cap = (unsigned)h->numCU * 16;                     // (block loops)
    const unsigned gridL = std::min<unsigned>((unsigned)(((long long)d.n + 256 / L - 1) / (256 / L)), cap);
    const unsigned gridN = std::min<unsigned>((unsigned)(((long long)d.n + 255) / 256), cap);
    return side_passes(h, ws, d.n, kCoreBatch, 2, CORE_INTS, passes_out, [&] {
        BHS_TRY(timed(h, "kcore_peel", d.n, [&] {
            hipLaunchKernelGGL(k_core_peel<L>, dim3(gridL), dim3(256), 0, h->stream, d, in.Sp, in.Sj, in.deg, in.queue, in.core, in.round, ctl);
            return 1;
        }));
        return timed(h, "kcore_advance", d.n, [&] {
            hipLaunchKernelGGL(k_core_min, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)in.deg, ctl);
            hipLaunchKernelGGL(k_core_gather, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)in.deg, in.queue, in.core, in.round, ctl);
            hipLaunchKernelGGL(k_core_advance, dim3(1), dim3(64), 0, h->stream, d.n, ctl);
            return 3;
        });
    });
}

int core_run(bhs_handle* h, CoreIn& in, int* kmax_out, int* rounds_out, double* ms_out)
{
    const AgDims& d = in.d;
    SideWs& ws = h->coreWs;
    const size_t n = (size_t)d.n;
    BHS_TRY(side_open(h, ws, CORE_INTS, sizeof(int) * 2 * n, 0));
    in.deg = (int*)ws.queue.p;
    in.queue = in.deg + n;
    BHS_TRY(side_start(h, ws));
    int* ctl = (int*)ws.ctl.p;
    const int L = side_lanes(d.n, d.nnzS);
    const unsigned cap = (unsigned)h->numCU * 16;
    BHS_TRY(with_lanes(L, [&](auto l) {
        return timed(h, "kcore_check", d.n, [&] {
            const unsigned grid = std::min<unsigned>((unsigned)(((long long)d.n + 256 / l.value - 1) / (256 / l.value)), cap);
            hipLaunchKernelGGL(k_rcm_check<l.value>, dim3(grid), dim3(256), 0, h->stream, d, in.Sp, in.Sj, in.deg, ctl);
            return 1;
        });
    }));
    BHS_TRY(timed(h, "kcore_advance", 0, [&] {
        hipLaunchKernelGGL(k_core_begin, dim3(1), dim3(64), 0, h->stream, ctl);
        return 1;
    }));
    int passes = 0;
    BHS_TRY(with_lanes(L, [&](auto l) { return core_passes<l.value>(h, in, ctl, &passes); }));
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, CORE_INTS));                         // the level and the round the last slice had
    BHS_TRY(side_close(h, ws, ms_out));
    const long long kmax = ws.host[CORE_K], rounds = ws.host[CORE_ROUND];
    if (ws.host[RD_ERR] || ws.host[CORE_TAIL] != d.n) return BHS_ERR_INTERNAL;   // (the check accepted the pattern)
    if (kmax < 0 || kmax >= (long long)d.n || rounds < 1 || rounds > (long long)passes) return BHS_ERR_INTERNAL;
    if (kmax_out) *kmax_out = (int)kmax;
    if (rounds_out) *rounds_out = (int)rounds;
    return BHS_SUCCESS;
}

}  // namespace

extern "C" {

int bhs_csr_kcore_device(bhs_handle* h, int n, int nnzS, const int* d_rowPtrS, const int* d_colIndS, int flags, int* d_core, int* d_round,
                         int* kmax_out, int* rounds_out, double* ms_out)
{
    if (!h || h->ps.open || n < 0 || nnzS < 0 || flags != 0) return BHS_ERR_INVALID_ARG;
    if ((n > 0 && (!d_rowPtrS || !d_core)) || (nnzS > 0 && !d_colIndS)) return BHS_ERR_INVALID_ARG;
    if (side_aliased({{d_core, sizeof(int) * (size_t)n}, {d_round, sizeof(int) * (size_t)n}},
                     {{d_rowPtrS, sizeof(int) * ((size_t)n + 1)}, {d_colIndS, sizeof(int) * (size_t)nnzS}}))
        return BHS_ERR_INVALID_ARG;
    if (n == 0) return side_nothing(kmax_out, rounds_out, ms_out);    // no vertex: nothing launched
    CoreIn in;
    in.d.n = n; in.d.nnzS = nnzS; in.d.seed = 0; in.d.hasPrio = 0;
    in.Sp = d_rowPtrS; in.Sj = d_colIndS; in.core = d_core; in.round = d_round;
    in.deg = in.queue = nullptr;
    return guarded(h, [&] { return core_run(h, in, kmax_out, rounds_out, ms_out); });
}

}  // extern "C"
