// bhs_host_color.inc.h -- greedy colouring of a pattern and multicolour Gauss-Seidel on top of it (bhs_csr_color_device,
// bhs_csr_gs_device; kernels in bhs_color.hip.h and bhs_gs.hip.h)
// (A part of bhsparse_hip.hip's translation unit, on the shared pieces of bhs_host_side.inc.h; co_order serves the level sets
// of bhs_host_trsv.inc.h too, which is included after this file.)
//
// A workspace of its own (h->colWs), shared by both calls: the control block of bhs_color.hip.h; in its queue buffer the
// second colour array of the rounds (an int a vertex; the first is the caller's d_color); in its count buffer the table of
// vertices per (colour, 64 vertices), colour-major, scanned in place, the scanned offsets copied to h->colOff.
// The colouring: a round is one launch and ONE round trip, for the error word, the count of uncoloured vertices and the
// colours in use (side_rounds: the loop ends when the count is zero, and with BHS_ERR_INTERNAL when a round colours nothing or
// after n + 1 rounds).  The order is three launches and a scan, whatever n, and the call's close one more round trip.
// The relaxation: a launch per non-empty colour and direction, ONE round trip at the end of the call.

#include "bhs_color.hip.h"
#include "bhs_gs.hip.h"

namespace {

// the table of the order (ints): 256 MiB of counts and as much of offsets; beyond it bhs_csr_color_device and
// bhs_csr_levels_device return BHS_ERR_ALLOC
constexpr long long kCoMaxTable = 1ll << 26;

struct CoIn {
    AgDims d;
    const int* Sp; const int* Sj;
    const unsigned* prio;
    int* color; int* order; int* colorPtr;
};

// the rounds between `first` (the caller's d_color, all -1) and `second`: odd rounds read first and write second
template <int L>
int co_rounds(bhs_handle* h, const CoIn& in, int* first, int* second, int* ctl, int* rounds_out)
{
    const AgDims& d = in.d;
    const unsigned rows = (unsigned)(((long long)d.n + 256 / L - 1) / (256 / L));
    const unsigned grid = std::min<unsigned>(rows, (unsigned)h->numCU * 16);   // (a block loop: one add to the count a workgroup)
    return side_rounds(h, h->colWs, d.n, CO_INTS, rounds_out, [&](long long round, long long left) {
        const int* from = (round & 1) ? first : second;
        int* to = (round & 1) ? second : first;
        return timed(h, "color_round", left, [&] {
            hipLaunchKernelGGL(k_col_round<L>, dim3(grid), dim3(256), 0, h->stream, d, in.Sp, in.Sj, in.prio, from, to, ctl);
            return 1;
        });
    });
}

// The order of n vertices by (label, index) and every label's first place, for labels in [0, nlabels): the vertices per
// (label, 64 vertices) counted into a label-major table in ws's count buffer, the library's one-pass scan over it, the
// numbering -- three launches and a scan under the kernel record `name`, whatever n.  The colouring's colours and the level
// sets' levels (bhs_host_trsv.inc.h) both come through here.  ws is prepared again with its ctlInts and queueBytes and the
// table; the caller reads the error word and the total (AG_TOTAL == n) with its next round trip.
int co_order(bhs_handle* h, SideWs& ws, const char* name, int ctlInts, size_t queueBytes, int n, long long nlabels, const int* label,
             int* order, int* labelPtr)
{
    const size_t nWords = ((size_t)n + 63) / 64;
    const long long table = nlabels * (long long)nWords;
    if (table > kCoMaxTable) return BHS_ERR_ALLOC;
    BHS_TRY(side_prepare(h, ws, ctlInts, queueBytes, (size_t)table + 1));
    BHS_TRY(ensure(h, h->colOff, sizeof(int) * ((size_t)table + 1)));
    int* ctl = (int*)ws.ctl.p;
    int* cnt = (int*)ws.cnt.p;
    int* off = (int*)h->colOff.p;
    BHS_HIP(hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)table, h->stream));
    BHS_TRY(timed(h, name, n, [&] {
        hipLaunchKernelGGL(k_col_count, dim3((unsigned)(((size_t)n + 255) / 256)), dim3(256), 0, h->stream, n, (int)nWords, (int)nlabels,
                           label, cnt, ctl);
        return 1;
    }));
    BHS_TRY(side_scan(h, ws, name, kAgScan, (int)table, off, off));
    BHS_TRY(timed(h, name, 0, [&] {
        hipLaunchKernelGGL(k_col_number, dim3((unsigned)(((size_t)n + 1 + 255) / 256)), dim3(256), 0, h->stream, n, (int)nWords, (int)nlabels,
                           label, (const int*)off, order, labelPtr, ctl);
        return 1;
    }));
    return BHS_SUCCESS;
}

int co_run(bhs_handle* h, const CoIn& in, int* ncolors_out, int* rounds_out, double* ms_out)
{
    const AgDims& d = in.d;
    SideWs& ws = h->colWs;
    const size_t n = (size_t)d.n;
    BHS_TRY(side_open(h, ws, CO_INTS, sizeof(int) * n, 0));
    BHS_TRY(side_start(h, ws));
    int* ctl = (int*)ws.ctl.p;
    BHS_HIP(hipMemsetAsync(in.color, 0xFF, sizeof(int) * n, h->stream));   // -1: no colour
    const int L = side_lanes(d.n, d.nnzS);
    int rounds = 0;
    int* second = (int*)ws.queue.p;
    BHS_TRY(with_lanes(L, [&](auto l) { return co_rounds<l.value>(h, in, in.color, second, ctl, &rounds); }));
    if (rounds & 1) BHS_HIP(hipMemcpyAsync(in.color, second, sizeof(int) * n, hipMemcpyDeviceToDevice, h->stream));   // (the last round wrote `second`)
    const long long ncolors = ws.host[CO_NCOL];
    if (ncolors < 1 || ncolors > (long long)d.n) return BHS_ERR_INTERNAL;
    BHS_TRY(co_order(h, ws, "color_order", CO_INTS, sizeof(int) * n, d.n, ncolors, in.color, in.order, in.colorPtr));
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, CO_INTS));                           // the order's error word and total
    BHS_TRY(side_close(h, ws, ms_out));
    long long total = 0;
    memcpy(&total, ws.host + AG_TOTAL, sizeof(total));
    if (ws.host[RD_ERR] || total != (long long)d.n) return BHS_ERR_INTERNAL;   // (the colours were this call's own)
    if (ncolors_out) *ncolors_out = (int)ncolors;
    if (rounds_out) *rounds_out = rounds;
    return BHS_SUCCESS;
}

struct GsIn {
    GsDims d;
    const int* Ap; const int* Aj; const value_t* Ax;
    const value_t* diag;
    int ncolors;
    const int* colorPtr;    // host
    const int* order; const int* color;
    const value_t* b; value_t* x;
    int sweeps, flags;
};

typedef void (*GsKernel)(GsDims, const int*, const int*, const value_t*, const value_t*, const int*, const int*, const value_t*, value_t*, int*);

template <bool V>
GsKernel gs_kernel(int L)
{
    return with_lanes(L, [](auto l) -> GsKernel { return k_gs_color<l.value, V>; });
}

int gs_run(bhs_handle* h, const GsIn& in, double* ms_out)
{
    SideWs& ws = h->colWs;
    BHS_TRY(side_open(h, ws, CO_INTS, 0, 0));
    BHS_TRY(side_start(h, ws));
    int* ctl = (int*)ws.ctl.p;
    const int L = side_lanes(in.d.n, in.d.nnzA);
    const GsKernel kern = (in.flags & BHS_GS_VERIFY) ? gs_kernel<true>(L) : gs_kernel<false>(L);
    const long long listed = in.ncolors > 0 ? in.colorPtr[in.ncolors] : 0;
    auto pass = [&](const char* name, bool backward) {
        return timed(h, name, listed, [&] {
            int launches = 0;
            for (int t = 0; t < in.ncolors; ++t) {
                const int c = backward ? in.ncolors - 1 - t : t;
                GsDims d = in.d;
                d.c = c; d.lo = in.colorPtr[c]; d.cnt = in.colorPtr[c + 1] - in.colorPtr[c];
                if (d.cnt == 0) continue;
                const unsigned grid = (unsigned)(((long long)d.cnt + 256 / L - 1) / (256 / L));
                hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, h->stream, d, in.Ap, in.Aj, in.Ax, in.diag, in.order, in.color,
                                   in.b, in.x, ctl);
                ++launches;
            }
            return launches;
        });
    };
    for (int s = 0; s < in.sweeps; ++s) {
        if (in.flags & BHS_GS_FORWARD) BHS_TRY(pass("gs_forward", false));
        if (in.flags & BHS_GS_BACKWARD) BHS_TRY(pass("gs_backward", true));
    }
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, CO_INTS));                           // the call's one round trip
    BHS_TRY(side_close(h, ws, ms_out));
    return ws.host[RD_ERR] ? (int)BHS_ERR_INVALID_ARG : (int)BHS_SUCCESS;
}

}  // namespace

extern "C" {

int bhs_csr_color_device(bhs_handle* h, int n, int nnzS, const int* d_rowPtrS, const int* d_colIndS, const unsigned* d_prio,
                         unsigned seed, int flags, int* d_color, int* d_order, int* d_colorPtr, int* ncolors_out, int* rounds_out,
                         double* ms_out)
{
    if (!h || h->ps.open || n < 0 || nnzS < 0 || flags != 0) return BHS_ERR_INVALID_ARG;
    if ((n > 0 && (!d_rowPtrS || !d_color || !d_order || !d_colorPtr)) || (nnzS > 0 && !d_colIndS)) return BHS_ERR_INVALID_ARG;
    if (side_aliased({{d_color, sizeof(int) * (size_t)n}, {d_order, sizeof(int) * (size_t)n}, {d_colorPtr, sizeof(int) * ((size_t)n + 1)}},
                     {{d_rowPtrS, sizeof(int) * ((size_t)n + 1)}, {d_colIndS, sizeof(int) * (size_t)nnzS}, {d_prio, sizeof(unsigned) * (size_t)n}}))
        return BHS_ERR_INVALID_ARG;
    if (n == 0) return side_nothing(ncolors_out, rounds_out, ms_out);  // nothing to colour, nothing launched
    CoIn in;
    in.d.n = n; in.d.nnzS = nnzS; in.d.seed = seed; in.d.hasPrio = d_prio ? 1 : 0;
    in.Sp = d_rowPtrS; in.Sj = d_colIndS; in.prio = d_prio; in.color = d_color; in.order = d_order; in.colorPtr = d_colorPtr;
    return guarded(h, [&] { return co_run(h, in, ncolors_out, rounds_out, ms_out); });
}

int bhs_csr_gs_device(bhs_handle* h, int n, int nnzA, const int* d_rowPtrA, const int* d_colIndA, const bhs_value_t* d_valA,
                      const bhs_value_t* d_diag, int ncolors, const int* h_colorPtr, const int* d_order, const int* d_color,
                      const bhs_value_t* d_b, bhs_value_t* d_x, double omega, int sweeps, int flags, double* ms_out)
{
    if (!h || h->ps.open || n < 0 || nnzA < 0 || ncolors < 0 || sweeps < 0) return BHS_ERR_INVALID_ARG;
    if ((flags & ~(BHS_GS_SYMMETRIC | BHS_GS_VERIFY)) || !(flags & BHS_GS_SYMMETRIC)) return BHS_ERR_INVALID_ARG;
    if ((flags & BHS_GS_VERIFY) && !d_color) return BHS_ERR_INVALID_ARG;
    if (ncolors > n || (ncolors > 0 && !h_colorPtr)) return BHS_ERR_INVALID_ARG;
    if (ncolors > 0) {                                                // the host's array: starts at 0, never falls, ends within n
        if (h_colorPtr[0] != 0) return BHS_ERR_INVALID_ARG;
        for (int c = 0; c < ncolors; ++c)
            if (h_colorPtr[c + 1] < h_colorPtr[c] || h_colorPtr[c + 1] > n) return BHS_ERR_INVALID_ARG;
    }
    const int listed = ncolors > 0 ? h_colorPtr[ncolors] : 0;
    if (listed > 0 && (!d_rowPtrA || !d_diag || !d_order || !d_b || !d_x)) return BHS_ERR_INVALID_ARG;
    if (nnzA > 0 && (!d_colIndA || !d_valA)) return BHS_ERR_INVALID_ARG;
    const size_t vec = sizeof(value_t) * (size_t)n;
    if (side_aliased({{d_x, vec}},                                    // (x is the one array written)
                     {{d_rowPtrA, sizeof(int) * ((size_t)n + 1)}, {d_colIndA, sizeof(int) * (size_t)nnzA}, {d_valA, sizeof(value_t) * (size_t)nnzA},
                      {d_diag, vec}, {d_order, sizeof(int) * (size_t)listed}, {d_color, sizeof(int) * (size_t)n}, {d_b, vec}}))
        return BHS_ERR_INVALID_ARG;
    if (listed == 0 || sweeps == 0) {                                 // nothing to relax, nothing launched
        if (ms_out) *ms_out = 0.0;
        return BHS_SUCCESS;
    }
    GsIn in;
    in.d.n = n; in.d.nnzA = nnzA; in.d.lo = in.d.cnt = in.d.c = 0; in.d.plain = omega == 1.0 ? 1 : 0; in.d.omega = omega;
    in.Ap = d_rowPtrA; in.Aj = d_colIndA; in.Ax = (const value_t*)d_valA; in.diag = (const value_t*)d_diag;
    in.ncolors = ncolors; in.colorPtr = h_colorPtr; in.order = d_order; in.color = d_color;
    in.b = (const value_t*)d_b; in.x = (value_t*)d_x; in.sweeps = sweeps; in.flags = flags;
    return guarded(h, [&] { return gs_run(h, in, ms_out); });
}

}  // extern "C"
