// bhs_host_scc.inc.h -- the strongly connected components of a pattern (bhs_csr_scc_device; kernels in bhs_scc.hip.h)
// (A part of bhsparse_hip.hip's translation unit, on the shared pieces of bhs_host_side.inc.h.)
//
// A workspace of its own (h->sccWs): the control block of bhs_scc.hip.h; in its queue buffer part, stamp and reach, n ints
// each, and where the components are numbered the root bitmap (a word per 64 vertices) and the scanned offsets behind them;
// in its count buffer the roots per bitmap word, scanned in place.  The labels are the caller's d_root itself.
// The rounds are side_rounds'; inside a round the trim, the forward labels and the backward reach are three side_passes
// loops: kSccBatch passes a control round trip, each ends after a batch whose last pass changed nothing, and with
// BHS_ERR_INTERNAL when more than n + 1 passes would be needed.  A round whose trim leaves no live vertex ends there.  The
// components decided are counted on the device as they are decided; the numbering adds four launches, the scan among them,
// and the call's close is one more round trip, whatever n.

#include "bhs_scc.hip.h"

namespace {

constexpr int kSccBatch = 8;        // passes of a phase between two reads of the control words

struct SccIn {
    AgDims d;
    const int* Sp; const int* Sj;
    int* root; int* comp; int* size;
    int* part; int* stamp; int* reach;
};

template <int L>
int scc_rounds(bhs_handle* h, const SccIn& in, int* ctl, int* rounds_out, int* passes_out)
{
    const AgDims& d = in.d;
    SideWs& ws = h->sccWs;
    const unsigned cap = (unsigned)h->numCU * 16;                     // (block loops: one add to a count a workgroup)
    const unsigned gridL = std::min<unsigned>((unsigned)(((long long)d.n + 256 / L - 1) / (256 / L)), cap);
    const unsigned gridN = std::min<unsigned>((unsigned)(((long long)d.n + 255) / 256), cap);
    long long total = 0;
    int stamp = 0;                                                    // a value of its own for every trim pass of the call
    auto phase = [&](auto&& launch) {
        int passes = 0;
        const int rc = side_passes(h, ws, d.n, kSccBatch, 3, SCC_INTS, &passes, launch);
        total += passes;
        return rc;
    };
    const int rc = side_rounds(h, ws, d.n, SCC_INTS, rounds_out, [&](long long, long long) -> int {
        BHS_TRY(phase([&] {
            return timed(h, "scc_trim", d.n, [&] {
                ++stamp;
                hipLaunchKernelGGL(k_scc_mark<L>, dim3(gridL), dim3(256), 0, h->stream, d, in.Sp, in.Sj, (const int*)in.part, in.stamp,
                                   stamp, ctl);
                hipLaunchKernelGGL(k_scc_trim<L>, dim3(gridL), dim3(256), 0, h->stream, d, in.Sp, in.Sj, in.part, (const int*)in.stamp,
                                   in.root, stamp, ctl);
                return 2;
            });
        }));
        if (ws.host[SCC_LIVE] == 0) return (int)BHS_SUCCESS;          // (the last trim pass killed nothing: its count is the live set)
        BHS_TRY(timed(h, "scc_forward", 0, [&] {
            hipLaunchKernelGGL(k_scc_start, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)in.part, in.root);
            return 1;
        }));
        BHS_TRY(phase([&] {
            return timed(h, "scc_forward", d.n, [&] {
                hipLaunchKernelGGL(k_scc_forward<L>, dim3(gridL), dim3(256), 0, h->stream, d, in.Sp, in.Sj, (const int*)in.part, in.root, ctl);
                return 1;
            });
        }));
        BHS_TRY(timed(h, "scc_backward", 0, [&] {
            hipLaunchKernelGGL(k_scc_seed, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)in.part, (const int*)in.root, in.reach);
            return 1;
        }));
        BHS_TRY(phase([&] {
            return timed(h, "scc_backward", d.n, [&] {
                hipLaunchKernelGGL(k_scc_backward<L>, dim3(gridL), dim3(256), 0, h->stream, d, in.Sp, in.Sj, (const int*)in.part,
                                   (const int*)in.root, in.reach, ctl);
                return 1;
            });
        }));
        return timed(h, "scc_decide", d.n, [&] {                      // (both loops left the count at zero: it is the decide's alone)
            hipLaunchKernelGGL(k_scc_decide, dim3(gridN), dim3(256), 0, h->stream, d.n, in.part, (const int*)in.root, (const int*)in.reach, ctl);
            return 1;
        });
    });
    *passes_out = (int)std::min<long long>(total, 0x7fffffff);
    return rc;
}

int scc_run(bhs_handle* h, SccIn& in, int* nscc_out, int* rounds_out, int* passes_out, double* ms_out)
{
    const AgDims& d = in.d;
    SideWs& ws = h->sccWs;
    const size_t n = (size_t)d.n, nWords = (n + 63) / 64;
    const size_t stateBytes = (sizeof(int) * 3 * n + 7) / 8 * 8;      // part, stamp, reach; the bitmap behind them is of 64-bit words
    const bool number = in.comp != nullptr;
    BHS_TRY(side_open(h, ws, SCC_INTS, stateBytes + (number ? sizeof(rd_u64) * nWords + sizeof(int) * (nWords + 1) : 0),
                      number ? nWords + 1 : 0));
    in.part = (int*)ws.queue.p;
    in.stamp = in.part + n;
    in.reach = in.stamp + n;
    BHS_HIP(hipMemsetAsync(in.part, 0, sizeof(int) * 2 * n, h->stream));   // one class, and no stamp of this call's
    BHS_TRY(side_start(h, ws));
    int* ctl = (int*)ws.ctl.p;
    const int L = side_lanes(d.n, d.nnzS);
    int rounds = 0, passes = 0;
    BHS_TRY(with_lanes(L, [&](auto l) { return scc_rounds<l.value>(h, in, ctl, &rounds, &passes); }));
    if (number) {
        rd_u64* map = (rd_u64*)((char*)ws.queue.p + stateBytes);
        int* off = (int*)(map + nWords);
        int* cnt = (int*)ws.cnt.p;
        const unsigned gridN = (unsigned)((n + 255) / 256);
        BHS_TRY(timed(h, "scc_number", d.n, [&] {
            hipLaunchKernelGGL(k_cc_flag, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)in.root, map, cnt);
            return 1;
        }));
        BHS_TRY(side_scan(h, ws, "scc_number", kAgScan, (int)nWords, off, off));
        BHS_TRY(timed(h, "scc_number", 0, [&] {
            int launches = 1;
            if (in.size) {
                hipLaunchKernelGGL(k_cc_clear, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)ctl, in.size);
                ++launches;
            }
            hipLaunchKernelGGL(k_cc_number, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)in.root, (const rd_u64*)map,
                               (const int*)off, in.comp, in.size, ctl);
            return launches;
        }));
    }
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, SCC_INTS));                          // the count, the numbering's error word and total
    BHS_TRY(side_close(h, ws, ms_out));
    const long long nscc = ws.host[SCC_COUNT];
    if (nscc < 1 || nscc > (long long)d.n) return BHS_ERR_INTERNAL;
    if (number) {
        long long total = 0;
        memcpy(&total, ws.host + AG_TOTAL, sizeof(total));
        if (ws.host[RD_ERR] || total != nscc) return BHS_ERR_INTERNAL;   // (the roots were this call's own)
    }
    if (nscc_out) *nscc_out = (int)nscc;
    if (rounds_out) *rounds_out = rounds;
    if (passes_out) *passes_out = passes;
    return BHS_SUCCESS;
}

}  // namespace

extern "C" {

int bhs_csr_scc_device(bhs_handle* h, int n, int nnzS, const int* d_rowPtrS, const int* d_colIndS, int flags, int* d_root, int* d_comp,
                       int* d_compSize, int* nscc_out, int* rounds_out, int* passes_out, double* ms_out)
{
    if (!h || h->ps.open || n < 0 || nnzS < 0 || flags != 0) return BHS_ERR_INVALID_ARG;
    if ((n > 0 && (!d_rowPtrS || !d_root)) || (nnzS > 0 && !d_colIndS)) return BHS_ERR_INVALID_ARG;
    if (d_compSize && !d_comp) return BHS_ERR_INVALID_ARG;
    if (side_aliased({{d_root, sizeof(int) * (size_t)n}, {d_comp, sizeof(int) * (size_t)n}, {d_compSize, sizeof(int) * (size_t)n}},
                     {{d_rowPtrS, sizeof(int) * ((size_t)n + 1)}, {d_colIndS, sizeof(int) * (size_t)nnzS}}))
        return BHS_ERR_INVALID_ARG;
    if (n == 0) {                                                     // no vertex, no component, nothing launched
        if (rounds_out) *rounds_out = 0;
        return side_nothing(nscc_out, passes_out, ms_out);
    }
    SccIn in;
    in.d.n = n; in.d.nnzS = nnzS; in.d.seed = 0; in.d.hasPrio = 0;
    in.Sp = d_rowPtrS; in.Sj = d_colIndS; in.root = d_root; in.comp = d_comp; in.size = d_compSize;
    in.part = in.stamp = in.reach = nullptr;
    return guarded(h, [&] { return scc_run(h, in, nscc_out, rounds_out, passes_out, ms_out); });
}

}  // extern "C"
