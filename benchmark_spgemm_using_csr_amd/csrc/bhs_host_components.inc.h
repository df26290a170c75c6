// bhs_host_components.inc.h -- the connected components of a pattern (bhs_csr_components_device; kernels in
// bhs_components.hip.h)
// (A part of bhsparse_hip.hip's translation unit, on the shared pieces of bhs_host_side.inc.h.)
//
// A workspace of its own (h->ccWs): the control block of bhs_components.hip.h; where the components are numbered, in its
// queue buffer the root bitmap (a word per 64 vertices) and the scanned offsets behind it, in its count buffer the roots per
// bitmap word, scanned in place.  The parent array is the caller's d_root itself.
// The relaxation is the level sets' loop (side_passes): kCcBatch passes a control round trip, for the error word, the words
// the batch's last pass lowered and the roots it saw; the loop ends after a batch whose last pass lowered nothing, and with
// BHS_ERR_INTERNAL when more than n + 1 passes would be needed.  The numbering adds four launches, the scan among them; the
// call's close is one more round trip, whatever n.

#include "bhs_components.hip.h"

namespace {

constexpr int kCcBatch = 8;         // passes of the relaxation between two reads of the control words

struct CcIn {
    AgDims d;
    const int* Sp; const int* Sj;
    int* root; int* comp; int* size;
};

template <int L>
int cc_passes(bhs_handle* h, const CcIn& in, int* ctl, int* passes_out)
{
    const AgDims& d = in.d;
    const unsigned rows = (unsigned)(((long long)d.n + 256 / L - 1) / (256 / L));
    const unsigned grid = std::min<unsigned>(rows, (unsigned)h->numCU * 16);   // (a block loop: one add to the count a workgroup)
    // (lowering both ends alone carries a minimum one edge a pass: n passes lower, one more finds nothing; the count and the
    // roots are the last pass's alone)
    return side_passes(h, h->ccWs, d.n, kCcBatch, 4, CC_INTS, passes_out, [&] {
        return timed(h, "components_pass", d.n, [&] {
            hipLaunchKernelGGL(k_cc_pass<L>, dim3(grid), dim3(256), 0, h->stream, d, in.Sp, in.Sj, in.root, ctl);
            return 1;
        });
    });
}

int cc_run(bhs_handle* h, const CcIn& in, int* ncomp_out, int* passes_out, double* ms_out)
{
    const AgDims& d = in.d;
    SideWs& ws = h->ccWs;
    const size_t n = (size_t)d.n, nWords = (n + 63) / 64;
    const bool number = in.comp != nullptr;
    BHS_TRY(side_open(h, ws, CC_INTS, number ? sizeof(rd_u64) * nWords + sizeof(int) * (nWords + 1) : 0, number ? nWords + 1 : 0));
    BHS_TRY(side_start(h, ws));
    int* ctl = (int*)ws.ctl.p;
    const unsigned gridN = (unsigned)((n + 255) / 256);
    BHS_TRY(timed(h, "components_pass", 0, [&] {
        hipLaunchKernelGGL(k_cc_init, dim3(gridN), dim3(256), 0, h->stream, d.n, in.root);
        return 1;
    }));
    const int L = side_lanes(d.n, d.nnzS);
    int passes = 0;
    BHS_TRY(with_lanes(L, [&](auto l) { return cc_passes<l.value>(h, in, ctl, &passes); }));
    const long long ncomp = ws.host[CC_ROOTS];                        // (the last pass read the fixed point: its roots are the components)
    if (ncomp < 1 || ncomp > (long long)d.n) return BHS_ERR_INTERNAL;
    if (number) {
        rd_u64* map = (rd_u64*)ws.queue.p;
        int* off = (int*)(map + nWords);
        int* cnt = (int*)ws.cnt.p;
        BHS_TRY(timed(h, "components_number", d.n, [&] {
            hipLaunchKernelGGL(k_cc_flag, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)in.root, map, cnt);
            return 1;
        }));
        BHS_TRY(side_scan(h, ws, "components_number", kAgScan, (int)nWords, off, off));
        BHS_TRY(timed(h, "components_number", 0, [&] {
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
    BHS_TRY(side_read_ctl(h, ws, CC_INTS));                           // the numbering's error word and total (the span's end in any case)
    BHS_TRY(side_close(h, ws, ms_out));
    if (number) {
        long long total = 0;
        memcpy(&total, ws.host + AG_TOTAL, sizeof(total));
        if (ws.host[RD_ERR] || total != ncomp) return BHS_ERR_INTERNAL;   // (the roots were this call's own)
    }
    if (ncomp_out) *ncomp_out = (int)ncomp;
    if (passes_out) *passes_out = passes;
    return BHS_SUCCESS;
}

}  // namespace

extern "C" {

int bhs_csr_components_device(bhs_handle* h, int n, int nnzS, const int* d_rowPtrS, const int* d_colIndS, int flags, int* d_root,
                              int* d_comp, int* d_compSize, int* ncomp_out, int* passes_out, double* ms_out)
{
    if (!h || h->ps.open || n < 0 || nnzS < 0 || flags != 0) return BHS_ERR_INVALID_ARG;
    if ((n > 0 && (!d_rowPtrS || !d_root)) || (nnzS > 0 && !d_colIndS)) return BHS_ERR_INVALID_ARG;
    if (d_compSize && !d_comp) return BHS_ERR_INVALID_ARG;
    if (side_aliased({{d_root, sizeof(int) * (size_t)n}, {d_comp, sizeof(int) * (size_t)n}, {d_compSize, sizeof(int) * (size_t)n}},
                     {{d_rowPtrS, sizeof(int) * ((size_t)n + 1)}, {d_colIndS, sizeof(int) * (size_t)nnzS}}))
        return BHS_ERR_INVALID_ARG;
    if (n == 0) return side_nothing(ncomp_out, passes_out, ms_out);    // no vertex, no component, nothing launched
    CcIn in;
    in.d.n = n; in.d.nnzS = nnzS; in.d.seed = 0; in.d.hasPrio = 0;
    in.Sp = d_rowPtrS; in.Sj = d_colIndS; in.root = d_root; in.comp = d_comp; in.size = d_compSize;
    return guarded(h, [&] { return cc_run(h, in, ncomp_out, passes_out, ms_out); });
}

}  // extern "C"
