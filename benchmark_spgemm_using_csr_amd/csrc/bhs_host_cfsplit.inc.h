// bhs_host_cfsplit.inc.h -- C/F splitting of a pattern of strong connections and direct interpolation on it
// (bhs_csr_cfsplit_device, bhs_csr_interp_symbolic_device, bhs_csr_interp_numeric_device; kernels in bhs_cfsplit.hip.h and
// bhs_interp.hip.h)
// (A part of bhsparse_hip.hip's translation unit, on the shared pieces of bhs_host_side.inc.h.)
//
// A workspace of its own (h->cfWs), shared by the three calls: the control block of bhs_aggregate.hip.h.
// The splitting: in its queue buffer the two arrays of the vertices' words (8 bytes a vertex each; a round reads one and
// writes the other), the C-point bitmap (a word per 64 vertices) and the scanned offsets behind it; in its count buffer the
// C points per bitmap word, scanned in place.  A round is one launch and ONE round trip, for the error word and the count of
// undecided vertices (side_rounds: the loop ends when the count is zero, and with BHS_ERR_INTERNAL when a round decides
// nothing or after n + 1 rounds).  The numbering adds three launches, the scan among them; the call's close is one more
// round trip, whatever n.
// The interpolation: in its count buffer the entries per row of P, scanned in place and copied to the caller's row pointer.
// The symbolic call makes ONE round trip (the error word and nnzP), the numeric call two: the count pass' error word ahead of
// the fill -- a row pointer that is not this splitting's writes nothing --, then the fill's.

#include "bhs_cfsplit.hip.h"
#include "bhs_interp.hip.h"

namespace {

struct CfIn {
    AgDims d;
    int degree;
    const int* Sp; const int* Sj;
    const unsigned* prio;
    int* cf; int* cpts;
};

// the rounds between the word arrays `first` (k_cf_init's) and `second`: odd rounds read first and write second
template <int L>
int cf_rounds(bhs_handle* h, const CfIn& in, rd_u64* first, rd_u64* second, int* ctl, int* rounds_out)
{
    const AgDims& d = in.d;
    const unsigned rows = (unsigned)(((long long)d.n + 256 / L - 1) / (256 / L));
    const unsigned grid = std::min<unsigned>(rows, (unsigned)h->numCU * 16);   // (a block loop: one add to the count a workgroup)
    return side_rounds(h, h->cfWs, d.n, AG_INTS, rounds_out, [&](long long round, long long left) {
        const rd_u64* from = (round & 1) ? first : second;
        rd_u64* to = (round & 1) ? second : first;
        return timed(h, "cf_round", left, [&] {
            hipLaunchKernelGGL(k_cf_round<L>, dim3(grid), dim3(256), 0, h->stream, d, in.Sp, in.Sj, from, to, ctl);
            return 1;
        });
    });
}

int cf_run(bhs_handle* h, const CfIn& in, int* nc_out, int* rounds_out, double* ms_out)
{
    const AgDims& d = in.d;
    SideWs& ws = h->cfWs;
    const size_t n = (size_t)d.n, nWords = (n + 63) / 64;
    BHS_TRY(side_open(h, ws, AG_INTS, sizeof(rd_u64) * (2 * n + nWords) + sizeof(int) * (nWords + 1), nWords + 1));
    BHS_TRY(side_start(h, ws));
    int* ctl = (int*)ws.ctl.p;
    int* cnt = (int*)ws.cnt.p;
    rd_u64* w0 = (rd_u64*)ws.queue.p;
    rd_u64* w1 = w0 + n;
    rd_u64* map = w1 + n;
    int* off = (int*)(map + nWords);
    const unsigned gridN = (unsigned)((n + 255) / 256);
    BHS_TRY(timed(h, "cf_init", d.n, [&] {
        hipLaunchKernelGGL(k_cf_init, dim3(gridN), dim3(256), 0, h->stream, d, in.degree, in.Sp, in.prio, w0, ctl);
        return 1;
    }));
    const int L = side_lanes(d.n, d.nnzS);
    int rounds = 0;
    BHS_TRY(with_lanes(L, [&](auto l) { return cf_rounds<l.value>(h, in, w0, w1, ctl, &rounds); }));
    const rd_u64* w = (rounds & 1) ? w1 : w0;                        // (the array the last round wrote)
    BHS_TRY(timed(h, "cf_number", d.n, [&] {
        hipLaunchKernelGGL(k_agg_count, dim3(gridN), dim3(256), 0, h->stream, d.n, w, map, cnt);
        return 1;
    }));
    BHS_TRY(side_scan(h, ws, "cf_number", kAgScan, (int)nWords, off, off));
    BHS_TRY(timed(h, "cf_number", 0, [&] {
        hipLaunchKernelGGL(k_cf_number, dim3(gridN), dim3(256), 0, h->stream, d.n, (const rd_u64*)map, (const int*)off, in.cf, in.cpts, ctl);
        return 1;
    }));
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, AG_INTS));                           // the number of C points
    BHS_TRY(side_close(h, ws, ms_out));
    long long nc = 0;
    memcpy(&nc, ws.host + AG_TOTAL, sizeof(nc));
    if (ws.host[RD_ERR] || nc < 1 || nc > (long long)d.n) return BHS_ERR_INTERNAL;   // (the words were this call's own)
    if (nc_out) *nc_out = (int)nc;
    if (rounds_out) *rounds_out = rounds;
    return BHS_SUCCESS;
}

struct IpIn {
    IpDims d;
    const int* Ap; const int* Aj; const value_t* Ax;
    const int* Sp; const int* Sj;
    const int* cf;
};

typedef void (*IpCount)(IpDims, const int*, const int*, const int*, const int*, const int*, const int*, int*, int*);
typedef void (*IpFill)(IpDims, const int*, const int*, const value_t*, const int*, const int*, const int*, const int*, int*, value_t*, int*);

// the count pass: into ws.cnt (Pp null), or against the row pointer Pp
int ip_count(bhs_handle* h, const IpIn& in, const int* Pp)
{
    SideWs& ws = h->cfWs;
    const int L = side_lanes(in.d.n, in.d.nnzA);                     // (lanes per row from A's mean row length)
    const IpCount kern = with_lanes(L, [](auto l) -> IpCount { return k_ip_count<l.value>; });
    const unsigned grid = (unsigned)(((long long)in.d.n + 256 / L - 1) / (256 / L));
    return timed(h, "interp_count", in.d.n, [&] {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, h->stream, in.d, in.Ap, in.Aj, in.Sp, in.Sj, in.cf, Pp, (int*)ws.cnt.p,
                           (int*)ws.ctl.p);
        return 1;
    });
}

int ip_symbolic_run(bhs_handle* h, const IpIn& in, int* Pp, long long* nnzP_out, double* ms_out)
{
    SideWs& ws = h->cfWs;
    const int n = in.d.n;
    BHS_TRY(side_open(h, ws, AG_INTS, sizeof(int) * ((size_t)n + 1), (size_t)n + 1));
    BHS_TRY(side_start(h, ws));
    BHS_TRY(ip_count(h, in, nullptr));
    // (without bins any array of n + 1 ints will do for the scan's row pointer: the queue buffer)
    BHS_TRY(side_scan(h, ws, "interp_count", kAgScan, n, (const int*)ws.queue.p, (int*)ws.queue.p));
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, AG_INTS));                           // the error word and nnzP: the call's one round trip
    BHS_TRY(side_close(h, ws, ms_out));
    if (ws.host[RD_ERR]) return BHS_ERR_INVALID_ARG;                  // (nothing caller-owned has been written)
    long long nnzP = 0;
    memcpy(&nnzP, ws.host + AG_TOTAL, sizeof(nnzP));
    if (nnzP < 0) return BHS_ERR_INTERNAL;
    if (nnzP > 0x7fffffffLL) return BHS_ERR_ALLOC;
    BHS_HIP(hipMemcpyAsync(Pp, ws.queue.p, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToDevice, h->stream));
    BHS_TRY(wait_stream(h));
    if (nnzP_out) *nnzP_out = nnzP;
    return BHS_SUCCESS;
}

int ip_numeric_run(bhs_handle* h, const IpIn& in, const int* Pp, int* Pj, value_t* Px, double* ms_out)
{
    SideWs& ws = h->cfWs;
    BHS_TRY(side_open(h, ws, AG_INTS, 0, 0));
    BHS_TRY(side_start(h, ws));
    int* ctl = (int*)ws.ctl.p;
    BHS_TRY(ip_count(h, in, Pp));                                     // (every row's count is what rowPtrP says, or nothing is written)
    BHS_TRY(side_read_ctl(h, ws, AG_INTS));
    if (ws.host[RD_ERR]) return BHS_ERR_INVALID_ARG;
    const int L = side_lanes(in.d.n, in.d.nnzA);
    const IpFill kern = with_lanes(L, [](auto l) -> IpFill { return k_ip_fill<l.value>; });
    const unsigned grid = (unsigned)(((long long)in.d.n + 256 / L - 1) / (256 / L));
    BHS_TRY(timed(h, "interp_fill", in.d.n, [&] {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, h->stream, in.d, in.Ap, in.Aj, in.Ax, in.Sp, in.Sj, in.cf, Pp, Pj, Px, ctl);
        return 1;
    }));
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, AG_INTS));
    BHS_TRY(side_close(h, ws, ms_out));
    return ws.host[RD_ERR] ? (int)BHS_ERR_INVALID_ARG : (int)BHS_SUCCESS;
}

bool ip_args_ok(bhs_handle* h, int n, int nnzA, const int* Ap, const int* Aj, int nnzS, const int* Sp, const int* Sj, const int* cf,
                int nc)
{
    if (!h || h->ps.open || n < 0 || nnzA < 0 || nnzS < 0 || nc < 0 || nc > n) return false;
    if (n > 0 && (!Ap || !Sp || !cf)) return false;
    return !(nnzA > 0 && !Aj) && !(nnzS > 0 && !Sj);
}

}  // namespace

extern "C" {

int bhs_csr_cfsplit_device(bhs_handle* h, int n, int nnzS, const int* d_rowPtrS, const int* d_colIndS, const unsigned* d_prio,
                           unsigned seed, int flags, int* d_cf, int* d_cpts, int* nc_out, int* rounds_out, double* ms_out)
{
    if (!h || h->ps.open || n < 0 || nnzS < 0 || (flags & ~BHS_CF_DEGREE)) return BHS_ERR_INVALID_ARG;
    if ((flags & BHS_CF_DEGREE) && d_prio) return BHS_ERR_INVALID_ARG;
    if ((n > 0 && (!d_rowPtrS || !d_cf)) || (nnzS > 0 && !d_colIndS)) return BHS_ERR_INVALID_ARG;
    const size_t outBytes = sizeof(int) * (size_t)n;
    if (side_aliased({{d_cf, outBytes}, {d_cpts, outBytes}},
                     {{d_rowPtrS, sizeof(int) * ((size_t)n + 1)}, {d_colIndS, sizeof(int) * (size_t)nnzS}, {d_prio, sizeof(unsigned) * (size_t)n}}))
        return BHS_ERR_INVALID_ARG;
    if (n == 0) return side_nothing(nc_out, rounds_out, ms_out);       // nothing to split, nothing launched
    CfIn in;
    in.d.n = n; in.d.nnzS = nnzS; in.d.seed = seed; in.d.hasPrio = d_prio ? 1 : 0;
    in.degree = (flags & BHS_CF_DEGREE) ? 1 : 0;
    in.Sp = d_rowPtrS; in.Sj = d_colIndS; in.prio = d_prio; in.cf = d_cf; in.cpts = d_cpts;
    return guarded(h, [&] { return cf_run(h, in, nc_out, rounds_out, ms_out); });
}

int bhs_csr_interp_symbolic_device(bhs_handle* h, int n, int nnzA, const int* d_rowPtrA, const int* d_colIndA, int nnzS,
                                   const int* d_rowPtrS, const int* d_colIndS, const int* d_cf, int nc, int* d_rowPtrP,
                                   long long* nnzP_out, double* ms_out)
{
    if (!ip_args_ok(h, n, nnzA, d_rowPtrA, d_colIndA, nnzS, d_rowPtrS, d_colIndS, d_cf, nc) || !d_rowPtrP) return BHS_ERR_INVALID_ARG;
    if (side_aliased({{d_rowPtrP, sizeof(int) * ((size_t)n + 1)}},
                     {{d_rowPtrA, sizeof(int) * ((size_t)n + 1)}, {d_colIndA, sizeof(int) * (size_t)nnzA},
                      {d_rowPtrS, sizeof(int) * ((size_t)n + 1)}, {d_colIndS, sizeof(int) * (size_t)nnzS}, {d_cf, sizeof(int) * (size_t)n}}))
        return BHS_ERR_INVALID_ARG;
    if (n == 0) {                                                     // an empty P: its row pointer is one zero
        return guarded(h, [&]() -> int {
            BHS_HIP(hipMemsetAsync(d_rowPtrP, 0, sizeof(int), h->stream));
            BHS_TRY(wait_stream(h));
            if (nnzP_out) *nnzP_out = 0;
            if (ms_out) *ms_out = 0.0;
            return BHS_SUCCESS;
        });
    }
    IpIn in;
    in.d.n = n; in.d.nnzA = nnzA; in.d.nnzS = nnzS; in.d.nc = nc; in.d.nnzP = 0;
    in.Ap = d_rowPtrA; in.Aj = d_colIndA; in.Ax = nullptr; in.Sp = d_rowPtrS; in.Sj = d_colIndS; in.cf = d_cf;
    return guarded(h, [&] { return ip_symbolic_run(h, in, d_rowPtrP, nnzP_out, ms_out); });
}

int bhs_csr_interp_numeric_device(bhs_handle* h, int n, int nnzA, const int* d_rowPtrA, const int* d_colIndA,
                                  const bhs_value_t* d_valA, int nnzS, const int* d_rowPtrS, const int* d_colIndS, const int* d_cf,
                                  int nc, const int* d_rowPtrP, long long nnzP, int* d_colIndP, bhs_value_t* d_valP, int flags,
                                  double* ms_out)
{
    if (!ip_args_ok(h, n, nnzA, d_rowPtrA, d_colIndA, nnzS, d_rowPtrS, d_colIndS, d_cf, nc) || !d_rowPtrP) return BHS_ERR_INVALID_ARG;
    if (flags != 0 || nnzP < 0 || nnzP > 0x7fffffffLL) return BHS_ERR_INVALID_ARG;
    if ((nnzA > 0 && !d_valA) || (nnzP > 0 && (!d_colIndP || !d_valP))) return BHS_ERR_INVALID_ARG;
    if (side_aliased({{d_colIndP, sizeof(int) * (size_t)nnzP}, {d_valP, sizeof(value_t) * (size_t)nnzP}},
                     {{d_rowPtrA, sizeof(int) * ((size_t)n + 1)}, {d_colIndA, sizeof(int) * (size_t)nnzA},
                      {d_valA, sizeof(value_t) * (size_t)nnzA}, {d_rowPtrS, sizeof(int) * ((size_t)n + 1)},
                      {d_colIndS, sizeof(int) * (size_t)nnzS}, {d_cf, sizeof(int) * (size_t)n}, {d_rowPtrP, sizeof(int) * ((size_t)n + 1)}}))
        return BHS_ERR_INVALID_ARG;
    if (n == 0) {                                                     // nothing to fill, nothing launched
        if (nnzP != 0) return BHS_ERR_INVALID_ARG;
        if (ms_out) *ms_out = 0.0;
        return BHS_SUCCESS;
    }
    IpIn in;
    in.d.n = n; in.d.nnzA = nnzA; in.d.nnzS = nnzS; in.d.nc = nc; in.d.nnzP = (int)nnzP;
    in.Ap = d_rowPtrA; in.Aj = d_colIndA; in.Ax = (const value_t*)d_valA; in.Sp = d_rowPtrS; in.Sj = d_colIndS; in.cf = d_cf;
    return guarded(h, [&] { return ip_numeric_run(h, in, d_rowPtrP, d_colIndP, (value_t*)d_valP, ms_out); });
}

}  // extern "C"
