// bhs_host_trsv.inc.h -- the level sets of a triangle, the sparse triangular solve and ILU(0) on them (bhs_csr_levels_device,
// bhs_csr_trsv_device, bhs_csr_ilu0_device; kernels in bhs_trsv.hip.h and bhs_ilu0.hip.h)
// (A part of bhsparse_hip.hip's translation unit, on the shared pieces of bhs_host_side.inc.h; included there after
// bhs_host_color.inc.h for its co_order.)
//
// A workspace of its own (h->trsvWs), shared by the three calls: the control block of bhs_trsv.hip.h and, in its count
// buffer, the table of rows per (level, 64 rows) of the order, which is the colouring's (co_order, bhs_host_color.inc.h).
// The analysis: kLvBatch passes of the relaxation a control round trip, for the error word, the rows the batch's last pass
// raised and the levels in use (side_passes: the loop ends after a batch whose last pass raised nothing, and with
// BHS_ERR_INTERNAL when more than n + 1 passes would be needed), then the order and the call's close, one more round trip.
// The solve and the factorisation: a launch per non-empty level, ONE round trip at the end of the call.

#include "bhs_trsv.hip.h"
#include "bhs_ilu0.hip.h"

namespace {

constexpr int kLvBatch = 8;         // passes of the relaxation between two reads of the control words

struct LvIn {
    AgDims d;
    int upper;
    const int* Ap; const int* Aj;
    int* level; int* order; int* levelPtr;
};

template <int L>
int lv_passes(bhs_handle* h, const LvIn& in, int* ctl, int* passes_out)
{
    const AgDims& d = in.d;
    const unsigned rows = (unsigned)(((long long)d.n + 256 / L - 1) / (256 / L));
    const unsigned grid = std::min<unsigned>(rows, (unsigned)h->numCU * 16);   // (a block loop: one add to the count a workgroup)
    // (n levels at the most: n passes raise, one more finds nothing; the count is the last pass's alone)
    return side_passes(h, h->trsvWs, d.n, kLvBatch, 2, TS_INTS, passes_out, [&] {
        return timed(h, "levels_pass", d.n, [&] {
            hipLaunchKernelGGL(k_lev_pass<L>, dim3(grid), dim3(256), 0, h->stream, d, in.upper, in.Ap, in.Aj, in.level, ctl);
            return 1;
        });
    });
}

int lv_run(bhs_handle* h, const LvIn& in, int* nlevels_out, int* passes_out, double* ms_out)
{
    const AgDims& d = in.d;
    SideWs& ws = h->trsvWs;
    BHS_TRY(side_open(h, ws, TS_INTS, 0, 0));
    BHS_TRY(side_start(h, ws));
    int* ctl = (int*)ws.ctl.p;
    BHS_HIP(hipMemsetAsync(in.level, 0, sizeof(int) * (size_t)d.n, h->stream));
    const int L = side_lanes(d.n, d.nnzS);
    int passes = 0;
    BHS_TRY(with_lanes(L, [&](auto l) { return lv_passes<l.value>(h, in, ctl, &passes); }));
    const long long nlevels = ws.host[CO_NCOL];
    if (nlevels < 1 || nlevels > (long long)d.n) return BHS_ERR_INTERNAL;
    BHS_TRY(co_order(h, ws, "levels_order", TS_INTS, 0, d.n, nlevels, in.level, in.order, in.levelPtr));
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, TS_INTS));                           // the order's error word and total
    BHS_TRY(side_close(h, ws, ms_out));
    long long total = 0;
    memcpy(&total, ws.host + AG_TOTAL, sizeof(total));
    if (ws.host[RD_ERR] || total != (long long)d.n) return BHS_ERR_INTERNAL;   // (the levels were this call's own)
    if (nlevels_out) *nlevels_out = (int)nlevels;
    if (passes_out) *passes_out = passes;
    return BHS_SUCCESS;
}

// the host's array of a solve or a factorisation: starts at 0, never falls, ends within n
bool ts_ptr_bad(int n, int nlevels, const int* h_levelPtr)
{
    if (nlevels < 0 || nlevels > n || (nlevels > 0 && !h_levelPtr)) return true;
    if (nlevels > 0 && h_levelPtr[0] != 0) return true;
    for (int c = 0; c < nlevels; ++c)
        if (h_levelPtr[c + 1] < h_levelPtr[c] || h_levelPtr[c + 1] > n) return true;
    return false;
}

struct TsIn {
    TsDims d;
    const int* Ap; const int* Aj; const value_t* Ax;
    int nlevels;
    const int* levelPtr;    // host
    const int* order;
    const value_t* b; value_t* x;
};

// a launch per non-empty level, ascending, under the kernel record `name`; launch(L, dims of the level, grid)
template <typename F>
int ts_levels(bhs_handle* h, const char* name, TsDims d, int nlevels, const int* levelPtr, F&& launch)
{
    const int L = side_lanes(d.n, d.nnzA);
    return timed(h, name, levelPtr[nlevels], [&] {
        int launches = 0;
        for (int c = 0; c < nlevels; ++c) {
            d.lo = levelPtr[c]; d.cnt = levelPtr[c + 1] - levelPtr[c];
            if (d.cnt == 0) continue;
            launch(L, d, (unsigned)(((long long)d.cnt + 256 / L - 1) / (256 / L)));
            ++launches;
        }
        return launches;
    });
}

// the shared frame as the solve and the factorisation have it: the pivot word at its identity ahead of the span, the
// launches of enqueue(ctl), the call's one round trip
template <typename F>
int ts_call(bhs_handle* h, double* ms_out, F&& enqueue)
{
    SideWs& ws = h->trsvWs;
    BHS_TRY(side_open(h, ws, TS_INTS, 0, 0));
    int* ctl = (int*)ws.ctl.p;
    BHS_HIP(hipMemsetD32Async((hipDeviceptr_t)(ctl + TS_PIVOT), 0x7fffffff, 1, h->stream));
    BHS_TRY(side_start(h, ws));
    BHS_TRY(enqueue(ctl));
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, TS_INTS));                           // the call's one round trip
    BHS_TRY(side_close(h, ws, ms_out));
    return ws.host[RD_ERR] ? (int)BHS_ERR_INVALID_ARG : (int)BHS_SUCCESS;
}

typedef void (*TsKernel)(TsDims, const int*, const int*, const value_t*, const int*, const value_t*, value_t*, int*);
typedef void (*IlKernel)(TsDims, const int*, const int*, value_t*, const int*, int*);

int ts_run(bhs_handle* h, const TsIn& in, double* ms_out)
{
    return ts_call(h, ms_out, [&](int* ctl) {
        return ts_levels(h, "trsv_level", in.d, in.nlevels, in.levelPtr, [&](int L, const TsDims& d, unsigned grid) {
            const TsKernel kern = with_lanes(L, [](auto l) -> TsKernel { return k_trsv_level<l.value>; });
            hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, h->stream, d, in.Ap, in.Aj, in.Ax, in.order, in.b, in.x, ctl);
        });
    });
}

int il_run(bhs_handle* h, const TsIn& in, value_t* Ax, int* pivot_out, double* ms_out)
{
    BHS_TRY(ts_call(h, ms_out, [&](int* ctl) {
        return ts_levels(h, "ilu0_level", in.d, in.nlevels, in.levelPtr, [&](int L, const TsDims& d, unsigned grid) {
            const IlKernel kern = with_lanes(L, [](auto l) -> IlKernel { return k_ilu0_level<l.value>; });
            hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, h->stream, d, in.Ap, in.Aj, Ax, in.order, ctl);
        });
    }));
    const int pivot = h->trsvWs.host[TS_PIVOT];
    if (pivot_out) *pivot_out = pivot == 0x7fffffff ? -1 : pivot;
    return BHS_SUCCESS;
}

}  // namespace

extern "C" {

int bhs_csr_levels_device(bhs_handle* h, int n, int nnzA, const int* d_rowPtrA, const int* d_colIndA, int flags, int* d_level,
                          int* d_order, int* d_levelPtr, int* nlevels_out, int* passes_out, double* ms_out)
{
    if (!h || h->ps.open || n < 0 || nnzA < 0) return BHS_ERR_INVALID_ARG;
    if (flags != BHS_TRI_LOWER && flags != BHS_TRI_UPPER) return BHS_ERR_INVALID_ARG;   // exactly one triangle, nothing else
    if ((n > 0 && (!d_rowPtrA || !d_level || !d_order || !d_levelPtr)) || (nnzA > 0 && !d_colIndA)) return BHS_ERR_INVALID_ARG;
    if (side_aliased({{d_level, sizeof(int) * (size_t)n}, {d_order, sizeof(int) * (size_t)n}, {d_levelPtr, sizeof(int) * ((size_t)n + 1)}},
                     {{d_rowPtrA, sizeof(int) * ((size_t)n + 1)}, {d_colIndA, sizeof(int) * (size_t)nnzA}}))
        return BHS_ERR_INVALID_ARG;
    if (n == 0) return side_nothing(nlevels_out, passes_out, ms_out);  // no row, no level, nothing launched
    LvIn in;
    in.d.n = n; in.d.nnzS = nnzA; in.d.seed = 0; in.d.hasPrio = 0;
    in.upper = flags == BHS_TRI_UPPER ? 1 : 0;
    in.Ap = d_rowPtrA; in.Aj = d_colIndA; in.level = d_level; in.order = d_order; in.levelPtr = d_levelPtr;
    return guarded(h, [&] { return lv_run(h, in, nlevels_out, passes_out, ms_out); });
}

int bhs_csr_trsv_device(bhs_handle* h, int n, int nnzA, const int* d_rowPtrA, const int* d_colIndA, const bhs_value_t* d_valA,
                        int nlevels, const int* h_levelPtr, const int* d_order, double alpha, const bhs_value_t* d_b,
                        bhs_value_t* d_x, int flags, double* ms_out)
{
    if (!h || h->ps.open || n < 0 || nnzA < 0) return BHS_ERR_INVALID_ARG;
    const int tri = flags & (BHS_TRI_LOWER | BHS_TRI_UPPER);
    if ((flags & ~(BHS_TRI_LOWER | BHS_TRI_UPPER | BHS_TRI_UNIT_DIAG)) || (tri != BHS_TRI_LOWER && tri != BHS_TRI_UPPER))
        return BHS_ERR_INVALID_ARG;
    if (ts_ptr_bad(n, nlevels, h_levelPtr)) return BHS_ERR_INVALID_ARG;
    const int listed = nlevels > 0 ? h_levelPtr[nlevels] : 0;
    if (listed > 0 && (!d_rowPtrA || !d_order || !d_b || !d_x)) return BHS_ERR_INVALID_ARG;
    if (nnzA > 0 && (!d_colIndA || !d_valA)) return BHS_ERR_INVALID_ARG;
    const size_t vec = sizeof(value_t) * (size_t)n;
    const void* b = (const void*)d_b == (const void*)d_x ? nullptr : d_b;   // (x == b exactly: in place)
    if (side_aliased({{d_x, vec}},                                    // (x is the one array written)
                     {{d_rowPtrA, sizeof(int) * ((size_t)n + 1)}, {d_colIndA, sizeof(int) * (size_t)nnzA}, {d_valA, sizeof(value_t) * (size_t)nnzA},
                      {d_order, sizeof(int) * (size_t)listed}, {b, vec}}))
        return BHS_ERR_INVALID_ARG;
    if (listed == 0) {                                                // no row to solve for, nothing launched
        if (ms_out) *ms_out = 0.0;
        return BHS_SUCCESS;
    }
    TsIn in;
    in.d.n = n; in.d.nnzA = nnzA; in.d.lo = in.d.cnt = 0; in.d.upper = tri == BHS_TRI_UPPER ? 1 : 0;
    in.d.unit = (flags & BHS_TRI_UNIT_DIAG) ? 1 : 0; in.d.alpha = alpha;
    in.Ap = d_rowPtrA; in.Aj = d_colIndA; in.Ax = (const value_t*)d_valA;
    in.nlevels = nlevels; in.levelPtr = h_levelPtr; in.order = d_order;
    in.b = (const value_t*)d_b; in.x = (value_t*)d_x;
    return guarded(h, [&] { return ts_run(h, in, ms_out); });
}

int bhs_csr_ilu0_device(bhs_handle* h, int n, int nnzA, const int* d_rowPtrA, const int* d_colIndA, bhs_value_t* d_valA,
                        int nlevels, const int* h_levelPtr, const int* d_order, int flags, int* pivot_out, double* ms_out)
{
    if (!h || h->ps.open || n < 0 || nnzA < 0 || flags != 0) return BHS_ERR_INVALID_ARG;
    if (ts_ptr_bad(n, nlevels, h_levelPtr)) return BHS_ERR_INVALID_ARG;
    const int listed = nlevels > 0 ? h_levelPtr[nlevels] : 0;
    if (listed > 0 && (!d_rowPtrA || !d_order)) return BHS_ERR_INVALID_ARG;
    if (nnzA > 0 && (!d_colIndA || !d_valA)) return BHS_ERR_INVALID_ARG;
    if (side_aliased({{d_valA, sizeof(value_t) * (size_t)nnzA}},      // (the values are the one array written)
                     {{d_rowPtrA, sizeof(int) * ((size_t)n + 1)}, {d_colIndA, sizeof(int) * (size_t)nnzA}, {d_order, sizeof(int) * (size_t)listed}}))
        return BHS_ERR_INVALID_ARG;
    if (listed == 0) {                                                // no row to factorise, nothing launched
        if (pivot_out) *pivot_out = -1;
        if (ms_out) *ms_out = 0.0;
        return BHS_SUCCESS;
    }
    TsIn in;
    in.d.n = n; in.d.nnzA = nnzA; in.d.lo = in.d.cnt = 0; in.d.upper = 0; in.d.unit = 0; in.d.alpha = 1.0;
    in.Ap = d_rowPtrA; in.Aj = d_colIndA; in.Ax = nullptr;
    in.nlevels = nlevels; in.levelPtr = h_levelPtr; in.order = d_order; in.b = nullptr; in.x = nullptr;
    return guarded(h, [&] { return il_run(h, in, (value_t*)d_valA, pivot_out, ms_out); });
}

}  // extern "C"
