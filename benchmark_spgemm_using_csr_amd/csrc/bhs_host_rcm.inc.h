// bhs_host_rcm.inc.h -- the reverse Cuthill-McKee ordering of a pattern (bhs_csr_rcm_device; kernels in bhs_rcm.hip.h)
// (A part of bhsparse_hip.hip's translation unit, on the shared pieces of bhs_host_side.inc.h; included there after
// bhs_host_color.inc.h for its co_order and after bhs_host_components.inc.h, whose kernels it launches under its own record.)
//
// A workspace of its own (h->rcmWs): the control block of bhs_rcm.hip.h; in its queue buffer the two 64-bit slots a vertex
// and the root bitmap, then the call's int arrays (RcmBufs); in its count buffer, one after the other, the roots per bitmap
// word, the table of the level order, every level's child counts and the components' sizes, each scanned in place.
// Round trips: one behind the check (a refusal ends the call there, ahead of everything else), one a batch of kRcmBatch
// passes (side_passes: the components' relaxation, and every sweep's level passes), one a sweep behind its far step, one for
// levelPtr behind the level order, and the call's close.  The numbering is a launch sequence per level with no round trip
// inside.  BHS_ERR_INTERNAL after n + 1 sweeps; BHS_ERR_ALLOC where the level order's table, depth x ceil(n / 64) counts,
// would exceed co_order's kCoMaxTable.  The regrouping by component needs no table: the numbering hands every vertex its
// place inside its component, and the components' first places are the library's scan of their sizes.

#include "bhs_rcm.hip.h"

namespace {

constexpr int kRcmBatch = 8;        // passes between two reads of the control words

struct RcmIn {
    AgDims d;
    const int* Sp; const int* Sj;
    int flags;
    int* perm; int* level; int* start;
};

// the call's arrays in the queue buffer, n ints each where nothing else is said
struct RcmBufs {
    rd_u64* eslot; rd_u64* xslot; rd_u64* map;     // per root: the greatest level, the least key; the root bitmap
    int* root; int* comp; int* deg; int* level;
    int* byLevel; int* levelPtr;                   // the vertices by (level, index); n + 1
    int* pos; int* parent; int* forest;
    int* off;                                      // n + 1: the numbering's offsets a bitmap word, then a level's child offsets
    int* size; int* ptr;                           // the components' sizes and, n + 1, their first places in the order
    int* start; int* ecc; int* done;               // per root
    RcmSeg seg;                                    // a vertex's component in its level, and its place inside its component
};

unsigned rcm_grid(bhs_handle* h, long long items, int per)
{
    return (unsigned)std::max<long long>(1, std::min<long long>((items + per - 1) / per, (long long)h->numCU * 16));
}

// The library's scan numbers its tiles from a ticket word that a call's control block holds at zero ONCE (side_open); a
// tile numbered beyond the scan's own would look back for words nobody publishes.  This call scans many times -- the
// components' numbering, the level order, every level's child counts, the sizes -- so the word is cleared ahead of each.
int rcm_scan_ticket(bhs_handle* h, int* ctl)
{
    BHS_HIP(hipMemsetAsync(ctl + AG_TICKET, 0, sizeof(int), h->stream));
    return BHS_SUCCESS;
}

// the components of bhs_components.hip.h under this call's record and workspace: root, comp, the sizes and their count
template <int L>
int rcm_components(bhs_handle* h, const RcmIn& in, const RcmBufs& w, int* ctl, int* ncomp_out, long long* passes)
{
    const AgDims& d = in.d;
    SideWs& ws = h->rcmWs;
    const size_t nWords = ((size_t)d.n + 63) / 64;
    const unsigned gridN = (unsigned)(((size_t)d.n + 255) / 256);
    BHS_TRY(timed(h, "rcm_components", 0, [&] {
        hipLaunchKernelGGL(k_cc_init, dim3(gridN), dim3(256), 0, h->stream, d.n, w.root);
        return 1;
    }));
    int p = 0;
    BHS_TRY(side_passes(h, ws, d.n, kRcmBatch, 4, RCM_INTS, &p, [&] {
        return timed(h, "rcm_components", d.n, [&] {
            hipLaunchKernelGGL(k_cc_pass<L>, dim3(rcm_grid(h, d.n, 256 / L)), dim3(256), 0, h->stream, d, in.Sp, in.Sj, w.root, ctl);
            return 1;
        });
    }));
    *passes += p;
    const long long ncomp = ws.host[CC_ROOTS];                        // (the last pass read the fixed point)
    if (ncomp < 1 || ncomp > (long long)d.n) return BHS_ERR_INTERNAL;
    *ncomp_out = (int)ncomp;
    BHS_TRY(timed(h, "rcm_components", d.n, [&] {
        hipLaunchKernelGGL(k_cc_flag, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)w.root, w.map, (int*)ws.cnt.p);
        return 1;
    }));
    BHS_TRY(rcm_scan_ticket(h, ctl));
    BHS_TRY(side_scan(h, ws, "rcm_components", kAgScan, (int)nWords, w.off, w.off));
    return timed(h, "rcm_components", 0, [&] {
        hipLaunchKernelGGL(k_cc_clear, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)ctl, w.size);
        hipLaunchKernelGGL(k_cc_number, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)w.root, (const rd_u64*)w.map,
                           (const int*)w.off, w.comp, w.size, ctl);
        return 2;
    });
}

// the sweeps: one without BHS_RCM_PERIPHERAL, else until no component moved its start
template <int L>
int rcm_sweeps(bhs_handle* h, const RcmIn& in, const RcmBufs& w, int* ctl, int* sweeps_out, int* depth_out, long long* passes)
{
    const AgDims& d = in.d;
    SideWs& ws = h->rcmWs;
    const unsigned gridN = rcm_grid(h, d.n, 256), gridL = rcm_grid(h, d.n, 256 / L);
    const int peripheral = (in.flags & kRcmPeripheral) ? 1 : 0;
    for (long long sweep = 0;; ++sweep) {
        if (sweep > d.n) return BHS_ERR_INTERNAL;                     // (a start moves only where the eccentricity grew)
        BHS_TRY(timed(h, "rcm_level", 0, [&] {
            hipLaunchKernelGGL(k_rcm_init, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)w.root, (const int*)w.start, w.level, ctl);
            return 1;
        }));
        int cur = 0, p = 0;
        BHS_TRY(side_passes(h, ws, d.n, kRcmBatch, 2, RCM_INTS, &p, [&] {
            return timed(h, "rcm_level", d.n, [&] {
                hipLaunchKernelGGL(k_rcm_level<L>, dim3(gridL), dim3(256), 0, h->stream, d, in.Sp, in.Sj, w.level, cur, ctl);
                ++cur;
                return 1;
            });
        }));
        *passes += p;
        BHS_HIP(hipMemsetAsync(w.eslot, 0, sizeof(rd_u64) * (size_t)d.n, h->stream));
        BHS_HIP(hipMemsetAsync(w.xslot, 0xFF, sizeof(rd_u64) * (size_t)d.n, h->stream));
        BHS_HIP(hipMemsetAsync(ctl + AG_UNDEC, 0, sizeof(rd_u64), h->stream));
        BHS_HIP(hipMemsetAsync(ctl + RCM_DEPTH, 0, sizeof(int), h->stream));
        BHS_TRY(timed(h, "rcm_far", d.n, [&] {
            hipLaunchKernelGGL(k_rcm_far_max, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)w.root, (const int*)w.level, w.eslot, ctl);
            hipLaunchKernelGGL(k_rcm_far_min, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)w.root, (const int*)w.level,
                               (const int*)w.deg, (const rd_u64*)w.eslot, w.xslot, ctl);
            hipLaunchKernelGGL(k_rcm_decide, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)w.root, (const rd_u64*)w.eslot,
                               (const rd_u64*)w.xslot, w.start, w.ecc, w.done, (int)std::min<long long>(sweep, 1), peripheral, ctl);
            return 3;
        }));
        BHS_TRY(side_read_ctl(h, ws, RCM_INTS));                      // the sweep's one round trip of its own
        if (ws.host[RD_ERR]) return BHS_ERR_INTERNAL;                 // (the check accepted the pattern)
        long long moved = 0;
        memcpy(&moved, ws.host + AG_UNDEC, sizeof(moved));
        *sweeps_out = (int)(sweep + 1);
        *depth_out = ws.host[RCM_DEPTH];
        if (!peripheral || (sweep >= 1 && moved == 0)) return BHS_SUCCESS;
    }
}

// the numbering: level 0, then a launch sequence per level over that level's slice
template <int L>
int rcm_number(bhs_handle* h, const RcmIn& in, const RcmBufs& w, int* ctl, int ncomp, int depth, const int* levelPtr)
{
    const AgDims& d = in.d;
    SideWs& ws = h->rcmWs;
    int* kids = (int*)ws.cnt.p;
    BHS_TRY(timed(h, "rcm_number", ncomp, [&] {
        hipLaunchKernelGGL(k_rcm_roots, dim3(rcm_grid(h, ncomp, 256)), dim3(256), 0, h->stream, d.n, ncomp, (const int*)w.byLevel,
                           (const int*)w.comp, w.pos, w.forest, w.seg, in.start, ctl);
        return 1;
    }));
    for (int l = 1; l < depth; ++l) {
        RcmLevel lv;
        lv.l = l; lv.lo = levelPtr[l]; lv.cnt = levelPtr[l + 1] - levelPtr[l];
        lv.prevLo = levelPtr[l - 1]; lv.prevCnt = levelPtr[l] - levelPtr[l - 1];
        const unsigned grid = rcm_grid(h, lv.cnt, 256 / L);
        BHS_HIP(hipMemsetAsync(kids, 0, sizeof(int) * ((size_t)lv.prevCnt + 1), h->stream));
        BHS_TRY(timed(h, "rcm_number", lv.cnt, [&] {
            hipLaunchKernelGGL(k_rcm_parent<L>, dim3(grid), dim3(256), 0, h->stream, d, lv, in.Sp, in.Sj, (const int*)w.byLevel,
                               (const int*)w.level, (const int*)w.pos, w.parent, kids, ctl);
            return 1;
        }));
        BHS_TRY(rcm_scan_ticket(h, ctl));
        BHS_TRY(side_scan(h, ws, "rcm_number", kAgScan, lv.prevCnt, w.off, w.off));
        BHS_TRY(timed(h, "rcm_number", 0, [&] {
            hipLaunchKernelGGL(k_rcm_place<L>, dim3(grid), dim3(256), 0, h->stream, d, lv, in.Sp, in.Sj, (const int*)w.byLevel,
                               (const int*)w.level, (const int*)w.deg, (const int*)w.parent, (const int*)w.off, w.pos, w.forest, w.seg, ctl);
            return 1;
        }));
    }
    return BHS_SUCCESS;
}

int rcm_run(bhs_handle* h, RcmIn& in, int* ncomp_out, int* depth_out, int* sweeps_out, int* passes_out, double* ms_out)
{
    const AgDims& d = in.d;
    SideWs& ws = h->rcmWs;
    const size_t n = (size_t)d.n, nWords = (n + 63) / 64;
    const int nInts = 18;                                             // RcmBufs' int arrays, n + 1 each with the two row pointers
    const size_t queueBytes = sizeof(rd_u64) * (2 * n + nWords) + sizeof(int) * (size_t)nInts * (n + 1);
    BHS_TRY(side_open(h, ws, RCM_INTS, queueBytes, n + 1));
    RcmBufs w;
    w.eslot = (rd_u64*)ws.queue.p; w.xslot = w.eslot + n; w.map = w.xslot + n;
    int* at = (int*)(w.map + nWords);
    auto take = [&] { int* p = at; at += n + 1; return p; };
    w.root = take(); w.comp = take(); w.deg = take(); w.level = in.level ? in.level : take();
    w.byLevel = take(); w.levelPtr = take(); w.pos = take(); w.parent = take(); w.forest = take(); w.off = take(); w.size = take(); w.ptr = take();
    w.start = take(); w.ecc = take(); w.done = take();
    w.seg.first = take(); w.seg.end = take(); w.seg.loc = take();
    BHS_HIP(hipMemsetAsync(w.xslot, 0xFF, sizeof(rd_u64) * n, h->stream));       // no key yet
    BHS_HIP(hipMemsetAsync(w.parent, 0xFF, sizeof(int) * n, h->stream));         // -1: no parent, no vertex at this place
    BHS_HIP(hipMemsetAsync(w.forest, 0xFF, sizeof(int) * n, h->stream));
    BHS_TRY(side_start(h, ws));
    int* ctl = (int*)ws.ctl.p;
    const int L = side_lanes(d.n, d.nnzS);
    const unsigned gridN = rcm_grid(h, d.n, 256);

    BHS_TRY(with_lanes(L, [&](auto l) {
        return timed(h, "rcm_check", d.n, [&] {
            hipLaunchKernelGGL(k_rcm_check<l.value>, dim3(rcm_grid(h, d.n, 256 / l.value)), dim3(256), 0, h->stream, d, in.Sp, in.Sj,
                               w.deg, ctl);
            return 1;
        });
    }));
    BHS_TRY(side_read_ctl(h, ws, RCM_INTS));
    if (ws.host[RD_ERR]) return BHS_ERR_INVALID_ARG;                  // (no output has been written)

    int ncomp = 0, sweeps = 0, depth = 0;
    long long passes = 0;
    BHS_TRY(with_lanes(L, [&](auto l) { return rcm_components<l.value>(h, in, w, ctl, &ncomp, &passes); }));
    BHS_TRY(timed(h, "rcm_far", d.n, [&] {
        hipLaunchKernelGGL(k_rcm_start, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)w.root, (const int*)w.deg, w.xslot, ctl);
        hipLaunchKernelGGL(k_rcm_seed, dim3(gridN), dim3(256), 0, h->stream, d.n, (const int*)w.root, (const rd_u64*)w.xslot, w.start,
                           w.ecc, w.done);
        return 2;
    }));
    BHS_TRY(with_lanes(L, [&](auto l) { return rcm_sweeps<l.value>(h, in, w, ctl, &sweeps, &depth, &passes); }));
    if (depth < 1 || depth > d.n) return BHS_ERR_INTERNAL;

    // the vertices by (level, index); levelPtr to the host once
    BHS_TRY(rcm_scan_ticket(h, ctl));
    BHS_TRY(co_order(h, ws, "rcm_order", RCM_INTS, queueBytes, d.n, depth, w.level, w.byLevel, w.levelPtr));
    std::vector<int> levelPtr((size_t)depth + 1);
    BHS_HIP(hipMemcpyAsync(levelPtr.data(), w.levelPtr, sizeof(int) * levelPtr.size(), hipMemcpyDeviceToHost, h->stream));
    BHS_TRY(side_read_ctl(h, ws, RCM_INTS));
    long long total = 0;
    memcpy(&total, ws.host + AG_TOTAL, sizeof(total));
    if (ws.host[RD_ERR] || total != (long long)d.n) return BHS_ERR_INTERNAL;   // (the levels were this call's own)
    if (levelPtr[0] != 0 || levelPtr[1] != ncomp || levelPtr[depth] != d.n) return BHS_ERR_INTERNAL;
    for (int l = 0; l < depth; ++l)
        if (levelPtr[l + 1] <= levelPtr[l]) return BHS_ERR_INTERNAL;  // (no level of a sweep is empty)
    BHS_TRY(side_prepare(h, ws, RCM_INTS, queueBytes, n + 1));        // (a level's child counts: the table may have been smaller)

    BHS_TRY(with_lanes(L, [&](auto l) { return rcm_number<l.value>(h, in, w, ctl, ncomp, depth, levelPtr.data()); }));

    // the forest order stably regrouped by component, reversed as a whole
    BHS_HIP(hipMemcpyAsync(ws.cnt.p, w.size, sizeof(int) * (size_t)ncomp, hipMemcpyDeviceToDevice, h->stream));
    BHS_TRY(rcm_scan_ticket(h, ctl));
    BHS_TRY(side_scan(h, ws, "rcm_group", kAgScan, ncomp, w.ptr, w.ptr));
    BHS_TRY(timed(h, "rcm_group", d.n, [&] {
        hipLaunchKernelGGL(k_rcm_perm, dim3(gridN), dim3(256), 0, h->stream, d.n, ncomp, (const int*)w.comp, (const int*)w.ptr,
                           (const int*)w.seg.loc, (in.flags & kRcmNoReverse) ? 0 : 1, in.perm, ctl);
        return 1;
    }));
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, RCM_INTS));                          // the numbering's error word and the sizes' total
    BHS_TRY(side_close(h, ws, ms_out));
    memcpy(&total, ws.host + AG_TOTAL, sizeof(total));
    if (ws.host[RD_ERR] || total != (long long)d.n) return BHS_ERR_INTERNAL;
    if (ncomp_out) *ncomp_out = ncomp;
    if (depth_out) *depth_out = depth;
    if (sweeps_out) *sweeps_out = sweeps;
    if (passes_out) *passes_out = (int)std::min<long long>(passes, 0x7fffffff);
    return BHS_SUCCESS;
}

}  // namespace

extern "C" {

int bhs_csr_rcm_device(bhs_handle* h, int n, int nnzS, const int* d_rowPtrS, const int* d_colIndS, int flags, int* d_perm, int* d_level,
                       int* d_start, int* ncomp_out, int* depth_out, int* sweeps_out, int* passes_out, double* ms_out)
{
    if (!h || h->ps.open || n < 0 || nnzS < 0 || (flags & ~(BHS_RCM_PERIPHERAL | BHS_RCM_NO_REVERSE))) return BHS_ERR_INVALID_ARG;
    if ((n > 0 && (!d_rowPtrS || !d_perm)) || (nnzS > 0 && !d_colIndS)) return BHS_ERR_INVALID_ARG;
    if (side_aliased({{d_perm, sizeof(int) * (size_t)n}, {d_level, sizeof(int) * (size_t)n}, {d_start, sizeof(int) * (size_t)n}},
                     {{d_rowPtrS, sizeof(int) * ((size_t)n + 1)}, {d_colIndS, sizeof(int) * (size_t)nnzS}}))
        return BHS_ERR_INVALID_ARG;
    if (n == 0) {                                                     // no vertex: nothing launched
        if (depth_out) *depth_out = 0;
        if (sweeps_out) *sweeps_out = 0;
        return side_nothing(ncomp_out, passes_out, ms_out);
    }
    static_assert(BHS_RCM_PERIPHERAL == kRcmPeripheral && BHS_RCM_NO_REVERSE == kRcmNoReverse, "flags");
    RcmIn in;
    in.d.n = n; in.d.nnzS = nnzS; in.d.seed = 0; in.d.hasPrio = 0;
    in.Sp = d_rowPtrS; in.Sj = d_colIndS; in.flags = flags; in.perm = d_perm; in.level = d_level; in.start = d_start;
    return guarded(h, [&] { return rcm_run(h, in, ncomp_out, depth_out, sweeps_out, passes_out, ms_out); });
}

}  // extern "C"
