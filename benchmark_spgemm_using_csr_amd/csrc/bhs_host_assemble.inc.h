// bhs_host_assemble.inc.h -- the assembly of a CSR matrix from triplets (bhs_coo_assemble_device,
// bhs_coo_assemble_values_device; kernels in bhs_assemble.hip.h)
// (A part of bhsparse_hip.hip's translation unit: included there directly after bhs_host_cfsplit.inc.h.)
//
// A workspace of its own (h->asWs): the control block of bhs_assemble.hip.h, the raw rows' queues by bin (3 x m ints) in its
// queue buffer, in its count buffer first the kept triplets per row and then the heads per bitmap word, each scanned in place
// by the library's one-pass scan and copied out.  The scratch arrays are buffers of its own from the grow-only pool (h->asBuf):
// rawPtr and the cursors (m + 1 ints each), the keys (8 bytes a triplet) and the row beside each (4 bytes), the head bitmap and
// its scanned offsets, and entryPtr where the caller wants values but not the map.
// The full call makes two round trips: the error word, the dropped triplets and the bins BEFORE anything caller-owned is written;
// at the end the number of entries.  The values call makes two as well: its map is checked whole before valZ is touched.

#include "bhs_assemble.hip.h"

namespace {

enum { AS_RAW = 0, AS_CUR, AS_KEYS, AS_ROWOF, AS_MAP, AS_OFF, AS_ENT, AS_BUFS };
static_assert(AS_BUFS == sizeof(((bhs_handle*)nullptr)->asBuf) / sizeof(DevBuf), "h->asBuf");

struct AsIn {
    int m, n, nnzIn, flags;
    const int* rows; const int* cols; const value_t* vals;
    int* Zp; int* Zj; value_t* Zx; int* entryPtr; int* perm;
};

constexpr SideScanWords kAsScanRows = {AS_TICKET_A, AS_TOTAL_A, AS_BINS_A, AS_MAXCNT_A};
constexpr SideScanWords kAsScanHeads = {AS_TICKET_B, AS_TOTAL_B, AS_BINS_B, AS_MAXCNT_B};

inline unsigned as_grid(long long items) { return (unsigned)std::max<long long>(1, (items + 255) / 256); }

// every raw row's keys in order, on the queues and bin counts in h->asWs.queue / h->asWs.host
int as_sort(bhs_handle* h, int m, int nkept)
{
    const int* queue = (const int*)h->asWs.queue.p;
    const int* count = h->asWs.host + AS_COUNT;
    const int* rawPtr = (const int*)h->asBuf[AS_RAW].p;
    tr_u64* keys = (tr_u64*)h->asBuf[AS_KEYS].p;
    if (count[kTrShort]) {
        const int nq = count[kTrShort];
        BHS_TRY(timed(h, "assemble_short", nq, [&] {
            hipLaunchKernelGGL(k_as_sort_short, dim3((unsigned)(((long long)nq + 15) / 16)), dim3(256), 0, h->stream, nq,
                               queue + (size_t)kTrShort * m, rawPtr, nkept, keys);
            return 1;
        }));
    }
    if (count[kTrWave]) {
        const int nq = count[kTrWave];
        BHS_TRY(timed(h, "assemble_wave", nq, [&] {
            hipLaunchKernelGGL(k_as_sort_wave, dim3((unsigned)(((long long)nq + 3) / 4)), dim3(256), 0, h->stream, nq,
                               queue + (size_t)kTrWave * m, rawPtr, nkept, keys);
            return 1;
        }));
    }
    if (count[kTrLong]) {
        const int nq = count[kTrLong];
        BHS_TRY(timed(h, "assemble_long", nq, [&] {
            hipLaunchKernelGGL(k_as_sort_long, dim3((unsigned)std::min<long long>(nq, (long long)h->numCU * 8)), dim3(256), 0,
                               h->stream, nq, queue + (size_t)kTrLong * m, rawPtr, nkept, keys);
            return 1;
        }));
    }
    return BHS_SUCCESS;
}

int as_run(bhs_handle* h, const AsIn& in, int* nnzZ_out, int* nkept_out, double* ms_out)
{
    const int m = in.m, n = in.n, nnzIn = in.nnzIn;
    SideWs& ws = h->asWs;
    const size_t maxWords = ((size_t)nnzIn + 63) / 64;
    BHS_TRY(side_prepare(h, ws, AS_INTS, sizeof(int) * (size_t)kTrBins * (size_t)std::max(m, 1), std::max((size_t)m, maxWords) + 1));
    BHS_TRY(ensure(h, h->asBuf[AS_RAW], sizeof(int) * ((size_t)m + 1)));
    BHS_TRY(ensure(h, h->asBuf[AS_CUR], sizeof(int) * ((size_t)m + 1)));
    BHS_TRY(ensure(h, h->asBuf[AS_KEYS], sizeof(tr_u64) * (size_t)std::max(nnzIn, 1)));
    BHS_TRY(ensure(h, h->asBuf[AS_ROWOF], sizeof(int) * (size_t)std::max(nnzIn, 1)));
    BHS_TRY(ensure(h, h->asBuf[AS_MAP], sizeof(tr_u64) * (maxWords + 1)));
    BHS_TRY(ensure(h, h->asBuf[AS_OFF], sizeof(int) * (maxWords + 1)));
    int* ent = in.entryPtr;
    if (!ent && in.Zx) {
        BHS_TRY(ensure(h, h->asBuf[AS_ENT], sizeof(int) * ((size_t)nnzIn + 1)));
        ent = (int*)h->asBuf[AS_ENT].p;
    }
    side_reset_stats(h);
    int* ctl = (int*)ws.ctl.p;
    int* cnt = (int*)ws.cnt.p;
    int* rawPtr = (int*)h->asBuf[AS_RAW].p;
    int* cur = (int*)h->asBuf[AS_CUR].p;
    tr_u64* keys = (tr_u64*)h->asBuf[AS_KEYS].p;
    int* rowOf = (int*)h->asBuf[AS_ROWOF].p;
    tr_u64* map = (tr_u64*)h->asBuf[AS_MAP].p;
    int* off = (int*)h->asBuf[AS_OFF].p;
    BHS_TRY(side_begin(h, ws));
    BHS_HIP(hipMemsetAsync(ctl, 0, sizeof(int) * AS_INTS, h->stream));
    BHS_HIP(hipMemsetAsync(cnt, 0, sizeof(int) * ((size_t)m + 1), h->stream));
    int stat = 0;
    if (nnzIn > 0) {
        BHS_TRY(timed(h, "assemble_count", nnzIn, [&] {
            hipLaunchKernelGGL(k_as_count, dim3(as_grid(nnzIn)), dim3(256), 0, h->stream, m, n, nnzIn, in.rows, in.cols, in.flags, cnt, ctl);
            if (m == 0) return 1;
            hipLaunchKernelGGL(k_tr_bin, dim3(as_grid(m)), dim3(256), 0, h->stream, m, (const int*)cnt, ctl, (int*)ws.queue.p);
            return 2;
        }, &stat));
    }
    BHS_TRY(side_read_ctl(h, ws, AS_INTS));
    if (ws.host[AS_ERR]) return BHS_ERR_INVALID_ARG;                  // (nothing caller-owned has been written)
    long long dropped = 0;
    for (int s = 0; s < kAsDropSlots; ++s) dropped += ws.host[AS_DROPPED + s];
    if (dropped < 0 || dropped > nnzIn) return BHS_ERR_INTERNAL;
    const int nkept = (int)(nnzIn - dropped);
    if (nnzIn > 0) h->stats[stat].nnz_out += nkept;
    if (nkept == 0) {
        BHS_HIP(hipMemsetAsync(in.Zp, 0, sizeof(int) * ((size_t)m + 1), h->stream));
        if (in.entryPtr) BHS_HIP(hipMemsetAsync(in.entryPtr, 0, sizeof(int), h->stream));
    } else {
        const int nWords = (int)(((long long)nkept + 63) / 64);
        BHS_TRY(side_scan(h, ws, "assemble_scan", kAsScanRows, m, rawPtr, rawPtr));
        BHS_HIP(hipMemcpyAsync(cur, rawPtr, sizeof(int) * ((size_t)m + 1), hipMemcpyDeviceToDevice, h->stream));
        BHS_TRY(timed(h, "assemble_scatter", nnzIn, [&] {
            hipLaunchKernelGGL(k_as_scatter, dim3(as_grid(nnzIn)), dim3(256), 0, h->stream, m, n, nnzIn, in.rows, in.cols, in.flags,
                               (const int*)rawPtr, cur, keys, rowOf, ctl);
            return 1;
        }));
        BHS_TRY(as_sort(h, m, nkept));
        BHS_TRY(timed(h, "assemble_dedupe", nkept, [&] {
            hipLaunchKernelGGL(k_as_flag, dim3(as_grid(nkept)), dim3(256), 0, h->stream, nkept, (const tr_u64*)keys, (const int*)rowOf,
                               (in.flags & kAsMode) == kAsKeep ? 1 : 0, map, cnt);
            return 1;
        }));
        BHS_TRY(side_scan(h, ws, "assemble_scan", kAsScanHeads, nWords, off, off));
        BHS_TRY(timed(h, "assemble_dedupe", 0, [&] {
            hipLaunchKernelGGL(k_as_emit, dim3(as_grid(nkept)), dim3(256), 0, h->stream, nkept, (const tr_u64*)keys, (const tr_u64*)map,
                               (const int*)off, in.Zj, ent, in.perm, ctl);
            hipLaunchKernelGGL(k_as_rowptr, dim3(as_grid((long long)m + 1)), dim3(256), 0, h->stream, m, nkept, (const int*)rawPtr,
                               (const tr_u64*)map, (const int*)off, in.Zp, ctl);
            return 2;
        }));
        if (in.Zx) {
            BHS_TRY(timed(h, "assemble_values", nkept, [&] {
                hipLaunchKernelGGL(k_as_values, dim3(as_grid(nkept)), dim3(256), 0, h->stream, nkept, (const long long*)(ctl + AS_TOTAL_B),
                                   nkept, nnzIn, (const int*)ent, (const int*)nullptr, (const tr_u64*)keys, in.vals,
                                   (in.flags & kAsMode) == kAsKeep ? (int)kAsFirst : (in.flags & kAsMode), (int)kAsBroken, in.Zx, ctl);
                return 1;
            }));
        }
    }
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, AS_INTS));                           // the number of entries, the error word of our own indices
    BHS_TRY(side_close(h, ws, ms_out));
    if (ws.host[AS_ERR]) return BHS_ERR_INTERNAL;                     // (a place outside its row: the triplets changed under the call)
    long long nnzZ = 0;
    if (nkept > 0) memcpy(&nnzZ, ws.host + AS_TOTAL_B, sizeof(nnzZ));
    if (nnzZ < 0 || nnzZ > nkept || (nkept > 0 && nnzZ == 0)) return BHS_ERR_INTERNAL;
    if (nnzZ_out) *nnzZ_out = (int)nnzZ;
    if (nkept_out) *nkept_out = nkept;
    return BHS_SUCCESS;
}

int as_values_run(bhs_handle* h, int nnzIn, const value_t* vals, int nnzZ, const int* entryPtr, const int* perm, int mode, value_t* Zx,
                  double* ms_out)
{
    SideWs& ws = h->asWs;
    BHS_TRY(side_prepare(h, ws, AS_INTS, 0, 0));
    side_reset_stats(h);
    int* ctl = (int*)ws.ctl.p;
    BHS_TRY(side_begin(h, ws));
    BHS_HIP(hipMemsetAsync(ctl, 0, sizeof(int) * AS_INTS, h->stream));
    BHS_TRY(timed(h, "assemble_check", nnzZ, [&] {
        hipLaunchKernelGGL(k_as_check_map, dim3(as_grid(std::max<long long>((long long)nnzZ + 1, nnzIn))), dim3(256), 0, h->stream, nnzZ,
                           nnzIn, entryPtr, perm, ctl);
        return 1;
    }));
    BHS_TRY(side_read_ctl(h, ws, AS_INTS));
    if (ws.host[AS_ERR]) return BHS_ERR_INVALID_ARG;                  // (valZ has not been written)
    if (nnzZ > 0) {
        int stat = 0;
        BHS_TRY(timed(h, "assemble_values", nnzZ, [&] {
            hipLaunchKernelGGL(k_as_values, dim3(as_grid(nnzZ)), dim3(256), 0, h->stream, nnzZ, (const long long*)nullptr, nnzIn, nnzIn,
                               entryPtr, perm, (const tr_u64*)nullptr, vals, mode, (int)kAsBadArg, Zx, ctl);
            return 1;
        }, &stat));
        h->stats[stat].nnz_out += nnzZ;
    }
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, AS_INTS));
    BHS_TRY(side_close(h, ws, ms_out));
    return ws.host[AS_ERR] ? (int)BHS_ERR_INVALID_ARG : (int)BHS_SUCCESS;   // (the map changed between the two kernels: not followed)
}

}  // namespace

extern "C" {

int bhs_coo_assemble_device(bhs_handle* h, int m, int n, int nnzIn, const int* d_rowInd, const int* d_colInd, const bhs_value_t* d_valIn,
                            int flags, int* d_rowPtrZ, int* d_colIndZ, bhs_value_t* d_valZ, int* d_entryPtr, int* d_perm, int* nnzZ_out,
                            int* nkept_out, double* ms_out)
{
    if (!h || h->ps.open || m < 0 || n < 0 || nnzIn < 0 || (flags & ~(kAsMode | kAsIgnoreNeg)) || !d_rowPtrZ) return BHS_ERR_INVALID_ARG;
    if (nnzIn > 0 && (!d_rowInd || !d_colInd || !d_colIndZ)) return BHS_ERR_INVALID_ARG;
    if (d_valZ && !d_valIn) return BHS_ERR_INVALID_ARG;
    const size_t nz = (size_t)nnzIn;
    if (side_aliased({{d_rowPtrZ, sizeof(int) * ((size_t)m + 1)}, {d_colIndZ, sizeof(int) * nz}, {d_valZ, sizeof(value_t) * nz},
                      {d_entryPtr, sizeof(int) * (nz + 1)}, {d_perm, sizeof(int) * nz}},
                     {{d_rowInd, sizeof(int) * nz}, {d_colInd, sizeof(int) * nz}, {d_valIn, sizeof(value_t) * nz}}))
        return BHS_ERR_INVALID_ARG;
    AsIn in;
    in.m = m; in.n = n; in.nnzIn = nnzIn; in.flags = flags;
    in.rows = d_rowInd; in.cols = d_colInd; in.vals = (const value_t*)d_valIn;
    in.Zp = d_rowPtrZ; in.Zj = d_colIndZ; in.Zx = nnzIn > 0 ? (value_t*)d_valZ : nullptr; in.entryPtr = d_entryPtr; in.perm = d_perm;
    return guarded(h, [&] { return as_run(h, in, nnzZ_out, nkept_out, ms_out); });
}

int bhs_coo_assemble_values_device(bhs_handle* h, int nnzIn, const bhs_value_t* d_valIn, int nnzZ, const int* d_entryPtr, const int* d_perm,
                                   int flags, bhs_value_t* d_valZ, double* ms_out)
{
    if (!h || h->ps.open || nnzIn < 0 || nnzZ < 0 || !d_entryPtr) return BHS_ERR_INVALID_ARG;
    if (flags != kAsSum && flags != kAsFirst && flags != kAsLast) return BHS_ERR_INVALID_ARG;
    if ((nnzIn > 0 && (!d_valIn || !d_perm)) || (nnzZ > 0 && !d_valZ)) return BHS_ERR_INVALID_ARG;
    const size_t zBytes = sizeof(value_t) * (size_t)nnzZ;
    if (side_aliased({{d_valZ, zBytes}}, {{d_valIn, sizeof(value_t) * (size_t)nnzIn}, {d_entryPtr, sizeof(int) * ((size_t)nnzZ + 1)},
                                          {d_perm, sizeof(int) * (size_t)nnzIn}}))
        return BHS_ERR_INVALID_ARG;
    return guarded(h, [&] {
        return as_values_run(h, nnzIn, (const value_t*)d_valIn, nnzZ, d_entryPtr, d_perm, flags, (value_t*)d_valZ, ms_out);
    });
}

}  // extern "C"
