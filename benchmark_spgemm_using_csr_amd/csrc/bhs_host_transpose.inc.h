// bhs_host_transpose.inc.h -- the transpose (bhs_csr_transpose_device, bhs_csr_transpose_values_device; kernels in
// bhs_transpose.hip.h)
// (A part of bhsparse_hip.hip's translation unit: included there after the entry selection.)
//
// Like the masked multiply, the add and the selection the transpose works beside the pipeline: its workspace (h->trWs: counters,
// queues, counts, tile words, events, the pinned mirror; set up, read and scanned by bhs_host_side.inc.h) and the scratch
// arrays are buffers of its own from the grow-only pool.  It binds nothing and serves nothing through the getters: every
// output array is the caller's.

namespace {

struct TrIn {
    int m, n, nnzX;
    const int* Xp; const int* Xj; const value_t* Xx;
};

constexpr SideScanWords kTrScanWords = {TR_TICKET, TR_SCANTOTAL, TR_SCANBINS, TR_MAXCNT};

// the ordering and fill pass on the queues and bin counts in h->trWs.queue / h->trWs.host
int tr_fill(bhs_handle* h, const TrIn& in, int* Tj, value_t* Tx, int* perm)
{
    const int n = in.n;
    const int* queue = (const int*)h->trWs.queue.p;
    const int* count = h->trWs.host + TR_COUNT;
    const int* Tp = (const int*)h->trWs.cnt.p;
    tr_u64* keys = (tr_u64*)h->trKeys.p;
    if (count[kTrShort]) {
        const int nq = count[kTrShort];
        BHS_TRY(timed(h, "transpose_short", nq, [&] {
            hipLaunchKernelGGL(k_tr_fill_short, dim3((unsigned)((nq + 15) / 16)), dim3(256), 0, h->stream, nq,
                               queue + (size_t)kTrShort * n, in.nnzX, Tp, (const tr_u64*)keys, in.Xx, Tj, Tx, perm);
            return 1;
        }));
    }
    if (count[kTrWave]) {
        const int nq = count[kTrWave];
        BHS_TRY(timed(h, "transpose_wave", nq, [&] {
            hipLaunchKernelGGL(k_tr_fill_wave, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, h->stream, nq,
                               queue + (size_t)kTrWave * n, in.nnzX, Tp, (const tr_u64*)keys, in.Xx, Tj, Tx, perm);
            return 1;
        }));
    }
    if (count[kTrLong]) {
        const int nq = count[kTrLong];
        BHS_TRY(timed(h, "transpose_long", nq, [&] {
            hipLaunchKernelGGL(k_tr_fill_long, dim3((unsigned)std::min<long long>(nq, (long long)h->numCU * 8)), dim3(256), 0,
                               h->stream, nq, queue + (size_t)kTrLong * n, in.nnzX, Tp, keys, in.Xx, Tj, Tx, perm);
            return 1;
        }));
    }
    return BHS_SUCCESS;
}

int tr_run(bhs_handle* h, const TrIn& in, int* d_rowPtrT, int* Tj, value_t* Tx, int* perm, double* ms_out)
{
    const int m = in.m, n = in.n;
    SideWs& ws = h->trWs;
    BHS_TRY(side_prepare(h, ws, TR_INTS, sizeof(int) * (size_t)kTrBins * (size_t)std::max(n, 1), (size_t)n + 1));
    const long long nWg = std::max<long long>(1, ((long long)m + kTrRows - 1) / kTrRows);
    BHS_TRY(ensure(h, h->trCur, sizeof(int) * ((size_t)n + 1)));
    BHS_TRY(ensure(h, h->trWin, sizeof(int2) * (size_t)nWg));
    BHS_TRY(ensure(h, h->trKeys, sizeof(tr_u64) * (size_t)std::max(in.nnzX, 1)));
    side_reset_stats(h);
    int* ctl = (int*)ws.ctl.p;
    int* cnt = (int*)ws.cnt.p;
    BHS_TRY(side_begin(h, ws));
    BHS_HIP(hipMemsetAsync(ctl, 0, sizeof(int) * TR_INTS, h->stream));
    BHS_HIP(hipMemsetAsync(cnt, 0, sizeof(int) * ((size_t)n + 1), h->stream));
    int stat = 0;
    BHS_TRY(timed(h, "transpose_count", m, [&] {
        hipLaunchKernelGGL(k_tr_count, dim3((unsigned)nWg), dim3(256), 0, h->stream, m, n, in.nnzX, in.Xp, in.Xj, cnt, ctl,
                           (int2*)h->trWin.p);
        if (n == 0) return 1;
        hipLaunchKernelGGL(k_tr_bin, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, n, (const int*)cnt, ctl,
                           (int*)ws.queue.p);
        return 2;
    }, &stat));
    BHS_TRY(side_read_ctl(h, ws, TR_INTS));
    if (ws.host[TR_ERR]) return BHS_ERR_INVALID_ARG;               // (nothing caller-owned has been written)
    h->stats[stat].nnz_out += in.nnzX;
    if (n == 0 || in.nnzX == 0) {
        BHS_HIP(hipMemsetAsync(d_rowPtrT, 0, sizeof(int) * ((size_t)n + 1), h->stream));
    } else {
        BHS_TRY(side_scan(h, ws, "transpose_scan", kTrScanWords, n, (const int*)h->trCur.p, d_rowPtrT));
        BHS_HIP(hipMemcpyAsync(h->trCur.p, cnt, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToDevice, h->stream));
        BHS_TRY(timed(h, "transpose_scatter", m, [&] {
            hipLaunchKernelGGL(k_tr_scatter, dim3((unsigned)nWg), dim3(256), 0, h->stream, m, in.nnzX, in.Xp, in.Xj, (int*)h->trCur.p,
                               (const int2*)h->trWin.p, (tr_u64*)h->trKeys.p);
            return 1;
        }));
        BHS_TRY(tr_fill(h, in, Tj, Tx, perm));
    }
    BHS_TRY(side_end(h, ws));
    BHS_TRY(wait_stream(h));
    BHS_TRY(side_elapsed(h, ws, ms_out));
    return side_collect(h, 0);
}

int tr_values_run(bhs_handle* h, int nnzX, const value_t* Xx, const int* perm, value_t* Tx, double* ms_out)
{
    SideWs& ws = h->trWs;
    BHS_TRY(side_prepare(h, ws, TR_INTS, 0, 0));
    side_reset_stats(h);
    int* ctl = (int*)ws.ctl.p;
    BHS_TRY(side_begin(h, ws));
    BHS_HIP(hipMemsetAsync(ctl, 0, sizeof(int) * TR_INTS, h->stream));
    if (nnzX > 0) {
        int stat = 0;
        BHS_TRY(timed(h, "transpose_values", 0, [&] {
            const long long per = 256LL * kTrVec;
            const long long gs = std::max<long long>(1, std::min<long long>((nnzX + per - 1) / per, (long long)h->numCU * 32));
            hipLaunchKernelGGL(k_tr_values, dim3((unsigned)gs), dim3(256), 0, h->stream, nnzX, Xx, perm, Tx,
                               ((uintptr_t)Tx & 15) == 0 ? 1 : 0, ctl);
            return 1;
        }, &stat));
        h->stats[stat].nnz_out += nnzX;
    }
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, TR_INTS));
    BHS_TRY(side_close(h, ws, ms_out));
    return ws.host[TR_ERR] ? (int)BHS_ERR_INVALID_ARG : (int)BHS_SUCCESS;
}

}  // namespace

extern "C" {

int bhs_csr_transpose_device(bhs_handle* h, int m, int n, int nnzX, const bhs_value_t* d_valX, const int* d_rowPtrX,
                             const int* d_colIndX, int* d_rowPtrT, int* d_colIndT, bhs_value_t* d_valT, int* d_perm, double* ms_out)
{
    if (!h || h->ps.open || m < 0 || n < 0 || nnzX < 0 || !d_rowPtrX || !d_rowPtrT) return BHS_ERR_INVALID_ARG;
    if (nnzX > 0 && (!d_colIndX || !d_colIndT || (d_valT && !d_valX))) return BHS_ERR_INVALID_ARG;
    if (d_rowPtrT == d_rowPtrX || (nnzX > 0 && (d_colIndT == d_colIndX || (d_valT && d_valT == d_valX) || d_perm == d_colIndX ||
                                                d_perm == d_colIndT)))
        return BHS_ERR_INVALID_ARG;                                  // (outputs must not overlap inputs)
    TrIn in;
    in.m = m; in.n = n; in.nnzX = nnzX; in.Xp = d_rowPtrX; in.Xj = d_colIndX; in.Xx = (const value_t*)d_valX;
    return guarded(h, [&] { return tr_run(h, in, d_rowPtrT, d_colIndT, (value_t*)d_valT, d_perm, ms_out); });
}

int bhs_csr_transpose_values_device(bhs_handle* h, int nnzX, const bhs_value_t* d_valX, const int* d_perm, bhs_value_t* d_valT,
                                    double* ms_out)
{
    if (!h || h->ps.open || nnzX < 0) return BHS_ERR_INVALID_ARG;
    if (nnzX > 0 && (!d_valX || !d_perm || !d_valT || d_valT == d_valX)) return BHS_ERR_INVALID_ARG;
    return guarded(h, [&] { return tr_values_run(h, nnzX, (const value_t*)d_valX, d_perm, (value_t*)d_valT, ms_out); });
}

}  // extern "C"
