// bhs_host_masked.inc.h -- the masked multiply (bhs_spgemm_masked[_device], kernels in bhs_masked.hip.h)
// (A part of bhsparse_hip.hip's translation unit: included there after the C-ABI of the ordinary multiply.)
//
// The call works beside the ordinary multiply, never through it: its workspace (h->maskWs: counters, queues, events, the
// pinned mirror; set up and read by bhs_host_side.inc.h) and its (host-array entry) staging copies are buffers of its own,
// so C of the last bhs_spgemm, the pipeline state, the class path's state and the speculative-launch figures stay as they were.  Only the kernel records are replaced: bhs_get_kernel_stats reports
// the last call, whichever it was.

namespace {

constexpr int kMaskHubItem = 8192;       // products per part of a hub row (k_masked_hub)
constexpr int kMaskHubMaxParts = 1024;

// What one bin's launch needs: its queue and the operands
struct MaskLaunch {
    int nq;
    const int2* q;
    const int *Mp, *Mj, *Ap, *Aj;
    const value_t* Ax;
    const int *Bp, *Bj;
    const value_t* Bx;
    int bSorted;
    value_t* valC;
    hipStream_t st;
};

enum { kMaskFamScan = 0, kMaskFamShort, kMaskFamWave, kMaskFamLong, kMaskFamHub };

// The kernel set of the plus-times masked multiply: the families' names and the launches of the bins.  (The semiring multiply
// brings a set of its own, bhs_host_semiring.inc.h; mask_drive below is the one driver of both.)
struct MaskedKernels {
    static const char* family(int f)
    {
        static const char* const names[] = {"masked_scan", "masked_short", "masked_wave", "masked_long", "masked_hub"};
        return names[f];
    }
    template <int G, int CAP, int BLOCK>
    static void lds(const MaskLaunch& a, unsigned grid)
    {
        hipLaunchKernelGGL((k_masked_lds<G, CAP, BLOCK>), dim3(grid), dim3(BLOCK), 0, a.st, a.nq, a.q, a.Mp, a.Mj, a.Ap, a.Aj, a.Ax,
                           a.Bp, a.Bj, a.Bx, a.bSorted, a.valC);
    }
    static void long_rows(const MaskLaunch& a)
    {
        hipLaunchKernelGGL(k_masked_long, dim3((unsigned)a.nq), dim3(256), 0, a.st, a.nq, a.q, a.Mp, a.Mj, a.Ap, a.Aj, a.Ax, a.Bp,
                           a.Bj, a.Bx, a.bSorted, a.valC);
    }
    static int hub(const MaskLaunch& a, int parts, unsigned gy, int ldsCap)    // returns the kernels launched
    {
        hipLaunchKernelGGL(k_masked_zero, dim3(gy), dim3(256), 0, a.st, a.nq, a.q, a.Mp, a.valC);
        hipLaunchKernelGGL(k_masked_hub, dim3((unsigned)parts, gy), dim3(256), 0, a.st, a.nq, a.q, a.Mp, a.Mj, a.Ap, a.Aj, a.Ax,
                           a.Bp, a.Bj, a.Bx, a.bSorted, ldsCap, a.valC);
        return 2;
    }
};

// The driver of a masked multiply with the kernel set K: validation and binning (k_masked_scan), the read-back, one launch
// block per non-empty bin, the timers.  keepStats: the call follows a multiply whose kernel records (and read-out events) stay.
template <typename K>
int mask_drive(bhs_handle* h, const int* dMp, const int* dMj, int nnzM, value_t* dValC, bool keepStats, int64_t* nnzCt_out,
               double* ms_out)
{
    const int m = h->m;
    SideWs& ws = h->maskWs;
    if (!keepStats) side_reset_stats(h);
    const size_t evFirst = h->evUsed;
    BHS_TRY(side_prepare(h, ws, MS_INTS, sizeof(int2) * (size_t)kMaskBins * (size_t)std::max(m, 1), 0));
    int* ctl = (int*)ws.ctl.p;
    const int2* queue = (const int2*)ws.queue.p;
    const int cap = 1 << h->maskTableLog2;
    MaskSpec spec;
    spec.shortLM = std::min(kMaskShortLM, cap);
    spec.shortP = kMaskShortP;
    spec.waveS = std::min(kMaskWaveTab, cap);
    spec.waveL = cap;
    spec.hubMin = h->maskHubMin;

    BHS_TRY(side_begin(h, ws));
    BHS_HIP(hipMemsetAsync(ctl, 0, sizeof(int) * MS_INTS, h->stream));
    int scanStat = 0;
    BHS_TRY(timed(h, K::family(kMaskFamScan), m, [&] {
        const long long gs = std::max<long long>(1, ((long long)m + kMaskScanRows - 1) / kMaskScanRows);
        hipLaunchKernelGGL(k_masked_scan, dim3((unsigned)gs), dim3(256), 0, h->stream, m, h->n, nnzM, dMp, dMj, h->dAp, h->dAj,
                           h->dBp, spec, ctl, (int2*)ws.queue.p);
        return 1;
    }, &scanStat));
    BHS_TRY(side_read_ctl(h, ws, MS_INTS));
    const int* hs = ws.host;
    if (hs[MS_ERR]) return BHS_ERR_INVALID_ARG;                    // (nothing has touched valC)
    unsigned long long total = 0, hubMax = 0, sums[kMaskBins];
    memcpy(&total, hs + MS_TOTAL, 8);
    memcpy(&hubMax, hs + MS_HUBMAX, 8);
    memcpy(sums, hs + MS_SUMS, sizeof(sums));
    h->stats[scanStat].products += (int64_t)total;
    int count[kMaskBins];
    memcpy(count, hs + MS_COUNT, sizeof(count));

    auto bin = [&](int b) {
        MaskLaunch a = {count[b], queue + (size_t)b * m, dMp, dMj, h->dAp, h->dAj, h->dAx, h->dBp, h->dBj, h->dBx,
                        h->bSorted ? 1 : 0, dValC, h->stream};
        return a;
    };
    int stat = 0;
    if (count[kMaskShort]) {
        const MaskLaunch a = bin(kMaskShort);
        BHS_TRY(timed(h, K::family(kMaskFamShort), a.nq, [&] {
            K::template lds<16, kMaskShortLM, 256>(a, (unsigned)((a.nq + 15) / 16));
            return 1;
        }, &stat));
        h->stats[stat].products += (int64_t)sums[kMaskShort];
    }
    if (count[kMaskWaveS] || count[kMaskWaveL]) {
        const MaskLaunch aS = bin(kMaskWaveS), aL = bin(kMaskWaveL);
        BHS_TRY(timed(h, K::family(kMaskFamWave), aS.nq + aL.nq, [&] {
            if (aS.nq) K::template lds<64, kMaskWaveTab, 256>(aS, (unsigned)((aS.nq + 3) / 4));
            if (aL.nq) K::template lds<64, kMaskHubLds, 64>(aL, (unsigned)aL.nq);
            return (aS.nq ? 1 : 0) + (aL.nq ? 1 : 0);
        }, &stat));
        h->stats[stat].products += (int64_t)(sums[kMaskWaveS] + sums[kMaskWaveL]);
    }
    if (count[kMaskLong]) {
        const MaskLaunch a = bin(kMaskLong);
        BHS_TRY(timed(h, K::family(kMaskFamLong), a.nq, [&] {
            K::long_rows(a);
            return 1;
        }, &stat));
        h->stats[stat].products += (int64_t)sums[kMaskLong];
    }
    if (count[kMaskHub]) {
        const MaskLaunch a = bin(kMaskHub);
        const int parts = (int)std::max<unsigned long long>(1, std::min<unsigned long long>(kMaskHubMaxParts, (hubMax + kMaskHubItem - 1) / kMaskHubItem));
        const unsigned gy = (unsigned)std::min(a.nq, 65535);
        BHS_TRY(timed(h, K::family(kMaskFamHub), a.nq, [&] { return K::hub(a, parts, gy, std::min(kMaskHubLds, cap)); }, &stat));
        h->stats[stat].products += (int64_t)sums[kMaskHub];
    }
    BHS_TRY(side_end(h, ws));
    BHS_TRY(wait_stream(h));
    if (nnzCt_out) *nnzCt_out = (int64_t)total;
    BHS_TRY(side_elapsed(h, ws, ms_out));
    return side_collect(h, evFirst);
}

int masked_run(bhs_handle* h, const int* dMp, const int* dMj, int nnzM, value_t* dValC, int64_t* nnzCt_out, double* ms_out)
{
    return mask_drive<MaskedKernels>(h, dMp, dMj, nnzM, dValC, false, nnzCt_out, ms_out);
}

int masked_check(bhs_handle* h, int nnzM)
{
    if (!h) return BHS_ERR_INVALID_ARG;
    if (!h->hasData) return BHS_ERR_NOT_READY;
    if (h->ps.open || nnzM < 0) return BHS_ERR_INVALID_ARG;          // (a split multiply owns the stream until its finish)
    return BHS_SUCCESS;
}

// The host-array entries (this one's and the semiring multiply's): M to the device copies of the masked multiply's own, `run`
// on them, valC back to the caller
template <typename F>
int mask_staged(bhs_handle* h, const int* rowPtrM, const int* colIndM, int nnzM, bhs_value_t* valC, F&& run)
{
    BHS_TRY(ensure(h, h->maskM[0], sizeof(int) * ((size_t)h->m + 1)));
    BHS_TRY(ensure(h, h->maskM[1], sizeof(int) * (size_t)std::max(nnzM, 1)));
    BHS_TRY(ensure(h, h->maskM[2], sizeof(value_t) * (size_t)std::max(nnzM, 1)));
    BHS_HIP(hipMemcpyAsync(h->maskM[0].p, rowPtrM, sizeof(int) * ((size_t)h->m + 1), hipMemcpyHostToDevice, h->stream));
    if (nnzM) BHS_HIP(hipMemcpyAsync(h->maskM[1].p, colIndM, sizeof(int) * (size_t)nnzM, hipMemcpyHostToDevice, h->stream));
    BHS_TRY(run((const int*)h->maskM[0].p, (const int*)h->maskM[1].p, (value_t*)h->maskM[2].p));
    if (nnzM) {
        BHS_HIP(hipMemcpyAsync(valC, h->maskM[2].p, sizeof(value_t) * (size_t)nnzM, hipMemcpyDeviceToHost, h->stream));
        BHS_HIP(hipStreamSynchronize(h->stream));
    }
    return BHS_SUCCESS;
}

}  // namespace

extern "C" {

int bhs_spgemm_masked_device(bhs_handle* h, const int* d_rowPtrM, const int* d_colIndM, int nnzM, bhs_value_t* d_valC,
                             int64_t* nnzCt_out, double* ms_out)
{
    BHS_TRY(masked_check(h, nnzM));
    if (!d_rowPtrM || (nnzM > 0 && (!d_colIndM || !d_valC))) return BHS_ERR_INVALID_ARG;
    return guarded(h, [&] { return masked_run(h, d_rowPtrM, d_colIndM, nnzM, (value_t*)d_valC, nnzCt_out, ms_out); });
}

int bhs_spgemm_masked(bhs_handle* h, const int* rowPtrM, const int* colIndM, int nnzM, bhs_value_t* valC, int64_t* nnzCt_out,
                      double* ms_out)
{
    BHS_TRY(masked_check(h, nnzM));
    if (!rowPtrM || (nnzM > 0 && (!colIndM || !valC))) return BHS_ERR_INVALID_ARG;
    return guarded(h, [&] {
        return mask_staged(h, rowPtrM, colIndM, nnzM, valC, [&](const int* dMp, const int* dMj, value_t* dValC) {
            return masked_run(h, dMp, dMj, nnzM, dValC, nnzCt_out, ms_out);
        });
    });
}

}  // extern "C"
