// bhs_host_extract.inc.h -- submatrix extraction and permutation (bhs_csr_extract_{symbolic,numeric}_device; kernels in
// bhs_extract.hip.h)
// (A part of bhsparse_hip.hip's translation unit: included there last, after the semiring multiply.)
//
// Like the add, the selection and the transpose the extraction works beside the pipeline: counters, queues, tile words, epoch,
// events, the pinned mirror, the column map and the scratch keys are buffers of its own from the grow-only pool.  It binds
// nothing and serves nothing through the getters: every output array is the caller's.
//
// The kernels' header is included here, not among the translation unit's kernel headers (as bhs_host_semiring.inc.h does).
#include "bhs_extract.hip.h"

namespace {

struct ExIn {
    int m, n, nnzX;
    const int* Xp; const int* Xj; const value_t* Xx;
    int mI; const int* rows;
    int nJ; const int* cols;
};

int ex_prepare(bhs_handle* h, const ExIn& in)
{
    h->ls = h->stream;
    if (!h->exEv[0]) {
        BHS_HIP(hipEventCreate(&h->exEv[0]));
        BHS_HIP(hipEventCreate(&h->exEv[1]));
    }
    if (!h->exHost) BHS_HIP(hipHostMalloc((void**)&h->exHost, sizeof(int) * EX_INTS, hipHostMallocDefault));
    BHS_TRY(ensure(h, h->exCtl, sizeof(int) * EX_INTS));
    BHS_TRY(ensure(h, h->exQueue, sizeof(int) * (size_t)kExBins * (size_t)std::max(in.mI, 1)));
    BHS_TRY(ensure(h, h->exCnt, sizeof(int) * ((size_t)in.mI + 1)));
    BHS_TRY(ensure(h, h->exTiles, sizeof(unsigned long long) * (size_t)std::max((in.mI + kScan1Tile - 1) / kScan1Tile, 1), true));
    if (in.cols) BHS_TRY(ensure(h, h->exInv, sizeof(int) * (size_t)std::max(in.n, 1)));
    return BHS_SUCCESS;
}

// the control words to the host: the one round trip of a symbolic call, the first of a numeric one
int ex_read_ctl(bhs_handle* h, int ints = EX_HEAD)
{
    BHS_HIP(hipMemcpyAsync(h->exHost, h->exCtl.p, sizeof(int) * (size_t)ints, hipMemcpyDeviceToHost, h->stream));
    BHS_TRY(wait_stream(h));
    return BHS_SUCCESS;
}

// Validation, the column map, the count pass and their round trip.  Afterwards h->exCnt holds the Z rows' counts, h->exQueue
// the bins' rows, h->exHost the control words; *nnzZ the number of survivors.  Zp (may be NULL): a row pointer of Z that
// every count must agree with.  Nothing caller-owned is written.
int ex_count(bhs_handle* h, const ExIn& in, const int* Zp, int nnzZ, long long* total_out)
{
    int* ctl = (int*)h->exCtl.p;
    const int* inv = in.cols ? (const int*)h->exInv.p : nullptr;
    BHS_HIP(hipMemsetAsync(ctl, 0, sizeof(int) * EX_INTS, h->stream));
    if (in.rows || in.cols) {
        const int most = std::max(in.m, std::max(in.rows ? in.mI : 0, in.cols ? in.nJ : 0));
        BHS_TRY(timed(h, "extract_map", most, [&]() -> int {
            if (in.cols && in.n > 0 && hipMemsetAsync(h->exInv.p, 0xff, sizeof(int) * (size_t)in.n, h->stream) != hipSuccess)
                return BHS_ERR_LAUNCH;
            hipLaunchKernelGGL(k_ex_map, dim3((unsigned)std::max(1, (most + 255) / 256)), dim3(256), 0, h->stream, in.m, in.n, in.nnzX,
                               in.Xp, in.mI, in.rows, in.nJ, in.cols, (int*)h->exInv.p, ctl);
            return 1;
        }));
    }
    int stat = 0;
    BHS_TRY(timed(h, "extract_count", in.mI, [&] {
        const long long gs = std::max<long long>(1, ((long long)in.mI + kExRows - 1) / kExRows);
        hipLaunchKernelGGL(k_ex_count, dim3((unsigned)gs), dim3(256), 0, h->stream, in.m, in.n, in.nnzX, in.Xp, in.Xj, in.mI, in.rows,
                           inv, Zp, nnzZ, (int*)h->exCnt.p, ctl, (int*)h->exQueue.p);
        if (in.nnzX <= kExWaveL) return 1;                           // (no row can be long)
        const long long gl = std::max<long long>(1, std::min<long long>(in.mI, (long long)h->numCU * 8));
        hipLaunchKernelGGL(k_ex_count_long, dim3((unsigned)gl), dim3(256), 0, h->stream, in.m, in.n, in.nnzX, in.Xp, in.Xj, in.mI,
                           in.rows, inv, Zp, (int*)h->exCnt.p, ctl, (const int*)h->exQueue.p);
        return 2;
    }, &stat));
    BHS_TRY(ex_read_ctl(h));
    if (h->exHost[EX_ERR]) return BHS_ERR_INVALID_ARG;
    unsigned long long total = 0;
    memcpy(&total, h->exHost + EX_TOTAL, 8);
    h->stats[stat].nnz_out += (int64_t)total;
    *total_out = (long long)total;
    return BHS_SUCCESS;
}

// rowPtrZ from the counts of ex_count: the library's one-pass scan over h->exCnt (tile words and epoch of the extraction's
// own), then a copy to where the row pointer is wanted
int ex_scan(bhs_handle* h, int mI, int* d_rowPtrZ)
{
    int* ctl = (int*)h->exCtl.p;
    int* cnt = (int*)h->exCnt.p;
    const int nTiles = (mI + kScan1Tile - 1) / kScan1Tile;
    if (nTiles == 0) {
        BHS_HIP(hipMemsetAsync(cnt, 0, sizeof(int), h->stream));
    } else {
        h->exEpoch = (h->exEpoch + 1) & 0x3FFFFu;
        if (h->exEpoch == 0) {                                       // (see scan_rowptr)
            BHS_HIP(hipMemsetAsync(h->exTiles.p, 0, sizeof(unsigned long long) * (size_t)nTiles, h->stream));
            h->exEpoch = 1;
        }
        BinSpec none;                                                // (no bins: the scan's histogram stays empty)
        memset(&none, 0, sizeof(none));
        BHS_TRY(timed(h, "extract_scan", mI, [&] {
            // (the scan reads a row pointer of mI + 1 ints for its bins; without bins any such array will do: the queues)
            hipLaunchKernelGGL(k_scan_onepass, dim3((unsigned)nTiles), dim3(kScan1Block), 0, h->stream, mI, cnt, (const int*)h->exQueue.p,
                               (unsigned long long*)h->exTiles.p, h->exEpoch, ctl + EX_TICKET, (long long*)(ctl + EX_SCANTOTAL),
                               ctl + EX_SCANBINS, none, ctl + EX_MAXCNT, (const int*)nullptr);
            return 1;
        }));
    }
    BHS_HIP(hipMemcpyAsync(d_rowPtrZ, cnt, sizeof(int) * ((size_t)mI + 1), hipMemcpyDeviceToDevice, h->stream));
    return BHS_SUCCESS;
}

// the fill pass on the queues and bin counts in h->exQueue / h->exHost
int ex_fill(bhs_handle* h, const ExIn& in, int nnzZ, const int* Zp, int* Zj, value_t* Zx, int* perm)
{
    const int mI = in.mI;
    const int* queue = (const int*)h->exQueue.p;
    const int* inv = in.cols ? (const int*)h->exInv.p : nullptr;
    int count[kExBins];
    for (int b = 0; b < kExBins; ++b) count[b] = h->exHost[EX_COUNT + b];
    int* ctl = (int*)h->exCtl.p;
    if (count[kExShort]) {
        const int nq = count[kExShort];
        BHS_TRY(timed(h, "extract_short", nq, [&] {
            hipLaunchKernelGGL(k_ex_fill_short, dim3((unsigned)((nq + 15) / 16)), dim3(256), 0, h->stream, nq,
                               queue + (size_t)kExShort * mI, in.m, in.n, in.nnzX, in.Xp, in.Xj, in.Xx, in.rows, inv, nnzZ, Zp, Zj, Zx,
                               perm, ctl);
            return 1;
        }));
    }
    if (count[kExWave]) {
        const int nq = count[kExWave];
        BHS_TRY(timed(h, "extract_wave", nq, [&] {
            hipLaunchKernelGGL(k_ex_fill_wave, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, h->stream, nq,
                               queue + (size_t)kExWave * mI, in.m, in.n, in.nnzX, in.Xp, in.Xj, in.Xx, in.rows, inv, nnzZ, Zp, Zj, Zx,
                               perm, ctl);
            return 1;
        }));
    }
    if (count[kExLong]) {
        const int nq = count[kExLong];
        BHS_TRY(ensure(h, h->exKeys, sizeof(ex_u64) * (size_t)std::max(nnzZ, 1)));
        BHS_TRY(timed(h, "extract_long", nq, [&] {
            hipLaunchKernelGGL(k_ex_fill_long, dim3((unsigned)std::min<long long>(nq, (long long)h->numCU * 8)), dim3(256), 0,
                               h->stream, nq, queue + (size_t)kExLong * mI, in.m, in.n, in.nnzX, in.Xp, in.Xj, in.Xx, in.rows, inv,
                               nnzZ, Zp, (ex_u64*)h->exKeys.p, Zj, Zx, perm, ctl);
            return 1;
        }));
    }
    return BHS_SUCCESS;
}

int ex_symbolic_run(bhs_handle* h, const ExIn& in, int* d_rowPtrZ, int* nnzZ_out)
{
    BHS_TRY(ex_prepare(h, in));
    add_reset_stats(h);
    long long nnzZ = 0;
    BHS_TRY(ex_count(h, in, nullptr, 0, &nnzZ));
    if (nnzZ > 0x7fffffffLL) return BHS_ERR_NNZ_OVERFLOW;            // (nothing caller-owned has been written)
    BHS_TRY(ex_scan(h, in.mI, d_rowPtrZ));
    BHS_TRY(wait_stream(h));
    BHS_TRY(add_collect(h, 0));
    if (nnzZ_out) *nnzZ_out = (int)nnzZ;
    return BHS_SUCCESS;
}

int ex_numeric_run(bhs_handle* h, const ExIn& in, int nnzZ, const int* Zp, int* Zj, value_t* Zx, int* perm, double* ms_out)
{
    BHS_TRY(ex_prepare(h, in));
    add_reset_stats(h);
    BHS_HIP(hipEventRecord(h->exEv[0], h->stream));
    long long total = 0;
    BHS_TRY(ex_count(h, in, Zp, nnzZ, &total));                      // (every row's survivors are what rowPtrZ says, or nothing is written)
    if (total != (long long)nnzZ) return BHS_ERR_INVALID_ARG;
    BHS_TRY(ex_fill(h, in, nnzZ, Zp, Zj, Zx, perm));
    BHS_HIP(hipEventRecord(h->exEv[1], h->stream));
    BHS_TRY(ex_read_ctl(h, EX_INTS));
    if (ms_out) {
        float ms = 0;
        BHS_HIP(hipEventElapsedTime(&ms, h->exEv[0], h->exEv[1]));
        *ms_out = ms;
    }
    BHS_TRY(add_collect(h, 0));
    if (h->exHost[EX_ERR]) return BHS_ERR_INVALID_ARG;
    long long reordered = 0;
    for (int s = 0; s < kExReordSlots; ++s) reordered += h->exHost[EX_REORD + s * kExReordStride];
    h->exReordered = reordered;
    return BHS_SUCCESS;
}

struct ExSpan {
    const void* p;
    size_t bytes;
};

bool ex_overlap(const ExSpan& a, const ExSpan& b)
{
    if (!a.p || !b.p || !a.bytes || !b.bytes) return false;
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

// does an output overlap an input or another output
bool ex_aliased(const ExSpan* outs, int nOut, const ExSpan* ins, int nIn)
{
    for (int o = 0; o < nOut; ++o) {
        for (int i = 0; i < nIn; ++i)
            if (ex_overlap(outs[o], ins[i])) return true;
        for (int p = o + 1; p < nOut; ++p)
            if (ex_overlap(outs[o], outs[p])) return true;
    }
    return false;
}

bool ex_args_ok(bhs_handle* h, int m, int n, int nnzX, const int* Xp, const int* Xj, int mI, const int* rows, int nJ, const int* cols)
{
    if (!h || h->ps.open || m < 0 || n < 0 || nnzX < 0 || mI < 0 || nJ < 0 || !Xp || (nnzX > 0 && !Xj)) return false;
    if (!rows && mI != m) return false;
    if (!cols && nJ != n) return false;
    return true;
}

}  // namespace

extern "C" {

int bhs_csr_extract_symbolic_device(bhs_handle* h, int m, int n, int nnzX, const int* d_rowPtrX, const int* d_colIndX, int mI,
                                    const int* d_rows, int nJ, const int* d_cols, int* d_rowPtrZ, int* nnzZ_out)
{
    if (!ex_args_ok(h, m, n, nnzX, d_rowPtrX, d_colIndX, mI, d_rows, nJ, d_cols) || !d_rowPtrZ) return BHS_ERR_INVALID_ARG;
    const ExSpan outs[1] = {{d_rowPtrZ, sizeof(int) * ((size_t)mI + 1)}};
    const ExSpan ins[4] = {{d_rowPtrX, sizeof(int) * ((size_t)m + 1)}, {d_colIndX, sizeof(int) * (size_t)nnzX},
                           {d_rows, sizeof(int) * (size_t)mI}, {d_cols, sizeof(int) * (size_t)nJ}};
    if (ex_aliased(outs, 1, ins, 4)) return BHS_ERR_INVALID_ARG;    // (outputs must not overlap inputs)
    BHS_HIP(hipSetDevice(h->device));
    ExIn in;
    in.m = m; in.n = n; in.nnzX = nnzX; in.Xp = d_rowPtrX; in.Xj = d_colIndX; in.Xx = nullptr;
    in.mI = mI; in.rows = d_rows; in.nJ = nJ; in.cols = d_cols;
    const int rc = ex_symbolic_run(h, in, d_rowPtrZ, nnzZ_out);
    if (rc) settle(h);
    return rc;
}

int bhs_csr_extract_numeric_device(bhs_handle* h, int m, int n, int nnzX, const bhs_value_t* d_valX, const int* d_rowPtrX,
                                   const int* d_colIndX, int mI, const int* d_rows, int nJ, const int* d_cols, int nnzZ,
                                   const int* d_rowPtrZ, int* d_colIndZ, bhs_value_t* d_valZ, int* d_perm, double* ms_out)
{
    if (!ex_args_ok(h, m, n, nnzX, d_rowPtrX, d_colIndX, mI, d_rows, nJ, d_cols) || !d_rowPtrZ || nnzZ < 0) return BHS_ERR_INVALID_ARG;
    if ((nnzZ > 0 && !d_colIndZ) || (d_valZ && !d_valX && nnzX > 0)) return BHS_ERR_INVALID_ARG;   // (without entries no value is read)
    const ExSpan outs[3] = {{d_colIndZ, sizeof(int) * (size_t)nnzZ}, {d_valZ, sizeof(value_t) * (size_t)nnzZ},
                            {d_perm, sizeof(int) * (size_t)nnzZ}};
    const ExSpan ins[6] = {{d_rowPtrX, sizeof(int) * ((size_t)m + 1)}, {d_colIndX, sizeof(int) * (size_t)nnzX},
                           {d_valX, sizeof(value_t) * (size_t)nnzX}, {d_rows, sizeof(int) * (size_t)mI},
                           {d_cols, sizeof(int) * (size_t)nJ}, {d_rowPtrZ, sizeof(int) * ((size_t)mI + 1)}};
    if (ex_aliased(outs, 3, ins, 6)) return BHS_ERR_INVALID_ARG;    // (outputs must not overlap inputs or one another)
    BHS_HIP(hipSetDevice(h->device));
    ExIn in;
    in.m = m; in.n = n; in.nnzX = nnzX; in.Xp = d_rowPtrX; in.Xj = d_colIndX; in.Xx = (const value_t*)d_valX;
    in.mI = mI; in.rows = d_rows; in.nJ = nJ; in.cols = d_cols;
    const int rc = ex_numeric_run(h, in, nnzZ, d_rowPtrZ, d_colIndZ, (value_t*)d_valZ, d_perm, ms_out);
    if (rc) settle(h);
    return rc;
}

}  // extern "C"
