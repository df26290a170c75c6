// bhs_host_extract.inc.h -- submatrix extraction and permutation (bhs_csr_extract_{symbolic,numeric}_device; kernels in
// bhs_extract.hip.h)
// (A part of bhsparse_hip.hip's translation unit: included there last, after the semiring multiply.)
//
// Like the add, the selection and the transpose the extraction works beside the pipeline: its workspace (h->exWs: counters,
// queues, counts, tile words, events, the pinned mirror; set up, read and scanned by bhs_host_side.inc.h), the column map and
// the scratch keys are buffers of its own from the grow-only pool.  It binds nothing and serves nothing through the getters:
// every output array is the caller's.
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
    BHS_TRY(side_prepare(h, h->exWs, EX_INTS, sizeof(int) * (size_t)kExBins * (size_t)std::max(in.mI, 1), (size_t)in.mI + 1));
    if (in.cols) BHS_TRY(ensure(h, h->exInv, sizeof(int) * (size_t)std::max(in.n, 1)));
    return BHS_SUCCESS;
}

constexpr SideScanWords kExScanWords = {EX_TICKET, EX_SCANTOTAL, EX_SCANBINS, EX_MAXCNT};

// Validation, the column map, the count pass and their round trip.  Afterwards h->exWs.cnt holds the Z rows' counts, h->exWs.queue
// the bins' rows, h->exWs.host the control words; *nnzZ the number of survivors.  Zp (may be NULL): a row pointer of Z that
// every count must agree with.  Nothing caller-owned is written.
int ex_count(bhs_handle* h, const ExIn& in, const int* Zp, int nnzZ, long long* total_out)
{
    int* ctl = (int*)h->exWs.ctl.p;
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
                           inv, Zp, nnzZ, (int*)h->exWs.cnt.p, ctl, (int*)h->exWs.queue.p);
        if (in.nnzX <= kExWaveL) return 1;                           // (no row can be long)
        const long long gl = std::max<long long>(1, std::min<long long>(in.mI, (long long)h->numCU * 8));
        hipLaunchKernelGGL(k_ex_count_long, dim3((unsigned)gl), dim3(256), 0, h->stream, in.m, in.n, in.nnzX, in.Xp, in.Xj, in.mI,
                           in.rows, inv, Zp, (int*)h->exWs.cnt.p, ctl, (const int*)h->exWs.queue.p);
        return 2;
    }, &stat));
    BHS_TRY(side_read_ctl(h, h->exWs, EX_HEAD));                 // (the one round trip of a symbolic call, the first of a numeric one)
    if (h->exWs.host[EX_ERR]) return BHS_ERR_INVALID_ARG;
    unsigned long long total = 0;
    memcpy(&total, h->exWs.host + EX_TOTAL, 8);
    h->stats[stat].nnz_out += (int64_t)total;
    *total_out = (long long)total;
    return BHS_SUCCESS;
}

// the fill pass on the queues and bin counts in h->exWs.queue / h->exWs.host
int ex_fill(bhs_handle* h, const ExIn& in, int nnzZ, const int* Zp, int* Zj, value_t* Zx, int* perm)
{
    const int mI = in.mI;
    const int* queue = (const int*)h->exWs.queue.p;
    const int* inv = in.cols ? (const int*)h->exInv.p : nullptr;
    int count[kExBins];
    for (int b = 0; b < kExBins; ++b) count[b] = h->exWs.host[EX_COUNT + b];
    int* ctl = (int*)h->exWs.ctl.p;
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
    side_reset_stats(h);
    long long nnzZ = 0;
    BHS_TRY(ex_count(h, in, nullptr, 0, &nnzZ));
    if (nnzZ > 0x7fffffffLL) return BHS_ERR_NNZ_OVERFLOW;            // (nothing caller-owned has been written)
    // (without bins any array of mI + 1 ints will do for the scan's row pointer: the queues)
    BHS_TRY(side_scan(h, h->exWs, "extract_scan", kExScanWords, in.mI, (const int*)h->exWs.queue.p, d_rowPtrZ));
    BHS_TRY(wait_stream(h));
    BHS_TRY(side_collect(h, 0));
    if (nnzZ_out) *nnzZ_out = (int)nnzZ;
    return BHS_SUCCESS;
}

int ex_numeric_run(bhs_handle* h, const ExIn& in, int nnzZ, const int* Zp, int* Zj, value_t* Zx, int* perm, double* ms_out)
{
    BHS_TRY(ex_prepare(h, in));
    side_reset_stats(h);
    BHS_TRY(side_begin(h, h->exWs));
    long long total = 0;
    BHS_TRY(ex_count(h, in, Zp, nnzZ, &total));                      // (every row's survivors are what rowPtrZ says, or nothing is written)
    if (total != (long long)nnzZ) return BHS_ERR_INVALID_ARG;
    BHS_TRY(ex_fill(h, in, nnzZ, Zp, Zj, Zx, perm));
    BHS_TRY(side_end(h, h->exWs));
    BHS_TRY(side_read_ctl(h, h->exWs, EX_INTS));
    BHS_TRY(side_close(h, h->exWs, ms_out));
    if (h->exWs.host[EX_ERR]) return BHS_ERR_INVALID_ARG;
    long long reordered = 0;
    for (int s = 0; s < kExReordSlots; ++s) reordered += h->exWs.host[EX_REORD + s * kExReordStride];
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
    ExIn in;
    in.m = m; in.n = n; in.nnzX = nnzX; in.Xp = d_rowPtrX; in.Xj = d_colIndX; in.Xx = nullptr;
    in.mI = mI; in.rows = d_rows; in.nJ = nJ; in.cols = d_cols;
    return guarded(h, [&] { return ex_symbolic_run(h, in, d_rowPtrZ, nnzZ_out); });
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
    ExIn in;
    in.m = m; in.n = n; in.nnzX = nnzX; in.Xp = d_rowPtrX; in.Xj = d_colIndX; in.Xx = (const value_t*)d_valX;
    in.mI = mI; in.rows = d_rows; in.nJ = nJ; in.cols = d_cols;
    return guarded(h, [&] { return ex_numeric_run(h, in, nnzZ, d_rowPtrZ, d_colIndZ, (value_t*)d_valZ, d_perm, ms_out); });
}

}  // extern "C"
