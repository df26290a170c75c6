// bhs_host_add.inc.h -- the sparse add (bhs_csr_add_{symbolic,numeric}_device, bhs_spgemm_add[_device]; kernels in bhs_add.hip.h)
// (A part of bhsparse_hip.hip's translation unit: included there after the masked multiply.)
//
// Like the masked multiply the add works beside the pipeline, never through its state: its workspace (h->addWs: counters,
// queues, counts, tile words, events, the pinned mirror; set up, read and scanned by bhs_host_side.inc.h) and its staging
// copies are buffers of its own.  bhs_spgemm_add runs the ordinary multiply and then either adds into its valC in place
// (D inside the pattern of A·B) or writes the sum to a second set of arrays that the getters serve until the next multiply
// (h->sumActive); the pipeline's own C arrays are never moved.

namespace {

struct AddIn {
    int m, n;
    int nnzX; const int* Xp; const int* Xj; const value_t* Xx;
    int nnzY; const int* Yp; const int* Yj; const value_t* Yx;
};

int add_prepare(bhs_handle* h, int m)
{
    return side_prepare(h, h->addWs, AD_INTS, sizeof(int) * (size_t)kAddBins * (size_t)std::max(m, 1), (size_t)m + 1);
}

constexpr SideScanWords kAddScanWords = {AD_TICKET, AD_SCANTOTAL, AD_SCANBINS, AD_MAXCNT};

// validity of one matrix alone (bhs_spgemm_add: D before the multiply)
int add_check(bhs_handle* h, int m, int n, int nnz, const int* P, const int* J)
{
    int* ctl = (int*)h->addWs.ctl.p;
    BHS_HIP(hipMemsetAsync(ctl, 0, sizeof(int) * AD_INTS, h->stream));
    BHS_TRY(timed(h, "add_count", m, [&] {
        const long long gs = std::max<long long>(1, ((long long)m + 15) / 16);
        hipLaunchKernelGGL(k_add_check, dim3((unsigned)gs), dim3(256), 0, h->stream, m, n, nnz, P, J, ctl);
        return 1;
    }));
    BHS_TRY(side_read_ctl(h, h->addWs, AD_INTS));
    return h->addWs.host[AD_ERR] ? (int)BHS_ERR_INVALID_ARG : (int)BHS_SUCCESS;
}

// The count pass and its round trip.  Afterwards h->addWs.cnt holds the rows' counts, h->addWs.queue the bins' rows, h->addWs.host
// the control words; *nnzZ the size of the union.  ypos (may be NULL): where in X every entry of Y sits.
int add_count(bhs_handle* h, const AddIn& in, int* ypos, long long* nnzZ)
{
    int* ctl = (int*)h->addWs.ctl.p;
    BHS_HIP(hipMemsetAsync(ctl, 0, sizeof(int) * AD_INTS, h->stream));
    int stat = 0;
    BHS_TRY(timed(h, "add_count", in.m, [&] {
        const long long gs = std::max<long long>(1, ((long long)in.m + kAddCountRows - 1) / kAddCountRows);
        hipLaunchKernelGGL(k_add_count, dim3((unsigned)gs), dim3(256), 0, h->stream, in.m, in.n, in.nnzX, in.Xp, in.Xj, in.nnzY,
                           in.Yp, in.Yj, (int*)h->addWs.cnt.p, ypos, ctl, (int*)h->addWs.queue.p);
        return 1;
    }, &stat));
    BHS_TRY(side_read_ctl(h, h->addWs, AD_INTS));
    if (h->addWs.host[AD_ERR]) return BHS_ERR_INVALID_ARG;
    unsigned long long total = 0;
    memcpy(&total, h->addWs.host + AD_TOTAL, 8);
    if (total > 0x7fffffffull) return BHS_ERR_NNZ_OVERFLOW;
    h->stats[stat].nnz_out += (int64_t)total;
    *nnzZ = (long long)total;
    return BHS_SUCCESS;
}

// the fill pass on the queues and bin counts in h->addWs.queue / h->addWs.host
int add_fill(bhs_handle* h, const AddIn& in, double alpha, double beta, const int* Zp, int* Zj, value_t* Zx)
{
    const int m = in.m;
    const int* queue = (const int*)h->addWs.queue.p;
    const int* count = h->addWs.host + AD_COUNT;
    if (count[kAddShort]) {
        const int nq = count[kAddShort];
        BHS_TRY(timed(h, "add_short", nq, [&] {
            hipLaunchKernelGGL((k_add_fill<16, kAddShortL, 256>), dim3((unsigned)((nq + 15) / 16)), dim3(256), 0, h->stream, nq,
                               queue + (size_t)kAddShort * m, alpha, in.Xp, in.Xj, in.Xx, beta, in.Yp, in.Yj, in.Yx, Zp, Zj, Zx);
            return 1;
        }));
    }
    if (count[kAddWave]) {
        const int nq = count[kAddWave];
        BHS_TRY(timed(h, "add_wave", nq, [&] {
            hipLaunchKernelGGL((k_add_fill<64, kAddWaveL, 256>), dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, h->stream, nq,
                               queue + (size_t)kAddWave * m, alpha, in.Xp, in.Xj, in.Xx, beta, in.Yp, in.Yj, in.Yx, Zp, Zj, Zx);
            return 1;
        }));
    }
    if (count[kAddLong]) {
        const int nq = count[kAddLong];
        BHS_TRY(timed(h, "add_long", nq, [&] {
            hipLaunchKernelGGL((k_add_fill<256, kAddChunk, 256>), dim3((unsigned)nq), dim3(256), 0, h->stream, nq,
                               queue + (size_t)kAddLong * m, alpha, in.Xp, in.Xj, in.Xx, beta, in.Yp, in.Yj, in.Yx, Zp, Zj, Zx);
            return 1;
        }));
    }
    return BHS_SUCCESS;
}

bool add_args_ok(int m, int n, int nnzX, const int* Xp, const int* Xj, int nnzY, const int* Yp, const int* Yj)
{
    return m >= 0 && n >= 0 && nnzX >= 0 && nnzY >= 0 && Xp && Yp && (nnzX == 0 || Xj) && (nnzY == 0 || Yj);
}

int add_symbolic_run(bhs_handle* h, const AddIn& in, int* d_rowPtrZ, int* nnzZ_out, int* inside_out)
{
    BHS_TRY(add_prepare(h, in.m));
    side_reset_stats(h);
    long long nnzZ = 0;
    BHS_TRY(add_count(h, in, nullptr, &nnzZ));
    BHS_TRY(side_scan(h, h->addWs, "add_scan", kAddScanWords, in.m, in.Xp, d_rowPtrZ));
    BHS_TRY(wait_stream(h));
    BHS_TRY(side_collect(h, 0));
    if (nnzZ_out) *nnzZ_out = (int)nnzZ;
    if (inside_out) *inside_out = h->addWs.host[AD_OUTSIDE] ? 0 : 1;
    return BHS_SUCCESS;
}

int add_numeric_run(bhs_handle* h, const AddIn& in, double alpha, double beta, const int* Zp, int* Zj, value_t* Zx, double* ms_out)
{
    BHS_TRY(add_prepare(h, in.m));
    side_reset_stats(h);
    int* ctl = (int*)h->addWs.ctl.p;
    BHS_TRY(side_begin(h, h->addWs));
    BHS_HIP(hipMemsetAsync(ctl, 0, sizeof(int) * AD_INTS, h->stream));
    BHS_TRY(timed(h, "add_bin", in.m, [&] {
        const long long gs = std::max<long long>(1, ((long long)in.m + 255) / 256);
        hipLaunchKernelGGL(k_add_bin, dim3((unsigned)gs), dim3(256), 0, h->stream, in.m, in.nnzX, in.Xp, in.nnzY, in.Yp, Zp, ctl,
                           (int*)h->addWs.queue.p);
        return 1;
    }));
    BHS_TRY(side_read_ctl(h, h->addWs, AD_INTS));
    if (h->addWs.host[AD_ERR]) return BHS_ERR_INVALID_ARG;
    BHS_TRY(add_fill(h, in, alpha, beta, Zp, Zj, Zx));
    BHS_TRY(side_end(h, h->addWs));
    BHS_TRY(wait_stream(h));
    BHS_TRY(side_elapsed(h, h->addWs, ms_out));
    return side_collect(h, 0);
}

// the add behind a finished multiply: X = the C of the pipeline, Y = D
int add_to_product(bhs_handle* h, double alpha, double beta, int nnzD, const value_t* dDx, const int* dDp, const int* dDj,
                   double* ms_out)
{
    const int m = h->m;
    const size_t evFirst = h->evUsed;                                // (the multiply's own events are read already)
    h->ls = h->stream;
    AddIn in;
    in.m = m; in.n = h->n;
    in.nnzX = (int)h->nnzC; in.Xp = (const int*)h->Cp.p; in.Xj = (const int*)h->Cj.p; in.Xx = (const value_t*)h->Cx.p;
    in.nnzY = nnzD; in.Yp = dDp; in.Yj = dDj; in.Yx = dDx;
    int* ypos = nullptr;
    if (h->addInplace && alpha == 1.0) {
        BHS_TRY(ensure(h, h->addPos, sizeof(int) * (size_t)std::max(nnzD, 1)));
        ypos = (int*)h->addPos.p;
    }
    BHS_TRY(side_begin(h, h->addWs));
    long long nnzZ = 0;
    BHS_TRY(add_count(h, in, ypos, &nnzZ));
    const bool inside = !h->addWs.host[AD_OUTSIDE];
    if (inside && h->addInplace) {
        if (nnzD > 0 || alpha != 1.0) {
            int stat = 0;
            BHS_TRY(timed(h, "add_inplace", m, [&] {
                if (alpha == 1.0) {
                    const long long gs = std::max<long long>(1, std::min<long long>(((long long)nnzD + 255) / 256, (long long)h->numCU * 16));
                    hipLaunchKernelGGL(k_add_inplace, dim3((unsigned)gs), dim3(256), 0, h->stream, nnzD, beta, dDx, (const int*)ypos,
                                       (value_t*)h->Cx.p);
                } else if (h->nnzC > 64LL * std::max(m, 1)) {
                    const long long gs = std::max<long long>(1, std::min<long long>(((long long)m + 3) / 4, (long long)h->numCU * 32));
                    hipLaunchKernelGGL(k_add_inplace_rows<64>, dim3((unsigned)gs), dim3(256), 0, h->stream, m, alpha, in.Xp, in.Xj,
                                       (value_t*)h->Cx.p, beta, dDp, dDj, dDx);
                } else {
                    const long long gs = std::max<long long>(1, std::min<long long>(((long long)m + 15) / 16, (long long)h->numCU * 32));
                    hipLaunchKernelGGL(k_add_inplace_rows<16>, dim3((unsigned)gs), dim3(256), 0, h->stream, m, alpha, in.Xp, in.Xj,
                                       (value_t*)h->Cx.p, beta, dDp, dDj, dDx);
                }
                return 1;
            }, &stat));
            h->stats[stat].nnz_out += alpha == 1.0 ? (int64_t)nnzD : (int64_t)h->nnzC;
        }
        h->addInplaceUsed = 1;
    } else {
        BHS_TRY(ensure(h, h->sumCp, sizeof(int) * ((size_t)m + 1)));
        BHS_TRY(ensure(h, h->sumCj, sizeof(int) * (size_t)std::max<long long>(nnzZ, 1)));
        BHS_TRY(ensure(h, h->sumCx, sizeof(value_t) * (size_t)std::max<long long>(nnzZ, 1)));
        BHS_TRY(side_scan(h, h->addWs, "add_scan", kAddScanWords, m, in.Xp, (int*)h->sumCp.p));
        BHS_TRY(add_fill(h, in, alpha, beta, (const int*)h->sumCp.p, (int*)h->sumCj.p, (value_t*)h->sumCx.p));
        h->addInplaceUsed = 0;
    }
    BHS_TRY(side_end(h, h->addWs));
    BHS_TRY(wait_stream(h));
    if (!h->addInplaceUsed) {                                        // from here on the getters serve the sum
        h->sumActive = true;
        h->sumNnz = nnzZ;
    }
    BHS_TRY(side_elapsed(h, h->addWs, ms_out));
    return side_collect(h, evFirst);
}

int spgemm_add_check(bhs_handle* h, int nnzD, const void* valD, const int* rowPtrD, const int* colIndD)
{
    if (!h) return BHS_ERR_INVALID_ARG;
    if (!h->hasData) return BHS_ERR_NOT_READY;
    if (h->ps.open || nnzD < 0 || h->extCj) return BHS_ERR_INVALID_ARG;   // (a split multiply owns the stream; bound output arrays cannot hold a sum of unknown size)
    if (!rowPtrD || (nnzD > 0 && (!colIndD || !valD))) return BHS_ERR_INVALID_ARG;
    return BHS_SUCCESS;
}

int spgemm_add_run(bhs_handle* h, double alpha, double beta, int nnzD, const value_t* dDx, const int* dDp, const int* dDj,
                   int* rowPtrC_out, int64_t* nnzCt_out, int* nnzC_out, double* ms_out)
{
    BHS_TRY(add_prepare(h, h->m));
    side_reset_stats(h);
    BHS_TRY(add_check(h, h->m, h->n, nnzD, dDp, dDj));               // an invalid D: nothing has been started, the last C stands
    double stage[4] = {0, 0, 0, 0};
    BHS_TRY(bhs_spgemm(h, rowPtrC_out, nnzCt_out, nullptr, stage));
    double addMs = 0;
    BHS_TRY(add_to_product(h, alpha, beta, nnzD, dDx, dDp, dDj, &addMs));
    if (rowPtrC_out && h->sumActive) {
        BHS_HIP(hipMemcpyAsync(rowPtrC_out, h->sumCp.p, sizeof(int) * ((size_t)h->m + 1), hipMemcpyDeviceToHost, h->stream));
        BHS_HIP(hipStreamSynchronize(h->stream));
    }
    if (nnzC_out) *nnzC_out = (int)(h->sumActive ? h->sumNnz : h->nnzC);
    if (ms_out) { ms_out[0] = stage[0] + stage[1] + stage[2] + stage[3]; ms_out[1] = addMs; }
    return BHS_SUCCESS;
}

}  // namespace

extern "C" {

int bhs_csr_add_symbolic_device(bhs_handle* h, int m, int n, int nnzX, const int* d_rowPtrX, const int* d_colIndX, int nnzY,
                                const int* d_rowPtrY, const int* d_colIndY, int* d_rowPtrZ, int* nnzZ_out, int* y_inside_x_out)
{
    if (!h || h->ps.open || !d_rowPtrZ || !add_args_ok(m, n, nnzX, d_rowPtrX, d_colIndX, nnzY, d_rowPtrY, d_colIndY))
        return BHS_ERR_INVALID_ARG;
    AddIn in;
    in.m = m; in.n = n;
    in.nnzX = nnzX; in.Xp = d_rowPtrX; in.Xj = d_colIndX; in.Xx = nullptr;
    in.nnzY = nnzY; in.Yp = d_rowPtrY; in.Yj = d_colIndY; in.Yx = nullptr;
    return guarded(h, [&] { return add_symbolic_run(h, in, d_rowPtrZ, nnzZ_out, y_inside_x_out); });
}

int bhs_csr_add_numeric_device(bhs_handle* h, int m, int n, double alpha, int nnzX, const bhs_value_t* d_valX, const int* d_rowPtrX,
                               const int* d_colIndX, double beta, int nnzY, const bhs_value_t* d_valY, const int* d_rowPtrY,
                               const int* d_colIndY, const int* d_rowPtrZ, int* d_colIndZ, bhs_value_t* d_valZ, double* ms_out)
{
    if (!h || h->ps.open || !d_rowPtrZ || !add_args_ok(m, n, nnzX, d_rowPtrX, d_colIndX, nnzY, d_rowPtrY, d_colIndY))
        return BHS_ERR_INVALID_ARG;
    if ((nnzX > 0 && !d_valX) || (nnzY > 0 && !d_valY) || ((nnzX > 0 || nnzY > 0) && (!d_colIndZ || !d_valZ))) return BHS_ERR_INVALID_ARG;
    AddIn in;
    in.m = m; in.n = n;
    in.nnzX = nnzX; in.Xp = d_rowPtrX; in.Xj = d_colIndX; in.Xx = (const value_t*)d_valX;
    in.nnzY = nnzY; in.Yp = d_rowPtrY; in.Yj = d_colIndY; in.Yx = (const value_t*)d_valY;
    return guarded(h, [&] { return add_numeric_run(h, in, alpha, beta, d_rowPtrZ, d_colIndZ, (value_t*)d_valZ, ms_out); });
}

int bhs_spgemm_add_device(bhs_handle* h, double alpha, double beta, int nnzD, const bhs_value_t* d_valD, const int* d_rowPtrD,
                          const int* d_colIndD, int* rowPtrC_out, int64_t* nnzCt_out, int* nnzC_out, double ms_out[2])
{
    BHS_TRY(spgemm_add_check(h, nnzD, d_valD, d_rowPtrD, d_colIndD));
    return guarded(h, [&] {
        return spgemm_add_run(h, alpha, beta, nnzD, (const value_t*)d_valD, d_rowPtrD, d_colIndD, rowPtrC_out, nnzCt_out, nnzC_out,
                              ms_out);
    });
}

int bhs_spgemm_add(bhs_handle* h, double alpha, double beta, int nnzD, const bhs_value_t* valD, const int* rowPtrD,
                   const int* colIndD, int* rowPtrC_out, int64_t* nnzCt_out, int* nnzC_out, double ms_out[2])
{
    BHS_TRY(spgemm_add_check(h, nnzD, valD, rowPtrD, colIndD));
    return guarded(h, [&]() -> int {
        BHS_TRY(ensure(h, h->addD[0], sizeof(int) * ((size_t)h->m + 1)));
        BHS_TRY(ensure(h, h->addD[1], sizeof(int) * (size_t)std::max(nnzD, 1)));
        BHS_TRY(ensure(h, h->addD[2], sizeof(value_t) * (size_t)std::max(nnzD, 1)));
        BHS_HIP(hipMemcpyAsync(h->addD[0].p, rowPtrD, sizeof(int) * ((size_t)h->m + 1), hipMemcpyHostToDevice, h->stream));
        if (nnzD) {
            BHS_HIP(hipMemcpyAsync(h->addD[1].p, colIndD, sizeof(int) * (size_t)nnzD, hipMemcpyHostToDevice, h->stream));
            BHS_HIP(hipMemcpyAsync(h->addD[2].p, valD, sizeof(value_t) * (size_t)nnzD, hipMemcpyHostToDevice, h->stream));
        }
        BHS_HIP(hipStreamSynchronize(h->stream));                    // (the caller's arrays are free again)
        return spgemm_add_run(h, alpha, beta, nnzD, (const value_t*)h->addD[2].p, (const int*)h->addD[0].p, (const int*)h->addD[1].p,
                              rowPtrC_out, nnzCt_out, nnzC_out, ms_out);
    });
}

}  // extern "C"
