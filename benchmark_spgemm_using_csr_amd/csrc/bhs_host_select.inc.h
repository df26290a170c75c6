// bhs_host_select.inc.h -- the entry selection (bhs_csr_select_{symbolic,numeric}_device, bhs_spgemm_select[_device]; kernels in
// bhs_select.hip.h)
// (A part of bhsparse_hip.hip's translation unit: included there after the sparse add.)
//
// Like the masked multiply and the add the selection works beside the pipeline: its workspace (h->selWs: counters, queues,
// counts, tile words, events, the pinned mirror; set up, read and scanned by bhs_host_side.inc.h) is its own.
// bhs_spgemm_select runs the ordinary multiply and then selects from its C; where entries were dropped the selected C goes
// to the second set of arrays bhs_spgemm_add uses (h->sumActive, served by the getters until the next multiply); the
// pipeline's own C arrays are never moved.

namespace {

struct SelIn {
    int m, n, nnzX;
    const int* Xp; const int* Xj; const value_t* Xx;
};

// the rule as the caller states it -> as the kernels take it; false: an invalid rule
bool sel_spec_from(const bhs_select* s, SelSpec* out)
{
    if (!s) return false;
    const unsigned known = BHS_SEL_BAND | BHS_SEL_DROP_DIAG | BHS_SEL_KEEP_DIAG | BHS_SEL_ABS | BHS_SEL_REL | BHS_SEL_TOPK;
    if (s->flags & ~known) return false;
    if ((s->flags & BHS_SEL_DROP_DIAG) && (s->flags & BHS_SEL_KEEP_DIAG)) return false;
    if (s->top_k < 0 || s->band_lo > s->band_hi) return false;
    if (!(s->abs_tol >= 0.0) || !(s->rel_tol >= 0.0) || s->abs_tol > 1.79769313486231570815e308 || s->rel_tol > 1.79769313486231570815e308)
        return false;                                                // (negative, NaN, Inf)
    out->flags = s->flags;
    out->topK = s->top_k;
    out->lo = s->band_lo;
    out->hi = s->band_hi;
    out->absTol = s->abs_tol;
    out->relTol = s->rel_tol;
    return true;
}

int sel_prepare(bhs_handle* h, int m)
{
    return side_prepare(h, h->selWs, SL_INTS, sizeof(int) * (size_t)kSelBins * (size_t)std::max(m, 1), (size_t)m + 1);
}

constexpr SideScanWords kSelScanWords = {SL_TICKET, SL_SCANTOTAL, SL_SCANBINS, SL_MAXCNT};

// The count pass and its round trip.  Afterwards h->selWs.cnt holds the rows' counts, h->selWs.queue the bins' rows, h->selWs.host
// the control words; *nnzZ the number of survivors.
int sel_count(bhs_handle* h, const SelIn& in, const SelSpec& spec, long long* nnzZ)
{
    int* ctl = (int*)h->selWs.ctl.p;
    BHS_HIP(hipMemsetAsync(ctl, 0, sizeof(int) * SL_INTS, h->stream));
    int stat = 0;
    BHS_TRY(timed(h, "select_count", in.m, [&] {
        const long long gs = std::max<long long>(1, ((long long)in.m + kSelCountRows - 1) / kSelCountRows);
        hipLaunchKernelGGL(k_sel_count, dim3((unsigned)gs), dim3(256), 0, h->stream, in.m, in.n, in.nnzX, in.Xp, in.Xj, in.Xx, spec,
                           (int*)h->selWs.cnt.p, ctl, (int*)h->selWs.queue.p);
        if (in.nnzX <= kSelWaveL) return 1;                          // (no row can be long)
        const long long gl = std::max<long long>(1, std::min<long long>(in.m, (long long)h->numCU * 8));
        hipLaunchKernelGGL(k_sel_count_long, dim3((unsigned)gl), dim3(256), 0, h->stream, in.m, in.n, in.Xp, in.Xj, in.Xx, spec,
                           (int*)h->selWs.cnt.p, ctl, (const int*)h->selWs.queue.p);
        return 2;
    }, &stat));
    BHS_TRY(side_read_ctl(h, h->selWs, SL_INTS));
    if (h->selWs.host[SL_ERR]) return BHS_ERR_INVALID_ARG;
    unsigned long long total = 0;
    memcpy(&total, h->selWs.host + SL_TOTAL, 8);
    h->stats[stat].nnz_out += (int64_t)total;
    *nnzZ = (long long)total;                                        // (at most nnz(X): no overflow of its own)
    return BHS_SUCCESS;
}

template <bool TOPK>
int sel_fill_bins(bhs_handle* h, const SelIn& in, const SelSpec& spec, const int* Zp, int* Zj, value_t* Zx)
{
    const int m = in.m;
    const int* queue = (const int*)h->selWs.queue.p;
    const int* count = h->selWs.host + SL_COUNT;
    int* ctl = (int*)h->selWs.ctl.p;
    if (count[kSelShort]) {
        const int nq = count[kSelShort];
        BHS_TRY(timed(h, "select_short", nq, [&] {
            hipLaunchKernelGGL((k_sel_fill<16, TOPK, 256>), dim3((unsigned)((nq + 15) / 16)), dim3(256), 0, h->stream, nq,
                               queue + (size_t)kSelShort * m, spec, in.Xp, in.Xj, in.Xx, Zp, Zj, Zx, ctl);
            return 1;
        }));
    }
    if (count[kSelWave]) {
        const int nq = count[kSelWave];
        BHS_TRY(timed(h, "select_wave", nq, [&] {
            if constexpr (TOPK)
                hipLaunchKernelGGL((k_sel_fill<64, TOPK, 64>), dim3((unsigned)nq), dim3(64), 0, h->stream, nq,
                                   queue + (size_t)kSelWave * m, spec, in.Xp, in.Xj, in.Xx, Zp, Zj, Zx, ctl);
            else
                hipLaunchKernelGGL((k_sel_fill<64, false, 256>), dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, h->stream, nq,
                                   queue + (size_t)kSelWave * m, spec, in.Xp, in.Xj, in.Xx, Zp, Zj, Zx, ctl);
            return 1;
        }));
    }
    if (count[kSelLong]) {
        const int nq = count[kSelLong];
        BHS_TRY(timed(h, "select_long", nq, [&] {
            hipLaunchKernelGGL((k_sel_fill<256, TOPK, 256>), dim3((unsigned)nq), dim3(256), 0, h->stream, nq,
                               queue + (size_t)kSelLong * m, spec, in.Xp, in.Xj, in.Xx, Zp, Zj, Zx, ctl);
            return 1;
        }));
    }
    return BHS_SUCCESS;
}

// the fill pass on the queues and bin counts in h->selWs.queue / h->selWs.host
int sel_fill(bhs_handle* h, const SelIn& in, const SelSpec& spec, const int* Zp, int* Zj, value_t* Zx)
{
    return (spec.flags & SEL_TOPK) ? sel_fill_bins<true>(h, in, spec, Zp, Zj, Zx) : sel_fill_bins<false>(h, in, spec, Zp, Zj, Zx);
}

bool sel_args_ok(int m, int n, int nnzX, const value_t* Xx, const int* Xp, const int* Xj, const SelSpec& spec)
{
    return m >= 0 && n >= 0 && nnzX >= 0 && Xp && (nnzX == 0 || Xj) && (nnzX == 0 || Xx || !(spec.flags & SEL_VALUE));
}

int sel_symbolic_run(bhs_handle* h, const SelIn& in, const SelSpec& spec, int* d_rowPtrZ, int* nnzZ_out)
{
    BHS_TRY(sel_prepare(h, in.m));
    side_reset_stats(h);
    long long nnzZ = 0;
    BHS_TRY(sel_count(h, in, spec, &nnzZ));
    BHS_TRY(side_scan(h, h->selWs, "select_scan", kSelScanWords, in.m, in.Xp, d_rowPtrZ));
    BHS_TRY(wait_stream(h));
    BHS_TRY(side_collect(h, 0));
    if (nnzZ_out) *nnzZ_out = (int)nnzZ;
    return BHS_SUCCESS;
}

int sel_numeric_run(bhs_handle* h, const SelIn& in, const SelSpec& spec, const int* Zp, int* Zj, value_t* Zx, double* ms_out)
{
    BHS_TRY(sel_prepare(h, in.m));
    side_reset_stats(h);
    int* ctl = (int*)h->selWs.ctl.p;
    BHS_TRY(side_begin(h, h->selWs));
    BHS_HIP(hipMemsetAsync(ctl, 0, sizeof(int) * SL_INTS, h->stream));
    BHS_TRY(timed(h, "select_count", in.m, [&] {
        const long long gs = std::max<long long>(1, ((long long)in.m + 255) / 256);
        hipLaunchKernelGGL(k_sel_bin, dim3((unsigned)gs), dim3(256), 0, h->stream, in.m, in.nnzX, in.Xp, Zp, ctl, (int*)h->selWs.queue.p);
        return 1;
    }));
    BHS_TRY(side_read_ctl(h, h->selWs, SL_INTS));
    if (h->selWs.host[SL_ERR]) return BHS_ERR_INVALID_ARG;
    BHS_TRY(sel_fill(h, in, spec, Zp, Zj, Zx));
    BHS_TRY(side_end(h, h->selWs));
    BHS_HIP(hipMemcpyAsync(h->selWs.host, ctl, sizeof(int) * SL_INTS, hipMemcpyDeviceToHost, h->stream));   // (a row that no longer matches rowPtrZ)
    BHS_TRY(wait_stream(h));
    BHS_TRY(side_elapsed(h, h->selWs, ms_out));
    BHS_TRY(side_collect(h, 0));
    return h->selWs.host[SL_ERR] ? (int)BHS_ERR_INVALID_ARG : (int)BHS_SUCCESS;
}

// the selection behind a finished multiply: X = the C of the pipeline
int sel_from_product(bhs_handle* h, const SelSpec& spec, double* ms_out)
{
    const int m = h->m;
    const size_t evFirst = h->evUsed;                                // (the multiply's own events are read already)
    h->ls = h->stream;
    SelIn in;
    in.m = m; in.n = h->n; in.nnzX = (int)h->nnzC;
    in.Xp = (const int*)h->Cp.p; in.Xj = (const int*)h->Cj.p; in.Xx = (const value_t*)h->Cx.p;
    BHS_TRY(side_begin(h, h->selWs));
    long long nnzZ = 0;
    BHS_TRY(sel_count(h, in, spec, &nnzZ));
    h->selDropped = h->nnzC - nnzZ;
    if (h->selDropped) {
        BHS_TRY(ensure(h, h->sumCp, sizeof(int) * ((size_t)m + 1)));
        BHS_TRY(ensure(h, h->sumCj, sizeof(int) * (size_t)std::max<long long>(nnzZ, 1)));
        BHS_TRY(ensure(h, h->sumCx, sizeof(value_t) * (size_t)std::max<long long>(nnzZ, 1)));
        BHS_TRY(side_scan(h, h->selWs, "select_scan", kSelScanWords, m, in.Xp, (int*)h->sumCp.p));
        BHS_TRY(sel_fill(h, in, spec, (const int*)h->sumCp.p, (int*)h->sumCj.p, (value_t*)h->sumCx.p));
    }
    BHS_TRY(side_end(h, h->selWs));
    BHS_TRY(wait_stream(h));
    if (h->selDropped) {                                             // from here on the getters serve the selection
        h->sumActive = true;
        h->sumNnz = nnzZ;
    }
    BHS_TRY(side_elapsed(h, h->selWs, ms_out));
    return side_collect(h, evFirst);
}

int spgemm_select_check(bhs_handle* h, const bhs_select* sel, SelSpec* spec)
{
    if (!h || !sel_spec_from(sel, spec)) return BHS_ERR_INVALID_ARG;
    if (!h->hasData) return BHS_ERR_NOT_READY;
    if (h->ps.open || h->extCj) return BHS_ERR_INVALID_ARG;         // (a split multiply owns the stream; bound output arrays are the caller's: the selection reads the library's)
    return BHS_SUCCESS;
}

int spgemm_select_run(bhs_handle* h, const SelSpec& spec, int* rowPtrC_out, bool rowPtrOnDevice, int64_t* nnzCt_out, int* nnzC_out,
                      double* ms_out)
{
    BHS_TRY(sel_prepare(h, h->m));
    double stage[4] = {0, 0, 0, 0};
    BHS_TRY(bhs_spgemm(h, rowPtrOnDevice ? nullptr : rowPtrC_out, nnzCt_out, nullptr, stage));
    double selMs = 0;
    BHS_TRY(sel_from_product(h, spec, &selMs));
    if (rowPtrC_out && (h->sumActive || rowPtrOnDevice)) {
        BHS_HIP(hipMemcpyAsync(rowPtrC_out, h->sumActive ? h->sumCp.p : h->Cp.p, sizeof(int) * ((size_t)h->m + 1),
                               rowPtrOnDevice ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
        BHS_HIP(hipStreamSynchronize(h->stream));
    }
    if (nnzC_out) *nnzC_out = (int)(h->sumActive ? h->sumNnz : h->nnzC);
    if (ms_out) { ms_out[0] = stage[0] + stage[1] + stage[2] + stage[3]; ms_out[1] = selMs; }
    return BHS_SUCCESS;
}

}  // namespace

extern "C" {

int bhs_csr_select_symbolic_device(bhs_handle* h, int m, int n, int nnzX, const bhs_value_t* d_valX, const int* d_rowPtrX,
                                   const int* d_colIndX, const bhs_select* sel, int* d_rowPtrZ, int* nnzZ_out)
{
    SelSpec spec;
    if (!h || h->ps.open || !d_rowPtrZ || !sel_spec_from(sel, &spec) ||
        !sel_args_ok(m, n, nnzX, (const value_t*)d_valX, d_rowPtrX, d_colIndX, spec))
        return BHS_ERR_INVALID_ARG;
    SelIn in;
    in.m = m; in.n = n; in.nnzX = nnzX; in.Xp = d_rowPtrX; in.Xj = d_colIndX; in.Xx = (const value_t*)d_valX;
    return guarded(h, [&] { return sel_symbolic_run(h, in, spec, d_rowPtrZ, nnzZ_out); });
}

int bhs_csr_select_numeric_device(bhs_handle* h, int m, int n, int nnzX, const bhs_value_t* d_valX, const int* d_rowPtrX,
                                  const int* d_colIndX, const bhs_select* sel, const int* d_rowPtrZ, int* d_colIndZ,
                                  bhs_value_t* d_valZ, double* ms_out)
{
    SelSpec spec;
    if (!h || h->ps.open || !d_rowPtrZ || !sel_spec_from(sel, &spec) ||
        !sel_args_ok(m, n, nnzX, (const value_t*)d_valX, d_rowPtrX, d_colIndX, spec))
        return BHS_ERR_INVALID_ARG;
    if (nnzX > 0 && (!d_colIndZ || (d_valZ && !d_valX))) return BHS_ERR_INVALID_ARG;
    if (nnzX > 0 && (d_colIndZ == d_colIndX || (d_valZ && d_valZ == d_valX))) return BHS_ERR_INVALID_ARG;   // (Z must not overlap X)
    SelIn in;
    in.m = m; in.n = n; in.nnzX = nnzX; in.Xp = d_rowPtrX; in.Xj = d_colIndX; in.Xx = (const value_t*)d_valX;
    return guarded(h, [&] { return sel_numeric_run(h, in, spec, d_rowPtrZ, d_colIndZ, (value_t*)d_valZ, ms_out); });
}

int bhs_spgemm_select_device(bhs_handle* h, const bhs_select* sel, int* d_rowPtrC_out, int64_t* nnzCt_out, int* nnzC_out,
                             double ms_out[2])
{
    SelSpec spec;
    BHS_TRY(spgemm_select_check(h, sel, &spec));
    return guarded(h, [&] { return spgemm_select_run(h, spec, d_rowPtrC_out, true, nnzCt_out, nnzC_out, ms_out); });
}

int bhs_spgemm_select(bhs_handle* h, const bhs_select* sel, int* rowPtrC_out, int64_t* nnzCt_out, int* nnzC_out, double ms_out[2])
{
    SelSpec spec;
    BHS_TRY(spgemm_select_check(h, sel, &spec));
    return guarded(h, [&] { return spgemm_select_run(h, spec, rowPtrC_out, false, nnzCt_out, nnzC_out, ms_out); });
}

}  // extern "C"
