// bhs_host_reduce.inc.h -- reductions and the diagonal scaling (bhs_csr_reduce_device, bhs_csr_scale_device; kernels in
// bhs_reduce.hip.h)
// (A part of bhsparse_hip.hip's translation unit: included there after the transpose.)
//
// Like the add, the selection, the transpose and the extraction both calls work beside the pipeline: their workspace (h->rdWs:
// counters, queues, events, the pinned mirror; set up and read by bhs_host_side.inc.h), the accumulators and the partials
// are buffers of their own from the grow-only pool.  They bind nothing and serve nothing through the getters: every output
// array is the caller's.
//
// The kernels' header is included here, not among the translation unit's kernel headers (as bhs_host_extract.inc.h does).
#include "bhs_reduce.hip.h"

namespace {

struct RdIn {
    int m, n, nnzX;
    const int* Xp; const int* Xj; const value_t* Xx;
};

// (no counts: nothing is scanned)
int rd_prepare(bhs_handle* h, int m)
{
    BHS_TRY(side_prepare(h, h->rdWs, RD_INTS, sizeof(int) * 2 * (size_t)std::max(m, 1), 0));
    BHS_HIP(hipMemsetAsync(h->rdWs.ctl.p, 0, sizeof(int) * RD_INTS, h->stream));
    return BHS_SUCCESS;
}

unsigned rd_grid(long long items, int per) { return (unsigned)std::max<long long>(1, (items + per - 1) / per); }

// The rows' results into acc (m words, or nRead for the diagonal): k_red_short on every row, one round trip for the
// queues' lengths, the wave and the long kernel where rows wait for them.  Returns BHS_ERR_INVALID_ARG where the short
// kernel has already refused the input.
template <int KIND>
int rd_rows(bhs_handle* h, const RdIn& in, int op, int filt, int nRead, rd_u64 id, rd_u64* acc)
{
    int* ctl = (int*)h->rdWs.ctl.p;
    int* queue = (int*)h->rdWs.queue.p;
    const int m = in.m;
    if (!in.Xx && op == kRdOpPlus && filt == kRdAll) {               // COUNT: the row pointer alone
        return timed(h, "reduce_short", m, [&] {
            hipLaunchKernelGGL(k_red_rowlen, dim3(rd_grid(m, 256)), dim3(256), 0, h->stream, m, in.nnzX, in.Xp, acc, ctl);
            return 1;
        });
    }
    BHS_TRY(timed(h, "reduce_short", m, [&] {
        hipLaunchKernelGGL(k_red_short<KIND>, dim3(rd_grid(m, kRdRows)), dim3(256), 0, h->stream, m, in.n, in.nnzX, in.Xp, in.Xj,
                           in.Xx, op, filt, nRead, id, acc, ctl, queue);
        return 1;
    }));
    if (in.nnzX <= kRdShortL) return BHS_SUCCESS;                    // (no row can be longer)
    BHS_TRY(side_read_ctl(h, h->rdWs, RD_INTS));
    if (h->rdWs.host[RD_ERR]) return BHS_ERR_INVALID_ARG;
    if (const int nq = h->rdWs.host[RD_CNT_WAVE]) {
        BHS_TRY(timed(h, "reduce_wave", nq, [&] {
            hipLaunchKernelGGL(k_red_wave<KIND>, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, h->stream, nq,
                               queue + (size_t)RD_CNT_WAVE * m, m, in.n, in.nnzX, in.Xp, in.Xj, in.Xx, op, filt, id, acc, ctl);
            return 1;
        }));
    }
    if (const int nq = h->rdWs.host[RD_CNT_LONG]) {
        BHS_TRY(timed(h, "reduce_long", nq, [&] {
            hipLaunchKernelGGL(k_red_long<KIND>, dim3((unsigned)std::min<long long>(nq, (long long)h->numCU * 8)), dim3(256), 0,
                               h->stream, nq, queue + (size_t)RD_CNT_LONG * m, m, in.n, in.nnzX, in.Xp, in.Xj, in.Xx, op, filt, id,
                               acc, ctl);
            return 1;
        }));
    }
    return BHS_SUCCESS;
}

// the partials of `count` items (values of X, or the accumulators `raw`) into h->rdPart; *nPart their number
template <int KIND, bool RAW>
int rd_all(bhs_handle* h, const RdIn& in, const rd_u64* raw, long long count, int op, rd_u64 id, int* nPart)
{
    const unsigned g = (unsigned)std::min<long long>(kRdAllMax, std::max<long long>(1, (count + kRdAllPer - 1) / kRdAllPer));
    BHS_TRY(ensure(h, h->rdPart, sizeof(rd_u64) * kRdAllMax));
    *nPart = (int)g;
    return timed(h, "reduce_all", in.m, [&] {
        hipLaunchKernelGGL((k_red_all<KIND, RAW>), dim3(g), dim3(256), 0, h->stream, in.m, in.nnzX, in.Xp, in.Xx, raw, count, op, id,
                           (rd_u64*)h->rdPart.p, (int*)h->rdWs.ctl.p);
        return 1;
    });
}

template <int KIND>
int rd_run(bhs_handle* h, const RdIn& in, int axis, int op, int filt, value_t* out, double* ms_out)
{
    BHS_TRY(rd_prepare(h, in.m));
    side_reset_stats(h);
    BHS_TRY(side_begin(h, h->rdWs));
    int* ctl = (int*)h->rdWs.ctl.p;
    const rd_u64 id = rd_identity(KIND, op);
    const int nDiag = std::min(in.m, in.n);
    const int nOut = axis == BHS_AXIS_ROWS ? in.m : axis == BHS_AXIS_COLS ? in.n : axis == BHS_AXIS_DIAG ? nDiag : 1;
    const size_t words = axis == BHS_AXIS_COLS ? (size_t)in.n : (size_t)in.m;
    BHS_TRY(ensure(h, h->rdAcc, sizeof(rd_u64) * std::max<size_t>(words, 1)));
    rd_u64* acc = (rd_u64*)h->rdAcc.p;
    const rd_u64* result = acc;
    int nPart = 0, rc = BHS_SUCCESS;
    if (axis == BHS_AXIS_ROWS || axis == BHS_AXIS_DIAG) {
        rc = rd_rows<KIND>(h, in, op, filt, axis == BHS_AXIS_DIAG ? nDiag : in.m, id, acc);
    } else if (axis == BHS_AXIS_COLS) {
        BHS_TRY(timed(h, "reduce_cols", in.n, [&] {
            hipLaunchKernelGGL(k_red_fill, dim3(rd_grid(in.n, 256)), dim3(256), 0, h->stream, (long long)in.n, id, acc);
            hipLaunchKernelGGL(k_red_cols<KIND>, dim3(rd_grid(in.nnzX, 256 * kRdColE)), dim3(256), 0, h->stream, in.m, in.n, in.nnzX,
                               in.Xp, in.Xj, in.Xx, op, filt, id, acc, ctl);
            return 2;
        }));
    } else if (filt == kRdAll) {
        BHS_TRY((rd_all<KIND, false>(h, in, nullptr, in.nnzX, op, id, &nPart)));
        result = (const rd_u64*)h->rdPart.p;
    } else {                                                         // the off-diagonal total: the rows' results, then their total
        rc = rd_rows<KIND>(h, in, op, filt, in.m, id, acc);
        if (rc == BHS_SUCCESS) BHS_TRY((rd_all<KIND, true>(h, in, acc, in.m, op, id, &nPart)));
        result = (const rd_u64*)h->rdPart.p;
    }
    if (rc != BHS_SUCCESS) return rc;
    BHS_TRY(timed(h, "reduce_finish", nOut, [&] {
        hipLaunchKernelGGL(k_red_finish<KIND>, dim3(nPart ? 1u : rd_grid(nOut, 256)), dim3(256), 0, h->stream, nOut, result, nPart, id,
                           out, ctl);
        return 1;
    }));
    BHS_TRY(side_end(h, h->rdWs));
    BHS_TRY(side_read_ctl(h, h->rdWs, RD_INTS));
    BHS_TRY(side_close(h, h->rdWs, ms_out));
    return h->rdWs.host[RD_ERR] ? (int)BHS_ERR_INVALID_ARG : (int)BHS_SUCCESS;
}

int sc_run(bhs_handle* h, const ScArgs& s, double* ms_out)
{
    BHS_TRY(rd_prepare(h, s.m));
    side_reset_stats(h);
    BHS_TRY(side_begin(h, h->rdWs));
    int* ctl = (int*)h->rdWs.ctl.p;
    int* queue = (int*)h->rdWs.queue.p;
    const unsigned gCheck = (unsigned)std::min<long long>(rd_grid(s.m, 256), (long long)h->numCU * 8);
    if (!s.left) {
        BHS_TRY(timed(h, "scale", s.m, [&] {
            hipLaunchKernelGGL(k_sc_check, dim3(gCheck), dim3(256), 0, h->stream, s.m, s.nnzX, s.Xp, ctl);
            hipLaunchKernelGGL(k_sc_flat, dim3(rd_grid(s.nnzX, 256 * kScFlatE)), dim3(256), 0, h->stream, s, ctl);
            return 2;
        }));
    } else {
        BHS_TRY(timed(h, "scale_short", s.m, [&] {
            hipLaunchKernelGGL(k_sc_check, dim3(gCheck), dim3(256), 0, h->stream, s.m, s.nnzX, s.Xp, ctl);
            hipLaunchKernelGGL(k_sc_short, dim3(rd_grid(s.m, kRdRows)), dim3(256), 0, h->stream, s, ctl, queue);
            return 2;
        }));
        if (s.nnzX > kRdShortL) {                                    // (else no row can be longer)
            BHS_TRY(side_read_ctl(h, h->rdWs, RD_INTS));
            if (h->rdWs.host[RD_ERR]) return BHS_ERR_INVALID_ARG;
            if (const int nq = h->rdWs.host[RD_CNT_WAVE]) {
                BHS_TRY(timed(h, "scale_wave", nq, [&] {
                    hipLaunchKernelGGL(k_sc_wave, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, h->stream, nq,
                                       queue + (size_t)RD_CNT_WAVE * s.m, s, ctl);
                    return 1;
                }));
            }
            if (const int nq = h->rdWs.host[RD_CNT_LONG]) {
                BHS_TRY(timed(h, "scale_long", nq, [&] {
                    hipLaunchKernelGGL(k_sc_long, dim3((unsigned)std::min<long long>(nq, (long long)h->numCU * 8)), dim3(256), 0,
                                       h->stream, nq, queue + (size_t)RD_CNT_LONG * s.m, s, ctl);
                    return 1;
                }));
            }
        }
    }
    BHS_TRY(side_end(h, h->rdWs));
    BHS_TRY(side_read_ctl(h, h->rdWs, RD_INTS));
    BHS_TRY(side_close(h, h->rdWs, ms_out));
    return h->rdWs.host[RD_ERR] ? (int)BHS_ERR_INVALID_ARG : (int)BHS_SUCCESS;
}

}  // namespace

extern "C" {

int bhs_csr_reduce_device(bhs_handle* h, int m, int n, int nnzX, const bhs_value_t* d_valX, const int* d_rowPtrX,
                          const int* d_colIndX, int axis, int op, int flags, bhs_value_t* d_out, double* ms_out)
{
    if (!h || h->ps.open || m < 0 || n < 0 || nnzX < 0 || !d_rowPtrX) return BHS_ERR_INVALID_ARG;
    if (axis < BHS_AXIS_ROWS || axis > BHS_AXIS_DIAG || op < BHS_RED_PLUS || op > BHS_RED_COUNT) return BHS_ERR_INVALID_ARG;
    if ((flags & ~BHS_RED_OFFDIAG) || (flags && axis == BHS_AXIS_DIAG)) return BHS_ERR_INVALID_ARG;
    const int filt = axis == BHS_AXIS_DIAG ? kRdDiag : flags ? kRdOffdiag : kRdAll;
    const bool readsCols = axis == BHS_AXIS_COLS || filt != kRdAll;
    if (readsCols && nnzX > 0 && !d_colIndX) return BHS_ERR_INVALID_ARG;
    const size_t nOut = axis == BHS_AXIS_ROWS ? (size_t)m : axis == BHS_AXIS_COLS ? (size_t)n
                      : axis == BHS_AXIS_DIAG ? (size_t)std::min(m, n) : 1;
    if (nOut && !d_out) return BHS_ERR_INVALID_ARG;
    const size_t outBytes = sizeof(value_t) * nOut;
    if (side_aliased({{d_out, outBytes}}, {{d_rowPtrX, sizeof(int) * ((size_t)m + 1)}, {d_colIndX, sizeof(int) * (size_t)nnzX},
                                           {d_valX, sizeof(value_t) * (size_t)nnzX}}))
        return BHS_ERR_INVALID_ARG;
    RdIn in;
    in.m = m; in.n = n; in.nnzX = nnzX; in.Xp = d_rowPtrX; in.Xj = d_colIndX; in.Xx = (const value_t*)d_valX;
    if (op == BHS_RED_COUNT) { in.Xx = nullptr; op = BHS_RED_PLUS; } // (a sum of ones: no value is read)
    return guarded(h, [&] {
        if (op == BHS_RED_MIN) return rd_run<kRdMin>(h, in, axis, op, filt, (value_t*)d_out, ms_out);
        if (op == BHS_RED_MAX || op == BHS_RED_ABS_MAX) return rd_run<kRdMax>(h, in, axis, op, filt, (value_t*)d_out, ms_out);
        return rd_run<kRdSum>(h, in, axis, op, filt, (value_t*)d_out, ms_out);
    });
}

int bhs_csr_scale_device(bhs_handle* h, int m, int n, int nnzX, const bhs_value_t* d_valX, const int* d_rowPtrX,
                         const int* d_colIndX, double alpha, const bhs_value_t* d_left, const bhs_value_t* d_right, int flags,
                         bhs_value_t* d_valZ, double* ms_out)
{
    if (!h || h->ps.open || m < 0 || n < 0 || nnzX < 0 || !d_rowPtrX) return BHS_ERR_INVALID_ARG;
    if (flags & ~(BHS_SCALE_LEFT_DIV | BHS_SCALE_RIGHT_DIV)) return BHS_ERR_INVALID_ARG;
    if (((flags & BHS_SCALE_LEFT_DIV) && !d_left) || ((flags & BHS_SCALE_RIGHT_DIV) && !d_right)) return BHS_ERR_INVALID_ARG;
    if (nnzX > 0 && (!d_valX || !d_valZ || (d_right && !d_colIndX))) return BHS_ERR_INVALID_ARG;
    const size_t zBytes = sizeof(value_t) * (size_t)nnzX;
    const void* valX = (const void*)d_valZ == (const void*)d_valX ? nullptr : d_valX;   // (in place on valX exactly, or apart from every input)
    if (side_aliased({{d_valZ, zBytes}}, {{d_rowPtrX, sizeof(int) * ((size_t)m + 1)}, {d_colIndX, sizeof(int) * (size_t)nnzX},
                                          {d_left, sizeof(value_t) * (size_t)m}, {d_right, sizeof(value_t) * (size_t)n}, {valX, zBytes}}))
        return BHS_ERR_INVALID_ARG;
    ScArgs s;
    s.m = m; s.n = n; s.nnzX = nnzX; s.Xp = d_rowPtrX; s.Xj = d_colIndX; s.Xx = (const value_t*)d_valX;
    s.left = (const value_t*)d_left; s.right = (const value_t*)d_right; s.alpha = alpha;
    s.leftDiv = (flags & BHS_SCALE_LEFT_DIV) ? 1 : 0; s.rightDiv = (flags & BHS_SCALE_RIGHT_DIV) ? 1 : 0;
    s.Zx = (value_t*)d_valZ;
    return guarded(h, [&] { return sc_run(h, s, ms_out); });
}

}  // extern "C"
