// bhs_host_relax.inc.h -- relaxation sweeps and the product with its reductions (bhs_csr_relax_device,
// bhs_chebyshev_coefficients, bhs_csr_spmv_dots_device; kernels in bhs_relax.hip.h)
// (A part of bhsparse_hip.hip's translation unit: included there after bhs_host_spmv.inc.h, whose MvIn, mv_kernels and
// mv_bytes the fused product uses.)
//
// Like CSR x dense both device calls work beside the pipeline, each on a workspace of its own from the grow-only pool:
// h->rxWs holds the relaxation's counters, the queues of the rows beyond the short bin and, behind them, three vectors of
// n values (the two x of the ping-pong and the d of the steps that may not write the caller's yet); h->dotWs the fused
// product's counters with the two results behind them, its queues and the workgroups' partials.  They bind nothing and
// serve nothing through the getters.
#include "bhs_relax.hip.h"

namespace {

struct RxIn {
    int n, nnzA, steps;
    const int* Ap; const int* Aj; const value_t* Ax;
    const value_t* diag; const value_t* b;
    value_t* x; value_t* d;
    const double* coef;
    bool zero;
};

size_t rx_pad(size_t bytes) { return (bytes + 15) / 16 * 16; }

int rx_run(bhs_handle* h, const RxIn& in, double* ms_out)
{
    SideWs& ws = h->rxWs;
    const int n = in.n;
    const size_t qBytes = rx_pad(sizeof(int) * 2 * (size_t)std::max(n, 1));
    const size_t vBytes = rx_pad(sizeof(value_t) * (size_t)std::max(n, 1));
    BHS_TRY(side_open(h, ws, RD_INTS, qBytes + 3 * vBytes, 0));
    BHS_TRY(side_start(h, ws));
    int* ctl = (int*)ws.ctl.p;
    int* queue = (int*)ws.queue.p;
    value_t* pool[2] = {(value_t*)((char*)ws.queue.p + qBytes), (value_t*)((char*)ws.queue.p + qBytes + vBytes)};
    value_t* dPool = (value_t*)((char*)ws.queue.p + qBytes + 2 * vBytes);
    const unsigned gRows = (unsigned)std::max<long long>(1, ((long long)n + kRdRows - 1) / kRdRows);
    const int firstPass = in.zero ? 1 : 0;                           // the step whose product pass reads every column first
    const value_t* xsrc = in.zero ? nullptr : in.x;
    const value_t* dsrc = in.d;
    int nqWave = 0, nqLong = 0;
    for (int s = 0; s < in.steps; ++s) {
        const bool scratch = s <= firstPass;                         // (nothing of the caller's before the validation is through)
        RxArgs g;
        g.n = n; g.nnzA = in.nnzA; g.Ap = in.Ap; g.Aj = in.Aj; g.Ax = in.Ax; g.diag = in.diag; g.b = in.b;
        g.a = in.coef[2 * s]; g.c = in.coef[2 * s + 1];
        g.xin = xsrc;
        g.xout = (!scratch && s == in.steps - 1) ? in.x : pool[s & 1];
        g.din = dsrc;
        g.dout = in.d ? (scratch ? dPool : in.d) : nullptr;
        const bool product = !(s == 0 && in.zero);
        if (!product) {
            BHS_TRY(timed(h, "relax_zero", n, [&] {
                hipLaunchKernelGGL(k_rx_zero, dim3(gRows), dim3(256), 0, h->stream, g, ctl, queue);
                return 1;
            }));
        } else {
            BHS_TRY(timed(h, "relax_short", n, [&] {
                if (s == 0) hipLaunchKernelGGL(k_rx_short<true>, dim3(gRows), dim3(256), 0, h->stream, g, ctl, queue);
                else hipLaunchKernelGGL(k_rx_short<false>, dim3(gRows), dim3(256), 0, h->stream, g, ctl, queue);
                return 1;
            }));
        }
        if (s == 0 && in.nnzA > kRdShortL && (product || in.steps > 1)) {   // (else no row is longer, or no product follows)
            BHS_TRY(side_read_ctl(h, ws, RD_INTS));
            if (ws.host[RD_ERR]) return BHS_ERR_INVALID_ARG;
            nqWave = ws.host[RD_CNT_WAVE];
            nqLong = ws.host[RD_CNT_LONG];
        }
        if (product && nqWave) {
            BHS_TRY(timed(h, "relax_wave", nqWave, [&] {
                hipLaunchKernelGGL(k_rx_wave, dim3((unsigned)((nqWave + 3) / 4)), dim3(256), 0, h->stream, nqWave,
                                   queue + (size_t)RD_CNT_WAVE * n, g, ctl);
                return 1;
            }));
        }
        if (product && nqLong) {
            BHS_TRY(timed(h, "relax_long", nqLong, [&] {
                hipLaunchKernelGGL(k_rx_long, dim3((unsigned)std::min<long long>(nqLong, (long long)h->numCU * 8)), dim3(256), 0,
                                   h->stream, nqLong, queue + (size_t)RD_CNT_LONG * n, g, ctl);
                return 1;
            }));
        }
        xsrc = g.xout;
        if (g.dout) dsrc = g.dout;
    }
    if (in.steps - 1 <= firstPass) {                                 // the last step wrote scratch
        BHS_TRY(timed(h, "relax_finish", n, [&] {
            hipLaunchKernelGGL(k_rx_finish, dim3(gRows), dim3(256), 0, h->stream, n, xsrc, in.x, in.d ? dsrc : nullptr, in.d, ctl);
            return 1;
        }));
    }
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, RD_INTS));
    BHS_TRY(side_close(h, ws, ms_out));
    return ws.host[RD_ERR] ? (int)BHS_ERR_INVALID_ARG : (int)BHS_SUCCESS;
}

// where the fused product keeps its two results: behind the counters, 8-byte aligned
enum { DOT_OUT = RD_INTS, DOT_INTS = RD_INTS + 4 };
static_assert(RD_INTS % 2 == 0, "the results are doubles");

int dots_run(bhs_handle* h, const MvIn& in, const value_t* yIn, const value_t* w, double* dots, double* ms_out)
{
    const MvDims& d = in.d;
    SideWs& ws = h->dotWs;
    const int nPart = (int)std::max<long long>(1, ((long long)d.m + kDotPer - 1) / kDotPer);
    const size_t qBytes = rx_pad(sizeof(int) * 2 * (size_t)std::max(d.m, 1));
    BHS_TRY(side_open(h, ws, DOT_INTS, qBytes + sizeof(double) * 2 * (size_t)nPart, 0));
    BHS_TRY(side_start(h, ws));
    int* ctl = (int*)ws.ctl.p;
    int* queue = (int*)ws.queue.p;
    double* part = (double*)((char*)ws.queue.p + qBytes);
    if (d.beta != 0.0 && yIn != in.Y && d.m > 0)                     // out of place: the product's kernels update z = y
        BHS_HIP(hipMemcpyAsync(in.Y, yIn, sizeof(value_t) * (size_t)d.m, hipMemcpyDeviceToDevice, h->stream));
    const MvKernels kern = mv_kernels(1);
    const unsigned gShort = (unsigned)std::max<long long>(1, ((long long)d.m + kRdRows - 1) / kRdRows);
    BHS_TRY(timed(h, "spmv_short", d.m, [&] {
        hipLaunchKernelGGL(kern.rowsShort, dim3(gShort), dim3(256), 0, h->stream, d, in.Ap, in.Aj, in.Ax, in.X, in.Y, ctl, queue);
        return 1;
    }));
    if (d.nnzA > kRdShortL) {                                        // (else no row can be longer)
        BHS_TRY(side_read_ctl(h, ws, RD_INTS));
        if (ws.host[RD_ERR]) return BHS_ERR_INVALID_ARG;
        if (const int nq = ws.host[RD_CNT_WAVE]) {
            BHS_TRY(timed(h, "spmv_wave", nq, [&] {
                hipLaunchKernelGGL(kern.rowsWave, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, h->stream, nq,
                                   queue + (size_t)RD_CNT_WAVE * d.m, d, in.Ap, in.Aj, in.Ax, in.X, in.Y, ctl);
                return 1;
            }));
        }
        if (const int nq = ws.host[RD_CNT_LONG]) {
            BHS_TRY(timed(h, "spmv_long", nq, [&] {
                hipLaunchKernelGGL(kern.rowsLong, dim3((unsigned)std::min<long long>(nq, (long long)h->numCU * 8)), dim3(256), 0,
                                   h->stream, nq, queue + (size_t)RD_CNT_LONG * d.m, d, in.Ap, in.Aj, in.Ax, in.X, in.Y, ctl);
                return 1;
            }));
        }
    }
    BHS_TRY(timed(h, "dots_part", d.m, [&] {
        hipLaunchKernelGGL(k_dot_part, dim3((unsigned)nPart), dim3(256), 0, h->stream, d.m, (const value_t*)in.Y, w, part);
        return 1;
    }));
    BHS_TRY(timed(h, "dots_finish", nPart, [&] {
        hipLaunchKernelGGL(k_dot_finish, dim3(1), dim3(256), 0, h->stream, nPart, (const double*)part, (double*)(ctl + DOT_OUT));
        return 1;
    }));
    BHS_TRY(side_end(h, ws));
    BHS_TRY(side_read_ctl(h, ws, DOT_INTS));
    BHS_TRY(side_close(h, ws, ms_out));
    if (ws.host[RD_ERR]) return BHS_ERR_INVALID_ARG;
    double out[2];
    memcpy(out, ws.host + DOT_OUT, sizeof(out));
    dots[0] = out[0];
    if (w) dots[1] = out[1];
    return BHS_SUCCESS;
}

}  // namespace

extern "C" {

int bhs_chebyshev_coefficients(double lmin, double lmax, int steps, double* coef)
{
    if (!coef || steps < 1 || !std::isfinite(lmin) || !std::isfinite(lmax) || !(lmin > 0.0) || !(lmin < lmax)) return BHS_ERR_INVALID_ARG;
    const double theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma = theta / delta;
    double rho = 1 / sigma;
    coef[0] = 0.0;
    coef[1] = 1 / theta;
    for (int s = 1; s < steps; ++s) {
        const double next = 1 / (2 * sigma - rho);
        coef[2 * s] = next * rho;
        coef[2 * s + 1] = 2 * next / delta;
        rho = next;
    }
    return BHS_SUCCESS;
}

int bhs_csr_relax_device(bhs_handle* h, int n, int nnzA, const bhs_value_t* d_valA, const int* d_rowPtrA, const int* d_colIndA,
                         const bhs_value_t* d_diag, int steps, const double* coef, const bhs_value_t* d_b, bhs_value_t* d_x,
                         bhs_value_t* d_d, unsigned flags, double* ms_out)
{
    if (!h || h->ps.open || n < 0 || nnzA < 0 || steps < 1 || !coef || (flags & ~(unsigned)BHS_RELAX_ZERO_GUESS)) return BHS_ERR_INVALID_ARG;
    if (!d_rowPtrA || (nnzA > 0 && !d_colIndA)) return BHS_ERR_INVALID_ARG;
    if (n > 0 && (!d_diag || !d_b || !d_x)) return BHS_ERR_INVALID_ARG;
    bool needD = false;
    for (int s = 0; s < 2 * steps; ++s) {
        if (!std::isfinite(coef[s])) return BHS_ERR_INVALID_ARG;
        if (s % 2 == 0 && coef[s] != 0.0) needD = true;
    }
    if (needD && n > 0 && !d_d) return BHS_ERR_INVALID_ARG;
    const size_t vBytes = sizeof(value_t) * (size_t)n;
    if (side_aliased({{d_x, vBytes}, {d_d, vBytes}},
                     {{d_rowPtrA, sizeof(int) * ((size_t)n + 1)}, {d_colIndA, sizeof(int) * (size_t)nnzA}, {d_valA, sizeof(value_t) * (size_t)nnzA},
                      {d_diag, vBytes}, {d_b, vBytes}}))
        return BHS_ERR_INVALID_ARG;
    RxIn in;
    in.n = n; in.nnzA = nnzA; in.steps = steps; in.Ap = d_rowPtrA; in.Aj = d_colIndA; in.Ax = (const value_t*)d_valA;
    in.diag = (const value_t*)d_diag; in.b = (const value_t*)d_b; in.x = (value_t*)d_x; in.d = (value_t*)d_d; in.coef = coef;
    in.zero = (flags & BHS_RELAX_ZERO_GUESS) != 0;
    return guarded(h, [&] { return rx_run(h, in, ms_out); });
}

int bhs_csr_spmv_dots_device(bhs_handle* h, int m, int n, int nnzA, const bhs_value_t* d_valA, const int* d_rowPtrA,
                             const int* d_colIndA, double alpha, const bhs_value_t* d_x, double beta, const bhs_value_t* d_y,
                             bhs_value_t* d_z, const bhs_value_t* d_w, double* dots, double* ms_out)
{
    if (!h || h->ps.open || m < 0 || n < 0 || nnzA < 0 || !d_rowPtrA || !dots) return BHS_ERR_INVALID_ARG;
    if (nnzA > 0 && (!d_colIndA || !d_x)) return BHS_ERR_INVALID_ARG;
    if (m > 0 && (!d_z || (beta != 0.0 && !d_y))) return BHS_ERR_INVALID_ARG;
    const size_t zBytes = sizeof(value_t) * (size_t)m;
    const void* y = (const void*)d_y == (const void*)d_z ? nullptr : d_y;   // (z == y exactly: in place)
    if (side_aliased({{d_z, zBytes}},                                // (z is the one array written)
                     {{d_rowPtrA, sizeof(int) * ((size_t)m + 1)}, {d_colIndA, sizeof(int) * (size_t)nnzA}, {d_valA, sizeof(value_t) * (size_t)nnzA},
                      {d_x, sizeof(value_t) * (size_t)n}, {d_w, zBytes}, {y, zBytes}}))
        return BHS_ERR_INVALID_ARG;
    MvIn in;
    in.d.m = m; in.d.n = n; in.d.nnzA = nnzA; in.d.k = 1; in.d.ldX = 1; in.d.ldY = 1; in.d.alpha = alpha; in.d.beta = beta;
    in.Ap = d_rowPtrA; in.Aj = d_colIndA; in.Ax = (const value_t*)d_valA; in.X = (const value_t*)d_x; in.Y = (value_t*)d_z;
    return guarded(h, [&] { return dots_run(h, in, (const value_t*)d_y, (const value_t*)d_w, dots, ms_out); });
}

}  // extern "C"
