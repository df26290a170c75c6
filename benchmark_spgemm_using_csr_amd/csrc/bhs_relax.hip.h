// bhs_relax.hip.h -- polynomial relaxation sweeps on a CSR matrix, and the reductions of a dense vector beside a product
// (bhs_csr_relax_device, bhs_csr_spmv_dots_device; the contract is worded in include/bhsparse_hip.h, "relaxation and fused
// products").
//
// One step of the relaxation is the vector product's row sum with another store: r = b - sum, q = r / diag,
// dn = c q (+ a d), d <- dn, x <- x + dn.  The sums are bhs_spmv.hip.h's own (mv_row, mv_lanes at the tile T = 1: the same
// bits as bhs_csr_spmv_device gives), the bins, the control words and the queues the reductions':
//
//   k_rx_zero    step 0 under BHS_RELAX_ZERO_GUESS, a thread per row: the row pointer's validation, the queues, and
//                dn = c b / diag without a product
//   k_rx_short   all rows in order, 256 rows a workgroup, the rows of up to 32 entries on the spot; BIN: the call's first
//                kernel -- the row pointer's validation and the queues for
//   k_rx_wave    up to 1024 entries, a wave per row, and
//   k_rx_long    a workgroup per row.
//   k_rx_finish  the copy of a call that ends before a kernel may write the caller's arrays
//
// A step reads x from one array and writes it to another, so no row sees an x of its own step.  Every kernel but the
// call's first leaves at once where ctl[RD_ERR] is raised: the host lets the kernels up to the first product pass -- the
// pass that reads every column -- write scratch only, so a refused call never writes x or d.
//
//   k_dot_part   z.z and w.z over 4096 consecutive elements a workgroup, one partial each: the number of workgroups is a
//                function of m alone
//   k_dot_finish the partials in workgroup order, by one workgroup
#pragma once
#include "bhs_spmv.hip.h"

namespace bhs {

struct RxArgs {
    int n, nnzA;
    const int* Ap; const int* Aj; const value_t* Ax;
    const value_t* diag; const value_t* b;
    const value_t* xin;               // the x from before the step (NULL: it counts as +0; k_rx_zero alone)
    value_t* xout;                    // never xin
    const value_t* din;               // read where a != 0 only (may be dout: row r is read and written by one thread)
    value_t* dout;                    // NULL: d is not kept
    double a, c;
};

constexpr int kDotPer = 4096;         // k_dot_part: elements a workgroup

// the dimensions mv_row wants: n columns, a vector of stride 1
__device__ __forceinline__ MvDims rx_dims(const RxArgs& g)
{
    MvDims d;
    d.m = g.n; d.n = g.n; d.nnzA = g.nnzA; d.k = 1; d.ldX = 1; d.ldY = 1; d.alpha = 1.0; d.beta = 0.0;
    return d;
}

// row r from its sum: every operation rounds by itself (no contraction), so the bits do not depend on the kernel a row
// runs in, nor on whether a call's steps come one by one
__device__ __forceinline__ void rx_update(const RxArgs& g, int r, double s)
{
#pragma clang fp contract(off)
    const double res = (double)g.b[r] - s;
    const double q = res / (double)g.diag[r];
    double dn = g.c * q;
    if (g.a != 0.0) {                                             // (a == 0 never reads d)
        const double ad = g.a * (double)g.din[r];
        dn = dn + ad;
    }
    if (g.dout) g.dout[r] = (value_t)dn;
    const double x0 = g.xin ? (double)g.xin[r] : 0.0;
    g.xout[r] = (value_t)(x0 + dn);
}

__global__ __launch_bounds__(256) void k_rx_zero(RxArgs g, int* __restrict__ ctl, int* __restrict__ queue)
{
    __shared__ int sCnt[2], sBase[2];
    const int tid = threadIdx.x;
    if (tid < 2) sCnt[tid] = 0;
    __syncthreads();
    const int r = blockIdx.x * kRdRows + tid;
    bool bad = blockIdx.x == 0 && tid == 0 && (g.Ap[0] != 0 || g.Ap[g.n] != g.nnzA);
    int len = 0;
    if (r < g.n) {
        const int a = g.Ap[r], b = g.Ap[r + 1];
        if (rd_bounds_bad(a, b, g.nnzA)) bad = true;
        else len = b - a;
        rx_update(g, r, 0.0);
    }
    rd_flag(bad, ctl);
    rd_enqueue(g.n, r, len, sCnt, sBase, ctl, queue);
}

template <bool BIN>
__global__ __launch_bounds__(256) void k_rx_short(RxArgs g, int* __restrict__ ctl, int* __restrict__ queue)
{
    constexpr int RPI = 256 / kRdG;                               // rows an iteration
    __shared__ int sLen[kRdRows];
    __shared__ int sCnt[2], sBase[2], sErr;
    const int tid = threadIdx.x, lane = tid & 63, sl = tid & (kRdG - 1);
    if (tid == 0) sErr = BIN ? 0 : ctl[RD_ERR];                   // (one read a workgroup: another one may raise the word meanwhile)
    if (tid < 2) sCnt[tid] = 0;
    sLen[tid] = 0;
    __syncthreads();
    if (sErr) return;
    const MvDims d = rx_dims(g);
    const int rowBase = blockIdx.x * kRdRows;
    bool bad = BIN && blockIdx.x == 0 && tid == 0 && (g.Ap[0] != 0 || g.Ap[g.n] != g.nnzA);
    for (int it = 0; it < kRdRows / RPI; ++it) {
        if (rowBase + it * RPI >= g.n) break;                     // (workgroup-uniform)
        const int rslot = it * RPI + tid / kRdG;
        const int r = rowBase + rslot;
        int a = 0, len = -1;                                      // -1: no row here, or bounds that are refused
        if (r < g.n) {
            a = g.Ap[r];
            const int b = g.Ap[r + 1];
            if (rd_bounds_bad(a, b, g.nnzA)) bad = true;
            else len = b - a;
        }
        const bool here = len >= 0 && len <= kRdShortL;
        double s = 0.0;
        if (here) s = mv_row<2>(d, g.Aj, g.Ax, g.xin, a, len, sl, kRdG, 0, bad);
        s = mv_lanes<1, kRdG>(s, lane);
        if (here && sl == 0) rx_update(g, r, s);
        if (BIN && sl == 0 && len > 0) sLen[rslot] = len;
    }
    rd_flag(bad, ctl);
    if constexpr (BIN) {
        __syncthreads();
        rd_enqueue(g.n, rowBase + tid, sLen[tid], sCnt, sBase, ctl, queue);
    }
}

__global__ __launch_bounds__(256) void k_rx_wave(int nq, const int* __restrict__ queue, RxArgs g, int* __restrict__ ctl)
{
    __shared__ int sErr;
    if (threadIdx.x == 0) sErr = ctl[RD_ERR];
    __syncthreads();
    if (sErr) return;
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;                                         // (wave-uniform, as everything below)
    const int r = queue[qi];
    if ((unsigned)r >= (unsigned)g.n) return;
    const int a = g.Ap[r], b = g.Ap[r + 1];
    if (rd_bounds_bad(a, b, g.nnzA)) return;                      // (no such row is queued)
    const MvDims d = rx_dims(g);
    bool bad = false;
    double s = mv_row<4>(d, g.Aj, g.Ax, g.xin, a, b - a, lane, 64, 0, bad);
    s = mv_lanes<1, 64>(s, lane);
    if (lane == 0) rx_update(g, r, s);
    rd_flag(bad, ctl);
}

__global__ __launch_bounds__(256) void k_rx_long(int nq, const int* __restrict__ queue, RxArgs g, int* __restrict__ ctl)
{
    __shared__ double sW[4];
    __shared__ int sErr;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) sErr = ctl[RD_ERR];
    __syncthreads();
    if (sErr) return;
    const MvDims d = rx_dims(g);
    bool bad = false;
    for (int qi = blockIdx.x; qi < nq; qi += gridDim.x) {         // (everything below is workgroup-uniform)
        const int r = queue[qi];
        if ((unsigned)r >= (unsigned)g.n) continue;
        const int a = g.Ap[r], b = g.Ap[r + 1];
        if (rd_bounds_bad(a, b, g.nnzA)) continue;
        double s = mv_row<4>(d, g.Aj, g.Ax, g.xin, a, b - a, tid, 256, 0, bad);
        s = mv_lanes<1, 64>(s, lane);
        if (lane == 0) sW[wave] = s;
        __syncthreads();
        if (tid == 0) rx_update(g, r, ((sW[0] + sW[1]) + sW[2]) + sW[3]);
        __syncthreads();                                          // (sW is the next row's)
    }
    rd_flag(bad, ctl);
}

// x and d from the scratch the call's kernels wrote, unless one of them refused the input
__global__ __launch_bounds__(256) void k_rx_finish(int n, const value_t* __restrict__ xs, value_t* __restrict__ x,
                                                   const value_t* __restrict__ ds, value_t* __restrict__ dd,
                                                   const int* __restrict__ ctl)
{
    if (ctl[RD_ERR]) return;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < n) {
        x[t] = xs[t];
        if (dd) dd[t] = ds[t];
    }
}

// ---------------------------------------------------------------- the reductions beside a product
// part[b] = sum of double(z)^2, part[gridDim.x + b] = sum of double(w) double(z) over the workgroup's elements: four chains
// a thread, then the lanes' butterfly and the waves in order -- a function of m alone
__global__ __launch_bounds__(256) void k_dot_part(int m, const value_t* __restrict__ z, const value_t* __restrict__ w,
                                                  double* __restrict__ part)
{
    __shared__ rd_u64 sZ[4], sWz[4];
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * kDotPer + tid;
    double zc[4] = {0.0, 0.0, 0.0, 0.0}, wc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < kDotPer / 256; j += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long i = base + (long long)(j + u) * 256;
            if (i < m) {
                const double zv = (double)z[i];
                zc[u] += zv * zv;
                if (w) wc[u] += (double)w[i] * zv;
            }
        }
    }
    const rd_u64 vz = rd_block<kRdSum>(rd_bits((zc[0] + zc[1]) + (zc[2] + zc[3])), tid, sZ);
    const rd_u64 vw = rd_block<kRdSum>(rd_bits((wc[0] + wc[1]) + (wc[2] + wc[3])), tid, sWz);
    if (tid == 0) {
        part[blockIdx.x] = rd_real(vz);
        part[gridDim.x + blockIdx.x] = rd_real(vw);
    }
}

// out[0], out[1] from the two runs of nPart partials: one workgroup, thread t adds partials t, t + 256, .. in that order
__global__ __launch_bounds__(256) void k_dot_finish(int nPart, const double* __restrict__ part, double* __restrict__ out)
{
    __shared__ rd_u64 sZ[4], sWz[4];
    const int tid = threadIdx.x;
    double vz = 0.0, vw = 0.0;
    for (int i = tid; i < nPart; i += 256) {
        vz += part[i];
        vw += part[nPart + i];
    }
    const rd_u64 rz = rd_block<kRdSum>(rd_bits(vz), tid, sZ);
    const rd_u64 rw = rd_block<kRdSum>(rd_bits(vw), tid, sWz);
    if (tid == 0) {
        out[0] = rd_real(rz);
        out[1] = rd_real(rw);
    }
}

}  // namespace bhs
