// bhs_gs.hip.h -- multicolour Gauss-Seidel / SOR on a vector, in place (bhs_csr_gs_device; the contract is worded in
// include/bhsparse_hip.h, "colouring and relaxation").
//
//   k_gs_color<L, VERIFY>   the rows order[lo .. lo + cnt) of ONE colour, a launch: L = 1, 4, 16 or 64 lanes a row (chosen on
//                           the host from the mean row length).  s = the sum over the entries with j != i of
//                           double(a_ij) * double(x_j): every lane sums its entries q = a + sub, a + sub + L, ... in double
//                           from +0, the L sums meet in a butterfly (lane_xor64) -- an order that depends on the row's
//                           length and L alone, as the SpMV's does.  t = (b_i - s) / d_i; x_i = t, or x_i + omega (t - x_i):
//                           one rounding to the value type, IEEE results where d_i is 0.  The rows of a colour share no
//                           entry, so a launch reads no x it writes; the kernel boundary is the only synchronisation.
//                           Every lane of a wave reaches the butterfly: a place beyond the colour's rows, or a row that is
//                           refused, has an empty range.  x_i is written by the lane that owns the row.
//
// VERIFY also checks color[i] == c for every listed row and color[j] != c for every off-diagonal entry read: a template
// switch, the plain kernel carries nothing of it.
//
// Validation ahead of each dependent read: an entry of order before it is a row, the row's bounds before its entries, a
// column before it indexes x; each raises ctl[RD_ERR] and the row (the entry) is skipped.
#pragma once
#include "bhs_reduce.hip.h"

namespace bhs {

struct GsDims {
    int n, nnzA;
    int lo, cnt;            // the colour's rows: order[lo .. lo + cnt)
    int c;                  // the colour (VERIFY)
    int plain;              // omega == 1
    double omega;
};

template <int L>
__device__ __forceinline__ double gs_lanes_sum(double s, int lane)
{
    rd_u64 v = rd_bits(s);
    if constexpr (L > 1) v = rd_comb<kRdSum>(v, lane_xor64<1>(v, lane));
    if constexpr (L > 2) v = rd_comb<kRdSum>(v, lane_xor64<2>(v, lane));
    if constexpr (L > 4) v = rd_comb<kRdSum>(v, lane_xor64<4>(v, lane));
    if constexpr (L > 8) v = rd_comb<kRdSum>(v, lane_xor64<8>(v, lane));
    if constexpr (L > 16) v = rd_comb<kRdSum>(v, lane_xor64<16>(v, lane));
    if constexpr (L > 32) v = rd_comb<kRdSum>(v, lane_xor64<32>(v, lane));
    return rd_real(v);
}

template <int L, bool VERIFY>
__global__ __launch_bounds__(256) void k_gs_color(GsDims d, const int* __restrict__ Ap, const int* __restrict__ Aj,
                                                  const value_t* __restrict__ Ax, const value_t* __restrict__ diag,
                                                  const int* __restrict__ order, const int* __restrict__ color,
                                                  const value_t* __restrict__ b, value_t* x, int* __restrict__ ctl)
{
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (L - 1);
    const long long k = (long long)blockIdx.x * (256 / L) + threadIdx.x / L;
    bool bad = false;
    int i = -1, a = 0, e = 0;
    if (k < d.cnt) {
        const int r = order[d.lo + k];
        if ((unsigned)r >= (unsigned)d.n) bad = true;                 // (never an index)
        else {
            const int lo = Ap[r], hi = Ap[r + 1];
            if (rd_bounds_bad(lo, hi, d.nnzA)) bad = true;
            else { i = r; a = lo; e = hi; }
        }
    }
    if constexpr (VERIFY) {
        if (i >= 0 && color[i] != d.c) bad = true;
    }
    double s = 0.0;
    for (int q = a + sub; q < e; q += L) {
        const int j = Aj[q];
        if ((unsigned)j >= (unsigned)d.n) { bad = true; continue; }   // (never an index)
        if (j == i) continue;
        if constexpr (VERIFY) {
            if (color[j] == d.c) bad = true;
        }
        s += (double)Ax[q] * (double)x[j];
    }
    s = gs_lanes_sum<L>(s, lane);
    if (i >= 0 && sub == 0) {
        const double t = ((double)b[i] - s) / (double)diag[i];
        if (d.plain) x[i] = (value_t)t;
        else {
            const double xi = (double)x[i];
            x[i] = (value_t)(xi + d.omega * (t - xi));
        }
    }
    rd_flag(bad, ctl);
}

}  // namespace bhs
