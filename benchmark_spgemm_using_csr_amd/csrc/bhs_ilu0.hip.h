// bhs_ilu0.hip.h -- the incomplete factorisation A = L U on A's own pattern, in place, level by level
// (bhs_csr_ilu0_device; the contract is worded in include/bhsparse_hip.h, "triangular solve and ILU(0)").
//
//   k_ilu0_level<L>  the rows order[lo .. lo + cnt) of ONE level of the LOWER analysis, a launch; a row takes L lanes of one
//                    wave.  Owner computes: lane `sub` owns the entries q = a + sub, a + sub + L, ... of its row and is the
//                    only lane that ever reads or writes their values.  Step t takes the row's t-th entry, column k < i:
//                    its owner makes l_ik = value_t(double(a_ik) / double(u_kk)), stores it and hands it to the row's other
//                    lanes (a shuffle); every lane then looks up each of its own columns j > k in row k's part beyond the
//                    diagonal (a binary search: rows are strictly ascending) and, where row k holds it, takes
//                    a_ij = value_t(double(a_ij) - double(l_ik) * double(u_kj)).  Row k belongs to an earlier level and is
//                    final by the kernel boundary; no value of row i is touched by two lanes, so nothing is ordered inside a
//                    wave and the result is a function of the input.  The steps of the rows of a wave go round together
//                    until none of them has an entry left below its diagonal -- a row of g entries at most g times.
//                    The smallest row whose pivot u_ii is 0 or not finite goes to ctl[TS_PIVOT] by an integer minimum.
//
// Validation ahead of each dependent read: an entry of order before it is a row, the row's bounds before its entries, its
// columns (in range, strictly ascending, the diagonal among them) before any value is taken, row k's bounds and its
// diagonal before u_kk; each raises ctl[RD_ERR] and the row (the step) is skipped.
#pragma once
#include "bhs_trsv.hip.h"

namespace bhs {

// the place of column c in Aj[lo .. hi), ascending; -1 where it is not there
__device__ __forceinline__ int il_find(const int* __restrict__ Aj, int lo, int hi, int c)
{
    while (lo < hi) {                                                 // (halves every turn)
        const int mid = lo + ((hi - lo) >> 1);
        const int j = Aj[mid];
        if (j == c) return mid;
        if (j < c) lo = mid + 1;
        else hi = mid;
    }
    return -1;
}

template <int L>
__global__ __launch_bounds__(256) void k_ilu0_level(TsDims d, const int* __restrict__ Ap, const int* __restrict__ Aj, value_t* Ax,
                                                    const int* __restrict__ order, int* __restrict__ ctl)
{
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (L - 1);
    const long long place = (long long)blockIdx.x * (256 / L) + threadIdx.x / L;
    bool bad = false;
    int a, e;
    int i = ts_listed(d.n, d.nnzA, d.lo, d.cnt, place, Ap, order, a, e, bad);
    // the row's columns: every lane checks its own entries, the row's lanes agree on the outcome
    unsigned wrong = 0, dq = 0xFFFFFFFFu;
    for (int q = a + sub; q < e; q += L) {
        const int j = Aj[q];
        if ((unsigned)j >= (unsigned)d.n || (q > a && Aj[q - 1] >= j)) wrong = 1;
        else if (j == i) dq = (unsigned)q;
    }
    wrong = ts_lanes_max<L>(wrong, lane);
    const bool mine = dq != 0xFFFFFFFFu;                              // this lane owns the diagonal entry
    dq = ts_lanes_min<L>(dq, lane);
    if (i >= 0 && (wrong || dq == 0xFFFFFFFFu)) { bad = true; i = -1; a = e = 0; }
    bool walk = i >= 0;                                               // (the same in the L lanes of a row)
    int t = 0;
    do {
        int k = -1, ka = 0, ke = 0, kd = -1;
        if (walk) {
            if (a + t < e) k = Aj[a + t];
            if (k >= i) k = -1;                                       // the diagonal is reached: the row is done
            if (k >= 0) {
                ka = Ap[k]; ke = Ap[k + 1];
                if (rd_bounds_bad(ka, ke, d.nnzA)) { bad = true; k = -1; }
                else {
                    kd = il_find(Aj, ka, ke, k);
                    if (kd < 0) { bad = true; k = -1; }               // row k has no diagonal entry
                }
            }
            if (k < 0) walk = false;
        }
        double l = 0.0;
        if (walk && sub == (t & (L - 1))) {                           // the owner of a_ik
            const value_t lv = (value_t)((double)Ax[a + t] / (double)Ax[kd]);
            Ax[a + t] = lv;
            l = (double)lv;
        }
        l = __shfl(l, (lane & ~(L - 1)) | (t & (L - 1)));             // (every lane of the wave comes here)
        if (walk) {
            const int first = t + 1 + ((sub - (t + 1)) & (L - 1));    // this lane's first entry behind a_ik
            for (int q = a + first; q < e; q += L) {
                const int p = il_find(Aj, kd + 1, ke, Aj[q]);
                if (p >= 0) Ax[q] = (value_t)((double)Ax[q] - l * (double)Ax[p]);
            }
        }
        ++t;
    } while (__ballot(walk) != 0ull);
    if (i >= 0 && mine) {
        const double u = (double)Ax[dq];
        if (u == 0.0 || !(fabs(u) <= 1.79769313486231570815e308)) (void)atomicMin(ctl + TS_PIVOT, i);
    }
    rd_flag(bad, ctl);
}

}  // namespace bhs
