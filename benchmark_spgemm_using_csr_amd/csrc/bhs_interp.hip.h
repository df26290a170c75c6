// bhs_interp.hip.h -- direct interpolation on a C/F splitting: P (n x nc) from A, the pattern S of strong connections and
// cf (bhs_csr_interp_symbolic_device, bhs_csr_interp_numeric_device; the contract is worded in include/bhsparse_hip.h,
// "C/F splitting and interpolation").  A row-wise kernel pair like the add, the selection and the extraction:
//
//   k_ip_count   the entries of every row of P: 1 for a C point, else the members of C_i = { j != i : (i, j) in A, j in row i
//                of S, cf[j] >= 0 }.  Everything the calls validate is validated here: the rows' bounds in A and S, every
//                column of both, that both rows ascend strictly, cf[i] and every cf[j] it reads; in the numeric call the
//                row's bounds in P and that the count is what rowPtrP says.  The symbolic call scans the counts with the
//                library's one-pass scan (host: side_scan).
//   k_ip_fill    the row again: the diagonal's place, the four sums N-, N+, C-, C+ in double, then the entries of C_i in row
//                order -- entry k of the row to rowPtrP[i] + k, only where k < rowPtrP[i+1] - rowPtrP[i] and the bounds of
//                the row in P passed: whatever the arrays hold, nothing is written outside [0, nnzP).
//
// A row is spread over L = 1, 4, 16 or 64 lanes (host: ag_lanes on A), lane `sub` takes entries sub, sub + L, ..: a lane adds
// its entries in row order, the L lanes meet in a butterfly (lane_xor64; both partners of a step compute the same bits), the
// SpMV's rule -- the order is a function of the row's length and L alone.  The place of a kept entry is the kept entries
// before it: those of earlier turns of L entries plus a ballot over the group's lanes below it.  Whether j is in S's row is a
// binary search in the sorted row.  No atomics on results, no LDS, no grid cap: a workgroup takes 256 / L rows.
#pragma once
#include "bhs_aggregate.hip.h"

namespace bhs {

struct IpDims {
    int n, nnzA, nnzS, nc, nnzP;
};

template <int L>
__device__ __forceinline__ int ip_lanes_sum(int x, int lane)
{
    unsigned v = (unsigned)x;
    if constexpr (L > 1) v += lane_xor<1>(v, lane);
    if constexpr (L > 2) v += lane_xor<2>(v, lane);
    if constexpr (L > 4) v += lane_xor<4>(v, lane);
    if constexpr (L > 8) v += lane_xor<8>(v, lane);
    if constexpr (L > 16) v += lane_xor<16>(v, lane);
    if constexpr (L > 32) v += lane_xor<32>(v, lane);
    return (int)v;
}

template <int L>
__device__ __forceinline__ int ip_lanes_max(int x, int lane)
{
    if constexpr (L > 1) x = max(x, (int)lane_xor<1>((unsigned)x, lane));
    if constexpr (L > 2) x = max(x, (int)lane_xor<2>((unsigned)x, lane));
    if constexpr (L > 4) x = max(x, (int)lane_xor<4>((unsigned)x, lane));
    if constexpr (L > 8) x = max(x, (int)lane_xor<8>((unsigned)x, lane));
    if constexpr (L > 16) x = max(x, (int)lane_xor<16>((unsigned)x, lane));
    if constexpr (L > 32) x = max(x, (int)lane_xor<32>((unsigned)x, lane));
    return x;
}

template <int L>
__device__ __forceinline__ double ip_lanes_add(double s, int lane)
{
    if constexpr (L > 1) s = s + rd_real(lane_xor64<1>(rd_bits(s), lane));
    if constexpr (L > 2) s = s + rd_real(lane_xor64<2>(rd_bits(s), lane));
    if constexpr (L > 4) s = s + rd_real(lane_xor64<4>(rd_bits(s), lane));
    if constexpr (L > 8) s = s + rd_real(lane_xor64<8>(rd_bits(s), lane));
    if constexpr (L > 16) s = s + rd_real(lane_xor64<16>(rd_bits(s), lane));
    if constexpr (L > 32) s = s + rd_real(lane_xor64<32>(rd_bits(s), lane));
    return s;
}

// The row of this thread's group of L lanes (n and beyond: no row), its checked ranges [a, b) in A and [sa, sb) in S and
// ci = cf[i].  Where A's bounds or cf[i] are refused the row is taken as empty and an F point (bad is raised), where S's are,
// S's row is empty.
template <int L>
__device__ __forceinline__ long long ip_row(const IpDims& d, const int* __restrict__ Ap, const int* __restrict__ Sp,
                                            const int* __restrict__ cf, int& a, int& b, int& sa, int& sb, int& ci, bool& ok, bool& bad)
{
    const long long i = (long long)blockIdx.x * (256 / L) + threadIdx.x / L;
    a = b = sa = sb = 0;
    ci = -1;
    ok = false;
    if (i < d.n) {
        const int lo = Ap[i], hi = Ap[i + 1], slo = Sp[i], shi = Sp[i + 1], c = cf[i];
        if (rd_bounds_bad(slo, shi, d.nnzS)) bad = true;
        else { sa = slo; sb = shi; }
        if (rd_bounds_bad(lo, hi, d.nnzA) || c < -1 || c >= d.nc) bad = true;
        else { a = lo; b = hi; ci = c; ok = true; }
    }
    return i;
}

enum { kIpNone = 0, kIpDiag = 1, kIpOther = 2, kIpCoarse = 3 };

// what entry q of row i of A (a <= q < b, bounds passed) is: no entry (a column that is refused), the diagonal, an
// off-diagonal entry outside C_i, or a member of C_i with cj = cf[j]
__device__ __forceinline__ int ip_entry(const IpDims& d, const int* __restrict__ Aj, const int* __restrict__ Sj,
                                        const int* __restrict__ cf, int i, int a, int q, int sa, int sb, int& cj, bool& bad)
{
    const int j = Aj[q];
    if ((unsigned)j >= (unsigned)d.n) { bad = true; return kIpNone; }    // (never an index)
    if (q > a && Aj[q - 1] >= j) bad = true;                             // the row ascends strictly
    if (j == i) return kIpDiag;
    int lo = sa, hi = sb;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (Sj[mid] < j) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= sb || Sj[lo] != j) return kIpOther;
    const int c = cf[j];
    if (c < -1 || c >= d.nc) { bad = true; return kIpOther; }            // (never an index)
    cj = c;
    return c >= 0 ? kIpCoarse : kIpOther;
}

// cnt[i] = the entries of row i of P (Pp null: the symbolic call); with Pp, the numeric call: nothing is written, the row's
// bounds in P are checked and that they hold this count
template <int L>
__global__ __launch_bounds__(256) void k_ip_count(IpDims d, const int* __restrict__ Ap, const int* __restrict__ Aj,
                                                  const int* __restrict__ Sp, const int* __restrict__ Sj, const int* __restrict__ cf,
                                                  const int* __restrict__ Pp, int* __restrict__ cnt, int* __restrict__ ctl)
{
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (L - 1);
    bool bad = false, ok;
    int a, b, sa, sb, ci;
    const long long i = ip_row<L>(d, Ap, Sp, cf, a, b, sa, sb, ci, ok, bad);
    for (int q = sa + sub; q < sb; q += L) {                             // S's row: columns in range, strictly ascending
        const int j = Sj[q];
        if ((unsigned)j >= (unsigned)d.n || (q > sa && Sj[q - 1] >= j)) bad = true;
    }
    int c = 0;
    if (ci < 0) {
        for (int q = a + sub; q < b; q += L) {
            int cj;
            if (ip_entry(d, Aj, Sj, cf, (int)i, a, q, sa, sb, cj, bad) == kIpCoarse) ++c;
        }
    } else {                                                             // a C point: its row of A gives nothing but is checked
        for (int q = a + sub; q < b; q += L) {
            const int j = Aj[q];
            if ((unsigned)j >= (unsigned)d.n || (q > a && Aj[q - 1] >= j)) bad = true;
        }
    }
    c = ip_lanes_sum<L>(c, lane);
    if (i < d.n && sub == 0) {
        if (ci >= 0) c = 1;
        if (Pp) {
            const int lo = Pp[i], hi = Pp[i + 1];
            if (rd_bounds_bad(lo, hi, d.nnzP) || hi - lo != c) bad = true;
        } else {
            cnt[i] = ok ? c : 0;
        }
    }
    if (Pp && blockIdx.x == 0 && threadIdx.x == 0 && (Pp[0] != 0 || Pp[d.n] != d.nnzP)) bad = true;
    rd_flag(bad, ctl);
}

template <int L>
__global__ __launch_bounds__(256) void k_ip_fill(IpDims d, const int* __restrict__ Ap, const int* __restrict__ Aj,
                                                 const value_t* __restrict__ Ax, const int* __restrict__ Sp,
                                                 const int* __restrict__ Sj, const int* __restrict__ cf, const int* __restrict__ Pp,
                                                 int* __restrict__ Pj, value_t* __restrict__ Px, int* __restrict__ ctl)
{
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (L - 1);
    bool bad = false, ok;
    int a, b, sa, sb, ci;
    const long long i = ip_row<L>(d, Ap, Sp, cf, a, b, sa, sb, ci, ok, bad);
    int plo = 0, room = 0;                                               // the row's place in P: [plo, plo + room) inside [0, nnzP)
    if (i < d.n) {
        const int lo = Pp[i], hi = Pp[i + 1];
        if (rd_bounds_bad(lo, hi, d.nnzP)) bad = true;
        else { plo = lo; room = hi - lo; }
    }
    if (!ok) room = 0;
    if (ci >= 0) {                                                       // a C point: the identity row
        if (sub == 0) {
            if (room >= 1) { Pj[plo] = ci; Px[plo] = (value_t)1; }
            else bad = true;
        }
        a = b = 0;
        room = 0;
    }
    int qd = -1;                                                         // the diagonal's place (a column that equals i is in range)
    for (int q = a + sub; q < b; q += L)
        if (Aj[q] == i) qd = q;
    qd = ip_lanes_max<L>(qd, lane);
    const double dg = qd >= 0 ? (double)Ax[qd] : 0.0;
    double Nn = 0.0, Np = 0.0, Cn = 0.0, Cp = 0.0;
    for (int q = a + sub; q < b; q += L) {
        int cj;
        const int kind = ip_entry(d, Aj, Sj, cf, (int)i, a, q, sa, sb, cj, bad);
        if (kind < kIpOther) continue;
        const double av = (double)Ax[q], t = av * dg;
        if (t < 0.0) { Nn += av; if (kind == kIpCoarse) Cn += av; }
        else if (t > 0.0) { Np += av; if (kind == kIpCoarse) Cp += av; }
    }
    Nn = ip_lanes_add<L>(Nn, lane);
    Np = ip_lanes_add<L>(Np, lane);
    Cn = ip_lanes_add<L>(Cn, lane);
    Cp = ip_lanes_add<L>(Cp, lane);
    double dp = dg;
    if (Cp == 0.0) dp = dp + Np;
    if (Cn == 0.0) dp = dp + Nn;
    const double fn = Nn / Cn, fp = Np / Cp;
    const rd_u64 group = L == 64 ? ~0ull : (((1ull << (L & 63)) - 1ull) << (lane & ~(L - 1)));
    const rd_u64 below = (1ull << lane) - 1ull;
    const int len = b - a;
    int base = 0;
    for (int q0 = 0; __ballot(q0 < len) != 0ull; q0 += L) {              // (uniform in the wave: every lane reaches the ballots)
        const int q = a + q0 + sub;
        int cj = 0;
        const bool kept = q < b && ip_entry(d, Aj, Sj, cf, (int)i, a, q, sa, sb, cj, bad) == kIpCoarse;
        const rd_u64 votes = __ballot(kept) & group;
        if (kept) {
            const int k = base + __popcll(votes & below);
            if (k < room) {
                const double av = (double)Ax[q], t = av * dg;
                const double w = t < 0.0 ? -(fn * av) / dp : t > 0.0 ? -(fp * av) / dp : -(0.0 * av) / dp;
                Pj[plo + k] = cj;
                Px[plo + k] = (value_t)w;
            } else {
                bad = true;
            }
        }
        base += __popcll(votes);
    }
    rd_flag(bad, ctl);
}

}  // namespace bhs
