// bhs_sddmm.hip.h -- the sampled dense-dense product Z(i, j) = alpha (X(i, :) . Y(j, :)) [M(i, j)] + beta Z(i, j) on the
// entries of a CSR pattern (bhs_csr_sddmm_device; the contract is worded in include/bhsparse_hip.h, "sampled dense-dense
// product").
//
// Rows are binned by length exactly as the reductions bin them (bhs_reduce.hip.h: its constants, its control words, its
// row-pointer check and its queues are used as they are) -- for load balance alone, since no sum crosses entries:
//
//   k_sd_short   all rows in order, 256 rows a workgroup: the row pointer's validation (every row), the rows of up to 32
//                entries on the spot, the longer ones queued for
//   k_sd_wave    up to 1024 entries, a wave per row, and
//   k_sd_long    a workgroup per row.
//
// Every kernel is a template of the tile T = min(64, the smallest power of two >= k).  It is bhs_spmv.hip.h's column tile
// turned around: the T lanes of an ENTRY lie along k, so one entry's gather of Y's row is ONE contiguous read of T values,
// and X's row piece is one register a lane that stays across the row's entries.  A group of T lanes walks a row with
// 16 / T (short rows), 64 / T (a wave) or 256 / T (a workgroup) entries in flight, four entries a step: their columns
// first, then their gathers (and values) together, as mv_row does it; the four butterflies of a step share their exchanges
// (sd_lanes) and end in four different lanes, each of which finishes and stores one entry.  k beyond 64 loops over tiles
// of 64 inside the lane and reads X's piece again per tile and step (from the cache) instead of keeping k / 64 registers
// of it.
//
// Arithmetic, all of it with contraction off: lane l starts at +0 and adds double(X(i, tT + l)) * double(Y(j, tT + l)) for
// t = 0, 1, .. while tT + l < k (product rounded, sum rounded); the T lanes meet in the butterfly xor 1, 2, .. T / 2 (both
// partners compute the same bits); then s * double(m_ij) under TIMES_M, t = alpha * s, t + beta * double(z_old) only where
// beta != 0, one rounding.  The bits of an entry are a function of its two rows of X and Y, k and the coefficients: all
// three kernels run the one body sd_row, so the bin, the row's length and the entry's place in it do not show.
//
// Validation precedes every dependent read: a row whose bounds the row pointer's check refuses is not read at all, a column
// outside [0, n) is never an index into Y (its entry is left as it was); both raise ctl[RD_ERR].  Stores go to entries
// q < nnzM of rows whose bounds hold only.
#pragma once
#include "bhs_reduce.hip.h"

namespace bhs {

struct SdDims {
    int m, n, nnzM, k;
    long long ldX, ldY;
    double alpha, beta;
    int timesM;
};

constexpr int kSdB = 4;               // entries a group has in flight a step

// lanes that share a short row: a DPP row of 16, or the tile where it is wider
template <int T> constexpr int sd_group() { return T > kRdG ? T : kRdG; }

// the lane of the group that ends with entry u's sum, finishes it and stores it
template <int T> constexpr int sd_owner(int u) { return T >= 4 ? u : T == 2 ? (u & 1) : 0; }

// a + the partner's b across xor X: what a butterfly step gives the lane that keeps a (an IEEE addition is commutative, so
// the partner, keeping its own, has the same bits)
template <int X>
__device__ __forceinline__ double sd_step(double a, double b, int lane)
{
    return a + rd_real(lane_xor64<X>(rd_bits(b), lane));
}

// The butterflies xor 1, 2, .. T / 2 of a step's four entries over the T lanes of the group (every lane of the wave active),
// with the additions nobody would read left out: across xor 1 a lane keeps entry 0 or 1 by its bit 0 (and 2 or 3), across
// xor 2 one of the two by its bit 1, and from xor 4 on it carries ONE entry's sum -- the same additions of the same
// operands as four whole butterflies in the lanes that are read, 9 exchanges for T = 64 instead of 24.  s[u] ends as entry
// u's sum in lane sd_owner<T>(u) of the group (other lanes hold another entry's there).
template <int T>
__device__ __forceinline__ void sd_lanes(double (&s)[kSdB], int lane)
{
    static_assert(kSdB == 4, "two halvings of four entries");
    if constexpr (T >= 2) {
        const bool odd = lane & 1;
        const double w01 = sd_step<1>(odd ? s[1] : s[0], odd ? s[0] : s[1], lane);
        const double w23 = sd_step<1>(odd ? s[3] : s[2], odd ? s[2] : s[3], lane);
        if constexpr (T == 2) {
            s[0] = s[1] = w01;
            s[2] = s[3] = w23;
        } else {
            const bool up = lane & 2;
            double w = sd_step<2>(up ? w23 : w01, up ? w01 : w23, lane);
            if constexpr (T > 4) w = sd_step<4>(w, w, lane);
            if constexpr (T > 8) w = sd_step<8>(w, w, lane);
            if constexpr (T > 16) w = sd_step<16>(w, w, lane);
            if constexpr (T > 32) w = sd_step<32>(w, w, lane);
            s[0] = s[1] = s[2] = s[3] = w;
        }
    }
}

// Entries a + slot, a + slot + step, .. of row r (len of them; len <= 0: none) for the group whose lane `col` this is.
// Every lane of the wave must come here together and lenAll be the same in all of them, no less than any lane's len: it
// bounds the loop, so that the butterflies find every lane active.  (Mx and Zx may be one array: no __restrict__.)
template <int T>
__device__ __forceinline__ void sd_row(const SdDims& d, const int* __restrict__ Mj, const value_t* Mx,
                                       const value_t* __restrict__ X, const value_t* __restrict__ Y, value_t* Zx, int r, int a,
                                       int len, int lenAll, int slot, int step, int col, int lane, bool& bad)
{
#pragma clang fp contract(off)
    const bool one = d.k <= T;                                    // a single tile: X's piece is read once a row
    const value_t* Xr = X + (long long)(len > 0 ? r : 0) * d.ldX;
    double x0 = 0.0;
    if (one && len > 0 && col < d.k) x0 = (double)Xr[col];
    for (int i0 = 0; i0 < lenAll; i0 += step * kSdB) {
        int c[kSdB];
        bool ok[kSdB];
#pragma unroll
        for (int u = 0; u < kSdB; ++u) {
            const int i = i0 + slot + u * step;
            ok[u] = i < len;
            c[u] = ok[u] ? Mj[a + i] : 0;
            if ((unsigned)c[u] >= (unsigned)d.n) { bad |= ok[u]; ok[u] = false; }   // (never an index)
        }
        double s[kSdB], mv[kSdB], zo[kSdB];
#pragma unroll
        for (int u = 0; u < kSdB; ++u) {
            const bool head = ok[u] && col == sd_owner<T>(u);     // the lane that finishes and stores the entry
            mv[u] = (head && d.timesM) ? (double)Mx[a + i0 + slot + u * step] : 1.0;
            zo[u] = (head && d.beta != 0.0) ? (double)Zx[a + i0 + slot + u * step] : 0.0;   // (beta == 0 never reads z)
            s[u] = 0.0;
        }
        if (one) {
            double y[kSdB];
#pragma unroll
            for (int u = 0; u < kSdB; ++u) y[u] = (ok[u] && col < d.k) ? (double)Y[(long long)c[u] * d.ldY + col] : 0.0;
#pragma unroll
            for (int u = 0; u < kSdB; ++u)
                if (ok[u] && col < d.k) {
                    const double p = x0 * y[u];
                    s[u] = s[u] + p;
                }
        } else {
            for (int t0 = 0; t0 < d.k; t0 += T) {
                const bool in = t0 + col < d.k;
                const double x = (in && len > 0) ? (double)Xr[t0 + col] : 0.0;
                double y[kSdB];
#pragma unroll
                for (int u = 0; u < kSdB; ++u) y[u] = (ok[u] && in) ? (double)Y[(long long)c[u] * d.ldY + t0 + col] : 0.0;
#pragma unroll
                for (int u = 0; u < kSdB; ++u)
                    if (ok[u] && in) {
                        const double p = x * y[u];
                        s[u] = s[u] + p;
                    }
            }
        }
        sd_lanes<T>(s, lane);
#pragma unroll
        for (int u = 0; u < kSdB; ++u)
            if (ok[u] && col == sd_owner<T>(u)) {
                double v = s[u];
                if (d.timesM) v = v * mv[u];
                double t = d.alpha * v;
                if (d.beta != 0.0) {
                    const double bz = d.beta * zo[u];
                    t = t + bz;
                }
                Zx[a + i0 + slot + u * step] = (value_t)t;
            }
    }
}

// the longest of the wave's lens (every lane active): the bound sd_row's loop wants
__device__ __forceinline__ int sd_wave_max(int len, int lane)
{
    unsigned v = (unsigned)max(len, 0);
    v = max(v, lane_xor<1>(v, lane));
    v = max(v, lane_xor<2>(v, lane));
    v = max(v, lane_xor<4>(v, lane));
    v = max(v, lane_xor<8>(v, lane));
    v = max(v, lane_xor<16>(v, lane));
    v = max(v, lane_xor<32>(v, lane));
    return (int)v;
}

template <int T>
__global__ __launch_bounds__(256) void k_sd_short(SdDims d, const int* __restrict__ Mp, const int* __restrict__ Mj, const value_t* Mx,
                                                  const value_t* __restrict__ X, const value_t* __restrict__ Y, value_t* Zx,
                                                  int* __restrict__ ctl, int* __restrict__ queue)
{
    constexpr int GS = sd_group<T>();                             // lanes a row
    constexpr int RPI = 256 / GS;                                 // rows an iteration
    __shared__ int sLen[kRdRows];
    __shared__ int sCnt[2], sBase[2];
    const int tid = threadIdx.x, lane = tid & 63, sl = tid & (GS - 1);
    const int col = sl % T, slot = sl / T;
    if (tid < 2) sCnt[tid] = 0;
    sLen[tid] = 0;
    __syncthreads();
    const int rowBase = blockIdx.x * kRdRows;
    bool bad = blockIdx.x == 0 && tid == 0 && (Mp[0] != 0 || Mp[d.m] != d.nnzM);
    for (int it = 0; it < kRdRows / RPI; ++it) {
        if (rowBase + it * RPI >= d.m) break;                     // (workgroup-uniform)
        const int rslot = it * RPI + tid / GS;
        const int r = rowBase + rslot;
        int a = 0, len = -1;                                      // -1: no row here, or bounds that are refused
        if (r < d.m) {
            a = Mp[r];
            const int b = Mp[r + 1];
            if (rd_bounds_bad(a, b, d.nnzM)) bad = true;
            else len = b - a;
        }
        const int mine = len <= kRdShortL ? len : 0;              // (a longer row is another kernel's)
        sd_row<T>(d, Mj, Mx, X, Y, Zx, r, a, mine, sd_wave_max(mine, lane), slot, GS / T, col, lane, bad);
        if (sl == 0 && len > 0) sLen[rslot] = len;
    }
    __syncthreads();
    rd_flag(bad, ctl);
    rd_enqueue(d.m, rowBase + tid, sLen[tid], sCnt, sBase, ctl, queue);
}

template <int T>
__global__ __launch_bounds__(256) void k_sd_wave(int nq, const int* __restrict__ queue, SdDims d, const int* __restrict__ Mp,
                                                 const int* __restrict__ Mj, const value_t* Mx, const value_t* __restrict__ X,
                                                 const value_t* __restrict__ Y, value_t* Zx, int* __restrict__ ctl)
{
    const int lane = threadIdx.x & 63, col = lane % T, slot = lane / T;
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;                                         // (wave-uniform, as everything below)
    const int r = queue[qi];
    if ((unsigned)r >= (unsigned)d.m) return;
    const int a = Mp[r], b = Mp[r + 1];
    if (rd_bounds_bad(a, b, d.nnzM)) return;                      // (k_sd_short queues no such row)
    bool bad = false;
    sd_row<T>(d, Mj, Mx, X, Y, Zx, r, a, b - a, b - a, slot, 64 / T, col, lane, bad);
    rd_flag(bad, ctl);
}

template <int T>
__global__ __launch_bounds__(256) void k_sd_long(int nq, const int* __restrict__ queue, SdDims d, const int* __restrict__ Mp,
                                                 const int* __restrict__ Mj, const value_t* Mx, const value_t* __restrict__ X,
                                                 const value_t* __restrict__ Y, value_t* Zx, int* __restrict__ ctl)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int col = lane % T, slot = tid / T;
    bool bad = false;
    for (int qi = blockIdx.x; qi < nq; qi += gridDim.x) {         // (everything below is workgroup-uniform)
        const int r = queue[qi];
        if ((unsigned)r >= (unsigned)d.m) continue;
        const int a = Mp[r], b = Mp[r + 1];
        if (rd_bounds_bad(a, b, d.nnzM)) continue;
        sd_row<T>(d, Mj, Mx, X, Y, Zx, r, a, b - a, b - a, slot, 256 / T, col, lane, bad);
    }
    rd_flag(bad, ctl);
}

}  // namespace bhs
