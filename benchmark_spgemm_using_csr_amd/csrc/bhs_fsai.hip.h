// bhs_fsai.hip.h -- the factorised sparse approximate inverse: the values of a lower-triangular G on a pattern the caller
// gives, with G A G^T ~ I and (G A G^T)_ii = 1 (bhs_csr_fsai_device; the contract is worded in include/bhsparse_hip.h,
// "approximate inverse").
//
// Row i of G with the columns J = (j_0 < .. < j_(d-1) = i) is the last row of the inverse Cholesky factor of A(J, J): n
// independent dense problems of order d <= 128.  Rows are binned by d:
//
//   k_fsai_short  all rows in order, 16 lanes a row, 16 rows a workgroup: the validation of G (every row, whatever its
//                 length), the rows of d <= 16 on the spot, the longer ones queued (two queues of n ints, their lengths in
//                 the control words) for
//   k_fsai_wave   17 <= d <= 64, a wave a row, 4 rows a workgroup, and
//   k_fsai_long   65 <= d <= 128, a workgroup a row.
//
// All three run the one body fs_row<W> on W = 16, 64 or 256 lanes.  M, the lower triangle of A(J, J), lies packed in LDS
// (element (p, q) at p (p + 1) / 2 + q: 136, 2080 and 8256 doubles a row -- 20, 68 and 66 KB a workgroup), J and the
// solution beside it.
//   gather     16 lanes take row j_p of A -- the W / 16 groups of a row of G the rows p, p + W / 16, .. -- in pieces of 16
//              consecutive entries, one coalesced read of the columns and one of the values, up to and including the
//              first entry whose column is >= j_p; every entry of that prefix is checked (column in [0, n), above its
//              predecessor's) and looked up in J[0 .. p] (il_find); the value of a column found goes to its place in M,
//              which starts as +0.  Entries behind the prefix -- the upper triangle of A -- are not looked at.  The
//              next row's bounds are loaded under this row's entries: two dependent reads of memory a row, not four.
//   factorise  column by column, lane r - c - 1 the row r of M: l_rc = m_rc / sqrt(m_cc), then m_rc' -= l_rc l_c'c for
//              c < c' <= r (the long kernel: two lanes a row, c' odd and even).  One lane owns an element during a column,
//              every element takes its updates in ascending c: the bits do not depend on how lanes share the work.
//   solve      L^T g = e_d from the last unknown to the first, lane p the running t_p; g_q goes round through LDS.
// Contraction is off and every division is one; the value is rounded once, at the store.
//
// Validation precedes every dependent read: a row of G whose bounds the row pointer's check refuses is not read at all, a
// row that is empty, longer than 128, not strictly ascending, with a column outside [0, i] or not ending in i gives no
// index into A's row pointer and no store; a row of A whose bounds are refused is not read, an entry of A that breaks the
// order or the range is never looked up.  All raise ctl[RD_ERR].  The smallest row with a pivot m_cc that is not > 0 or
// not finite goes to ctl[FS_BAD_ROW] by an integer minimum.  Stores go to entries q < nnzG of rows whose checks hold only.
#pragma once
#include "bhs_ilu0.hip.h"
#include "bhs_reduce.hip.h"

namespace bhs {

constexpr int kFsShortD = 16;         // short bin: a lane an unknown of a 16-lane group
constexpr int kFsWaveD = 64;          // wave bin
constexpr int kFsMaxD = 128;          // BHS_FSAI_MAX_ROW
constexpr int kFsRows = 16;           // rows a workgroup of k_fsai_short
constexpr int kFsPiece = 16;          // lanes that share a row of A in the gather: its entries in pieces of 16

// control words: the reductions' (the two queues' lengths, the error word), then the smallest row with a bad pivot
enum { FS_BAD_ROW = 3, FS_INTS = RD_INTS };
static_assert(FS_BAD_ROW > RD_ERR && FS_BAD_ROW < RD_INTS, "a free word of the reductions' block");

struct FsDims {
    int n, nnzA, nnzG;
};

// packed lower triangle: the place of (p, q), q <= p
__device__ __forceinline__ int fs_tri(int p, int q) { return ((p * (p + 1)) >> 1) + q; }

// orders LDS traffic among the W lanes of a row (within a wave the LDS pipe keeps a wave's instructions in order: only the
// compiler has to be held)
template <int W>
__device__ __forceinline__ void fs_sync()
{
    if constexpr (W == 256) __syncthreads();
    else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// the bits of a ballot that belong to this lane's piece of C = 16 or 64 lanes
template <int C>
__device__ __forceinline__ unsigned long long fs_piece(unsigned long long m, int lane)
{
    if constexpr (C == 64) return m;
    else return (m >> (lane & 48)) & 0xFFFFull;
}

// does `pred` hold in any of the W lanes of the row (all of them come here together)
template <int W>
__device__ __forceinline__ bool fs_any(bool pred, int lane)
{
    if constexpr (W == 256) return __syncthreads_or(pred ? 1 : 0) != 0;
    else return fs_piece<W>(__ballot(pred), lane) != 0ull;
}

// Row i of G, entries a .. a + d (1 <= d <= 128, inside the arrays), for W lanes of which this is lane sl: is it one the
// contract refuses?  The same answer in all W lanes.
template <int W>
__device__ __forceinline__ bool fs_row_wrong(const int* __restrict__ Gj, int i, int a, int d, int sl, int lane)
{
    bool wrong = false;
    for (int t = sl; t < d; t += W) {
        const int c = Gj[a + t];
        if ((unsigned)c > (unsigned)i || (t > 0 && Gj[a + t - 1] >= c) || (t == d - 1 && c != i)) wrong = true;
    }
    return fs_any<W>(wrong, lane);
}

// One row of G by W lanes (lane sl of them; `lane` its place in the wave): row i, entries a .. a + d with 1 <= d <= W / S
// unknowns, the row's checks passed.  M: d (d + 1) / 2 doubles, g: d doubles, J: d ints of LDS, the row's own.  `bad`: an
// entry of A refused; `pivot`: a bad pivot met (the same in all W lanes).
template <int W>
__device__ __forceinline__ void fs_row(const FsDims& dm, const int* __restrict__ Ap, const int* __restrict__ Aj,
                                       const value_t* __restrict__ Ax, const int* __restrict__ Gj, value_t* __restrict__ Gx, int i,
                                       int a, int d, double* M, double* g, int* J, int sl, int lane, bool& bad, bool& pivot)
{
#pragma clang fp contract(off)
    constexpr int S = W == 256 ? 2 : 1;                           // lanes a row of M
    constexpr int C = kFsPiece;                                   // lanes a piece of a row of A
    static_assert(W == 16 || W == 64 || W == 256, "a DPP row, a wave or the workgroup");
    const int cl = sl & (C - 1);
    for (int t = sl; t < ((d * (d + 1)) >> 1); t += W) M[t] = 0.0;
    for (int t = sl; t < d; t += W) J[t] = Gj[a + t];
    fs_sync<W>();
    // gather: row j_p of A against J[0 .. p], W / 16 rows at a time; the next row's bounds are in flight under this row's
    // entries, and an entry's value comes with its column (it is used only where the column is found)
    int p = sl / C, jp = 0, ra = 0, re = 0;
    if (p < d) { jp = J[p]; ra = Ap[jp]; re = Ap[jp + 1]; }       // (jp in [0, i]: a row of A)
    for (; p < d; p += W / C) {
        int jn = 0, na = 0, ne = 0;
        if (p + W / C < d) { jn = J[p + W / C]; na = Ap[jn]; ne = Ap[jn + 1]; }
        if (rd_bounds_bad(ra, re, dm.nnzA)) bad = true;
        else
            for (int k0 = ra; k0 < re; k0 += C) {
                const int q = k0 + cl;
                const bool in = q < re;
                const int c = in ? Aj[q] : -1;
                const int prev = (in && q > ra) ? Aj[q - 1] : -1;
                const double v = in ? (double)Ax[q] : 0.0;
                const unsigned long long past = fs_piece<C>(__ballot(in && c >= jp), lane);
                const int first = past ? __ffsll((long long)past) - 1 : C;   // the piece's first entry at or beyond the diagonal
                if (in && cl <= first) {
                    if ((unsigned)c >= (unsigned)dm.n || c <= prev) bad = true;
                    else if (c <= jp) {
                        const int at = il_find(J, 0, p + 1, c);
                        if (at >= 0) M[fs_tri(p, at)] = v;
                    }
                }
                if (past) break;
            }
        jp = jn; ra = na; re = ne;
    }
    fs_sync<W>();
    // factorise: M = L L^T in place
    const int ro = sl / S, co = sl % S;
    for (int c = 0; c < d; ++c) {
        const double mcc = M[fs_tri(c, c)];
        if (!(mcc > 0.0) || !(mcc <= 1.79769313486231570815e308)) pivot = true;
        const double lcc = sqrt(mcc);
        const int r = c + 1 + ro;
        if (co == 0 && r < d) M[fs_tri(r, c)] = M[fs_tri(r, c)] / lcc;
        fs_sync<W>();
        if (sl == 0) M[fs_tri(c, c)] = lcc;                       // (nobody reads the diagonal of column c from here on but the solve)
        if (r < d) {
            const double lrc = M[fs_tri(r, c)];
            double* row = M + fs_tri(r, 0);
            int c2 = c + 1 + co;
            for (; c2 + 3 * S <= r; c2 += 4 * S) {                // four elements' reads in flight: column c is not written here
                double l[4], m[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    l[u] = M[fs_tri(c2 + u * S, c)];
                    m[u] = row[c2 + u * S];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const double prod = lrc * l[u];
                    row[c2 + u * S] = m[u] - prod;
                }
            }
            for (; c2 <= r; c2 += S) {
                const double prod = lrc * M[fs_tri(c2, c)];
                row[c2] = row[c2] - prod;
            }
        }
        fs_sync<W>();
    }
    // solve: L^T g = e_d, lane p the unknown p
    double t = sl == d - 1 ? 1.0 : 0.0, gp = 0.0;
    for (int q = d - 1; q >= 0; --q) {
        if (sl == q) {
            gp = t / M[fs_tri(q, q)];
            g[q] = gp;
        }
        fs_sync<W>();
        if (sl < q) {
            const double prod = M[fs_tri(q, sl)] * g[q];
            t = t - prod;
        }
    }
    if (sl < d) Gx[a + sl] = (value_t)gp;
}

// thread t < 16 of the workgroup owns row rowBase + t of d unknowns (0: nothing to queue): rows beyond the short bin join
// the wave or the long queue (n ints each)
__device__ __forceinline__ void fs_enqueue(int n, int r, int d, int* sCnt, int* sBase, int* __restrict__ ctl, int* __restrict__ queue)
{
    const int tid = threadIdx.x;
    const int bin = (tid >= kFsRows || r >= n || d <= kFsShortD) ? -1 : d <= kFsWaveD ? RD_CNT_WAVE : RD_CNT_LONG;
    int rank = 0;
    if (bin >= 0) rank = atomicAdd(&sCnt[bin], 1);
    __syncthreads();
    if (tid < 2 && sCnt[tid]) sBase[tid] = atomicAdd(ctl + tid, sCnt[tid]);
    __syncthreads();
    if (bin >= 0) queue[(size_t)bin * n + sBase[bin] + rank] = r;
}

__device__ __forceinline__ void fs_flag_pivot(bool pivot, int i, int sl, int* __restrict__ ctl)
{
    if (pivot && sl == 0) (void)atomicMin(ctl + FS_BAD_ROW, i);
}

__global__ __launch_bounds__(256) void k_fsai_short(FsDims dm, const int* __restrict__ Ap, const int* __restrict__ Aj,
                                                    const value_t* __restrict__ Ax, const int* __restrict__ Gp,
                                                    const int* __restrict__ Gj, value_t* __restrict__ Gx, int* __restrict__ ctl,
                                                    int* __restrict__ queue)
{
    constexpr int W = kFsShortD;
    __shared__ double sM[kFsRows][(kFsShortD * (kFsShortD + 1)) / 2];
    __shared__ double sG[kFsRows][kFsShortD];
    __shared__ int sJ[kFsRows][kFsShortD];
    __shared__ int sLen[kFsRows];
    __shared__ int sCnt[2], sBase[2];
    const int tid = threadIdx.x, lane = tid & 63, sl = tid & (W - 1), slot = tid / W;
    if (tid < 2) sCnt[tid] = 0;
    if (tid < kFsRows) sLen[tid] = 0;
    __syncthreads();
    const int rowBase = blockIdx.x * kFsRows;
    const int i = rowBase + slot;
    bool bad = blockIdx.x == 0 && tid == 0 && (Gp[0] != 0 || Gp[dm.n] != dm.nnzG);
    bool pivot = false;
    if (i < dm.n) {                                               // (the same in the 16 lanes of a row, as everything below)
        const int a = Gp[i], b = Gp[i + 1];
        int d = 0;                                                // 0: a row that is refused
        if (rd_bounds_bad(a, b, dm.nnzG) || b - a < 1 || b - a > kFsMaxD) bad = true;
        else if (fs_row_wrong<W>(Gj, i, a, b - a, sl, lane)) bad = true;
        else d = b - a;
        if (d >= 1 && d <= kFsShortD) {
            fs_row<W>(dm, Ap, Aj, Ax, Gj, Gx, i, a, d, sM[slot], sG[slot], sJ[slot], sl, lane, bad, pivot);
            fs_flag_pivot(pivot, i, sl, ctl);
        }
        if (sl == 0) sLen[slot] = d;
    }
    __syncthreads();
    rd_flag(bad, ctl);
    fs_enqueue(dm.n, rowBase + tid, tid < kFsRows ? sLen[tid] : 0, sCnt, sBase, ctl, queue);
}

// Row queue[qi] for the W lanes that take it: its bounds and its columns once more (k_fsai_short queues no row that fails),
// so that no word of the queue can lead outside the arrays or the row's LDS; -1: nothing to do.
template <int W>
__device__ __forceinline__ int fs_queued(const FsDims& dm, const int* __restrict__ queue, int qi, const int* __restrict__ Gp,
                                         const int* __restrict__ Gj, int lo, int hi, int sl, int lane, int& a, int& d)
{
    const int i = queue[qi];
    if ((unsigned)i >= (unsigned)dm.n) return -1;
    a = Gp[i];
    const int b = Gp[i + 1];
    if (rd_bounds_bad(a, b, dm.nnzG) || b - a < lo || b - a > hi) return -1;
    d = b - a;
    if (fs_row_wrong<W>(Gj, i, a, d, sl, lane)) return -1;
    return i;
}

__global__ __launch_bounds__(256) void k_fsai_wave(int nq, const int* __restrict__ queue, FsDims dm, const int* __restrict__ Ap,
                                                   const int* __restrict__ Aj, const value_t* __restrict__ Ax,
                                                   const int* __restrict__ Gp, const int* __restrict__ Gj, value_t* __restrict__ Gx,
                                                   int* __restrict__ ctl)
{
    constexpr int W = 64;
    __shared__ double sM[4][(kFsWaveD * (kFsWaveD + 1)) / 2];
    __shared__ double sG[4][kFsWaveD];
    __shared__ int sJ[4][kFsWaveD];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int qi = blockIdx.x * 4 + w;
    if (qi >= nq) return;                                         // (wave-uniform, as everything below)
    int a = 0, d = 0;
    const int i = fs_queued<W>(dm, queue, qi, Gp, Gj, kFsShortD + 1, kFsWaveD, lane, lane, a, d);
    if (i < 0) return;
    bool bad = false, pivot = false;
    fs_row<W>(dm, Ap, Aj, Ax, Gj, Gx, i, a, d, sM[w], sG[w], sJ[w], lane, lane, bad, pivot);
    fs_flag_pivot(pivot, i, lane, ctl);
    rd_flag(bad, ctl);
}

__global__ __launch_bounds__(256) void k_fsai_long(int nq, const int* __restrict__ queue, FsDims dm, const int* __restrict__ Ap,
                                                   const int* __restrict__ Aj, const value_t* __restrict__ Ax,
                                                   const int* __restrict__ Gp, const int* __restrict__ Gj, value_t* __restrict__ Gx,
                                                   int* __restrict__ ctl)
{
    constexpr int W = 256;
    __shared__ double sM[(kFsMaxD * (kFsMaxD + 1)) / 2];
    __shared__ double sG[kFsMaxD];
    __shared__ int sJ[kFsMaxD];
    const int tid = threadIdx.x, lane = tid & 63;
    const int qi = blockIdx.x;                                    // (everything below is workgroup-uniform)
    if (qi >= nq) return;
    int a = 0, d = 0;
    const int i = fs_queued<W>(dm, queue, qi, Gp, Gj, kFsWaveD + 1, kFsMaxD, tid, lane, a, d);
    if (i < 0) return;
    bool bad = false, pivot = false;
    fs_row<W>(dm, Ap, Aj, Ax, Gj, Gx, i, a, d, sM, sG, sJ, tid, lane, bad, pivot);
    fs_flag_pivot(pivot, i, tid, ctl);
    rd_flag(bad, ctl);
}

}  // namespace bhs
