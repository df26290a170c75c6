// The factorised sparse approximate inverse through the C++ facade (host/bhsparse.h): for a banded SPD matrix of 48 rows
// and 20 sub-diagonals, stored with both triangles, the values of G on the pattern of tril(A) -- rows of 1 .. 16 entries
// for the short kernel and of 17 .. 21 for the wave's -- are formed on the device and compared bit for bit with a host
// loop written in the rule's order: the lower triangle of A(J, J), the Cholesky factor column by column, the solve of
// L^T g = e_d from the last unknown, one rounding.  Then (G A G^T)_ii = 1 up to rounding, a negated diagonal entry is
// reported as the smallest bad row while the rows above it keep their bits, and an output that overlaps an input and an
// unknown flag are refused with nothing written.  Prints PASS and exits 0 on success.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../benchmark_spgemm_using_csr_amd/host/bhsparse.h"

template <typename T>
static T *to_device(const std::vector<T> &v)
{
    T *d = 0;
    if (hipMalloc((void **)&d, std::max<size_t>(v.size(), 1) * sizeof(T)) != hipSuccess) return 0;
    if (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return 0;
    return d;
}

template <typename T>
static std::vector<T> to_host(const T *d, size_t count)
{
    std::vector<T> v(count);
    if (count && hipMemcpy(v.data(), d, count * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) v.clear();
    return v;
}

static bool same_bits(const value_type *got, const value_type *ref, size_t count)
{
    return count == 0 || memcmp(got, ref, count * sizeof(value_type)) == 0;
}

// the rule of include/bhsparse_hip.h, "approximate inverse", row by row; every operation rounds by itself (the Makefile
// turns contraction off).  A's rows are ascending.  *bad_row: the smallest row with a pivot that is not > 0 and finite.
static std::vector<value_type> rule(int n, const std::vector<int> &Ap, const std::vector<int> &Aj, const std::vector<value_type> &Ax,
                                    const std::vector<int> &Gp, const std::vector<int> &Gj, int *bad_row)
{
    std::vector<value_type> G(Gj.size());
    *bad_row = -1;
    for (int i = 0; i < n; ++i) {
        const int a = Gp[i], d = Gp[i + 1] - a;
        std::vector<double> M((size_t)d * d, 0.0), t(d, 0.0), g(d, 0.0);
        for (int p = 0; p < d; ++p)
            for (int k = Ap[Gj[a + p]]; k < Ap[Gj[a + p] + 1] && Aj[k] <= Gj[a + p]; ++k)
                for (int q = 0; q <= p; ++q)
                    if (Gj[a + q] == Aj[k]) M[(size_t)p * d + q] = (double)Ax[k];
        bool bad = false;
        for (int c = 0; c < d; ++c) {
            const double mcc = M[(size_t)c * d + c];
            if (!(mcc > 0.0) || !std::isfinite(mcc)) bad = true;
            const double lcc = std::sqrt(mcc);
            M[(size_t)c * d + c] = lcc;
            for (int r = c + 1; r < d; ++r) M[(size_t)r * d + c] = M[(size_t)r * d + c] / lcc;
            for (int r = c + 1; r < d; ++r)
                for (int c2 = c + 1; c2 <= r; ++c2) {
                    const double prod = M[(size_t)r * d + c] * M[(size_t)c2 * d + c];
                    M[(size_t)r * d + c2] = M[(size_t)r * d + c2] - prod;
                }
        }
        t[d - 1] = 1.0;
        for (int q = d - 1; q >= 0; --q) {
            g[q] = t[q] / M[(size_t)q * d + q];
            for (int p = 0; p < q; ++p) {
                const double prod = M[(size_t)q * d + p] * g[q];
                t[p] = t[p] - prod;
            }
        }
        for (int p = 0; p < d; ++p) G[a + p] = (value_type)g[p];
        if (bad && *bad_row < 0) *bad_row = i;
    }
    return G;
}

int main()
{
    const int n = 48, band = 20;
    std::vector<int> Ap = {0}, Aj, Gp = {0}, Gj;
    std::vector<value_type> Ax;
    for (int i = 0; i < n; ++i) {
        double sum = 0.0;
        for (int j = std::max(0, i - band); j <= std::min(n - 1, i + band); ++j)
            if (j != i) sum += 1.0 / (1 + std::abs(i - j) + (i + j) % 3);
        for (int j = std::max(0, i - band); j <= std::min(n - 1, i + band); ++j) {
            Aj.push_back(j);
            Ax.push_back((value_type)(j == i ? sum + 1.0 : -1.0 / (1 + std::abs(i - j) + (i + j) % 3)));
            if (j <= i) Gj.push_back(j);
        }
        Ap.push_back((int)Aj.size());
        Gp.push_back((int)Gj.size());
    }
    const int nnzA = (int)Aj.size(), nnzG = (int)Gj.size();
    std::vector<value_type> G0(nnzG + 1, (value_type)NAN);
    G0[nnzG] = -7;                                                   // a guard behind the values

    bool plat[NUM_PLATFORMS] = {false};
    plat[BHSPARSE_HIP] = true;
    bhsparse bh;
    int err = bh.initPlatform(plat);
    if (err) { printf("initPlatform: %d\n", err); return 2; }
    int *dAp = to_device(Ap), *dAj = to_device(Aj), *dGp = to_device(Gp), *dGj = to_device(Gj);
    value_type *dAx = to_device(Ax), *dG = to_device(G0);
    if (!dAp || !dAj || !dGp || !dGj || !dAx || !dG) { printf("device memory\n"); return 2; }

    // G on the pattern of tril(A)
    int want_bad = 0, bad = 0;
    std::vector<value_type> ref = rule(n, Ap, Aj, Ax, Gp, Gj, &want_bad);
    err = bh.csr_fsai_device(n, nnzA, dAp, dAj, dAx, nnzG, dGp, dGj, dG, 0, &bad);
    std::vector<value_type> got = to_host(dG, nnzG + 1);
    if (err || got.empty() || !same_bits(got.data(), ref.data(), nnzG) || got[nnzG] != -7 || bad != -1 || want_bad != -1) {
        printf("G on tril(A): %d, bad row %d\n", err, bad);
        return 1;
    }
    // (G A G^T)_ii = 1
    for (int i = 0; i < n; ++i) {
        double s = 0.0;
        for (int p = Gp[i]; p < Gp[i + 1]; ++p)
            for (int k = Ap[Gj[p]]; k < Ap[Gj[p] + 1]; ++k)
                for (int q = Gp[i]; q < Gp[i + 1]; ++q)
                    if (Gj[q] == Aj[k]) s += (double)got[p] * (double)Ax[k] * (double)got[q];
        if (std::fabs(s - 1.0) > 1e-5) { printf("(G A G^T)_%d%d = %.17g\n", i, i, s); return 1; }
    }

    // a negated diagonal entry: reported, the rows above it untouched
    const int at = 30;
    std::vector<value_type> Bx(Ax);
    for (int k = Ap[at]; k < Ap[at + 1]; ++k)
        if (Aj[k] == at) Bx[k] = -Bx[k];
    value_type *dBx = to_device(Bx);
    if (!dBx) { printf("device memory\n"); return 2; }
    std::vector<value_type> ref2 = rule(n, Ap, Aj, Bx, Gp, Gj, &want_bad);
    err = bh.csr_fsai_device(n, nnzA, dAp, dAj, dBx, nnzG, dGp, dGj, dG, 0, &bad);
    got = to_host(dG, nnzG + 1);
    if (err || got.empty() || bad != at || want_bad != at || !same_bits(got.data(), ref.data(), Gp[at]) || got[nnzG] != -7) {
        printf("a negated diagonal entry: %d, bad row %d\n", err, bad);
        return 1;
    }
    for (int q = 0; q < nnzG; ++q)                                   // (which NaN a root returns is the machine's choice)
        if (ref2[q] == ref2[q] ? !same_bits(&got[q], &ref2[q], 1) : got[q] == got[q]) { printf("entry %d under the bad pivot\n", q); return 1; }

    // G's values overlapping A's: refused, nothing written; an unknown flag: refused
    if (bh.csr_fsai_device(n, nnzA, dAp, dAj, dAx, nnzG, dGp, dGj, dAx, 0, 0) != BHS_ERR_INVALID_ARG) { printf("valG overlapping valA\n"); return 1; }
    if (bh.csr_fsai_device(n, nnzA, dAp, dAj, dAx, nnzG, dGp, dGj, dG, 1, 0) != BHS_ERR_INVALID_ARG) { printf("unknown flag\n"); return 1; }
    std::vector<value_type> after = to_host(dG, nnzG + 1), ax = to_host(dAx, nnzA);
    if (after.empty() || !same_bits(after.data(), got.data(), nnzG + 1) || !same_bits(ax.data(), Ax.data(), nnzA)) { printf("a refused call wrote\n"); return 1; }

    for (void *p : {(void *)dAp, (void *)dAj, (void *)dGp, (void *)dGj, (void *)dAx, (void *)dBx, (void *)dG}) (void)hipFree(p);
    bh.freePlatform();
    printf("fsai %d rows, %d entries of G, rows of up to %d: PASS\n", n, nnzG, band + 1);
    return 0;
}
