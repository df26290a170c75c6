// The sampled dense-dense product through the C++ facade (host/bhsparse.h): on a 5 x 7 pattern with an empty row, a row
// that is not ascending and holds a pair twice, and a row of 40 entries (beyond the short bin), Z = X Y^T on the pattern
// with k = 5 (a tile of 8 whose tail is masked) and leading dimensions beyond k whose gap columns hold NaN, then in place
// on M's values Z = -1/2 (X Y^T) .* M + Z under BHS_SDDMM_TIMES_M, are formed on the device and compared bit for bit with a
// host loop written in the rule's order: T partial sums along k from +0, the adjacent-pair tree, the factors, one
// rounding.  Prints PASS and exits 0 on success.
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

static bool same_bits(const std::vector<value_type> &got, const std::vector<value_type> &ref)
{
    return got.size() == ref.size() && (ref.empty() || memcmp(got.data(), ref.data(), ref.size() * sizeof(value_type)) == 0);
}

// the rule of include/bhsparse_hip.h, "sampled dense-dense product", entry by entry; every operation rounds by itself
static std::vector<value_type> rule(const std::vector<int> &Mp, const std::vector<int> &Mj, const std::vector<value_type> *Mx, int k,
                                    double alpha, const std::vector<value_type> &X, long long ldX, const std::vector<value_type> &Y,
                                    long long ldY, double beta, const std::vector<value_type> &Zold)
{
#pragma STDC FP_CONTRACT OFF
    int T = 1;
    while (T < k && T < 64) T *= 2;
    std::vector<value_type> Z(Zold);
    for (size_t i = 0; i + 1 < Mp.size(); ++i)
        for (int q = Mp[i]; q < Mp[i + 1]; ++q) {
            std::vector<double> s(T, 0.0);
            for (int t0 = 0; t0 < k; t0 += T)
                for (int l = 0; l < T && t0 + l < k; ++l) {
                    const double p = (double)X[i * ldX + t0 + l] * (double)Y[Mj[q] * ldY + t0 + l];
                    s[l] = s[l] + p;
                }
            for (int w = 1; w < T; w *= 2)
                for (int l = 0; l < T; l += 2 * w) s[l] = s[l] + s[l + w];
            double v = s[0];
            if (Mx) v = v * (double)(*Mx)[q];
            double t = alpha * v;
            if (beta != 0.0) {
                const double bz = beta * (double)Zold[q];
                t = t + bz;
            }
            Z[q] = (value_type)t;
        }
    return Z;
}

int main()
{
    const int m = 5, n = 7, k = 5;
    const long long ldX = 7, ldY = 6;
    std::vector<int> Mp = {0}, Mj;
    for (int j : {6, 0, 3, 0}) Mj.push_back(j);                      // row 0: not ascending, (0, 0) twice
    Mp.push_back((int)Mj.size());
    Mp.push_back((int)Mj.size());                                    // row 1: empty
    for (int q = 0; q < 40; ++q) Mj.push_back((q * 3) % n);           // row 2: 40 entries, a wave's
    Mp.push_back((int)Mj.size());
    for (int j = 0; j < n; ++j) Mj.push_back(j);                     // row 3: full
    Mp.push_back((int)Mj.size());
    Mj.push_back(4);                                                 // row 4: one entry
    Mp.push_back((int)Mj.size());
    const int nnz = (int)Mj.size();
    unsigned state = 12345u;
    auto next = [&]() { state = state * 1664525u + 1013904223u; return (value_type)((double)(state >> 8) / 16777216.0 * 2.0 - 1.0) / (value_type)3; };
    std::vector<value_type> X((size_t)m * ldX, (value_type)NAN), Y((size_t)n * ldY, (value_type)NAN), Mx(nnz + 1), Z0(nnz + 1, (value_type)NAN);
    for (int i = 0; i < m; ++i)
        for (int c = 0; c < k; ++c) X[i * ldX + c] = next();
    for (int j = 0; j < n; ++j)
        for (int c = 0; c < k; ++c) Y[j * ldY + c] = next();
    for (int q = 0; q < nnz; ++q) Mx[q] = next();
    Mx[nnz] = -7; Z0[nnz] = -7;                                      // guards behind the entries

    bool plat[NUM_PLATFORMS] = {false};
    plat[BHSPARSE_HIP] = true;
    bhsparse bh;
    int err = bh.initPlatform(plat);
    if (err) { printf("initPlatform: %d\n", err); return 2; }
    int *dMp = to_device(Mp), *dMj = to_device(Mj);
    value_type *dX = to_device(X), *dY = to_device(Y), *dMx = to_device(Mx), *dZ = to_device(Z0);
    if (!dMp || !dMj || !dX || !dY || !dMx || !dZ) { printf("device memory\n"); return 2; }

    // Z = X Y^T on the pattern: beta == 0 over a Z of NaN, no values of M
    std::vector<value_type> ref = rule(Mp, Mj, 0, k, 1.0, X, ldX, Y, ldY, 0.0, Z0);
    err = bh.csr_sddmm_device(m, n, nnz, 0, dMp, dMj, k, 1.0, dX, ldX, dY, ldY, 0.0, dZ, 0);
    if (err || !same_bits(to_host(dZ, nnz + 1), ref)) { printf("Z = X Y^T on the pattern: %d\n", err); return 1; }
    for (int q = 0; q < nnz; ++q)
        if (!(ref[q] == ref[q])) { printf("a gap column was read\n"); return 1; }
    if (ref[1] != ref[3]) { printf("the pair stored twice\n"); return 1; }

    // in place on M's values: M <- -1/2 (X Y^T) .* M + M
    ref = rule(Mp, Mj, &Mx, k, -0.5, X, ldX, Y, ldY, 1.0, Mx);
    err = bh.csr_sddmm_device(m, n, nnz, dMx, dMp, dMj, k, -0.5, dX, ldX, dY, ldY, 1.0, dMx, BHS_SDDMM_TIMES_M);
    if (err || !same_bits(to_host(dMx, nnz + 1), ref)) { printf("in place under TIMES_M: %d\n", err); return 1; }

    // Z overlapping Y: refused, nothing written; an unknown flag: refused
    if (bh.csr_sddmm_device(m, n, nnz, 0, dMp, dMj, k, 1.0, dX, ldX, dY, ldY, 0.0, dY, 0) != BHS_ERR_INVALID_ARG) { printf("Z overlapping Y\n"); return 1; }
    if (bh.csr_sddmm_device(m, n, nnz, dMx, dMp, dMj, k, 1.0, dX, ldX, dY, ldY, 0.0, dZ, 2u) != BHS_ERR_INVALID_ARG) { printf("unknown flag\n"); return 1; }
    if (!same_bits(to_host(dMx, nnz + 1), ref)) { printf("a refused call wrote\n"); return 1; }

    for (void *p : {(void *)dMp, (void *)dMj, (void *)dX, (void *)dY, (void *)dMx, (void *)dZ}) (void)hipFree(p);
    bh.freePlatform();
    printf("sddmm %d x %d, %d entries, k = %d: PASS\n", m, n, nnz, k);
    return 0;
}
