// Relaxation and the fused product through the C++ facade (host/bhsparse.h): on the 1-D Laplacian of 6 unknowns with a row
// that is not ascending, two Jacobi sweeps (a = 0, c = 1/2) in one call from x = 0 under BHS_RELAX_ZERO_GUESS -- x holds
// NaN on entry --, then a step that carries d (a = 1/2, c = 1), then r = b - A x with r.r and b.r, are formed on the
// device and compared with the results written out below (dyadic numbers: exact in both builds).  Prints PASS and exits 0
// on success.
#include <algorithm>
#include <cmath>
#include <cstdio>
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

static bool same(const std::vector<value_type> &got, const std::vector<double> &ref)
{
    if (got.size() != ref.size()) return false;
    for (size_t i = 0; i < ref.size(); ++i)
        if (!((double)got[i] == ref[i])) return false;
    return true;
}

int main()
{
    const int n = 6;
    std::vector<int> Ap = {0}, Aj;
    std::vector<value_type> Ax;
    for (int i = 0; i < n; ++i) {                                   // row i: (i + 1, -1), (i, 2), (i - 1, -1): descending
        if (i + 1 < n) { Aj.push_back(i + 1); Ax.push_back(-1); }
        Aj.push_back(i); Ax.push_back(2);
        if (i > 0) { Aj.push_back(i - 1); Ax.push_back(-1); }
        Ap.push_back((int)Aj.size());
    }
    const int nnz = (int)Aj.size();
    const std::vector<value_type> diag(n, 2), b = {4, 0, 8, 0, 0, 4};
    // the host's restatement, in double: dyadic numbers throughout
    auto residual = [&](const std::vector<double> &x) {
        std::vector<double> r(n);
        for (int i = 0; i < n; ++i) r[i] = b[i] - (2 * x[i] - (i ? x[i - 1] : 0) - (i + 1 < n ? x[i + 1] : 0));
        return r;
    };
    std::vector<double> x(n, 0.0), d(n, 0.0);
    const double coefJ[4] = {0, 0.5, 0, 0.5}, coefD[2] = {0.5, 1};
    for (int s = 0; s < 2; ++s) {
        const std::vector<double> r = residual(x);
        for (int i = 0; i < n; ++i) { d[i] = 0.5 * (r[i] / 2); x[i] += d[i]; }
    }
    const std::vector<double> x2 = x, d2 = d;
    {
        const std::vector<double> r = residual(x);
        for (int i = 0; i < n; ++i) { d[i] = 1 * (r[i] / 2) + 0.5 * d[i]; x[i] += d[i]; }
    }
    const std::vector<double> r3 = residual(x);
    double rr = 0, br = 0;
    for (int i = 0; i < n; ++i) { rr += r3[i] * r3[i]; br += b[i] * r3[i]; }

    bool plat[NUM_PLATFORMS] = {false};
    plat[BHSPARSE_HIP] = true;
    bhsparse bh;
    int err = bh.initPlatform(plat);
    if (err) { printf("initPlatform: %d\n", err); return 2; }
    int *dAp = to_device(Ap), *dAj = to_device(Aj);
    std::vector<value_type> xin(n + 1, (value_type)NAN), din(n + 1, (value_type)-7), zin(n + 1, (value_type)-7);
    xin[n] = -7;
    value_type *dAx = to_device(Ax), *ddiag = to_device(diag), *db = to_device(b), *dx = to_device(xin), *dd = to_device(din),
               *dz = to_device(zin);
    if (!dAp || !dAj || !dAx || !ddiag || !db || !dx || !dd || !dz) { printf("device memory\n"); return 2; }

    err = bh.csr_relax_device(n, nnz, dAx, dAp, dAj, ddiag, 2, coefJ, db, dx, dd, BHS_RELAX_ZERO_GUESS);
    if (err || !same(to_host(dx, n), x2) || !same(to_host(dd, n), d2)) { printf("two Jacobi sweeps from zero: %d\n", err); return 1; }
    err = bh.csr_relax_device(n, nnz, dAx, dAp, dAj, ddiag, 1, coefD, db, dx, dd, 0);
    if (err || !same(to_host(dx, n), x) || !same(to_host(dd, n), d)) { printf("a step that carries d: %d\n", err); return 1; }
    if (to_host(dx, n + 1)[n] != (value_type)-7 || to_host(dd, n + 1)[n] != (value_type)-7) { printf("written past the end\n"); return 1; }
    double dots[2] = {-1, -1};
    err = bh.csr_spmv_dots_device(n, n, nnz, dAx, dAp, dAj, -1.0, dx, 1.0, db, dz, db, dots);
    if (err || !same(to_host(dz, n), r3) || dots[0] != rr || dots[1] != br) { printf("r = b - A x with its dots: %d %g %g\n", err, dots[0], dots[1]); return 1; }
    if (to_host(dz, n + 1)[n] != (value_type)-7) { printf("written past the end of d_z\n"); return 1; }

    // x overlapping b: refused, nothing written; a NULL d_d with a != 0: refused
    if (bh.csr_relax_device(n, nnz, dAx, dAp, dAj, ddiag, 1, coefD, dx, dx, dd, 0) != BHS_ERR_INVALID_ARG) { printf("x overlapping b\n"); return 1; }
    if (bh.csr_relax_device(n, nnz, dAx, dAp, dAj, ddiag, 1, coefD, db, dx, 0, 0) != BHS_ERR_INVALID_ARG) { printf("NULL d_d\n"); return 1; }
    double coef[4];
    if (bhsparse::chebyshev_coefficients(0.5, 1.5, 2, coef) || coef[0] != 0 || coef[1] != 1.0) { printf("chebyshev_coefficients\n"); return 1; }
    if (bhsparse::chebyshev_coefficients(1.5, 0.5, 2, coef) != BHS_ERR_INVALID_ARG) { printf("chebyshev_coefficients refusal\n"); return 1; }

    for (void *p : {(void *)dAp, (void *)dAj, (void *)dAx, (void *)ddiag, (void *)db, (void *)dx, (void *)dd, (void *)dz}) (void)hipFree(p);
    bh.freePlatform();
    printf("relax / spmv_dots %d x %d, %d entries: PASS\n", n, n, nnz);
    return 0;
}
