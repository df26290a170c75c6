// CSR x dense through the C++ facade (host/bhsparse.h): on a 5 x 7 matrix with a row that is not ascending and holds a
// duplicate pair, an empty row, a -0 and a +0, y = A x, the residual b - A x and Y = 2 A X - Y for three columns of a
// four-column array are formed on the device and compared with the results written out below (small integers: exact in
// both builds).  Prints PASS and exits 0 on success.
#include <algorithm>
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

// equal as numbers (the sign of a zero result is not specified)
static bool same(const std::vector<value_type> &got, const std::vector<value_type> &ref)
{
    if (got.size() != ref.size()) return false;
    for (size_t i = 0; i < ref.size(); ++i)
        if (!(got[i] == ref[i])) return false;
    return true;
}

int main()
{
    const int m = 5, n = 7, k = 3, ld = 4;
    //                         row 0: (0,0) twice | row 1 empty | row 2    | row 3: (3,3) twice | row 4
    const std::vector<int> Ap = {0, 4, 4, 7, 10, 12};
    const std::vector<int> Aj = {5, 2, 0, 0, /**/ 1, 2, 6, /**/ 0, 3, 3, /**/ 6, 4};
    const std::vector<value_type> Ax = {1, 2, 3, 4, (value_type)-0.0, 0, 5, 2, 6, -7, 8, -9};
    const int nnz = (int)Aj.size();
    const std::vector<value_type> x = {1, 2, 3, 4, 5, 6, 7};
    const std::vector<value_type> b = {19, 1, 35, -2, 12};
    const std::vector<value_type> refY = {19, 0, 35, -2, 11}, refR = {0, 1, 0, 0, 1};
    // X: 7 x 3 in an array of leading dimension 4 (the gap column holds a value that must never reach a result); column c
    // is (c + 1) * x
    std::vector<value_type> X(n * ld, (value_type)1e30), Y(m * ld, (value_type)-7), refYY(m * ld, (value_type)-7);
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < k; ++c) X[i * ld + c] = (c + 1) * x[i];
    for (int i = 0; i < m; ++i)
        for (int c = 0; c < k; ++c) {
            Y[i * ld + c] = (value_type)(i + c);
            refYY[i * ld + c] = 2 * (c + 1) * refY[i] - (value_type)(i + c);
        }

    bool plat[NUM_PLATFORMS] = {false};
    plat[BHSPARSE_HIP] = true;
    bhsparse bh;
    int err = bh.initPlatform(plat);
    if (err) { printf("initPlatform: %d\n", err); return 2; }
    int *dAp = to_device(Ap), *dAj = to_device(Aj);
    value_type *dAx = to_device(Ax), *dx = to_device(x), *dX = to_device(X), *dY = to_device(Y);
    const std::vector<value_type> sentinel(m + 1, (value_type)-7);
    value_type *dy = to_device(sentinel);
    if (!dAp || !dAj || !dAx || !dx || !dX || !dY || !dy) { printf("device memory\n"); return 2; }

    err = bh.csr_spmv_device(m, n, nnz, dAx, dAp, dAj, 1.0, dx, 0.0, dy);
    if (err || !same(to_host(dy, m), refY)) { printf("y = A x: %d\n", err); return 1; }
    if (to_host(dy, m + 1)[m] != (value_type)-7) { printf("written past the end of d_y\n"); return 1; }
    if (hipMemcpy(dy, b.data(), m * sizeof(value_type), hipMemcpyHostToDevice) != hipSuccess) return 2;
    err = bh.csr_spmv_device(m, n, nnz, dAx, dAp, dAj, -1.0, dx, 1.0, dy);
    if (err || !same(to_host(dy, m), refR)) { printf("b - A x: %d\n", err); return 1; }
    err = bh.csr_spmm_device(m, n, nnz, dAx, dAp, dAj, k, 2.0, dX, ld, -1.0, dY, ld);
    if (err || !same(to_host(dY, (size_t)m * ld), refYY)) { printf("Y = 2 A X - Y: %d\n", err); return 1; }

    // y overlapping x: refused, d_y stays as it is
    err = bh.csr_spmv_device(n, n, 0, dAx, dAp, dAj, 1.0, dx, 0.0, dx);
    if (err != BHS_ERR_INVALID_ARG) { printf("y overlapping x: %d\n", err); return 1; }

    for (void *p : {(void *)dAp, (void *)dAj, (void *)dAx, (void *)dx, (void *)dX, (void *)dY, (void *)dy}) (void)hipFree(p);
    bh.freePlatform();
    printf("spmv / spmm %d x %d, %d entries: PASS\n", m, n, nnz);
    return 0;
}
