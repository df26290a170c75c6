// Reductions and the diagonal scaling through the C++ facade (host/bhsparse.h): on a 5 x 7 matrix with a row that is not
// ascending and holds a duplicate diagonal pair, an empty row, a -0, a +0 and a NaN, the row sums, diag(X), the columns'
// entry counts, the number of entries and D^-1 X (in place) are formed on the device and compared with the results written
// out below.  Prints PASS and exits 0 on success.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
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

// the same bits, or both NaN
static bool same(const std::vector<value_type> &got, const std::vector<value_type> &ref)
{
    if (got.size() != ref.size()) return false;
    for (size_t i = 0; i < ref.size(); ++i) {
        if (std::isnan(ref[i]) ? !std::isnan(got[i]) : memcmp(&got[i], &ref[i], sizeof(value_type)) != 0) return false;
    }
    return true;
}

int main()
{
    const int m = 5, n = 7;
    const value_type nan = std::numeric_limits<value_type>::quiet_NaN();
    //                         row 0: (0,0) twice | row 1 empty | row 2    | row 3: (3,3) twice | row 4
    const std::vector<int> Xp = {0, 4, 4, 7, 10, 12};
    const std::vector<int> Xj = {5, 2, 0, 0, /**/ 1, 2, 6, /**/ 0, 3, 3, /**/ 6, 4};
    const std::vector<value_type> Xx = {1, 2, 3, 4, (value_type)-0.0, 0, 5, nan, 6, -7, 8, -9};
    const int nnz = (int)Xj.size();
    const std::vector<value_type> left = {2, 3, 4, 0.5, -1};
    const std::vector<value_type> refRows = {10, 0, 5, nan, -1}, refDiag = {7, 0, 0, -1, -9}, refCols = {3, 1, 2, 2, 1, 1, 2};
    // x / left[row] * -2
    const std::vector<value_type> refZ = {-1, -2, -3, -4, 0, (value_type)-0.0, -2.5, nan, -24, 28, 16, -18};

    bool plat[NUM_PLATFORMS] = {false};
    plat[BHSPARSE_HIP] = true;
    bhsparse bh;
    int err = bh.initPlatform(plat);
    if (err) { printf("initPlatform: %d\n", err); return 2; }
    int *dXp = to_device(Xp), *dXj = to_device(Xj);
    value_type *dXx = to_device(Xx), *dLeft = to_device(left);
    const std::vector<value_type> sentinel(n + 1, (value_type)-7);
    value_type *dOut = to_device(sentinel);
    if (!dXp || !dXj || !dXx || !dLeft || !dOut) { printf("device memory\n"); return 2; }

    err = bh.csr_reduce_device(m, n, nnz, dXx, dXp, dXj, BHS_AXIS_ROWS, BHS_RED_PLUS, 0, dOut);
    if (err || !same(to_host(dOut, m), refRows)) { printf("row sums: %d\n", err); return 1; }
    err = bh.csr_reduce_device(m, n, nnz, dXx, dXp, dXj, BHS_AXIS_DIAG, BHS_RED_PLUS, 0, dOut);
    if (err || !same(to_host(dOut, m), refDiag)) { printf("diag(X): %d\n", err); return 1; }
    err = bh.csr_reduce_device(m, n, nnz, 0, dXp, dXj, BHS_AXIS_COLS, BHS_RED_COUNT, 0, dOut);
    if (err || !same(to_host(dOut, n), refCols)) { printf("column counts: %d\n", err); return 1; }
    if (to_host(dOut, n + 1)[n] != (value_type)-7) { printf("written past the end of d_out\n"); return 1; }
    err = bh.csr_reduce_device(m, n, nnz, dXx, dXp, dXj, BHS_AXIS_ALL, BHS_RED_COUNT, 0, dOut);
    if (err || to_host(dOut, 1)[0] != (value_type)nnz) { printf("number of entries: %d\n", err); return 1; }

    // the diagonal has no off-diagonal part: refused, d_out stays as it is
    err = bh.csr_reduce_device(m, n, nnz, dXx, dXp, dXj, BHS_AXIS_DIAG, BHS_RED_PLUS, BHS_RED_OFFDIAG, dOut);
    if (err != BHS_ERR_INVALID_ARG || to_host(dOut, 1)[0] != (value_type)nnz) { printf("OFFDIAG with DIAG: %d\n", err); return 1; }

    err = bh.csr_scale_device(m, n, nnz, dXx, dXp, dXj, -2.0, dLeft, 0, BHS_SCALE_LEFT_DIV, dXx);
    if (err || !same(to_host(dXx, nnz), refZ)) { printf("D^-1 X in place: %d\n", err); return 1; }

    for (void *p : {(void *)dXp, (void *)dXj, (void *)dXx, (void *)dLeft, (void *)dOut}) (void)hipFree(p);
    bh.freePlatform();
    printf("reduce / scale %d x %d, %d entries: PASS\n", m, n, nnz);
    return 0;
}
