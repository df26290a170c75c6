// Level sets, ILU(0) and the two triangular solves through the C++ facade (host/bhsparse.h): poisson5pt 33 x 33 (gallery.h;
// diagonal 4, -1 beside it), every array on the device.  Checks the levels of both triangles against the definition, row
// by row on the host (the lower triangle of the five-point stencil has nx + ny - 1 of them), factorises a copy of the
// values in place and compares L and U with the same elimination on the host, then solves L U x = b for b = A 1 with the
// unit lower and the upper solve in place and checks x against the host's substitution; prints the levels and exits 0 on
// success, non-zero on a status code or a wrong answer.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../benchmark_spgemm_using_csr_amd/host/bhsparse.h"
#include "../../benchmark_spgemm_using_csr_amd/host/gallery.h"

template <typename T>
static T *to_device(const std::vector<T> &v, size_t room)
{
    T *d = 0;
    if (hipMalloc((void **)&d, std::max<size_t>(room, 1) * sizeof(T)) != hipSuccess) return 0;
    if (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return 0;
    return d;
}

static std::vector<int> host_levels(const CsrHost &A, bool upper)
{
    const int n = A.num_rows;
    std::vector<int> level(n, 0);
    for (int t = 0; t < n; ++t) {
        const int i = upper ? n - 1 - t : t;
        for (int q = A.row_offsets[i]; q < A.row_offsets[i + 1]; ++q) {
            const int j = A.column_indices[q];
            if (upper ? j > i : j < i) level[i] = std::max(level[i], level[j] + 1);
        }
    }
    return level;
}

int main()
{
    CsrHost A;
    const int nx = 33, ny = 33;
    if (!gallery_poisson("poisson5pt", nx, ny, 1, A)) { printf("gallery\n"); return 2; }
    const int n = A.num_rows, nnz = A.num_entries;
    std::vector<value_type> val(nnz), b(n, (value_type)0);
    for (int i = 0; i < n; ++i)
        for (int q = A.row_offsets[i]; q < A.row_offsets[i + 1]; ++q) {
            val[q] = A.column_indices[q] == i ? (value_type)4 : (value_type)-1;
            b[i] += val[q];                                          // b = A 1
        }

    bool plat[NUM_PLATFORMS] = {false};
    plat[BHSPARSE_HIP] = true;
    bhsparse bh;
    int err = bh.initPlatform(plat);
    if (err) { printf("initPlatform: %d\n", err); return 2; }
    int *dAp = to_device(A.row_offsets, A.row_offsets.size()), *dAj = to_device(A.column_indices, A.column_indices.size());
    int *dLevel = to_device(std::vector<int>(), (size_t)n), *dPtr = to_device(std::vector<int>(), (size_t)n + 1);
    int *dOrder[2] = {to_device(std::vector<int>(), (size_t)n), to_device(std::vector<int>(), (size_t)n)};
    value_type *dVal = to_device(val, val.size()), *dX = to_device(b, b.size());
    if (!dAp || !dAj || !dLevel || !dPtr || !dOrder[0] || !dOrder[1] || !dVal || !dX) { printf("device memory\n"); return 2; }

    std::vector<int> ptr[2];
    int nlevels[2] = {-1, -1};
    for (int upper = 0; upper < 2; ++upper) {
        int passes = -1;
        err = bh.csr_levels_device(n, nnz, dAp, dAj, upper ? BHS_TRI_UPPER : BHS_TRI_LOWER, dLevel, dOrder[upper], dPtr, &nlevels[upper],
                                   &passes);
        if (err) { printf("csr_levels_device: %d\n", err); return 1; }
        if (nlevels[upper] != nx + ny - 1 || passes < 1) { printf("nlevels %d, passes %d\n", nlevels[upper], passes); return 1; }
        std::vector<int> level(n), order(n);
        ptr[upper].resize(nlevels[upper] + 1);
        if (hipMemcpy(level.data(), dLevel, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(order.data(), dOrder[upper], sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(ptr[upper].data(), dPtr, sizeof(int) * (nlevels[upper] + 1), hipMemcpyDeviceToHost) != hipSuccess) return 2;
        if (level != host_levels(A, upper != 0)) { printf("levels, upper %d\n", upper); return 1; }
        if (ptr[upper][0] != 0 || ptr[upper][nlevels[upper]] != n) { printf("levelPtr ends\n"); return 1; }
        for (int l = 0; l < nlevels[upper]; ++l)
            for (int k = ptr[upper][l]; k < ptr[upper][l + 1]; ++k) {
                const int v = order[k];
                if (v < 0 || v >= n || level[v] != l || (k > ptr[upper][l] && v <= order[k - 1])) { printf("order[%d] = %d\n", k, v); return 1; }
            }
    }

    // ILU(0) on the host, in the value type with double intermediates, row by row
    std::vector<value_type> lu(val);
    for (int i = 0; i < n; ++i)
        for (int q = A.row_offsets[i]; q < A.row_offsets[i + 1] && A.column_indices[q] < i; ++q) {
            const int k = A.column_indices[q];
            int kd = A.row_offsets[k];
            while (A.column_indices[kd] != k) ++kd;
            lu[q] = (value_type)((double)lu[q] / (double)lu[kd]);
            for (int p = kd + 1; p < A.row_offsets[k + 1]; ++p)
                for (int r = q + 1; r < A.row_offsets[i + 1]; ++r)
                    if (A.column_indices[r] == A.column_indices[p]) lu[r] = (value_type)((double)lu[r] - (double)lu[q] * (double)lu[p]);
        }
    int pivot = 0;
    err = bh.csr_ilu0_device(n, nnz, dAp, dAj, dVal, nlevels[0], ptr[0].data(), dOrder[0], 0, &pivot);
    if (err || pivot != -1) { printf("csr_ilu0_device: %d, pivot %d\n", err, pivot); return 1; }
    std::vector<value_type> got(nnz);
    if (hipMemcpy(got.data(), dVal, sizeof(value_type) * nnz, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    // the two differ only where the compiler fuses a multiply and a subtraction: a rounding of the value type an update,
    // at most two updates an entry on this stencil
    const double u = sizeof(value_type) == 8 ? 1.2e-16 : 6.0e-8;
    for (int q = 0; q < nnz; ++q)
        if (!(std::fabs((double)got[q] - (double)lu[q]) <= 16.0 * u * 4.0)) { printf("lu[%d] = %.17g, on the host %.17g\n", q, (double)got[q], (double)lu[q]); return 1; }

    // L y = b (unit diagonal), U x = y, in place on dX; the same substitutions on the host in double
    err = bh.csr_trsv_device(n, nnz, dAp, dAj, dVal, nlevels[0], ptr[0].data(), dOrder[0], 1.0, dX, dX, BHS_TRI_LOWER | BHS_TRI_UNIT_DIAG);
    if (err) { printf("csr_trsv_device, lower: %d\n", err); return 1; }
    err = bh.csr_trsv_device(n, nnz, dAp, dAj, dVal, nlevels[1], ptr[1].data(), dOrder[1], 1.0, dX, dX, BHS_TRI_UPPER);
    if (err) { printf("csr_trsv_device, upper: %d\n", err); return 1; }
    std::vector<value_type> x(n);
    if (hipMemcpy(x.data(), dX, sizeof(value_type) * n, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    std::vector<double> ref(b.begin(), b.end());
    for (int i = 0; i < n; ++i)
        for (int q = A.row_offsets[i]; q < A.row_offsets[i + 1]; ++q)
            if (A.column_indices[q] < i) ref[i] -= (double)got[q] * ref[A.column_indices[q]];
    for (int i = n - 1; i >= 0; --i) {
        double d = 1.0;
        for (int q = A.row_offsets[i]; q < A.row_offsets[i + 1]; ++q) {
            if (A.column_indices[q] > i) ref[i] -= (double)got[q] * ref[A.column_indices[q]];
            if (A.column_indices[q] == i) d = (double)got[q];
        }
        ref[i] /= d;
    }
    // 2 (nx + ny - 1) levels, each a row of at most 3 products and 3 more roundings on numbers below 4; L and U of this
    // M-matrix are diagonally dominant, so what a level commits is not amplified by the ones behind it
    const double tol = 2.0 * (nx + ny - 1) * 6.0 * 4.0 * u;
    for (int i = 0; i < n; ++i)
        if (!(std::fabs((double)x[i] - ref[i]) <= tol)) { printf("x[%d] = %.17g, on the host %.17g\n", i, (double)x[i], ref[i]); return 1; }
    // both triangles at once are refused
    err = bh.csr_trsv_device(n, nnz, dAp, dAj, dVal, nlevels[0], ptr[0].data(), dOrder[0], 1.0, dX, dX, BHS_TRI_LOWER | BHS_TRI_UPPER);
    if (err != BHS_ERR_INVALID_ARG) { printf("both triangles: %d\n", err); return 1; }

    for (void *p : {(void *)dAp, (void *)dAj, (void *)dLevel, (void *)dPtr, (void *)dOrder[0], (void *)dOrder[1], (void *)dVal, (void *)dX})
        (void)hipFree(p);
    bh.freePlatform();
    printf("trsv poisson5pt 33x33: levels %d and %d PASS\n", nlevels[0], nlevels[1]);
    return 0;
}
