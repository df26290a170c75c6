// Colouring and Gauss-Seidel through the C++ facade (host/bhsparse.h): poisson5pt 33 x 33 (gallery.h; diagonal 4, -1 beside
// it) coloured with the hashed priorities of seed 0 (or of the seed given as the first argument), then symmetric
// Gauss-Seidel sweeps on A x = b for b = A 1 from x = 0, every array on the device.  Checks what the contract promises of any
// result -- colours in range and proper, the order sorted by (colour, index), the offsets consistent -- and that two verified
// symmetric sweeps give what the same sweeps give on the host, colour by colour in the device's order, and a smaller
// residual; prints the colours and the rounds, and exits 0 on success, non-zero on a status code or a wrong answer.
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

static double residual(const CsrHost &A, const std::vector<value_type> &val, const std::vector<value_type> &b,
                       const std::vector<value_type> &x)
{
    double sq = 0;
    for (int i = 0; i < A.num_rows; ++i) {
        double r = b[i];
        for (int q = A.row_offsets[i]; q < A.row_offsets[i + 1]; ++q) r -= (double)val[q] * (double)x[A.column_indices[q]];
        sq += r * r;
    }
    return std::sqrt(sq);
}

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)strtoul(argv[1], 0, 10) : 0u;
    CsrHost A;
    if (!gallery_poisson("poisson5pt", 33, 33, 1, A)) { printf("gallery\n"); return 2; }
    const int n = A.num_rows, nnz = A.num_entries;
    std::vector<value_type> val(nnz), diag(n, (value_type)4), b(n, (value_type)0), x(n, (value_type)0);
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
    int *dColor = to_device(std::vector<int>(), (size_t)n), *dOrder = to_device(std::vector<int>(), (size_t)n);
    int *dPtr = to_device(std::vector<int>(), (size_t)n + 1);
    value_type *dVal = to_device(val, val.size()), *dDiag = to_device(diag, diag.size());
    value_type *dB = to_device(b, b.size()), *dX = to_device(x, x.size());
    if (!dAp || !dAj || !dColor || !dOrder || !dPtr || !dVal || !dDiag || !dB || !dX) { printf("device memory\n"); return 2; }

    int ncolors = -1, rounds = -1;
    err = bh.csr_color_device(n, nnz, dAp, dAj, 0, seed, 0, dColor, dOrder, dPtr, &ncolors, &rounds);
    if (err) { printf("csr_color_device: %d\n", err); return 1; }
    if (ncolors < 2 || ncolors > 5 || rounds < 1) { printf("ncolors %d, rounds %d\n", ncolors, rounds); return 1; }   // (first fit: at most degree + 1)
    std::vector<int> color(n), order(n), ptr(ncolors + 1);
    if (hipMemcpy(color.data(), dColor, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(order.data(), dOrder, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(ptr.data(), dPtr, sizeof(int) * (ncolors + 1), hipMemcpyDeviceToHost) != hipSuccess) return 2;
    for (int i = 0; i < n; ++i) {
        if (color[i] < 0 || color[i] >= ncolors) { printf("color[%d] = %d\n", i, color[i]); return 1; }
        for (int q = A.row_offsets[i]; q < A.row_offsets[i + 1]; ++q) {
            const int j = A.column_indices[q];
            if (j != i && color[j] == color[i]) { printf("vertices %d and %d share colour %d\n", i, j, color[i]); return 1; }
        }
    }
    if (ptr[0] != 0 || ptr[ncolors] != n) { printf("colorPtr ends %d .. %d\n", ptr[0], ptr[ncolors]); return 1; }
    for (int c = 0; c < ncolors; ++c)
        for (int k = ptr[c]; k < ptr[c + 1]; ++k) {
            const int v = order[k];
            if (v < 0 || v >= n || color[v] != c || (k > ptr[c] && v <= order[k - 1])) { printf("order[%d] = %d\n", k, v); return 1; }
        }

    const double r0 = residual(A, val, b, x);
    err = bh.csr_gs_device(n, nnz, dAp, dAj, dVal, dDiag, ncolors, ptr.data(), dOrder, dColor, dB, dX, 1.0, 2,
                           BHS_GS_SYMMETRIC | BHS_GS_VERIFY);
    if (err) { printf("csr_gs_device: %d\n", err); return 1; }
    if (hipMemcpy(x.data(), dX, sizeof(value_type) * n, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    std::vector<double> ref(n, 0.0);                                 // the same sweeps on the host, in double
    for (int pass = 0; pass < 4; ++pass)
        for (int t = 0; t < ncolors; ++t) {
            const int c = (pass & 1) ? ncolors - 1 - t : t;
            for (int k = ptr[c]; k < ptr[c + 1]; ++k) {
                const int i = order[k];
                double sum = 0;
                for (int q = A.row_offsets[i]; q < A.row_offsets[i + 1]; ++q)
                    if (A.column_indices[q] != i) sum += (double)val[q] * ref[A.column_indices[q]];
                ref[i] = ((double)b[i] - sum) / (double)diag[i];
            }
        }
    // 4 * ncolors steps, each an update of at most 5 + 4 roundings of the value type on numbers below 2, none amplified
    // (the matrix is weakly diagonally dominant)
    const double tol = 4.0 * ncolors * 9.0 * 2.0 * (sizeof(value_type) == 8 ? 1.2e-16 : 6.0e-8);
    for (int i = 0; i < n; ++i)
        if (!(std::fabs((double)x[i] - ref[i]) <= tol)) { printf("x[%d] = %.17g, on the host %.17g\n", i, (double)x[i], ref[i]); return 1; }
    const double r1 = residual(A, val, b, x);
    if (!(r1 < r0)) { printf("residual %g -> %g\n", r0, r1); return 1; }
    // no direction is refused
    err = bh.csr_gs_device(n, nnz, dAp, dAj, dVal, dDiag, ncolors, ptr.data(), dOrder, dColor, dB, dX, 1.0, 1, 0);
    if (err != BHS_ERR_INVALID_ARG) { printf("flags = 0: %d\n", err); return 1; }

    for (void *p : {(void *)dAp, (void *)dAj, (void *)dColor, (void *)dOrder, (void *)dPtr, (void *)dVal, (void *)dDiag, (void *)dB,
                    (void *)dX})
        (void)hipFree(p);
    bh.freePlatform();
    printf("gs poisson5pt 33x33 seed %u: ncolors %d rounds %d PASS\n", seed, ncolors, rounds);
    return 0;
}
