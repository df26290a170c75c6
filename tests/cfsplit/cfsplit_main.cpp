// C/F splitting and direct interpolation through the C++ facade (host/bhsparse.h): the 5-point operator on a 35 x 35 grid
// built here, every array on the device; the matrix's own pattern is the pattern of strong connections.  Checks that the C
// points are independent (no two are neighbours) and maximal (every F point has a C neighbour), that they are numbered in
// ascending order, that P has an identity row at every C point and ascending rows, and that the weights of an interior F row
// -- where the row of A sums to 0 -- sum to 1; prints the counts and exits 0 on success, non-zero on a status code or a wrong
// answer.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../benchmark_spgemm_using_csr_amd/host/bhsparse.h"

template <typename T>
static T *to_device(const std::vector<T> &v, size_t room)
{
    T *d = 0;
    if (hipMalloc((void **)&d, std::max<size_t>(room, 1) * sizeof(T)) != hipSuccess) return 0;
    if (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return 0;
    return d;
}

int main()
{
    const int nx = 35, ny = 35, n = nx * ny;
    std::vector<int> Ap(n + 1, 0), Aj;
    std::vector<value_type> Ax;
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            const int i = y * nx + x;
            if (y > 0) { Aj.push_back(i - nx); Ax.push_back(-1.0); }
            if (x > 0) { Aj.push_back(i - 1); Ax.push_back(-1.0); }
            Aj.push_back(i); Ax.push_back(4.0);
            if (x + 1 < nx) { Aj.push_back(i + 1); Ax.push_back(-1.0); }
            if (y + 1 < ny) { Aj.push_back(i + nx); Ax.push_back(-1.0); }
            Ap[i + 1] = (int)Aj.size();
        }
    const int nnz = (int)Aj.size();

    bool plat[NUM_PLATFORMS] = {false};
    plat[BHSPARSE_HIP] = true;
    bhsparse bh;
    int err = bh.initPlatform(plat);
    if (err) { printf("initPlatform: %d\n", err); return 2; }
    int *dAp = to_device(Ap, Ap.size()), *dAj = to_device(Aj, Aj.size());
    value_type *dAx = to_device(Ax, Ax.size());
    int *dCf = to_device(std::vector<int>(), (size_t)n), *dCpts = to_device(std::vector<int>(), (size_t)n);
    int *dPp = to_device(std::vector<int>(), (size_t)n + 1);
    if (!dAp || !dAj || !dAx || !dCf || !dCpts || !dPp) { printf("device memory\n"); return 2; }

    int nc = -1, rounds = -1;
    err = bh.csr_cfsplit_device(n, nnz, dAp, dAj, 0, 0u, BHS_CF_DEGREE, dCf, dCpts, &nc, &rounds);
    if (err) { printf("csr_cfsplit_device: %d\n", err); return 1; }
    if (nc < 1 || nc >= n || rounds < 1 || rounds > n) { printf("nc %d, rounds %d\n", nc, rounds); return 1; }
    std::vector<int> cf(n), cpts(nc);
    if (hipMemcpy(cf.data(), dCf, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(cpts.data(), dCpts, sizeof(int) * nc, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    int next = 0;
    for (int i = 0; i < n; ++i) {
        bool covered = cf[i] >= 0;
        if (cf[i] >= 0 && (cf[i] != next || cpts[next] != i)) { printf("C point %d: number %d, expected %d\n", i, cf[i], next); return 1; }
        if (cf[i] >= 0) ++next;
        if (cf[i] < -1) { printf("vertex %d: cf %d\n", i, cf[i]); return 1; }
        for (int q = Ap[i]; q < Ap[i + 1]; ++q) {
            const int j = Aj[q];
            if (j == i) continue;
            if (cf[i] >= 0 && cf[j] >= 0) { printf("C points %d and %d are neighbours\n", i, j); return 1; }
            if (cf[j] >= 0) covered = true;
        }
        if (!covered) { printf("F point %d has no C neighbour\n", i); return 1; }
    }
    if (next != nc) { printf("%d C points, expected %d\n", next, nc); return 1; }

    long long nnzP = -1;
    err = bh.csr_interp_symbolic_device(n, nnz, dAp, dAj, nnz, dAp, dAj, dCf, nc, dPp, &nnzP);
    if (err) { printf("csr_interp_symbolic_device: %d\n", err); return 1; }
    if (nnzP < n || nnzP > nnz) { printf("nnzP %lld\n", nnzP); return 1; }
    int *dPj = to_device(std::vector<int>(), (size_t)nnzP);
    value_type *dPx = to_device(std::vector<value_type>(), (size_t)nnzP);
    if (!dPj || !dPx) { printf("device memory\n"); return 2; }
    err = bh.csr_interp_numeric_device(n, nnz, dAp, dAj, dAx, nnz, dAp, dAj, dCf, nc, dPp, nnzP, dPj, dPx);
    if (err) { printf("csr_interp_numeric_device: %d\n", err); return 1; }
    std::vector<int> Pp(n + 1), Pj((size_t)nnzP);
    std::vector<value_type> Px((size_t)nnzP);
    if (hipMemcpy(Pp.data(), dPp, sizeof(int) * (n + 1), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(Pj.data(), dPj, sizeof(int) * (size_t)nnzP, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(Px.data(), dPx, sizeof(value_type) * (size_t)nnzP, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    if (Pp[0] != 0 || Pp[n] != nnzP) { printf("rowPtrP runs from %d to %d, nnzP %lld\n", Pp[0], Pp[n], nnzP); return 1; }
    int interior = 0;
    for (int i = 0; i < n; ++i) {
        const int len = Pp[i + 1] - Pp[i];
        if (cf[i] >= 0) {
            if (len != 1 || Pj[Pp[i]] != cf[i] || Px[Pp[i]] != (value_type)1) { printf("C point %d: no identity row\n", i); return 1; }
            continue;
        }
        double sum = 0.0;
        for (int q = Pp[i]; q < Pp[i + 1]; ++q) {
            if (Pj[q] < 0 || Pj[q] >= nc || (q > Pp[i] && Pj[q - 1] >= Pj[q])) { printf("row %d of P: column %d\n", i, Pj[q]); return 1; }
            sum += (double)Px[q];
        }
        const int x = i % nx, y = i / nx;
        if (x == 0 || y == 0 || x == nx - 1 || y == ny - 1) continue;
        ++interior;                                                   // the row of A sums to 0: the weights sum to 1
        if (len < 1 || std::fabs(sum - 1.0) > 1e-6) { printf("interior F point %d: %d weights that sum to %.9g\n", i, len, sum); return 1; }
    }
    // the splitting over its own list is refused, and so is a row pointer with another nnzP
    err = bh.csr_cfsplit_device(n, nnz, dAp, dAj, 0, 0u, 0, dCf, dCf, 0, 0);
    if (err != BHS_ERR_INVALID_ARG) { printf("d_cpts == d_cf: %d\n", err); return 1; }
    err = bh.csr_interp_numeric_device(n, nnz, dAp, dAj, dAx, nnz, dAp, dAj, dCf, nc, dPp, nnzP - 1, dPj, dPx);
    if (err != BHS_ERR_INVALID_ARG) { printf("nnzP - 1: %d\n", err); return 1; }

    for (void *p : {(void *)dAp, (void *)dAj, (void *)dAx, (void *)dCf, (void *)dCpts, (void *)dPp, (void *)dPj, (void *)dPx}) (void)hipFree(p);
    bh.freePlatform();
    printf("C/F splitting of %d vertices, %d entries: %d C points in %d rounds; P has %lld entries, %d interior F rows sum to 1 PASS\n", n,
           nnz, nc, rounds, nnzP, interior);
    return 0;
}
