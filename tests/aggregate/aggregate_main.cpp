// Aggregation through the C++ facade (host/bhsparse.h): the MIS(2) aggregates of poisson5pt 33 x 33 (gallery.h) with the
// hashed priorities of seed 0 (or of the seed given as the first argument), every array on the device.  Checks what the
// contract promises of any result -- roots ascending, agg[roots[a]] == a, every aggregate number in range, every vertex
// within two steps of its root -- prints nagg and rounds, and exits 0 on success, non-zero on a status code or a wrong answer.
#include <algorithm>
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

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)strtoul(argv[1], 0, 10) : 0u;
    CsrHost S;
    if (!gallery_poisson("poisson5pt", 33, 33, 1, S)) { printf("gallery\n"); return 2; }
    const int n = S.num_rows, nnz = S.num_entries;

    bool plat[NUM_PLATFORMS] = {false};
    plat[BHSPARSE_HIP] = true;
    bhsparse bh;
    int err = bh.initPlatform(plat);
    if (err) { printf("initPlatform: %d\n", err); return 2; }
    int *dSp = to_device(S.row_offsets, S.row_offsets.size()), *dSj = to_device(S.column_indices, S.column_indices.size());
    int *dAgg = to_device(std::vector<int>(), (size_t)n), *dRoots = to_device(std::vector<int>(), (size_t)n);
    if (!dSp || !dSj || !dAgg || !dRoots) { printf("device memory\n"); return 2; }

    int nagg = -1, rounds = -1;
    err = bh.csr_aggregate_device(n, nnz, dSp, dSj, 0, seed, 0, dAgg, dRoots, &nagg, &rounds);
    if (err) { printf("csr_aggregate_device: %d\n", err); return 1; }
    if (nagg < 1 || nagg > n || rounds < 1) { printf("nagg %d, rounds %d\n", nagg, rounds); return 1; }
    std::vector<int> agg(n), roots(nagg);
    if (hipMemcpy(agg.data(), dAgg, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(roots.data(), dRoots, sizeof(int) * nagg, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    for (int a = 0; a < nagg; ++a) {
        if (roots[a] < 0 || roots[a] >= n || (a > 0 && roots[a] <= roots[a - 1])) { printf("root %d: %d\n", a, roots[a]); return 1; }
        if (agg[roots[a]] != a) { printf("agg[roots[%d]] = %d\n", a, agg[roots[a]]); return 1; }
    }
    for (int i = 0; i < n; ++i) {
        if (agg[i] < 0 || agg[i] >= nagg) { printf("agg[%d] = %d\n", i, agg[i]); return 1; }
        const int r = roots[agg[i]];
        bool near = r == i;
        for (int q = S.row_offsets[i]; q < S.row_offsets[i + 1] && !near; ++q) {
            const int j = S.column_indices[q];
            near = j == r;
            for (int p = S.row_offsets[j]; p < S.row_offsets[j + 1] && !near; ++p) near = S.column_indices[p] == r;
        }
        if (!near) { printf("vertex %d is beyond two steps of its root %d\n", i, r); return 1; }
    }
    // a flag is refused
    err = bh.csr_aggregate_device(n, nnz, dSp, dSj, 0, seed, 1, dAgg, dRoots, &nagg, &rounds);
    if (err != BHS_ERR_INVALID_ARG) { printf("flags = 1: %d\n", err); return 1; }

    for (void *p : {(void *)dSp, (void *)dSj, (void *)dAgg, (void *)dRoots}) (void)hipFree(p);
    bh.freePlatform();
    printf("aggregate poisson5pt 33x33 seed %u: nagg %d rounds %d PASS\n", seed, nagg, rounds);
    return 0;
}
