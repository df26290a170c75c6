// Semiring CSR x dense through the C++ facade (host/bhsparse.h): on the path graph 0 - 1 - .. - 11 (undirected; the edge
// between v and v + 1 weighs v + 1), from vertex 0, with every array on the device:
//   - BFS levels: each step is one OR_AND call under the complement of the levels into a fresh frontier (k = 1, the vector
//     call), ended by the call's count of changed elements;
//   - shortest distances from vertices 0 and 11 at once: Bellman-Ford sweeps, each one MIN_PLUS call with accumulation
//     (k = 2 in arrays of leading dimension 3, the matrix call).
// The level update and the copies between sweeps go through the host: the demo shows the calls, not a tuned loop.  Prints
// PASS and exits 0 on success, non-zero on a wrong answer.
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
static bool to_host(std::vector<T> &v, const T *d)
{
    return hipMemcpy(v.data(), d, v.size() * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess;
}

template <typename T>
static bool put(T *d, const std::vector<T> &v)
{
    return hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
}

int main()
{
    const int n = 12;
    std::vector<int> Ap(1, 0), Aj;
    std::vector<value_type> Ax;
    for (int v = 0; v < n; ++v) {                 // row v pulls from its neighbours, the larger one first: not ascending
        if (v + 1 < n) { Aj.push_back(v + 1); Ax.push_back((value_type)(v + 1)); }
        if (v > 0) { Aj.push_back(v - 1); Ax.push_back((value_type)v); }
        Ap.push_back((int)Aj.size());
    }
    const int nnz = (int)Aj.size();

    bool plat[NUM_PLATFORMS] = {false};
    plat[BHSPARSE_HIP] = true;
    bhsparse bh;
    int err = bh.initPlatform(plat);
    if (err) { printf("initPlatform: %d\n", err); return 2; }
    int *dAp = to_device(Ap), *dAj = to_device(Aj);
    value_type *dAx = to_device(Ax);

    // ---- BFS from vertex 0: level = depth + 1, 0 for unreached
    std::vector<value_type> levels(n, 0), frontier(n, 0), next(n, 0);
    levels[0] = frontier[0] = 1;
    value_type *dLevels = to_device(levels), *dFrontier = to_device(frontier), *dNext = to_device(next);
    if (!dAp || !dAj || !dAx || !dLevels || !dFrontier || !dNext) { printf("device memory\n"); return 2; }
    int steps = 0;
    for (int depth = 1; depth <= n; ++depth) {
        long long changed = -1;
        std::fill(next.begin(), next.end(), (value_type)0);
        if (!put(dNext, next)) return 2;
        err = bh.csr_spmv_semiring_device(BHS_SR_OR_AND, n, n, nnz, 0, dAp, dAj, dFrontier, BHS_MV_MASK_COMPLEMENT, dLevels, dNext,
                                          &changed);
        if (err) { printf("BFS step %d: %d\n", depth, err); return 1; }
        ++steps;
        if (changed == 0) break;
        if (changed != 1) { printf("BFS step %d: frontier of %lld vertices on a path\n", depth, changed); return 1; }
        if (!to_host(next, dNext)) return 2;
        for (int v = 0; v < n; ++v)
            if (next[v] != 0) levels[v] = (value_type)(depth + 1);
        if (!put(dLevels, levels) || !put(dFrontier, next)) return 2;
    }
    for (int v = 0; v < n; ++v)
        if (levels[v] != (value_type)(v + 1)) { printf("BFS: level of vertex %d is %g\n", v, (double)levels[v]); return 1; }
    if (steps != n) { printf("BFS: %d steps\n", steps); return 1; }

    // ---- shortest paths from vertices 0 and n - 1 at once: n x 2 in arrays of leading dimension 3 (the gap holds a
    // sentinel that must stay)
    const int k = 2, ld = 3;
    const value_type inf = (value_type)INFINITY, gap = (value_type)-7;
    std::vector<value_type> D(n * ld, inf);
    for (int v = 0; v < n; ++v) D[v * ld + 2] = gap;
    D[0 * ld + 0] = 0;
    D[(n - 1) * ld + 1] = 0;
    value_type *dD = to_device(D), *dD2 = to_device(D);
    if (!dD || !dD2) { printf("device memory\n"); return 2; }
    int sweeps = 0;
    long long changed = -1;
    while (changed != 0 && sweeps < n) {
        err = bh.csr_spmm_semiring_device(BHS_SR_MIN_PLUS, n, n, nnz, dAx, dAp, dAj, k, dD, ld, BHS_MV_ACCUM, 0, 0, dD2, ld, &changed);
        if (err) { printf("sweep %d: %d\n", sweeps, err); return 1; }
        ++sweeps;
        if (hipMemcpy(dD, dD2, D.size() * sizeof(value_type), hipMemcpyDeviceToDevice) != hipSuccess) return 2;
    }
    if (!to_host(D, dD)) return 2;
    if (changed != 0 || sweeps != n) { printf("shortest paths: %d sweeps, %lld changed\n", sweeps, changed); return 1; }
    for (int v = 0; v < n; ++v) {
        const value_type from0 = (value_type)(v * (v + 1) / 2), fromLast = (value_type)(n * (n - 1) / 2 - v * (v + 1) / 2);
        if (D[v * ld] != from0 || D[v * ld + 1] != fromLast || D[v * ld + 2] != gap) {
            printf("shortest paths: vertex %d: %g %g %g\n", v, (double)D[v * ld], (double)D[v * ld + 1], (double)D[v * ld + 2]);
            return 1;
        }
    }
    // a complement without a mask is refused
    err = bh.csr_spmv_semiring_device(BHS_SR_OR_AND, n, n, nnz, 0, dAp, dAj, dFrontier, BHS_MV_MASK_COMPLEMENT, 0, dNext, 0);
    if (err != BHS_ERR_INVALID_ARG) { printf("complement without a mask: %d\n", err); return 1; }

    for (void *p : {(void *)dAp, (void *)dAj, (void *)dAx, (void *)dLevels, (void *)dFrontier, (void *)dNext, (void *)dD, (void *)dD2})
        (void)hipFree(p);
    bh.freePlatform();
    printf("bfs / sssp on a path of %d vertices, %d entries: PASS\n", n, nnz);
    return 0;
}
