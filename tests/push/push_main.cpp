// Sparse frontier x CSR through the C++ facade (host/bhsparse.h): on the path graph 0 - 1 - .. - 11 (undirected, so the
// matrix is its own out-edge list; the edge between v and v + 1 weighs v + 1), with every array on the device:
//   - BFS levels from vertex 0: each level is one OR_AND push call from the list of the last level's vertices, under the
//     complement of the levels; the list the call returns is the next call's frontier;
//   - shortest distances from vertices 0 and 11 at once: round-synchronous Bellman-Ford, each round one MIN_PLUS push call
//     from the rows the last round changed (k = 2, D in an array of leading dimension 3).
// The level update and the gather of F go through the host: the demo shows the calls, not a tuned loop.  Prints PASS and
// exits 0 on success, non-zero on a wrong answer.
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
static bool to_host(T *v, const T *d, size_t count)
{
    return count == 0 || hipMemcpy(v, d, count * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess;
}

template <typename T>
static bool put(T *d, const T *v, size_t count)
{
    return count == 0 || hipMemcpy(d, v, count * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
}

int main()
{
    const int n = 12;
    std::vector<int> Gp(1, 0), Gj;
    std::vector<value_type> Gx;
    for (int v = 0; v < n; ++v) {                 // row v pushes to its neighbours, the larger one first: not ascending
        if (v + 1 < n) { Gj.push_back(v + 1); Gx.push_back((value_type)(v + 1)); }
        if (v > 0) { Gj.push_back(v - 1); Gx.push_back((value_type)v); }
        Gp.push_back((int)Gj.size());
    }
    const int nnz = (int)Gj.size();

    bool plat[NUM_PLATFORMS] = {false};
    plat[BHSPARSE_HIP] = true;
    bhsparse bh;
    int err = bh.initPlatform(plat);
    if (err) { printf("initPlatform: %d\n", err); return 2; }
    int *dGp = to_device(Gp), *dGj = to_device(Gj);
    value_type *dGx = to_device(Gx);

    // ---- BFS from vertex 0: level = depth + 1, 0 for unreached
    std::vector<value_type> levels(n, 0), zeros(n, 0), ones(n, 1);
    std::vector<int> list(n, 0);
    levels[0] = 1;
    value_type *dLevels = to_device(levels), *dReach = to_device(zeros), *dOnes = to_device(ones);
    int *dFront = to_device(list), *dNext = to_device(list);
    if (!dGp || !dGj || !dGx || !dLevels || !dReach || !dOnes || !dFront || !dNext) { printf("device memory\n"); return 2; }
    int steps = 0, nf = 1;                        // the frontier: vertex 0
    for (int depth = 1; depth <= n; ++depth) {
        long long changed = -1;
        int count = -1;
        err = bh.csr_push_semiring_device(BHS_SR_OR_AND, n, n, nnz, 0, dGp, dGj, nf, dFront, 1, dOnes, 1, BHS_MV_MASK_COMPLEMENT,
                                          dLevels, 1, dReach, 1, dNext, &count, &changed);
        if (err) { printf("BFS level %d: %d\n", depth, err); return 1; }
        ++steps;
        if (changed == 0 && count == 0) break;
        if (changed != 1 || count != 1) { printf("BFS level %d: %lld changed, %d listed on a path\n", depth, changed, count); return 1; }
        if (!to_host(list.data(), dNext, (size_t)count)) return 2;
        for (int i = 0; i < count; ++i) levels[list[i]] = (value_type)(depth + 1);
        if (!put(dLevels, levels.data(), (size_t)n) || !put(dReach, zeros.data(), (size_t)n)) return 2;
        std::swap(dFront, dNext);
        nf = count;
    }
    for (int v = 0; v < n; ++v)
        if (levels[v] != (value_type)(v + 1)) { printf("BFS: level of vertex %d is %g\n", v, (double)levels[v]); return 1; }
    if (steps != n) { printf("BFS: %d calls\n", steps); return 1; }

    // ---- shortest paths from vertices 0 and n - 1 at once: n x 2 in an array of leading dimension 3 (the gap holds a
    // sentinel that must stay)
    const int k = 2, ld = 3;
    const value_type inf = (value_type)INFINITY, gap = (value_type)-7;
    std::vector<value_type> D(n * ld, inf), F(n * k, 0);
    for (int v = 0; v < n; ++v) D[v * ld + 2] = gap;
    D[0 * ld + 0] = 0;
    D[(n - 1) * ld + 1] = 0;
    value_type *dD = to_device(D), *dF = to_device(F);
    if (!dD || !dF) { printf("device memory\n"); return 2; }
    list[0] = 0;
    list[1] = n - 1;
    nf = 2;
    if (!put(dFront, list.data(), 2)) return 2;
    int rounds = 0;
    long long changed = -1;
    while (changed != 0 && rounds < n) {
        for (int p = 0; p < nf; ++p)              // F: a snapshot of D at the frontier
            for (int c = 0; c < k; ++c) F[p * k + c] = D[list[p] * ld + c];
        if (!put(dF, F.data(), (size_t)nf * k)) return 2;
        int count = -1;
        err = bh.csr_push_semiring_device(BHS_SR_MIN_PLUS, n, n, nnz, dGx, dGp, dGj, nf, dFront, k, dF, k, 0, 0, 0, dD, ld, dNext,
                                          &count, &changed);
        if (err) { printf("round %d: %d\n", rounds, err); return 1; }
        ++rounds;
        if (!to_host(D.data(), dD, D.size()) || !to_host(list.data(), dNext, (size_t)count)) return 2;
        std::swap(dFront, dNext);
        nf = count;
    }
    if (changed != 0 || rounds != n) { printf("shortest paths: %d rounds, %lld changed\n", rounds, changed); return 1; }
    for (int v = 0; v < n; ++v) {
        const value_type from0 = (value_type)(v * (v + 1) / 2), fromLast = (value_type)(n * (n - 1) / 2 - v * (v + 1) / 2);
        if (D[v * ld] != from0 || D[v * ld + 1] != fromLast || D[v * ld + 2] != gap) {
            printf("shortest paths: vertex %d: %g %g %g\n", v, (double)D[v * ld], (double)D[v * ld + 1], (double)D[v * ld + 2]);
            return 1;
        }
    }
    // the sum that would arrive through atomics is refused
    err = bh.csr_push_semiring_device(BHS_SR_PLUS_TIMES, n, n, nnz, dGx, dGp, dGj, nf, dFront, k, dF, k, 0, 0, 0, dD, ld, 0, 0, 0);
    if (err != BHS_ERR_INVALID_ARG) { printf("plus-times: %d\n", err); return 1; }

    for (void *p : {(void *)dGp, (void *)dGj, (void *)dGx, (void *)dLevels, (void *)dReach, (void *)dOnes, (void *)dFront,
                    (void *)dNext, (void *)dD, (void *)dF})
        (void)hipFree(p);
    bh.freePlatform();
    printf("push bfs / sssp on a path of %d vertices, %d entries: PASS\n", n, nnz);
    return 0;
}
