// Heavy-edge matching through the C++ facade (host/bhsparse.h): the 5-point operator on a 40 x 30 grid built here, the
// coupling along x of magnitude 1 and along y of magnitude 1/64, every array on the device.  Checks that the mates are a
// matching (mate[mate[i]] == i, a partner is a neighbour), that it is maximal (no two unmatched neighbours), that every pair
// along the weak direction has no strong edge left to take at either end, the numbering of pairs and
// singletons by ascending smaller member, and that the unit-weight call without values gives a maximal matching too; prints
// the counts and exits 0 on success, non-zero on a status code or a wrong answer.
#include <algorithm>
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

// is `mate` a maximal matching along the stored entries; counts its pairs
static bool check_matching(int n, const std::vector<int> &Ap, const std::vector<int> &Aj, const std::vector<int> &mate, int *pairs)
{
    *pairs = 0;
    for (int i = 0; i < n; ++i) {
        const int m = mate[i];
        if (m < 0 || m >= n || mate[m] != i) { printf("vertex %d: mate %d is no matching\n", i, m); return false; }
        bool neighbour = m == i;
        for (int q = Ap[i]; q < Ap[i + 1]; ++q) {
            const int j = Aj[q];
            if (j == m) neighbour = true;
            if (m == i && j != i && mate[j] == j) { printf("vertices %d and %d are both unmatched\n", i, j); return false; }
        }
        if (!neighbour) { printf("vertex %d: mate %d is no neighbour\n", i, m); return false; }
        if (m > i) ++*pairs;
    }
    return true;
}

int main()
{
    const int nx = 40, ny = 30, n = nx * ny;
    std::vector<int> Ap(n + 1, 0), Aj;
    std::vector<value_type> Ax;
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            const int i = y * nx + x;
            if (y > 0) { Aj.push_back(i - nx); Ax.push_back(-1.0 / 64); }
            if (x > 0) { Aj.push_back(i - 1); Ax.push_back(-1.0); }
            Aj.push_back(i); Ax.push_back(2.0 + 2.0 / 64);
            if (x + 1 < nx) { Aj.push_back(i + 1); Ax.push_back(-1.0); }
            if (y + 1 < ny) { Aj.push_back(i + nx); Ax.push_back(-1.0 / 64); }
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
    int *dMate = to_device(std::vector<int>(), (size_t)n), *dAgg = to_device(std::vector<int>(), (size_t)n);
    if (!dAp || !dAj || !dAx || !dMate || !dAgg) { printf("device memory\n"); return 2; }

    int npairs = -1, rounds = -1, pairs = 0;
    err = bh.csr_match_device(n, nnz, dAp, dAj, dAx, 0u, 0, dMate, dAgg, &npairs, &rounds);
    if (err) { printf("csr_match_device: %d\n", err); return 1; }
    std::vector<int> mate(n), agg(n);
    if (hipMemcpy(mate.data(), dMate, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(agg.data(), dAgg, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    if (!check_matching(n, Ap, Aj, mate, &pairs)) return 1;
    if (pairs != npairs || rounds < 1 || rounds > n / 2) { printf("npairs %d, counted %d; rounds %d\n", npairs, pairs, rounds); return 1; }
    // a pair along y is taken only once both ends have no strong edge left: their neighbours along x are matched along x
    int along_y = 0;
    for (int i = 0; i < n; ++i) {
        if (mate[i] == i - 1 || mate[i] == i + 1 || mate[i] == i) continue;
        ++along_y;
        for (int k : {i - 1, i + 1}) {
            if (k < 0 || k >= n || k / nx != i / nx) continue;
            if (mate[k] != k - 1 && mate[k] != k + 1) { printf("vertex %d is paired along y beside %d, which is not paired along x\n", i, k); return 1; }
        }
    }
    // the numbering: the rank of the smaller member among the smaller members
    int next = 0;
    for (int i = 0; i < n; ++i) {
        const int want = mate[i] >= i ? next++ : agg[mate[i]];
        if (agg[i] != want) { printf("vertex %d: aggregate %d, expected %d\n", i, agg[i], want); return 1; }
    }
    if (next != n - npairs) { printf("%d aggregates, expected %d\n", next, n - npairs); return 1; }

    // without values and without the numbering: every weight 1
    int unit_pairs = -1, unit_rounds = -1;
    err = bh.csr_match_device(n, nnz, dAp, dAj, 0, 1u, 0, dMate, 0, &unit_pairs, &unit_rounds);
    if (err) { printf("csr_match_device without values: %d\n", err); return 1; }
    if (hipMemcpy(mate.data(), dMate, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    if (!check_matching(n, Ap, Aj, mate, &pairs) || pairs != unit_pairs) { printf("unit weights: npairs %d, counted %d\n", unit_pairs, pairs); return 1; }
    // the mates over the numbering are refused
    err = bh.csr_match_device(n, nnz, dAp, dAj, dAx, 0u, 0, dMate, dMate, 0, 0);
    if (err != BHS_ERR_INVALID_ARG) { printf("d_agg == d_mate: %d\n", err); return 1; }

    for (void *p : {(void *)dAp, (void *)dAj, (void *)dAx, (void *)dMate, (void *)dAgg}) (void)hipFree(p);
    bh.freePlatform();
    printf("matching of %d vertices, %d entries: %d pairs (%d along y) in %d rounds; unit weights: %d pairs in %d rounds PASS\n", n, nnz,
           npairs, along_y / 2, rounds, unit_pairs, unit_rounds);
    return 0;
}
