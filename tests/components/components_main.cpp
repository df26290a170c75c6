// Connected components through the C++ facade (host/bhsparse.h): a pattern of 3000 vertices built here -- chains of 1 to 400
// vertices under a fixed shuffle of the labels, every edge stored ONE way only and in either direction, with a few self-loops
// and repeated columns, and 200 extra random edges that join some of the chains -- every array on the device.  Checks the
// roots, the numbering by ascending smallest vertex and the sizes against a union-find on the host; prints ncomp and the
// largest sizes and exits 0 on success, non-zero on a status code or a wrong answer.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
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

static unsigned next_random(unsigned &s)
{
    s = s * 1664525u + 1013904223u;
    return s >> 8;
}

static int find(std::vector<int> &up, int v)
{
    while (up[v] != v) v = up[v] = up[up[v]];
    return v;
}

int main()
{
    const int n = 3000;
    unsigned seed = 12345u;
    std::vector<int> label(n);
    std::iota(label.begin(), label.end(), 0);
    for (int i = n - 1; i > 0; --i) std::swap(label[i], label[next_random(seed) % (unsigned)(i + 1)]);
    std::vector<std::vector<int> > rows(n);
    for (int at = 0; at < n;) {                                       // chains over consecutive places of the shuffle
        const int len = 1 + (int)(next_random(seed) % 400u);
        for (int k = at; k + 1 < std::min(at + len, n); ++k) {
            const int a = label[k], b = label[k + 1];
            if (next_random(seed) & 1u) rows[a].push_back(b); else rows[b].push_back(a);
        }
        at += len;
    }
    for (int e = 0; e < 200; ++e) {
        const int a = (int)(next_random(seed) % (unsigned)n), b = (int)(next_random(seed) % (unsigned)n);
        rows[a].push_back(b);
        if (e % 7 == 0) rows[a].push_back(b);                         // a repeated column
        if (e % 11 == 0) rows[b].push_back(b);                        // a self-loop
    }
    std::vector<int> Sp(n + 1, 0), Sj;
    for (int i = 0; i < n; ++i) {
        Sj.insert(Sj.end(), rows[i].begin(), rows[i].end());
        Sp[i + 1] = (int)Sj.size();
    }
    const int nnz = (int)Sj.size();

    // the host's answer: union-find, then the smallest vertex of every set, the roots' ranks, the sizes
    std::vector<int> up(n);
    std::iota(up.begin(), up.end(), 0);
    for (int i = 0; i < n; ++i)
        for (int q = Sp[i]; q < Sp[i + 1]; ++q) {
            const int a = find(up, i), b = find(up, Sj[q]);
            if (a != b) up[std::max(a, b)] = std::min(a, b);          // (the smaller index stays the set's representative)
        }
    std::vector<int> root(n), rank(n, -1), comp(n), sizes;
    for (int i = 0; i < n; ++i) root[i] = find(up, i);
    for (int i = 0; i < n; ++i)
        if (root[i] == i) { rank[i] = (int)sizes.size(); sizes.push_back(0); }
    for (int i = 0; i < n; ++i) { comp[i] = rank[root[i]]; ++sizes[comp[i]]; }
    const int ncomp = (int)sizes.size();

    bool plat[NUM_PLATFORMS] = {false};
    plat[BHSPARSE_HIP] = true;
    bhsparse bh;
    int err = bh.initPlatform(plat);
    if (err) { printf("initPlatform: %d\n", err); return 2; }
    int *dSp = to_device(Sp, Sp.size()), *dSj = to_device(Sj, Sj.size());
    int *dRoot = to_device(std::vector<int>(), (size_t)n), *dComp = to_device(std::vector<int>(), (size_t)n);
    int *dSize = to_device(std::vector<int>(), (size_t)n);
    if (!dSp || !dSj || !dRoot || !dComp || !dSize) { printf("device memory\n"); return 2; }

    int got_ncomp = -1, passes = -1;
    err = bh.csr_components_device(n, nnz, dSp, dSj, 0, dRoot, dComp, dSize, &got_ncomp, &passes);
    if (err) { printf("csr_components_device: %d\n", err); return 1; }
    if (got_ncomp != ncomp || passes < 8 || passes % 8) { printf("ncomp %d, on the host %d; passes %d\n", got_ncomp, ncomp, passes); return 1; }
    std::vector<int> gRoot(n), gComp(n), gSize(ncomp);
    if (hipMemcpy(gRoot.data(), dRoot, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(gComp.data(), dComp, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(gSize.data(), dSize, sizeof(int) * ncomp, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    for (int i = 0; i < n; ++i)
        if (gRoot[i] != root[i] || gComp[i] != comp[i]) {
            printf("vertex %d: root %d comp %d, on the host %d %d\n", i, gRoot[i], gComp[i], root[i], comp[i]);
            return 1;
        }
    if (gSize != sizes) { printf("sizes\n"); return 1; }
    // the roots alone: the same answer without the numbering
    int again = -1;
    err = bh.csr_components_device(n, nnz, dSp, dSj, 0, dRoot, 0, 0, &again, 0);
    if (err || again != ncomp) { printf("roots alone: %d, ncomp %d\n", err, again); return 1; }
    // sizes without the numbering are refused
    err = bh.csr_components_device(n, nnz, dSp, dSj, 0, dRoot, 0, dSize, 0, 0);
    if (err != BHS_ERR_INVALID_ARG) { printf("sizes without the numbering: %d\n", err); return 1; }

    for (void *p : {(void *)dSp, (void *)dSj, (void *)dRoot, (void *)dComp, (void *)dSize}) (void)hipFree(p);
    bh.freePlatform();
    std::vector<int> big(sizes);
    std::sort(big.begin(), big.end(), [](int a, int b) { return a > b; });
    printf("components of %d vertices, %d entries: ncomp %d, passes %d, largest sizes", n, nnz, ncomp, passes);
    for (int c = 0; c < std::min(ncomp, 5); ++c) printf(" %d", big[c]);
    printf(" PASS\n");
    return 0;
}
