// Strongly connected components through the C++ facade (host/bhsparse.h): a seeded directed graph of 3000 vertices built here
// -- one-way rings of 2 to 60 vertices over consecutive places of a fixed shuffle of the labels, a one-way bridge from every
// third ring to the next, 700 random one-way edges among the first 1200 places (which melt their rings into larger
// components), tails that nothing enters, a few self-loops and repeated columns -- every array on the device.  Checks the
// roots, the numbering by ascending smallest vertex and the sizes against Tarjan's algorithm on the host, and that the
// transposed pattern gives the same answer; prints nscc, the rounds and the largest sizes and exits 0 on success, non-zero on
// a status code or a wrong answer.
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

// Tarjan's algorithm with a stack of its own (no recursion): scc[v] = the number of v's component in the order they close
static int tarjan(int n, const std::vector<int> &Sp, const std::vector<int> &Sj, std::vector<int> &scc)
{
    std::vector<int> index(n, -1), lowlink(n, 0), at(n, 0), stack, path;
    std::vector<char> on(n, 0);
    int next = 0, count = 0;
    scc.assign(n, -1);
    for (int s = 0; s < n; ++s) {
        if (index[s] >= 0) continue;
        path.push_back(s);
        while (!path.empty()) {
            const int v = path.back();
            if (index[v] < 0) {
                index[v] = lowlink[v] = next++;
                at[v] = Sp[v];
                stack.push_back(v);
                on[v] = 1;
            }
            bool down = false;
            while (at[v] < Sp[v + 1]) {
                const int w = Sj[at[v]++];
                if (index[w] < 0) { path.push_back(w); down = true; break; }
                if (on[w]) lowlink[v] = std::min(lowlink[v], index[w]);
            }
            if (down) continue;
            if (lowlink[v] == index[v]) {
                for (;;) {
                    const int w = stack.back();
                    stack.pop_back();
                    on[w] = 0;
                    scc[w] = count;
                    if (w == v) break;
                }
                ++count;
            }
            path.pop_back();
            if (!path.empty()) lowlink[path.back()] = std::min(lowlink[path.back()], lowlink[v]);
        }
    }
    return count;
}

int main()
{
    const int n = 3000;
    unsigned seed = 2468u;
    std::vector<int> label(n);
    std::iota(label.begin(), label.end(), 0);
    for (int i = n - 1; i > 0; --i) std::swap(label[i], label[next_random(seed) % (unsigned)(i + 1)]);
    std::vector<std::vector<int> > rows(n);
    int ring = 0;
    for (int at = 0; at < n; ++ring) {                                // one-way rings over consecutive places of the shuffle
        const int len = std::min(2 + (int)(next_random(seed) % 59u), n - at);
        if (ring % 5 == 4) {                                          // a tail instead: nothing enters its first vertex
            for (int k = at; k + 1 < at + len; ++k) rows[label[k]].push_back(label[k + 1]);
        } else {
            for (int k = at; k < at + len; ++k) rows[label[k]].push_back(label[k + 1 < at + len ? k + 1 : at]);
            if (ring % 3 == 0 && at + len < n) rows[label[at]].push_back(label[at + len]);   // a bridge to what follows
        }
        at += len;
    }
    for (int e = 0; e < 700; ++e) {
        const int a = label[next_random(seed) % 1200u], b = label[next_random(seed) % 1200u];
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
    std::vector<int> Tp(n + 1, 0), Tj(nnz);                           // the transposed pattern
    for (int q = 0; q < nnz; ++q) ++Tp[Sj[q] + 1];
    for (int i = 0; i < n; ++i) Tp[i + 1] += Tp[i];
    {
        std::vector<int> fill(Tp.begin(), Tp.end() - 1);
        for (int i = 0; i < n; ++i)
            for (int q = Sp[i]; q < Sp[i + 1]; ++q) Tj[fill[Sj[q]]++] = i;
    }

    // the host's answer: Tarjan, then the smallest vertex of every component, the roots' ranks, the sizes
    std::vector<int> scc;
    const int nscc = tarjan(n, Sp, Sj, scc);
    std::vector<int> least(nscc, n), root(n), rank(n, -1), comp(n), sizes;
    for (int i = n - 1; i >= 0; --i) least[scc[i]] = i;
    for (int i = 0; i < n; ++i) root[i] = least[scc[i]];
    for (int i = 0; i < n; ++i)
        if (root[i] == i) { rank[i] = (int)sizes.size(); sizes.push_back(0); }
    for (int i = 0; i < n; ++i) { comp[i] = rank[root[i]]; ++sizes[comp[i]]; }
    if ((int)sizes.size() != nscc) { printf("the host's own count\n"); return 2; }

    bool plat[NUM_PLATFORMS] = {false};
    plat[BHSPARSE_HIP] = true;
    bhsparse bh;
    int err = bh.initPlatform(plat);
    if (err) { printf("initPlatform: %d\n", err); return 2; }
    int *dSp = to_device(Sp, Sp.size()), *dSj = to_device(Sj, Sj.size());
    int *dTp = to_device(Tp, Tp.size()), *dTj = to_device(Tj, Tj.size());
    int *dRoot = to_device(std::vector<int>(), (size_t)n), *dComp = to_device(std::vector<int>(), (size_t)n);
    int *dSize = to_device(std::vector<int>(), (size_t)n);
    if (!dSp || !dSj || !dTp || !dTj || !dRoot || !dComp || !dSize) { printf("device memory\n"); return 2; }

    int rounds = -1, passes = -1;
    for (int pass = 0; pass < 2; ++pass) {                            // S, then its transpose: the same answer
        int got = -1, r = -1, p = -1;
        err = bh.csr_scc_device(n, nnz, pass ? dTp : dSp, pass ? dTj : dSj, 0, dRoot, dComp, dSize, &got, &r, &p);
        if (err) { printf("csr_scc_device: %d\n", err); return 1; }
        if (got != nscc || r < 1 || p < 8 || p % 8) { printf("nscc %d, on the host %d; rounds %d, passes %d\n", got, nscc, r, p); return 1; }
        std::vector<int> gRoot(n), gComp(n), gSize(nscc);
        if (hipMemcpy(gRoot.data(), dRoot, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(gComp.data(), dComp, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(gSize.data(), dSize, sizeof(int) * nscc, hipMemcpyDeviceToHost) != hipSuccess) return 2;
        for (int i = 0; i < n; ++i)
            if (gRoot[i] != root[i] || gComp[i] != comp[i]) {
                printf("vertex %d: root %d comp %d, on the host %d %d\n", i, gRoot[i], gComp[i], root[i], comp[i]);
                return 1;
            }
        if (gSize != sizes) { printf("sizes\n"); return 1; }
        if (!pass) { rounds = r; passes = p; }
    }
    // the roots alone: the same count without the numbering
    int again = -1;
    err = bh.csr_scc_device(n, nnz, dSp, dSj, 0, dRoot, 0, 0, &again, 0, 0);
    if (err || again != nscc) { printf("roots alone: %d, nscc %d\n", err, again); return 1; }
    // sizes without the numbering are refused
    err = bh.csr_scc_device(n, nnz, dSp, dSj, 0, dRoot, 0, dSize, 0, 0, 0);
    if (err != BHS_ERR_INVALID_ARG) { printf("sizes without the numbering: %d\n", err); return 1; }

    for (void *p : {(void *)dSp, (void *)dSj, (void *)dTp, (void *)dTj, (void *)dRoot, (void *)dComp, (void *)dSize}) (void)hipFree(p);
    bh.freePlatform();
    std::vector<int> big(sizes);
    std::sort(big.begin(), big.end(), [](int a, int b) { return a > b; });
    printf("strongly connected components of %d vertices, %d entries: nscc %d, rounds %d, passes %d, largest sizes", n, nnz, nscc, rounds,
           passes);
    for (int c = 0; c < std::min(nscc, 5); ++c) printf(" %d", big[c]);
    printf(" PASS\n");
    return 0;
}
