// The k-core decomposition through the C++ facade (host/bhsparse.h): a 30 x 40 five-point grid, cliques of 4, 9 and 16, a
// hub with 200 pendant leaves on a triangle and 11 single vertices under one seeded shuffle of the 1443 labels, every array on
// the device.  Checks the core numbers against a bucket peel on the host (Batagelj-Zaversnik, one vertex at a time), the
// rounds against a host loop that removes a whole round at once, that the degeneracy is 15, and that a pattern with one
// mirror entry missing is refused with the outputs untouched; prints the counts and exits 0 on success, non-zero on a status
// code or a wrong answer.
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

int main()
{
    const int nx = 30, ny = 40, grid = nx * ny, cl[3] = {4, 9, 16}, leaves = 200, single = 11;
    const int hub = grid + 4 + 9 + 16, n = hub + 3 + leaves + single;
    unsigned seed = 2468u;
    std::vector<int> label(n);
    std::iota(label.begin(), label.end(), 0);
    for (int i = n - 1; i > 0; --i) std::swap(label[i], label[next_random(seed) % (unsigned)(i + 1)]);
    std::vector<std::vector<int> > rows(n);
    auto join = [&](int a, int b) { rows[label[a]].push_back(label[b]); rows[label[b]].push_back(label[a]); };
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            if (x + 1 < nx) join(y * nx + x, y * nx + x + 1);
            if (y + 1 < ny) join(y * nx + x, (y + 1) * nx + x);
        }
    int at = grid;
    for (int q : cl) {
        for (int a = 0; a < q; ++a)
            for (int b = a + 1; b < q; ++b) join(at + a, at + b);
        at += q;
    }
    join(hub, hub + 1); join(hub, hub + 2); join(hub + 1, hub + 2);
    for (int k = 0; k < leaves; ++k) join(hub, hub + 3 + k);
    for (int i = 0; i < n; i += 2) rows[i].push_back(i);             // a diagonal on every other row: allowed and ignored
    std::vector<int> Sp(n + 1, 0), Sj, deg(n);
    for (int i = 0; i < n; ++i) {
        std::sort(rows[i].begin(), rows[i].end());
        deg[i] = (int)rows[i].size() - (i % 2 == 0 ? 1 : 0);
        Sj.insert(Sj.end(), rows[i].begin(), rows[i].end());
        Sp[i + 1] = (int)Sj.size();
    }
    const int nnz = (int)Sj.size();

    // the host's bucket peel: always the vertex of least current degree
    std::vector<int> want(deg), order(n), pos(n), start;
    {
        const int md = *std::max_element(deg.begin(), deg.end());
        std::vector<int> count(md + 2, 0);
        for (int v = 0; v < n; ++v) ++count[deg[v] + 1];
        for (int d = 0; d <= md; ++d) count[d + 1] += count[d];
        start.assign(count.begin(), count.end() - 1);
        std::vector<int> fill(start);
        for (int v = 0; v < n; ++v) { pos[v] = fill[deg[v]]++; order[pos[v]] = v; }
        for (int i = 0; i < n; ++i) {
            const int v = order[i];
            for (int q = Sp[v]; q < Sp[v + 1]; ++q) {
                const int u = Sj[q];
                if (u == v || want[u] <= want[v]) continue;
                const int du = want[u], pu = pos[u], pw = start[du], w = order[pw];
                if (u != w) { order[pu] = w; order[pw] = u; pos[u] = pw; pos[w] = pu; }
                ++start[du];
                --want[u];
            }
        }
    }
    // the host's rounds: everything at or below the level leaves at once
    std::vector<int> wantRound(n, 0), now(deg);
    int rounds = 0, level = 0;
    for (int left = n; left > 0;) {
        int least = n;
        for (int v = 0; v < n; ++v)
            if (!wantRound[v]) least = std::min(least, now[v]);
        level = std::max(level, least);
        ++rounds;
        std::vector<int> out;
        for (int v = 0; v < n; ++v)
            if (!wantRound[v] && now[v] <= level) out.push_back(v);
        for (int v : out) wantRound[v] = rounds;
        for (int v : out)
            for (int q = Sp[v]; q < Sp[v + 1]; ++q)
                if (Sj[q] != v) --now[Sj[q]];
        left -= (int)out.size();
    }

    bool plat[NUM_PLATFORMS] = {false};
    plat[BHSPARSE_HIP] = true;
    bhsparse bh;
    int err = bh.initPlatform(plat);
    if (err) { printf("initPlatform: %d\n", err); return 2; }
    int *dSp = to_device(Sp, Sp.size()), *dSj = to_device(Sj, Sj.size());
    int *dCore = to_device(std::vector<int>(n, -7), (size_t)n), *dRound = to_device(std::vector<int>(n, -7), (size_t)n);
    if (!dSp || !dSj || !dCore || !dRound) { printf("device memory\n"); return 2; }

    // one mirror entry missing: refused, and the outputs stay as they were
    std::vector<int> Bp(Sp), Bj;
    const int victim = label[0];                                      // a grid corner: its first off-diagonal entry goes
    int gone = -1;
    for (int i = 0; i < n; ++i) {
        for (int q = Sp[i]; q < Sp[i + 1]; ++q) {
            if (i == victim && gone < 0 && Sj[q] != i) { gone = i; continue; }
            Bj.push_back(Sj[q]);
        }
        Bp[i + 1] = (int)Bj.size();
    }
    int *dBp = to_device(Bp, Bp.size()), *dBj = to_device(Bj, Bj.size());
    if (!dBp || !dBj) { printf("device memory\n"); return 2; }
    std::vector<int> core(n), round(n);
    err = bh.csr_kcore_device(n, nnz - 1, dBp, dBj, 0, dCore, dRound, 0, 0);
    if (err != BHS_ERR_INVALID_ARG) { printf("a missing mirror entry: %d\n", err); return 1; }
    if (hipMemcpy(core.data(), dCore, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(round.data(), dRound, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    for (int v = 0; v < n; ++v)
        if (core[v] != -7 || round[v] != -7) { printf("a refused call wrote vertex %d\n", v); return 1; }

    int kmax = -1, got = -1;
    err = bh.csr_kcore_device(n, nnz, dSp, dSj, 0, dCore, dRound, &kmax, &got);
    if (err) { printf("csr_kcore_device: %d\n", err); return 1; }
    if (hipMemcpy(core.data(), dCore, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(round.data(), dRound, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    for (int v = 0; v < n; ++v) {
        if (core[v] != want[v]) { printf("vertex %d: core %d, the bucket peel's %d\n", v, core[v], want[v]); return 1; }
        if (round[v] != wantRound[v]) { printf("vertex %d: round %d, on the host %d\n", v, round[v], wantRound[v]); return 1; }
    }
    if (kmax != 15 || got != rounds) { printf("kmax %d, rounds %d, on the host %d\n", kmax, got, rounds); return 1; }
    if (core[label[hub]] != 2 || core[label[hub + 3]] != 1 || core[label[n - 1]] != 0 || core[label[0]] != 2) {
        printf("the hub %d, a leaf %d, a single vertex %d, a grid corner %d\n", core[label[hub]], core[label[hub + 3]], core[label[n - 1]],
               core[label[0]]);
        return 1;
    }

    // without the rounds
    err = bh.csr_kcore_device(n, nnz, dSp, dSj, 0, dRound, 0, 0, 0);
    if (err || hipMemcpy(round.data(), dRound, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess) { printf("no rounds: %d\n", err); return 1; }
    if (round != core) { printf("the core numbers without the rounds\n"); return 1; }

    for (void *p : {(void *)dSp, (void *)dSj, (void *)dCore, (void *)dRound, (void *)dBp, (void *)dBj}) (void)hipFree(p);
    bh.freePlatform();
    printf("k-core decomposition of %d vertices, %d entries: kmax %d, rounds %d PASS\n", n, nnz, kmax, got);
    return 0;
}
