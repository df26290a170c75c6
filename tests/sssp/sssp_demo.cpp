// Shortest paths through the C++ facade (host/bhsparse.h): a 48 x 37 road-like grid of 1776 vertices, edges both ways with
// seeded weights of their own (every ninth one zero), two sources, every array on the device.  Checks the distances bit for
// bit against a host relaxation loop (sweeps over all edges until nothing changes: the least fixed point, one rounding an
// edge) at the bucket widths 0.5, 4 and +Inf, that every parent has a strictly smaller distance and a tight edge, that a
// path walked back from the far corner sums to its distance, and that a negative weight is refused with the outputs
// untouched; prints the counts and exits 0 on success, non-zero on a status code or a wrong answer.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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
    const int nx = 48, ny = 37, n = nx * ny;
    const value_type inf = std::numeric_limits<value_type>::infinity();
    unsigned seed = 1357u;
    std::vector<std::vector<std::pair<int, value_type> > > rows(n);
    int drawn = 0;
    auto weight = [&]() {
        const value_type w = (value_type)(1 + next_random(seed) % 1000) / (value_type)97;
        return ++drawn % 9 == 0 ? (value_type)0 : w;
    };
    auto join = [&](int a, int b) { rows[a].push_back({b, weight()}); rows[b].push_back({a, weight()}); };
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            if (x + 1 < nx) join(y * nx + x, y * nx + x + 1);
            if (y + 1 < ny) join(y * nx + x, (y + 1) * nx + x);
        }
    std::vector<int> Gp(n + 1, 0), Gj;
    std::vector<value_type> Gx;
    for (int i = 0; i < n; ++i) {
        for (auto &e : rows[i]) { Gj.push_back(e.first); Gx.push_back(e.second); }
        Gp[i + 1] = (int)Gj.size();
    }
    const int nnz = (int)Gj.size();
    const std::vector<int> sources = {nx / 2, n - nx};

    // the host loop: sweeps over all edges until a sweep changes nothing
    std::vector<value_type> want(n, inf);
    for (int s : sources) want[s] = 0;
    int sweeps = 0;
    for (bool changed = true; changed; ++sweeps) {
        changed = false;
        for (int u = 0; u < n; ++u) {
            if (want[u] == inf) continue;
            for (int q = Gp[u]; q < Gp[u + 1]; ++q) {
                const value_type nd = want[u] + Gx[q];
                if (nd < want[Gj[q]]) { want[Gj[q]] = nd; changed = true; }
            }
        }
    }

    bool plat[NUM_PLATFORMS] = {false};
    plat[BHSPARSE_HIP] = true;
    bhsparse bh;
    int err = bh.initPlatform(plat);
    if (err) { printf("initPlatform: %d\n", err); return 2; }
    int *dGp = to_device(Gp, Gp.size()), *dGj = to_device(Gj, Gj.size()), *dSrc = to_device(sources, sources.size());
    value_type *dGx = to_device(Gx, Gx.size());
    value_type *dDist = to_device(std::vector<value_type>(n, (value_type)-7), (size_t)n);
    int *dPar = to_device(std::vector<int>(n, -7), (size_t)n);
    if (!dGp || !dGj || !dGx || !dSrc || !dDist || !dPar) { printf("device memory\n"); return 2; }

    // a negative weight: refused, and the outputs stay as they were
    std::vector<value_type> Bx(Gx);
    Bx[nnz / 2] = (value_type)-1;
    value_type *dBx = to_device(Bx, Bx.size());
    if (!dBx) { printf("device memory\n"); return 2; }
    std::vector<value_type> dist(n);
    std::vector<int> par(n);
    err = bh.csr_sssp_device(n, nnz, dGp, dGj, dBx, 2, dSrc, 1.0, 0, dDist, dPar, 0, 0);
    if (err != BHS_ERR_INVALID_ARG) { printf("a negative weight: %d\n", err); return 1; }
    if (hipMemcpy(dist.data(), dDist, sizeof(value_type) * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(par.data(), dPar, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    for (int v = 0; v < n; ++v)
        if (dist[v] != (value_type)-7 || par[v] != -7) { printf("a refused call wrote vertex %d\n", v); return 1; }

    int reached = -1, passes[3] = {-1, -1, -1};
    const double deltas[3] = {0.5, 4.0, (double)inf};
    for (int k = 0; k < 3; ++k) {
        err = bh.csr_sssp_device(n, nnz, dGp, dGj, dGx, 2, dSrc, deltas[k], 0, dDist, dPar, &reached, &passes[k]);
        if (err) { printf("csr_sssp_device at delta %g: %d\n", deltas[k], err); return 1; }
        if (hipMemcpy(dist.data(), dDist, sizeof(value_type) * n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(par.data(), dPar, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess) return 2;
        if (memcmp(dist.data(), want.data(), sizeof(value_type) * n) != 0) {
            for (int v = 0; v < n; ++v)
                if (dist[v] != want[v]) { printf("delta %g, vertex %d: %.17g, the host loop's %.17g\n", deltas[k], v, (double)dist[v], (double)want[v]); return 1; }
        }
        if (reached != n || passes[k] < 8 || passes[k] % 8) { printf("delta %g: reached %d, passes %d\n", deltas[k], reached, passes[k]); return 1; }
        for (int v = 0; v < n; ++v) {
            const int p = par[v];
            if (p == -1 && (v == sources[0] || v == sources[1])) continue;
            if (p == -2) continue;                                    // reached over edges that gain nothing only
            if (p < 0 || p >= n || !(dist[p] < dist[v])) { printf("vertex %d: parent %d\n", v, p); return 1; }
            bool tight = false;
            for (int q = Gp[p]; q < Gp[p + 1]; ++q) tight = tight || (Gj[q] == v && dist[p] + Gx[q] == dist[v]);
            if (!tight) { printf("vertex %d: no tight edge from its parent %d\n", v, p); return 1; }
        }
    }
    // the far corner's path, summed left to right
    std::vector<int> walk(1, n - 1);
    while (par[walk.back()] >= 0 && (int)walk.size() <= n) walk.push_back(par[walk.back()]);
    if (par[walk.back()] == -1) {
        value_type sum = 0;
        for (size_t k = walk.size() - 1; k > 0; --k) {
            value_type w = inf;
            for (int q = Gp[walk[k]]; q < Gp[walk[k] + 1]; ++q)
                if (Gj[q] == walk[k - 1] && sum + Gx[q] == dist[walk[k - 1]]) w = Gx[q];
            sum = sum + w;
        }
        if (sum != dist[n - 1]) { printf("the far corner's path sums to %.17g, its distance is %.17g\n", (double)sum, (double)dist[n - 1]); return 1; }
    }

    // without the parents
    err = bh.csr_sssp_device(n, nnz, dGp, dGj, dGx, 2, dSrc, 4.0, 0, dDist, 0, 0, 0);
    if (err || hipMemcpy(dist.data(), dDist, sizeof(value_type) * n, hipMemcpyDeviceToHost) != hipSuccess) { printf("no parents: %d\n", err); return 1; }
    if (memcmp(dist.data(), want.data(), sizeof(value_type) * n) != 0) { printf("the distances without the parents\n"); return 1; }

    for (void *p : {(void *)dGp, (void *)dGj, (void *)dGx, (void *)dBx, (void *)dSrc, (void *)dDist, (void *)dPar}) (void)hipFree(p);
    bh.freePlatform();
    printf("shortest paths of %d vertices, %d edges from 2 sources: %d host sweeps; passes %d, %d, %d at delta 0.5, 4, inf; path of %d vertices PASS\n",
           n, nnz, sweeps, passes[0], passes[1], passes[2], (int)walk.size());
    return 0;
}
