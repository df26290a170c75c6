// The spanning forest through the C++ facade (host/bhsparse.h), every array on the device.  First the six vertices written out
// in include/bhsparse_hip.h's tests -- a NaN, both zeros, an edge stored from both ends with two weights, a diagonal -- whose
// minimum and maximum forests are compared entry by entry; then the 5-point pattern of a 40 x 30 grid with heavily tied
// integer weights stored from one end only, whose forest is compared with Kruskal's algorithm on the host over the key
// (weight, lo, hi), and whose labels must all be equal.  Prints the counts and exits 0 on success, non-zero on a status code
// or a wrong answer.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <tuple>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../benchmark_spgemm_using_csr_amd/host/bhsparse.h"

typedef std::tuple<int, int, double> Edge;                            // (lo, hi, weight)

template <typename T>
static T *to_device(const std::vector<T> &v, size_t room)
{
    T *d = 0;
    if (hipMalloc((void **)&d, std::max<size_t>(room, 1) * sizeof(T)) != hipSuccess) return 0;
    if (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return 0;
    return d;
}

struct Forest {
    std::vector<Edge> edges;                                          // in the order the call wrote them
    std::vector<int> label;
    int rounds;
};

static int run(bhsparse &bh, int n, const std::vector<int> &Ap, const std::vector<int> &Aj, const std::vector<value_type> &Ax, int flags,
               Forest *out)
{
    int *dAp = to_device(Ap, Ap.size()), *dAj = to_device(Aj, Aj.size());
    value_type *dAx = to_device(Ax, Ax.size());
    int *dLabel = to_device(std::vector<int>(), (size_t)n), *dLo = to_device(std::vector<int>(), (size_t)n),
        *dHi = to_device(std::vector<int>(), (size_t)n);
    value_type *dVal = to_device(std::vector<value_type>(), (size_t)n);
    if (!dAp || !dAj || !dAx || !dLabel || !dLo || !dHi || !dVal) { printf("device memory\n"); return 2; }
    int nedges = -1;
    out->rounds = -1;
    int err = bh.csr_spanning_forest_device(n, (int)Aj.size(), dAp, dAj, dAx, flags, dLabel, dLo, dHi, dVal, &nedges, &out->rounds);
    if (err) { printf("csr_spanning_forest_device: %d\n", err); return 1; }
    if (nedges < 0 || nedges >= n) { printf("%d edges on %d vertices\n", nedges, n); return 1; }
    std::vector<int> lo(n), hi(n);
    std::vector<value_type> val(n);
    out->label.resize(n);
    if (hipMemcpy(lo.data(), dLo, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(hi.data(), dHi, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(val.data(), dVal, sizeof(value_type) * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(out->label.data(), dLabel, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    out->edges.clear();
    for (int e = 0; e < nedges; ++e) out->edges.push_back(Edge(lo[e], hi[e], (double)val[e]));
    // the labels over the edge list are refused
    err = bh.csr_spanning_forest_device(n, (int)Aj.size(), dAp, dAj, dAx, flags, dLabel, dLabel, dHi, dVal, 0, 0);
    if (err != BHS_ERR_INVALID_ARG) { printf("d_edgeLo == d_label: %d\n", err); return 1; }
    for (void *p : {(void *)dAp, (void *)dAj, (void *)dAx, (void *)dLabel, (void *)dLo, (void *)dHi, (void *)dVal}) (void)hipFree(p);
    return 0;
}

static bool same(const std::vector<Edge> &got, const std::vector<Edge> &want, const char *what)
{
    if (got.size() != want.size()) { printf("%s: %zu edges, expected %zu\n", what, got.size(), want.size()); return false; }
    for (size_t e = 0; e < got.size(); ++e)
        if (std::get<0>(got[e]) != std::get<0>(want[e]) || std::get<1>(got[e]) != std::get<1>(want[e]) ||
            std::get<2>(got[e]) != std::get<2>(want[e]) || std::signbit(std::get<2>(got[e])) != std::signbit(std::get<2>(want[e]))) {
            printf("%s: edge %zu is (%d, %d, %g), expected (%d, %d, %g)\n", what, e, std::get<0>(got[e]), std::get<1>(got[e]),
                   std::get<2>(got[e]), std::get<0>(want[e]), std::get<1>(want[e]), std::get<2>(want[e]));
            return false;
        }
    return true;
}

int main()
{
    bool plat[NUM_PLATFORMS] = {false};
    plat[BHSPARSE_HIP] = true;
    bhsparse bh;
    int err = bh.initPlatform(plat);
    if (err) { printf("initPlatform: %d\n", err); return 2; }

    // by hand: (0,1) 2, (0,4) 2 | (1,0) 5, (1,2) 2 | (2,3) NaN, (2,4) +0 | (3,2) -0, (3,4) 1 | -- | (5,5) -7
    {
        const std::vector<int> Ap = {0, 2, 4, 6, 8, 8, 9}, Aj = {1, 4, 0, 2, 3, 4, 2, 4, 5};
        const std::vector<value_type> Ax = {2, 2, 5, 2, (value_type)NAN, 0.0, -0.0, 1, -7};
        Forest f;
        if ((err = run(bh, 6, Ap, Aj, Ax, 0, &f))) return err;
        if (!same(f.edges, {Edge(0, 1, 2.0), Edge(0, 4, 2.0), Edge(2, 3, -0.0), Edge(2, 4, 0.0)}, "by hand, minimum")) return 1;
        if (f.rounds != 2 || f.label != std::vector<int>({0, 0, 0, 0, 0, 5})) { printf("by hand: %d rounds, or the labels\n", f.rounds); return 1; }
        if ((err = run(bh, 6, Ap, Aj, Ax, BHS_FOREST_MAXIMUM, &f))) return err;
        std::sort(f.edges.begin(), f.edges.end());
        if (!same(f.edges, {Edge(0, 1, 5.0), Edge(0, 4, 2.0), Edge(1, 2, 2.0), Edge(3, 4, 1.0)}, "by hand, maximum")) return 1;
    }

    // the grid: every edge stored from its smaller end only, weights 1 .. 5
    const int nx = 40, ny = 30, n = nx * ny;
    std::vector<int> Ap(n + 1, 0), Aj;
    std::vector<value_type> Ax;
    std::vector<Edge> all;
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            const int i = y * nx + x;
            Aj.push_back(i); Ax.push_back(4.0);
            if (x + 1 < nx) { Aj.push_back(i + 1); Ax.push_back((value_type)((x * 7 + y * 13) % 5 + 1)); all.push_back(Edge(i, i + 1, Ax.back())); }
            if (y + 1 < ny) { Aj.push_back(i + nx); Ax.push_back((value_type)((x * 3 + y * 11) % 5 + 1)); all.push_back(Edge(i, i + nx, Ax.back())); }
            Ap[i + 1] = (int)Aj.size();
        }
    Forest f;
    if ((err = run(bh, n, Ap, Aj, Ax, 0, &f))) return err;
    // Kruskal on the host in ascending (weight, lo, hi)
    std::sort(all.begin(), all.end(), [](const Edge &a, const Edge &b) {
        return std::make_tuple(std::get<2>(a), std::get<0>(a), std::get<1>(a)) < std::make_tuple(std::get<2>(b), std::get<0>(b), std::get<1>(b));
    });
    std::vector<int> up(n);
    std::iota(up.begin(), up.end(), 0);
    auto find = [&](int v) { while (up[v] != v) v = up[v] = up[up[v]]; return v; };
    std::vector<Edge> want;
    double weight = 0;
    for (const Edge &e : all) {
        const int a = find(std::get<0>(e)), b = find(std::get<1>(e));
        if (a != b) { up[a] = b; want.push_back(e); weight += std::get<2>(e); }
    }
    std::sort(want.begin(), want.end());
    std::vector<Edge> got = f.edges;
    std::sort(got.begin(), got.end());
    if (!same(got, want, "grid") || (int)got.size() != n - 1) return 1;
    for (int i = 0; i < n; ++i)
        if (f.label[i] != f.label[0] || f.label[f.label[i]] != f.label[i]) { printf("vertex %d: label %d\n", i, f.label[i]); return 1; }
    if (f.rounds < 1 || f.rounds > 10) { printf("%d rounds\n", f.rounds); return 1; }   // floor(log2 1200) = 10

    bh.freePlatform();
    printf("spanning forest of %d vertices, %d entries: %d edges of weight %g in %d rounds; the case by hand PASS\n", n, (int)Aj.size(),
           (int)got.size(), weight, f.rounds);
    return 0;
}
