// Betweenness centrality through the C++ facade (host/bhsparse.h): a 24 x 19 grid of 456 vertices, edges both ways to the four
// neighbours and, where (x + y) % 3 == 0, along the diagonal to (x + 1, y + 1) -- an undirected graph, so the in-edges are the
// out-edges -- from ALL sources, every array on the device.  Checks the sums bit for bit against a host Brandes of its own
// that restates the summation rule (lanes by the mean row length, a lane an entry modulo the lanes, the xor butterfly), that
// two chained calls under BHS_BC_ACCUMULATE give the bits of one, the levels and path counts of the last source, and that a
// column equal to n is refused with the outputs untouched; prints the counts and an FNV-1a hash of the sums' bytes and
// exits 0 on success, non-zero on a status code or a wrong answer.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// the contract's sum over one row: term(q) is what entry q adds, a negative value where it does not qualify
template <typename F>
static double rule_sum(int lo, int hi, int L, F term)
{
    const int W = hi - lo > 32 * L ? 64 : L;
    double t[64];
    for (int l = 0; l < W; ++l) t[l] = 0.0;
    for (int q = lo; q < hi; ++q) {
        const double x = term(q);
        if (x >= 0.0) t[(q - lo) % W] = t[(q - lo) % W] + x;
    }
    for (int off = W / 2; off >= 1; off /= 2) {
        double u[64];
        for (int l = 0; l < W; ++l) u[l] = t[l] + t[l ^ off];
        for (int l = 0; l < W; ++l) t[l] = u[l];
    }
    return t[0];
}

// the host loop: Brandes' algorithm from source s, added to bc
static void host_brandes(int n, const std::vector<int> &Gp, const std::vector<int> &Gj, int L, int s, std::vector<double> &bc,
                         std::vector<int> &level, std::vector<double> &sigma)
{
    level.assign(n, -1);
    sigma.assign(n, 0.0);
    std::vector<double> delta(n, 0.0);
    std::vector<std::vector<int> > slices(1, std::vector<int>(1, s));
    level[s] = 0;
    sigma[s] = 1.0;
    for (;;) {
        std::vector<int> next;
        const int l = (int)slices.size() - 1;
        for (int u : slices.back())
            for (int q = Gp[u]; q < Gp[u + 1]; ++q)
                if (level[Gj[q]] == -1) { level[Gj[q]] = l + 1; next.push_back(Gj[q]); }
        if (next.empty()) break;
        for (int v : next)                                            // (undirected: row v of T is row v of G)
            sigma[v] = rule_sum(Gp[v], Gp[v + 1], L, [&](int q) { return level[Gj[q]] == l ? sigma[Gj[q]] : -1.0; });
        slices.push_back(next);
    }
    for (int l = (int)slices.size() - 2; l >= 1; --l)
        for (int u : slices[l]) {
            const double S = rule_sum(Gp[u], Gp[u + 1], L, [&](int q) {
                const int v = Gj[q];
                return level[v] == l + 1 ? (1.0 + delta[v]) / sigma[v] : -1.0;
            });
            delta[u] = sigma[u] * S;
            bc[u] = bc[u] + delta[u];
        }
}

int main()
{
    const int nx = 24, ny = 19, n = nx * ny;
    std::vector<std::vector<int> > rows(n);
    auto join = [&](int a, int b) { rows[a].push_back(b); rows[b].push_back(a); };
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            if (x + 1 < nx) join(y * nx + x, y * nx + x + 1);
            if (y + 1 < ny) join(y * nx + x, (y + 1) * nx + x);
            if ((x + y) % 3 == 0 && x + 1 < nx && y + 1 < ny) join(y * nx + x, (y + 1) * nx + x + 1);
        }
    std::vector<int> Gp(n + 1, 0), Gj;
    for (int i = 0; i < n; ++i) {
        for (int c : rows[i]) Gj.push_back(c);
        Gp[i + 1] = (int)Gj.size();
    }
    const int nnz = (int)Gj.size();
    const double mean = (double)nnz / n;
    const int L = mean <= 4.0 ? 1 : mean <= 16.0 ? 4 : mean <= 64.0 ? 16 : 64;
    std::vector<int> sources(n);
    for (int i = 0; i < n; ++i) sources[i] = (i * 7) % n;             // (7 and 456 are coprime: every vertex once)

    std::vector<double> want(n, 0.0), wantSigma;
    std::vector<int> wantLevel;
    long long wantLevels = 0;
    for (int s : sources) {
        host_brandes(n, Gp, Gj, L, s, want, wantLevel, wantSigma);
        wantLevels += *std::max_element(wantLevel.begin(), wantLevel.end()) + 1;
    }

    bool plat[NUM_PLATFORMS] = {false};
    plat[BHSPARSE_HIP] = true;
    bhsparse bh;
    int err = bh.initPlatform(plat);
    if (err) { printf("initPlatform: %d\n", err); return 2; }
    int *dGp = to_device(Gp, Gp.size()), *dGj = to_device(Gj, Gj.size()), *dSrc = to_device(sources, sources.size());
    double *dBc = to_device(std::vector<double>(n, -7.0), (size_t)n), *dSigma = to_device(std::vector<double>(n, -7.0), (size_t)n);
    int *dLevel = to_device(std::vector<int>(n, -7), (size_t)n);
    if (!dGp || !dGj || !dSrc || !dBc || !dSigma || !dLevel) { printf("device memory\n"); return 2; }

    // a column equal to n: refused, and the outputs stay as they were
    std::vector<int> Bj(Gj);
    Bj[nnz / 2] = n;
    int *dBj = to_device(Bj, Bj.size());
    if (!dBj) { printf("device memory\n"); return 2; }
    std::vector<double> bc(n), sigma(n);
    std::vector<int> level(n);
    auto fetch = [&]() {
        return hipMemcpy(bc.data(), dBc, sizeof(double) * n, hipMemcpyDeviceToHost) == hipSuccess &&
               hipMemcpy(sigma.data(), dSigma, sizeof(double) * n, hipMemcpyDeviceToHost) == hipSuccess &&
               hipMemcpy(level.data(), dLevel, sizeof(int) * n, hipMemcpyDeviceToHost) == hipSuccess;
    };
    err = bh.csr_betweenness_device(n, nnz, dGp, dBj, nnz, dGp, dBj, n, dSrc, 0, dBc, dLevel, dSigma, 0, 0);
    if (err != BHS_ERR_INVALID_ARG) { printf("a column equal to n: %d\n", err); return 1; }
    if (!fetch()) return 2;
    for (int v = 0; v < n; ++v)
        if (bc[v] != -7.0 || sigma[v] != -7.0 || level[v] != -7) { printf("a refused call wrote vertex %d\n", v); return 1; }

    // all sources in one call
    int reached = -1, passes = -1;
    err = bh.csr_betweenness_device(n, nnz, dGp, dGj, nnz, dGp, dGj, n, dSrc, 0, dBc, dLevel, dSigma, &reached, &passes);
    if (err) { printf("csr_betweenness_device: %d\n", err); return 1; }
    if (!fetch()) return 2;
    for (int v = 0; v < n; ++v) {
        if (memcmp(&bc[v], &want[v], sizeof(double)) != 0) { printf("vertex %d: %a, the host loop's %a\n", v, bc[v], want[v]); return 1; }
        if (level[v] != wantLevel[v] || memcmp(&sigma[v], &wantSigma[v], sizeof(double)) != 0) {
            printf("vertex %d of the last source: level %d sigma %a, the host loop's %d and %a\n", v, level[v], sigma[v], wantLevel[v], wantSigma[v]);
            return 1;
        }
    }
    if (reached != n * n || passes < 8 * n || passes % 8) { printf("reached %d, passes %d\n", reached, passes); return 1; }

    // the same in two chained calls
    const int half = n / 2;
    err = bh.csr_betweenness_device(n, nnz, dGp, dGj, nnz, dGp, dGj, half, dSrc, 0, dBc, 0, 0, 0, 0);
    if (!err) err = bh.csr_betweenness_device(n, nnz, dGp, dGj, nnz, dGp, dGj, n - half, dSrc + half, BHS_BC_ACCUMULATE, dBc, 0, 0, 0, 0);
    if (err) { printf("the chained calls: %d\n", err); return 1; }
    if (!fetch()) return 2;
    if (memcmp(bc.data(), want.data(), sizeof(double) * n) != 0) { printf("two chained calls differ from one\n"); return 1; }

    unsigned long long hash = 1469598103934665603ull;
    const unsigned char *bytes = (const unsigned char *)bc.data();
    for (size_t k = 0; k < sizeof(double) * (size_t)n; ++k) hash = (hash ^ bytes[k]) * 1099511628211ull;
    const int top = (int)(std::max_element(bc.begin(), bc.end()) - bc.begin());

    for (void *p : {(void *)dGp, (void *)dGj, (void *)dBj, (void *)dSrc, (void *)dBc, (void *)dSigma, (void *)dLevel}) (void)hipFree(p);
    bh.freePlatform();
    printf("betweenness of %d vertices, %d entries, %d lanes from all sources: levels %lld, passes %d; the most central vertex %d at %a; hash %016llx PASS\n",
           n, nnz, L, wantLevels, passes, top, bc[top], hash);
    return 0;
}
