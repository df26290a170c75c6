// Reverse Cuthill-McKee through the C++ facade (host/bhsparse.h): a 40 x 50 five-point grid, a path of 300 and 17 single
// vertices under one seeded shuffle of the 2317 labels, every array on the device.  Checks the permutation against a queue
// algorithm on the host -- per component in ascending smallest vertex, from the start the device reports, a dequeued vertex
// appending its unnumbered neighbours by ascending (degree, index), the whole reversed --, that the grid's bandwidth comes
// out at 40 and the path's at 1, and that a pattern with one mirror entry missing is refused; prints the counts and exits 0
// on success, non-zero on a status code or a wrong answer.
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
    const int nx = 40, ny = 50, path = 300, single = 17, n = nx * ny + path + single;
    unsigned seed = 1357u;
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
    for (int k = 0; k + 1 < path; ++k) join(nx * ny + k, nx * ny + k + 1);
    for (int i = 0; i < n; i += 2) rows[i].push_back(i);             // a diagonal on every other row: allowed and ignored
    std::vector<int> Sp(n + 1, 0), Sj, deg(n);
    for (int i = 0; i < n; ++i) {
        std::sort(rows[i].begin(), rows[i].end());
        deg[i] = (int)rows[i].size() - (i % 2 == 0 ? 1 : 0);
        Sj.insert(Sj.end(), rows[i].begin(), rows[i].end());
        Sp[i + 1] = (int)Sj.size();
    }
    const int nnz = (int)Sj.size();

    bool plat[NUM_PLATFORMS] = {false};
    plat[BHSPARSE_HIP] = true;
    bhsparse bh;
    int err = bh.initPlatform(plat);
    if (err) { printf("initPlatform: %d\n", err); return 2; }
    int *dSp = to_device(Sp, Sp.size()), *dSj = to_device(Sj, Sj.size());
    int *dPerm = to_device(std::vector<int>(), (size_t)n), *dLevel = to_device(std::vector<int>(), (size_t)n);
    int *dStart = to_device(std::vector<int>(), (size_t)n);
    if (!dSp || !dSj || !dPerm || !dLevel || !dStart) { printf("device memory\n"); return 2; }

    int ncomp = -1, depth = -1, sweeps = -1, passes = -1;
    err = bh.csr_rcm_device(n, nnz, dSp, dSj, BHS_RCM_PERIPHERAL, dPerm, dLevel, dStart, &ncomp, &depth, &sweeps, &passes);
    if (err) { printf("csr_rcm_device: %d\n", err); return 1; }
    if (ncomp != 2 + single || sweeps < 2 || passes < 8 || passes % 8) {
        printf("ncomp %d, sweeps %d, passes %d\n", ncomp, sweeps, passes);
        return 1;
    }
    std::vector<int> perm(n), start(ncomp);
    if (hipMemcpy(perm.data(), dPerm, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(start.data(), dStart, sizeof(int) * ncomp, hipMemcpyDeviceToHost) != hipSuccess) return 2;

    // the host's queue from the device's starts; a start must belong to the component of its number
    std::vector<int> queue, number(n, -1);
    std::vector<char> taken(n, 0);
    int c = 0;
    for (int r = 0; r < n; ++r) {                                     // ascending smallest vertex
        if (taken[r]) continue;
        if (c >= ncomp) { printf("more components than %d\n", ncomp); return 1; }
        size_t head = queue.size();
        queue.push_back(start[c]);
        taken[start[c]] = 1;
        while (head < queue.size()) {
            const int u = queue[head++];
            std::vector<int> fresh;
            for (int q = Sp[u]; q < Sp[u + 1]; ++q)
                if (!taken[Sj[q]]) { taken[Sj[q]] = 1; fresh.push_back(Sj[q]); }
            std::sort(fresh.begin(), fresh.end(), [&](int a, int b) { return deg[a] != deg[b] ? deg[a] < deg[b] : a < b; });
            queue.insert(queue.end(), fresh.begin(), fresh.end());
        }
        if (!taken[r]) { printf("start %d is not in the component of vertex %d\n", start[c], r); return 1; }
        ++c;
    }
    if (c != ncomp || (int)queue.size() != n) { printf("components on the host %d, vertices %d\n", c, (int)queue.size()); return 1; }
    for (int k = 0; k < n; ++k)
        if (perm[k] != queue[n - 1 - k]) { printf("place %d: vertex %d, on the host %d\n", k, perm[k], queue[n - 1 - k]); return 1; }
    for (int k = 0; k < n; ++k) number[perm[k]] = k;
    int band[2] = {0, 0};                                             // of the grid's rows, of the path's
    for (int a = 0; a < nx * ny + path; ++a) {
        const int i = label[a];
        for (int q = Sp[i]; q < Sp[i + 1]; ++q) band[a < nx * ny ? 0 : 1] = std::max(band[a < nx * ny ? 0 : 1], std::abs(number[i] - number[Sj[q]]));
    }
    if (band[0] != nx || band[1] != 1) { printf("bandwidths %d and %d\n", band[0], band[1]); return 1; }

    // the Cuthill-McKee order itself is the same list backwards
    err = bh.csr_rcm_device(n, nnz, dSp, dSj, BHS_RCM_PERIPHERAL | BHS_RCM_NO_REVERSE, dPerm, 0, 0, 0, 0, 0, 0);
    std::vector<int> forward(n);
    if (err || hipMemcpy(forward.data(), dPerm, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess) { printf("no reverse: %d\n", err); return 1; }
    if (forward != queue) { printf("the order without the reversal\n"); return 1; }

    // one mirror entry missing: refused
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
    err = bh.csr_rcm_device(n, nnz - 1, dBp, dBj, 0, dPerm, 0, 0, 0, 0, 0, 0);
    if (err != BHS_ERR_INVALID_ARG) { printf("a missing mirror entry: %d\n", err); return 1; }

    for (void *p : {(void *)dSp, (void *)dSj, (void *)dPerm, (void *)dLevel, (void *)dStart, (void *)dBp, (void *)dBj}) (void)hipFree(p);
    bh.freePlatform();
    printf("reverse Cuthill-McKee of %d vertices, %d entries: ncomp %d, depth %d, sweeps %d, passes %d, bandwidths %d and %d PASS\n", n, nnz,
           ncomp, depth, sweeps, passes, band[0], band[1]);
    return 0;
}
