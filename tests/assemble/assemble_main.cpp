// The assembly through the C++ facade (host/bhsparse.h), every array on the device.  A 24 x 17 mesh of quadrilaterals gives 16
// contributions an element, element after element -- up to four to an entry between two vertices of one element, up to nine
// runs a row; the vertices on the left edge are constrained and carry the index -1, which BHS_COO_IGNORE_NEGATIVE drops.  Z is
// compared entry by entry with a std::map on the host (small integer values: every order of adding is exact), the map is
// checked for shape, then new values go through coo_assemble_values_device and are compared again; without the flag the same
// triplets must be refused with the outputs untouched.  Prints the counts and exits 0 on success, non-zero on a status
// code or a wrong answer.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../benchmark_spgemm_using_csr_amd/host/bhsparse.h"

template <typename T>
static T *to_device(const std::vector<T> &v, size_t room)
{
    T *d = 0;
    if (hipMalloc((void **)&d, (room > 0 ? room : 1) * sizeof(T)) != hipSuccess) return 0;
    const size_t count = v.size() < room ? v.size() : room;           // (the head of v where it is longer than the room)
    if (count && hipMemcpy(d, v.data(), count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return 0;
    return d;
}

template <typename T>
static bool to_host(std::vector<T> &v, const T *d, size_t count)
{
    v.resize(count);
    return count == 0 || hipMemcpy(v.data(), d, count * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess;
}

typedef std::map<std::pair<int, int>, double> Ref;

static bool same(const Ref &want, int m, const std::vector<int> &Zp, const std::vector<int> &Zj, const std::vector<value_type> &Zx,
                 const char *what)
{
    if ((size_t)Zp[m] != want.size()) { printf("%s: %d entries, expected %zu\n", what, Zp[m], want.size()); return false; }
    Ref::const_iterator it = want.begin();
    for (int i = 0; i < m; ++i)
        for (int q = Zp[i]; q < Zp[i + 1]; ++q, ++it)
            if (it->first != std::make_pair(i, Zj[q]) || it->second != (double)Zx[q]) {
                printf("%s: entry %d is (%d, %d, %g), expected (%d, %d, %g)\n", what, q, i, Zj[q], (double)Zx[q], it->first.first,
                       it->first.second, it->second);
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

    const int ex = 24, ey = 17, nx = ex + 1, n = nx * (ey + 1);
    std::vector<int> rows, cols;
    std::vector<value_type> v0, v1;
    Ref want0, want1;
    for (int y = 0; y < ey; ++y)
        for (int x = 0; x < ex; ++x) {
            const int corner[4] = {y * nx + x, y * nx + x + 1, (y + 1) * nx + x, (y + 1) * nx + x + 1};
            for (int a = 0; a < 4; ++a)
                for (int b = 0; b < 4; ++b) {
                    const int i = corner[a] % nx == 0 ? -1 : corner[a], j = corner[b] % nx == 0 ? -1 : corner[b];
                    const double w0 = a == b ? 4 : -1 - (x + y + a) % 2, w1 = (x * 3 + y * 5 + a * 4 + b) % 7 - 3;
                    rows.push_back(i); cols.push_back(j); v0.push_back((value_type)w0); v1.push_back((value_type)w1);
                    if (i >= 0 && j >= 0) { want0[std::make_pair(i, j)] += w0; want1[std::make_pair(i, j)] += w1; }
                }
        }
    const int nnzIn = (int)rows.size();
    int *dRows = to_device(rows, rows.size()), *dCols = to_device(cols, cols.size());
    value_type *dV0 = to_device(v0, v0.size()), *dV1 = to_device(v1, v1.size());
    const std::vector<int> sentinel((size_t)nnzIn + 1, -77);
    int *dZp = to_device(sentinel, (size_t)n + 1), *dZj = to_device(sentinel, nnzIn), *dEnt = to_device(sentinel, (size_t)nnzIn + 1),
        *dPerm = to_device(sentinel, nnzIn);
    value_type *dZx = to_device(std::vector<value_type>(), nnzIn);
    if (!dRows || !dCols || !dV0 || !dV1 || !dZp || !dZj || !dEnt || !dPerm || !dZx) { printf("device memory\n"); return 2; }

    // a negative index without the flag: refused, nothing written
    int nnzZ = -1, nkept = -1;
    err = bh.coo_assemble_device(n, n, nnzIn, dRows, dCols, dV0, BHS_COO_SUM, dZp, dZj, dZx, dEnt, dPerm, &nnzZ, &nkept);
    std::vector<int> Zp, Zj, ent, perm;
    if (err != BHS_ERR_INVALID_ARG || !to_host(Zp, dZp, (size_t)n + 1) || !to_host(Zj, dZj, nnzIn) || Zp[0] != -77 || Zp[n] != -77 ||
        Zj[0] != -77) {
        printf("negative indices without the flag: %d, or an output was written\n", err);
        return 1;
    }
    err = bh.coo_assemble_device(n, n, nnzIn, dRows, dCols, dV0, BHS_COO_SUM | BHS_COO_IGNORE_NEGATIVE, dZp, dZj, dZx, dEnt, dPerm, &nnzZ,
                                 &nkept);
    if (err) { printf("coo_assemble_device: %d\n", err); return 1; }
    std::vector<value_type> Zx;
    if (nnzZ < 0 || nnzZ > nkept || nkept > nnzIn) { printf("%d entries from %d kept of %d\n", nnzZ, nkept, nnzIn); return 1; }
    if (!to_host(Zp, dZp, (size_t)n + 1) || !to_host(Zj, dZj, nnzZ) || !to_host(Zx, dZx, nnzZ) || !to_host(ent, dEnt, (size_t)nnzZ + 1) ||
        !to_host(perm, dPerm, nkept)) return 2;
    if (!same(want0, n, Zp, Zj, Zx, "assembly")) return 1;
    if (ent[0] != 0 || ent[nnzZ] != nkept) { printf("entryPtr runs from %d to %d, %d kept\n", ent[0], ent[nnzZ], nkept); return 1; }
    for (int i = 0, q = 0; i < n; ++i)
        for (; q < Zp[i + 1]; ++q)
            for (int k = ent[q]; k < ent[q + 1]; ++k)
                if (rows[perm[k]] != i || cols[perm[k]] != Zj[q] || (k > ent[q] && perm[k] <= perm[k - 1])) {
                    printf("map: position %d of entry %d names triplet %d\n", k, q, perm[k]);
                    return 1;
                }

    // new values on the same connectivity
    err = bh.coo_assemble_values_device(nnzIn, dV1, nnzZ, dEnt, dPerm, BHS_COO_SUM, dZx);
    if (err) { printf("coo_assemble_values_device: %d\n", err); return 1; }
    if (!to_host(Zx, dZx, nnzZ) || !same(want1, n, Zp, Zj, Zx, "new values")) return 1;
    err = bh.coo_assemble_values_device(nnzIn, dV1, nnzZ, dEnt, dPerm, BHS_COO_KEEP, dZx);
    if (err != BHS_ERR_INVALID_ARG) { printf("BHS_COO_KEEP in the values call: %d\n", err); return 1; }

    for (void *p : {(void *)dRows, (void *)dCols, (void *)dV0, (void *)dV1, (void *)dZp, (void *)dZj, (void *)dEnt, (void *)dPerm, (void *)dZx})
        (void)hipFree(p);
    bh.freePlatform();
    printf("assembly of %d contributions on %d vertices: %d kept, %d entries; new values through the map PASS\n", nnzIn, n, nkept, nnzZ);
    return 0;
}
