// (X^T)^T through the C++ facade (host/bhsparse.h): a 6 x 9 matrix with an empty row, an empty column, rows that are not
// ascending and a duplicate pair is transposed twice on the device.  X^T is checked against a counting transpose on the
// host, perm against the values it moved, and (X^T)^T against X with every row stably sorted by column.  Prints PASS and
// exits 0 on success.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
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
static std::vector<T> to_host(const T *d, size_t count)
{
    std::vector<T> v(count);
    if (count && hipMemcpy(v.data(), d, count * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) v.clear();
    return v;
}

static bool same_bits(const std::vector<value_type> &a, const std::vector<value_type> &b)
{
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(value_type)));
}

int main()
{
    const int m = 6, n = 9;
    const std::vector<int> Xp = {0, 4, 4, 7, 9, 13, 14};
    const std::vector<int> Xj = {7, 0, 3, 0, /* row 1 empty */ 8, 2, 1, 3, 3, 6, 0, 2, 1, 8};   // column 4 and 5 empty; (0,0) and (3,3) twice
    std::vector<value_type> Xx(Xj.size());
    for (size_t i = 0; i < Xx.size(); ++i) Xx[i] = (value_type)(1.5 + (double)i);
    Xx[3] = (value_type)-0.0;
    const int nnz = (int)Xj.size();

    bool plat[NUM_PLATFORMS] = {false};
    plat[BHSPARSE_HIP] = true;
    bhsparse bh;
    int err = bh.initPlatform(plat);
    if (err) { printf("initPlatform: %d\n", err); return 2; }
    int *dXp = to_device(Xp), *dXj = to_device(Xj);
    value_type *dXx = to_device(Xx);
    std::vector<int> zi(std::max(n, m) + 1, 0), zn(nnz, 0);
    std::vector<value_type> zv(nnz, 0);
    int *dTp = to_device(zi), *dTj = to_device(zn), *dPerm = to_device(zn), *dUp = to_device(zi), *dUj = to_device(zn);
    value_type *dTx = to_device(zv), *dUx = to_device(zv);
    if (!dXp || !dXj || !dXx || !dTp || !dTj || !dPerm || !dUp || !dUj || !dTx || !dUx) { printf("device memory\n"); return 2; }

    err = bh.csr_transpose_device(m, n, nnz, dXx, dXp, dXj, dTp, dTj, dTx, dPerm);
    if (err) { printf("csr_transpose_device(X): %d\n", err); return 1; }
    err = bh.csr_transpose_device(n, m, nnz, dTx, dTp, dTj, dUp, dUj, dUx, 0);
    if (err) { printf("csr_transpose_device(X^T): %d\n", err); return 1; }
    const std::vector<int> Tp = to_host(dTp, n + 1), Tj = to_host(dTj, nnz), perm = to_host(dPerm, nnz);
    const std::vector<int> Up = to_host(dUp, m + 1), Uj = to_host(dUj, nnz);
    const std::vector<value_type> Tx = to_host(dTx, nnz), Ux = to_host(dUx, nnz);

    // the counting transpose: entries in the order of their position, each to the next free place of its column
    std::vector<int> refTp(n + 1, 0), refTj(nnz), refPerm(nnz);
    std::vector<value_type> refTx(nnz);
    for (int q = 0; q < nnz; ++q) ++refTp[Xj[q] + 1];
    std::partial_sum(refTp.begin(), refTp.end(), refTp.begin());
    std::vector<int> next(refTp.begin(), refTp.end() - 1);
    for (int i = 0; i < m; ++i)
        for (int q = Xp[i]; q < Xp[i + 1]; ++q) {
            const int at = next[Xj[q]]++;
            refTj[at] = i; refTx[at] = Xx[q]; refPerm[at] = q;
        }
    if (Tp != refTp || Tj != refTj || perm != refPerm || !same_bits(Tx, refTx)) { printf("X^T differs\n"); return 1; }

    // X with every row stably sorted by column
    std::vector<int> refUj(nnz);
    std::vector<value_type> refUx(nnz);
    for (int i = 0; i < m; ++i) {
        std::vector<int> idx(Xp[i + 1] - Xp[i]);
        std::iota(idx.begin(), idx.end(), Xp[i]);
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return Xj[a] < Xj[b]; });
        for (size_t t = 0; t < idx.size(); ++t) { refUj[Xp[i] + t] = Xj[idx[t]]; refUx[Xp[i] + t] = Xx[idx[t]]; }
    }
    if (Up != Xp || Uj != refUj || !same_bits(Ux, refUx)) { printf("(X^T)^T differs from the row-sorted X\n"); return 1; }

    for (void *p : {(void *)dXp, (void *)dXj, (void *)dXx, (void *)dTp, (void *)dTj, (void *)dPerm, (void *)dUp, (void *)dUj,
                    (void *)dTx, (void *)dUx})
        (void)hipFree(p);
    bh.freePlatform();
    printf("transpose %d x %d, %d entries: PASS\n", m, n, nnz);
    return 0;
}
