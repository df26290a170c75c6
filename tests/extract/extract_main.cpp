// Z = X(rows, cols) through the C++ facade (host/bhsparse.h): from a 5 x 7 matrix with a row that is not ascending and
// holds a duplicate pair, an empty row, a NaN with a payload and a -0, four rows (one of them twice) and five columns in
// descending order are extracted on the device.  rowPtrZ, colIndZ, perm and the values' bits are compared with the result
// written out below.  Prints PASS and exits 0 on success.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
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

int main()
{
    const int m = 5, n = 7;
    //                         row 0: (0,2) twice | row 1 empty | row 2 | row 3      | row 4
    const std::vector<int> Xp = {0, 4, 4, 6, 9, 11};
    const std::vector<int> Xj = {5, 2, 0, 2, /**/ 1, 6, /**/ 0, 2, 3, /**/ 6, 5};
    std::vector<value_type> Xx = {1, 2, 3, 4, (value_type)-0.0, 5, std::numeric_limits<value_type>::quiet_NaN(), 6, 7, 8, 9};
    const int nnz = (int)Xj.size();
    const std::vector<int> rows = {3, 0, 1, 0}, cols = {6, 5, 2, 1, 0};
    const int mI = (int)rows.size(), nJ = (int)cols.size();
    // places: column 6 -> 0, 5 -> 1, 2 -> 2, 1 -> 3, 0 -> 4; column 3 and 4 are not named
    const std::vector<int> refZp = {0, 2, 6, 6, 10};
    const std::vector<int> refZj = {2, 4, /**/ 1, 2, 2, 4, /**/ 1, 2, 2, 4};
    const std::vector<int> refPerm = {7, 6, /**/ 0, 1, 3, 2, /**/ 0, 1, 3, 2};

    bool plat[NUM_PLATFORMS] = {false};
    plat[BHSPARSE_HIP] = true;
    bhsparse bh;
    int err = bh.initPlatform(plat);
    if (err) { printf("initPlatform: %d\n", err); return 2; }
    int *dXp = to_device(Xp), *dXj = to_device(Xj), *dRows = to_device(rows), *dCols = to_device(cols);
    value_type *dXx = to_device(Xx);
    const std::vector<int> zi(mI + 1, -7), zn(refZj.size(), -7);
    const std::vector<value_type> zv(refZj.size(), 0);
    int *dZp = to_device(zi), *dZj = to_device(zn), *dPerm = to_device(zn);
    value_type *dZx = to_device(zv);
    if (!dXp || !dXj || !dRows || !dCols || !dXx || !dZp || !dZj || !dPerm || !dZx) { printf("device memory\n"); return 2; }

    int nnzZ = -1;
    err = bh.csr_extract_symbolic_device(m, n, nnz, dXp, dXj, mI, dRows, nJ, dCols, dZp, &nnzZ);
    if (err) { printf("csr_extract_symbolic_device: %d\n", err); return 1; }
    if (nnzZ != (int)refZj.size()) { printf("nnz(Z) = %d\n", nnzZ); return 1; }
    err = bh.csr_extract_numeric_device(m, n, nnz, dXx, dXp, dXj, mI, dRows, nJ, dCols, nnzZ, dZp, dZj, dZx, dPerm);
    if (err) { printf("csr_extract_numeric_device: %d\n", err); return 1; }
    const std::vector<int> Zp = to_host(dZp, mI + 1), Zj = to_host(dZj, nnzZ), perm = to_host(dPerm, nnzZ);
    const std::vector<value_type> Zx = to_host(dZx, nnzZ);
    if (Zp != refZp || Zj != refZj || perm != refPerm) { printf("Z's pattern differs\n"); return 1; }
    for (int p = 0; p < nnzZ; ++p)
        if (memcmp(&Zx[p], &Xx[refPerm[p]], sizeof(value_type))) { printf("value %d differs\n", p); return 1; }

    // a repeated column is refused and the outputs stay as they are
    const std::vector<int> twice = {6, 5, 2, 5, 0};
    int *dTwice = to_device(twice);
    err = bh.csr_extract_symbolic_device(m, n, nnz, dXp, dXj, mI, dRows, nJ, dTwice, dZp, &nnzZ);
    if (err != BHS_ERR_INVALID_ARG || to_host(dZp, mI + 1) != refZp) { printf("a repeated column: %d\n", err); return 1; }

    for (void *p : {(void *)dXp, (void *)dXj, (void *)dRows, (void *)dCols, (void *)dXx, (void *)dZp, (void *)dZj, (void *)dPerm,
                    (void *)dZx, (void *)dTwice})
        (void)hipFree(p);
    bh.freePlatform();
    printf("extract %d x %d -> %d x %d, %d entries: PASS\n", m, n, mI, nJ, (int)refZj.size());
    return 0;
}
