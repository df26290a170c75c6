// C = select(A·A) through the C++ facade (host/bhsparse.h): poisson5pt 12 x 12.  First the strict lower triangle of A·A
// (band_hi = -1), then A·A pruned to its 3 largest entries per row; both are checked against the same rule applied on the
// host to the plain product.  Prints nnz(C); "select OK" and exit 0 on success.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../benchmark_spgemm_using_csr_amd/host/bhsparse.h"
#include "../../benchmark_spgemm_using_csr_amd/host/gallery.h"

int main()
{
    CsrHost A;
    gallery_poisson("poisson5pt", 12, 12, 1, A);
    fill_values(A.values);
    const int m = A.num_rows;
    std::vector<value_type> val(A.values.begin(), A.values.end());
    bool plat[NUM_PLATFORMS] = {false};
    plat[BHSPARSE_HIP] = true;
    bhsparse bh;
    int err = bh.initPlatform(plat);
    if (err) { printf("initPlatform: %d\n", err); return 2; }
    std::vector<int> Cp(m + 1);
    err = bh.initData(m, m, m, A.num_entries, val.data(), A.row_offsets.data(), A.column_indices.data(), A.num_entries,
                      val.data(), A.row_offsets.data(), A.column_indices.data(), Cp.data());
    if (!err) err = bh.spgemm();
    const int nnzP = bh.get_nnzC();
    std::vector<int> Pp(Cp), Pj(nnzP);
    std::vector<value_type> Px(nnzP);
    if (!err) err = bh.get_C(Pj.data(), Px.data());
    if (err) { printf("spgemm: %d\n", err); return 1; }

    bhs_select tril = {BHS_SEL_BAND, 0, INT64_MIN, -1, 0.0, 0.0};
    err = bh.spgemm_select(tril);
    if (err) { printf("spgemm_select(tril): %d\n", err); return 1; }
    const int nnzL = bh.get_nnzC();
    std::vector<int> Lj(nnzL);
    std::vector<value_type> Lx(nnzL);
    err = bh.get_C(Lj.data(), Lx.data());
    if (err) { printf("get_C: %d\n", err); return 1; }
    std::vector<int> refJ;
    std::vector<value_type> refX;
    for (int i = 0; i < m; ++i)
        for (int p = Pp[i]; p < Pp[i + 1]; ++p)
            if (Pj[p] < i) { refJ.push_back(Pj[p]); refX.push_back(Px[p]); }
    if (Lj != refJ || Lx != refX) { printf("tril(A*A, -1) differs\n"); return 1; }

    const int K = 3;
    bhs_select top = {BHS_SEL_TOPK, K, 0, 0, 0.0, 0.0};
    err = bh.spgemm_select(top);
    if (err) { printf("spgemm_select(topk): %d\n", err); return 1; }
    const int nnzT = bh.get_nnzC();
    std::vector<int> Tj(nnzT);
    std::vector<value_type> Tx(nnzT);
    err = bh.get_C(Tj.data(), Tx.data());
    if (err) { printf("get_C: %d\n", err); return 1; }
    refJ.clear();
    refX.clear();
    for (int i = 0; i < m; ++i) {
        std::vector<int> idx;
        for (int p = Pp[i]; p < Pp[i + 1]; ++p) idx.push_back(p);
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return std::fabs((double)Px[a]) > std::fabs((double)Px[b]); });
        if ((int)idx.size() > K) idx.resize(K);
        std::sort(idx.begin(), idx.end());
        for (int p : idx) { refJ.push_back(Pj[p]); refX.push_back(Px[p]); }
    }
    if (Tj != refJ || Tx != refX) { printf("top-%d of A*A differs\n", K); return 1; }
    bh.free_mem();
    bh.freePlatform();
    printf("nnz(A*A) = %d, nnz(tril) = %d, nnz(top-%d) = %d\n", nnzP, nnzL, K, nnzT);
    printf("select OK: %d rows\n", m);
    return 0;
}
