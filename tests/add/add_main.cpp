// C = A·A + A through the C++ facade (host/bhsparse.h): poisson5pt 12 x 12.  A has a full diagonal, so A sits inside the
// pattern of A·A and the sum has A·A's pattern.  Prints nnz(C) and a checksum; "add OK" and exit 0 on success.
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
    std::vector<int> Cp(m + 1), Sp(m + 1);
    err = bh.initData(m, m, m, A.num_entries, val.data(), A.row_offsets.data(), A.column_indices.data(), A.num_entries,
                      val.data(), A.row_offsets.data(), A.column_indices.data(), Cp.data());
    if (!err) err = bh.spgemm();
    const int nnzP = bh.get_nnzC();
    std::vector<int> Pj(nnzP);
    std::vector<value_type> Px(nnzP);
    if (!err) err = bh.get_C(Pj.data(), Px.data());
    if (err) { printf("spgemm: %d\n", err); return 1; }
    double sumP = 0, sumA = 0, sumC = 0;
    for (value_type v : Px) sumP += v;
    for (value_type v : val) sumA += v;
    err = bh.spgemm_add(1, 1, A.num_entries, val.data(), A.row_offsets.data(), A.column_indices.data());
    if (err) { printf("spgemm_add: %d\n", err); return 1; }
    const int nnzC = bh.get_nnzC();
    std::vector<int> Cj(nnzC);
    std::vector<value_type> Cx(nnzC);
    err = bh.get_C(Cj.data(), Cx.data());
    if (err) { printf("get_C: %d\n", err); return 1; }
    for (value_type v : Cx) sumC += v;
    bh.free_mem();
    bh.freePlatform();
    printf("nnz(C) = %d, checksum = %.17g\n", nnzC, sumC);
    if (nnzC != nnzP || Cj != Pj || sumC != sumP + sumA) { printf("A*A + A differs from A*A plus A\n"); return 1; }   // (integer values: sums are exact)
    printf("add OK: %d rows\n", m);
    return 0;
}
