// The masked multiply through the C++ facade (host/bhsparse.h): poisson5pt 12 x 12, M = pattern(A·A) from the ordinary
// multiply plus one entry no product lands on.  The masked values must equal get_C's and the extra entry must read 0;
// get_C's result must be the same after the masked call.  Prints "masked OK" and exits 0 on success.
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
    const int nnzC = bh.get_nnzC();
    std::vector<int> Cj(nnzC);
    std::vector<value_type> Cx(nnzC);
    if (!err) err = bh.get_C(Cj.data(), Cx.data());
    if (err) { printf("spgemm: %d\n", err); return 1; }
    // M: C's pattern, and in row 0 one more column (m - 1: poisson5pt^2 reaches 2 rows away, not to the far corner)
    std::vector<int> Mp(m + 1), Mj;
    int extra = -1;
    for (int i = 0; i < m; ++i) {
        Mp[i] = (int)Mj.size();
        for (int p = Cp[i]; p < Cp[i + 1]; ++p) Mj.push_back(Cj[p]);
        if (i == 0) { extra = (int)Mj.size(); Mj.push_back(m - 1); }
    }
    Mp[m] = (int)Mj.size();
    std::vector<value_type> Mx(Mj.size(), (value_type)-1);
    err = bh.spgemm_masked(Mp.data(), Mj.data(), (int)Mj.size(), Mx.data());
    if (err) { printf("spgemm_masked: %d\n", err); return 1; }
    int bad = Mx[extra] != 0;
    for (int i = 0; i < m; ++i)
        for (int p = Cp[i]; p < Cp[i + 1]; ++p) bad += Mx[Mp[i] + (p - Cp[i])] != Cx[p];   // (row 0's extra entry comes after its own)
    std::vector<int> Cj2(nnzC);
    std::vector<value_type> Cx2(nnzC);
    err = bh.get_C(Cj2.data(), Cx2.data());
    if (err || Cj2 != Cj || Cx2 != Cx) { printf("get_C after the masked call differs (%d)\n", err); return 1; }
    bh.free_mem();
    bh.freePlatform();
    if (bad) { printf("masked values differ in %d entries\n", bad); return 1; }
    printf("masked OK: %d rows, %zu mask entries\n", m, Mj.size());
    return 0;
}
