// The semiring multiply through the C++ facade (host/bhsparse.h): min-plus A^2 of a small weighted path graph -- the
// lengths of the shortest walks of exactly two edges.  spgemm_semiring's C must have the pattern of A·A and the values of a
// dense min-plus product; spgemm_semiring_masked on that pattern plus one entry no walk reaches must give the same values
// and +Inf there.  Prints "semiring PASS" and exits 0 on success.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../benchmark_spgemm_using_csr_amd/host/bhsparse.h"

int main()
{
    const int n = 9;
    const double inf = std::numeric_limits<double>::infinity();
    // node i -- node i+1 with weight 1.5 + i (both directions), node 0 with a loop of weight 0.25
    std::vector<int> Ap(n + 1, 0), Aj;
    std::vector<value_type> Ax;
    std::vector<double> dense(n * n, inf);
    for (int i = 0; i < n; ++i) {
        if (i == 0) { Aj.push_back(0); Ax.push_back(0.25); dense[0] = 0.25; }
        if (i > 0) { Aj.push_back(i - 1); Ax.push_back(1.5 + (i - 1)); dense[i * n + i - 1] = 1.5 + (i - 1); }
        if (i + 1 < n) { Aj.push_back(i + 1); Ax.push_back(1.5 + i); dense[i * n + i + 1] = 1.5 + i; }
        Ap[i + 1] = (int)Aj.size();
    }
    const int nnzA = (int)Aj.size();
    bool plat[NUM_PLATFORMS] = {false};
    plat[BHSPARSE_HIP] = true;
    bhsparse bh;
    int err = bh.initPlatform(plat);
    if (err) { printf("initPlatform: %d\n", err); return 2; }
    std::vector<int> Cp(n + 1);
    err = bh.initData(n, n, n, nnzA, Ax.data(), Ap.data(), Aj.data(), nnzA, Ax.data(), Ap.data(), Aj.data(), Cp.data());
    if (!err) err = bh.spgemm_semiring(BHS_SR_MIN_PLUS);
    if (err) { printf("spgemm_semiring: %d\n", err); return 1; }
    const int nnzC = bh.get_nnzC();
    std::vector<int> Cj(nnzC);
    std::vector<value_type> Cx(nnzC);
    err = bh.get_C(Cj.data(), Cx.data());
    if (err) { printf("get_C: %d\n", err); return 1; }
    int bad = 0, entries = 0;
    for (int i = 0; i < n; ++i) {
        int p = Cp[i];
        for (int j = 0; j < n; ++j) {
            double best = inf;
            bool any = false;
            for (int k = 0; k < n; ++k)
                if (dense[i * n + k] < inf && dense[k * n + j] < inf) { any = true; best = std::fmin(best, dense[i * n + k] + dense[k * n + j]); }
            if (!any) continue;
            ++entries;
            if (p >= Cp[i + 1] || Cj[p] != j || Cx[p] != (value_type)best) ++bad;
            ++p;
        }
        if (p != Cp[i + 1]) ++bad;
    }
    if (entries != nnzC) ++bad;
    // the masked call: C's pattern, and in the last row one more column (0: eight edges away)
    std::vector<int> Mp(n + 1), Mj;
    for (int i = 0; i < n; ++i) {
        Mp[i] = (int)Mj.size();
        if (i == n - 1) Mj.push_back(0);
        for (int p = Cp[i]; p < Cp[i + 1]; ++p) Mj.push_back(Cj[p]);
    }
    Mp[n] = (int)Mj.size();
    std::vector<value_type> Mx(Mj.size(), (value_type)-1);
    err = bh.spgemm_semiring_masked(BHS_SR_MIN_PLUS, Mp.data(), Mj.data(), (int)Mj.size(), Mx.data());
    if (err) { printf("spgemm_semiring_masked: %d\n", err); return 1; }
    for (int i = 0; i < n; ++i)
        for (int p = Cp[i]; p < Cp[i + 1]; ++p) bad += Mx[Mp[i] + (p - Cp[i]) + (i == n - 1 ? 1 : 0)] != Cx[p];
    bad += Mx[Mp[n - 1]] != (value_type)inf;
    bh.free_mem();
    bh.freePlatform();
    if (bad) { printf("semiring values differ in %d places\n", bad); return 1; }
    printf("semiring PASS: min-plus A^2 of a path of %d nodes, %d entries\n", n, nnzC);
    return 0;
}
