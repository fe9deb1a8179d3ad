// Host build of embedding_amd/csrc/ridge_rule.h: the per-element pieces every lane of ridge.hip runs and rg_solve_host, the whole rule as one plain host loop
// over them, handed to tests/test_ridge_host.py, tests/test_gpu_ridge.py and scripts/ridge_rate.py through ctypes.  Build with -ffp-contract=off.
// Built as a program (its own main) with -fsanitize=address,undefined it solves generated tables at block edges and prints what it saw.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../embedding_amd/csrc/ridge_rule.h"

extern "C" {
// the outputs as rg_solve_host lays them out; why: kind, lambda, index.  -> 0, or the refusal's kind; -1: arguments outside the limits
int harness_ridge(const float* x, const double* y, int64_t n, int dim, int T, const double* lambda, int nl, double* M, double* d, double* L, double* beta, double* h,
                  double* e, double* mae, double* mre, int64_t* why) {
    if (n < 2 || dim < 1 || dim > RG_MAX_DIM || T < 1 || T > RG_MAX_TARGETS || nl < 1 || nl > RG_MAX_LAMBDA) return -1;
    rg_refusal r;
    const int rc = rg_solve_host(x, y, n, dim, T, lambda, nl, M, d, L, beta, h, e, mae, mre, &r);
    why[0] = r.kind; why[1] = r.lambda; why[2] = r.index;
    return rc;
}
double harness_ridge_predict(const float* x, const double* beta, int dim) { return rg_predict(x, beta, dim); }
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 4;
    uint64_t st = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    auto next = [&]() { st = st * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(st >> 11) * 0x1.0p-53; };
    int64_t bad = 0, rows_seen = 0;
    const int64_t ns[] = {2, 5, 255, 256, 257, 700};
    for (int round = 0; round < rounds; round++)
        for (int64_t n : ns) {
            const int dim = 1 + (int)(next() * 9), T = 1 + (int)(next() * 3), nl = 1 + (int)(next() * 3), P = dim + 1;
            std::vector<float> x((size_t)n * dim);
            std::vector<double> y((size_t)n * T), lam((size_t)nl);
            for (auto& v : x) v = (float)(next() * 4.0 - 2.0);
            for (auto& v : y) v = next() * 10.0;
            for (auto& v : lam) v = 0.5 + next();
            std::vector<double> M((size_t)P * (P + T)), d((size_t)nl * P), L((size_t)nl * P * P), beta((size_t)nl * T * P), h((size_t)nl * n), e((size_t)nl * T * n), mae((size_t)nl * T),
                mre((size_t)nl * T);
            int64_t why[3];
            if (harness_ridge(x.data(), y.data(), n, dim, T, lam.data(), nl, M.data(), d.data(), L.data(), beta.data(), h.data(), e.data(), mae.data(), mre.data(), why)) { bad++; continue; }
            rows_seen += n;
            for (double v : d) if (!(v > 0.0)) bad++;
            for (double v : h) if (!(v >= 0.0 && v < 1.0)) bad++;
            for (double v : mae) if (!(v >= 0.0)) bad++;
        }
    // the two refusals: a column twice under lambda = 0, and two rows with nothing to spare under lambda = 0
    {
        const float x[] = {1, 1, 2, 2, 3, 3, 5, 5};
        const double y[] = {1, 2, 3, 4}, lam[] = {1.0, 0.0};
        double M[3 * 4], d[2 * 3], L[2 * 9], beta[2 * 3], h[2 * 4], e[2 * 4], mae[2], mre[2];
        int64_t why[3];
        if (harness_ridge(x, y, 4, 2, 1, lam, 2, M, d, L, beta, h, e, mae, mre, why) != RG_PIVOT || why[1] != 1 || why[2] != 2) bad++;
        const float x2[] = {1, 3};
        const double lam0[] = {0.0};
        if (harness_ridge(x2, y, 2, 1, 1, lam0, 1, M, d, L, beta, h, e, mae, mre, why) != RG_LEVERAGE || why[1] != 0 || why[2] != 0) bad++;
    }
    printf("rounds %d rows %lld wrong %lld\n", rounds, (long long)rows_seen, (long long)bad);
    return bad ? 1 : 0;
}
