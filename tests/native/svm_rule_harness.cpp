// Host build of embedding_amd/csrc/svm_rule.h: the per-element pieces every lane of svm.hip runs and svm_solve_host, the whole rule as one plain host loop over
// them, handed to tests/test_svm_host.py, tests/test_gpu_svm.py and scripts/svm_rate.py through ctypes.  Build with -ffp-contract=off.
// Built as a program (its own main) with -fsanitize=address,undefined it solves generated tables at block edges and prints what it saw.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../embedding_amd/csrc/svm_rule.h"

extern "C" {
double harness_svm_exp(double x) { return sw_exp_neg(x); }
// K: [n x n]
int harness_svm_kernel(const float* x, int32_t n, int dim, double gamma, double* K) {
    if (n < 1 || n > SV_MAX_ROWS || dim < 1 || dim > SV_MAX_DIM) return -1;
    svm_kernel_host(x, n, dim, gamma, K);
    return 0;
}
// sgn: int8 [n], +1 / -1 / 0; alpha, G, coef: [n]; out: bias; counts: iterations, converged, support
int harness_svm_solve(const double* K, int32_t n, const int8_t* sgn, double C, double eps, int64_t max_iter, double* alpha, double* G, double* coef, double* bias, int64_t* counts) {
    if (n < 1 || n > SV_MAX_ROWS) return -1;
    int32_t conv = 0;
    counts[0] = svm_solve_host(K, n, sgn, C, eps, max_iter, alpha, G, bias, &conv);
    counts[1] = conv; counts[2] = 0;
    for (int32_t t = 0; t < n; t++) { coef[t] = sgn[t] ? sv_coef(sgn[t], alpha[t]) : 0.0; if (coef[t] != 0.0) counts[2]++; }
    return 0;
}
// f(x) for the rows whose kernel rows are Kx [nx x n]; coef [n]: 0 or NaN = not support
int harness_svm_decide(const double* Kx, int32_t nx, int32_t n, const double* coef, double bias, double* out) {
    std::vector<int32_t> sup;
    std::vector<double> c;
    for (int32_t t = 0; t < n; t++) if (coef[t] != 0.0 && coef[t] == coef[t]) { sup.push_back(t); c.push_back(coef[t]); }
    for (int32_t r = 0; r < nx; r++) out[r] = sv_decide(Kx + (size_t)r * (size_t)n, sup.data(), c.data(), (int64_t)sup.size(), bias);
    return 0;
}
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 2;
    uint64_t st = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    auto next = [&]() { st = st * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(st >> 11) * 0x1.0p-53; };
    int64_t bad = 0, rows_seen = 0, updates = 0;
    const int32_t ns[] = {2, 3, 63, 64, 65, 255, 256, 257, 300};
    for (int round = 0; round < rounds; round++)
        for (int32_t n : ns) {
            const int dim = 1 + (int)(next() * 9);
            const double C = round % 2 ? 0.25 : 4.0, gamma = 1.0 / dim;
            std::vector<float> x((size_t)n * dim);
            std::vector<int8_t> sgn((size_t)n);
            for (int32_t t = 0; t < n; t++) {
                sgn[(size_t)t] = t % 7 == 6 ? 0 : (next() < 0.5 ? 1 : -1);            // every seventh row does not train
                for (int c = 0; c < dim; c++) x[(size_t)t * dim + c] = (float)(next() * 4.0 - 2.0 + sgn[(size_t)t]);
            }
            sgn[0] = 1; sgn[1] = -1;
            if (n > 8) for (int c = 0; c < dim; c++) x[(size_t)(n - 1) * dim + c] = x[c];      // a repeated row: the a <= 0 branch when the pair is chosen
            if (n > 8) sgn[(size_t)n - 1] = -1;
            std::vector<double> K((size_t)n * n), alpha((size_t)n), G((size_t)n), coef((size_t)n), out((size_t)n);
            double bias = 0.0;
            int64_t counts[3];
            if (harness_svm_kernel(x.data(), n, dim, gamma, K.data())) { bad++; continue; }
            if (harness_svm_solve(K.data(), n, sgn.data(), C, 1e-3, 1000000, alpha.data(), G.data(), coef.data(), &bias, counts)) { bad++; continue; }
            harness_svm_decide(K.data(), n, n, coef.data(), bias, out.data());
            rows_seen += n; updates += counts[0];
            if (counts[1] != 1) bad++;
            for (int32_t t = 0; t < n; t++) {
                if (!(alpha[(size_t)t] >= 0.0 && alpha[(size_t)t] <= C)) bad++;
                if (!sgn[(size_t)t] && alpha[(size_t)t] != 0.0) bad++;
                if (K[(size_t)t * n + t] != 1.0) bad++;
                if (!(out[(size_t)t] == out[(size_t)t])) bad++;
            }
        }
    // one class: nothing to do, the bias is the class
    {
        const double K[4] = {1.0, 0.5, 0.5, 1.0};
        const int8_t sgn[2] = {-1, -1};
        double alpha[2], G[2], coef[2], bias = 0.0;
        int64_t counts[3];
        harness_svm_solve(K, 2, sgn, 1.0, 1e-3, 10, alpha, G, coef, &bias, counts);
        if (counts[0] != 0 || counts[1] != 1 || counts[2] != 0 || bias != -1.0) bad++;
    }
    printf("rounds %d rows %lld updates %lld wrong %lld\n", rounds, (long long)rows_seen, (long long)updates, (long long)bad);
    return bad ? 1 : 0;
}
