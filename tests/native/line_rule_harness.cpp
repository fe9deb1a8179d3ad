// Host build of embedding_amd/csrc/line_rule.h: the LINE rule of include/dge.h as a one-thread loop over the pieces every lane of line.hip runs, with std::fma.
// tests/test_line_host.py holds it to tests/line_ref.py bit for bit; tests/test_gpu_line.py holds the kernels to it at a size Python cannot reach.
//   g++ -O2 -shared -fPIC -std=c++17 -ffp-contract=off -o libline_rule_harness.so line_rule_harness.cpp
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -DLINE_HARNESS_MAIN -o line_rule_harness line_rule_harness.cpp   (a stand-alone program)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../embedding_amd/csrc/line_rule.h"

namespace {

const double* sig_table() {
    static double T[LINE_SIG_N];
    static bool done = false;
    if (!done) { for (int k = 0; k < LINE_SIG_N; k++) T[k] = line_sig_entry(k); done = true; }
    return T;
}

}  // namespace

extern "C" {

uint64_t harness_line_seed2(uint64_t seed) { return line_seed2(seed); }
double harness_line_u(uint64_t seed2, uint64_t t) { return line_u(seed2, t); }
int64_t harness_line_quant(double x) { return line_quant(x); }
double harness_line_value(int64_t P) { return line_value(P); }
int64_t harness_line_init_cell(uint64_t seed2, uint64_t t, int dim) { return line_init_cell(seed2, t, dim); }
int64_t harness_line_search(const int64_t* C, int64_t cnt, uint64_t r, int64_t total) { return line_search(C, cnt, r, total); }
int64_t harness_line_neg_weight(int64_t d) { return line_neg_weight(d); }
uint64_t harness_line_draw(uint64_t seed, uint64_t s, uint64_t d) { return line_draw(seed, s, d); }
double harness_line_rho(double rho0, int64_t first, int64_t samples) { return line_rho(rho0, first, samples); }
double harness_line_sig_entry(int k) { return line_sig_entry(k); }
double harness_line_sig(double f) { return line_sig(sig_table(), f); }
double harness_line_dot(const double* a, const double* b, int dim) { return line_dot(a, b, dim); }
int64_t harness_line_term(double g, double x) { return line_term(g, x); }

// The rule on the kept edges in (src, dst) order (es, ed, ew: ne of them).  init_X / init_Y: host doubles or NULL.  X, Y: double[n x dim]; touched: uint8[n];
// totals: W, N, the greatest |P|, the batches.  -> 0; 1: a bad argument; 2: the bound is left after batch *over (the outputs are then untouched).
int harness_line(const int32_t* es, const int32_t* ed, const int64_t* ew, int64_t ne, int64_t n, int dim, int order, int K, int64_t batch, int64_t samples, double rho0, uint64_t seed,
                 const double* init_X, const double* init_Y, double* X, double* Y, uint8_t* touched, int64_t* totals, int64_t* over) {
    if (ne < 1 || n < 1 || n > LINE_MAX_N || dim < 1 || dim > LINE_MAX_DIM || (order != 1 && order != 2) || K < 0 || K > LINE_MAX_NEG || batch < 1 || batch > LINE_MAX_BATCH ||
        samples < 1 || samples > LINE_MAX_SAMPLES || !(rho0 > 0.0 && rho0 <= 1.0) || (init_Y && !init_X)) return 1;
    const size_t cells = (size_t)n * (size_t)dim;
    std::vector<int64_t> C((size_t)ne), d((size_t)n, 0), NC((size_t)n), PX(cells), PY(cells, 0), DX(cells, 0), DY(order == 2 ? cells : 0, 0);
    std::vector<uint8_t> mark((size_t)n, 0);
    int64_t run = 0;
    for (int64_t e = 0; e < ne; e++) {
        if (es[e] < 0 || es[e] >= n || ed[e] < 0 || ed[e] >= n || ew[e] < 1 || ew[e] >= LINE_MAX_WEIGHT) return 1;
        run += ew[e]; C[(size_t)e] = run; d[(size_t)es[e]] += ew[e];
        mark[(size_t)es[e]] = 1; mark[(size_t)ed[e]] = 1;
    }
    const int64_t W = run;
    if (W >= LINE_MAX_TOTAL) return 1;
    run = 0;
    for (int64_t v = 0; v < n; v++) { run += line_neg_weight(d[(size_t)v]); NC[(size_t)v] = run; }
    const int64_t N = run;
    const uint64_t s2 = line_seed2(seed);
    for (size_t t = 0; t < cells; t++) {
        if (init_X && !(std::isfinite(init_X[t]) && std::fabs(init_X[t]) < LINE_INIT_LIMIT)) return 1;
        if (init_Y && !(std::isfinite(init_Y[t]) && std::fabs(init_Y[t]) < LINE_INIT_LIMIT)) return 1;
        PX[t] = init_X ? line_quant(init_X[t]) : line_init_cell(s2, (uint64_t)t, dim);
        if (init_Y) PY[t] = line_quant(init_Y[t]);
    }
    const double* T = sig_table();
    std::vector<int64_t>& PB = order == 1 ? PX : PY;
    std::vector<int64_t>& DB = order == 1 ? DX : DY;
    const int64_t batches = (samples + batch - 1) / batch;
    std::vector<int32_t> dr((size_t)batch * (size_t)(K + 2));
    std::vector<double> A((size_t)dim), B((size_t)dim);
    for (int64_t b = 0; b < batches; b++) {
        const int64_t first = b * batch, cnt = samples - first < batch ? samples - first : batch;
        const double rho = line_rho(rho0, first, samples);
        for (int64_t s = 0; s < cnt; s++) {
            int32_t* o = dr.data() + (size_t)s * (size_t)(K + 2);
            const int64_t e = line_search(C.data(), ne, line_draw(seed, (uint64_t)(first + s), 0), W);
            o[0] = es[e]; o[1] = ed[e];
            for (int k = 1; k <= K; k++) o[1 + k] = (int32_t)line_search(NC.data(), n, line_draw(seed, (uint64_t)(first + s), (uint64_t)k), N);
            const size_t u = (size_t)o[0] * (size_t)dim;
            for (int j = 0; j < dim; j++) A[(size_t)j] = line_value(PX[u + j]);
            for (int k = 0; k <= K; k++) {
                const size_t t = (size_t)o[1 + k] * (size_t)dim;
                for (int j = 0; j < dim; j++) B[(size_t)j] = line_value(PB[t + j]);
                const double g = line_g(k == 0 ? 1.0 : 0.0, line_sig(T, line_dot(A.data(), B.data(), dim)), rho);
                for (int j = 0; j < dim; j++) {
                    DB[t + j] += line_term(g, A[(size_t)j]);
                    DX[u + j] += line_term(g, B[(size_t)j]);
                }
            }
        }
        bool left = false;
        for (int64_t i = 0; i < cnt * (K + 2); i++) {
            const bool target = (i % (K + 2)) != 0 && order != 1;
            std::vector<int64_t>& P = target ? PY : PX;
            std::vector<int64_t>& D = target ? DY : DX;
            const size_t row = (size_t)dr[(size_t)i] * (size_t)dim;
            for (int j = 0; j < dim; j++) {
                const int64_t dl = D[row + j];
                if (dl == 0) continue;
                D[row + j] = 0;
                P[row + j] += dl;
                if (line_cell_over(P[row + j])) left = true;
            }
        }
        if (left) { *over = b; return 2; }
    }
    int64_t big = 0;
    for (size_t t = 0; t < cells; t++) {
        const int64_t a = PX[t] < 0 ? -PX[t] : PX[t], c = PY[t] < 0 ? -PY[t] : PY[t];
        if (a > big) big = a;
        if (c > big) big = c;
    }
    for (size_t t = 0; t < cells; t++) { X[t] = line_value(PX[t]); if (Y) Y[t] = line_value(PY[t]); }
    if (touched) std::memcpy(touched, mark.data(), (size_t)n);
    totals[0] = W; totals[1] = N; totals[2] = big; totals[3] = batches;
    return 0;
}

}  // extern "C"

#ifdef LINE_HARNESS_MAIN
// a graph of 23 vertices: a ring with chords, a hub every vertex points at, a vertex without out-edges and an isolated one; both orders, K = 0 and 5, dims around 16;
// then a run that leaves the bound
int main() {
    const int64_t n = 23;
    std::vector<int32_t> es, ed;
    std::vector<int64_t> ew;
    for (int32_t i = 0; i < 21; i++)                 // vertex 21 has no out-edge, vertex 22 no edge at all
        for (int32_t j = 0; j < 22; j++)
            if (j == 3 || j == (i + 1) % 21 || (j == 21 && i % 5 == 0) || (i == j && i == 7) || (i * 7 + j * 3) % 11 == 0) { es.push_back(i); ed.push_back(j); ew.push_back(1 + (i * 5 + j) % 9); }
    uint64_t sum = 0;
    const int dims[] = {1, 15, 16, 17, 33};
    for (int order = 1; order <= 2; order++)
        for (int K = 0; K <= 5; K += 5)
            for (int dim : dims) {
                std::vector<double> X((size_t)n * dim), Y((size_t)n * dim);
                std::vector<uint8_t> touched((size_t)n);
                int64_t totals[4], over = -1;
                const int rc = harness_line(es.data(), ed.data(), ew.data(), (int64_t)ew.size(), n, dim, order, K, 7, 300, 0.025, 12345, nullptr, nullptr, X.data(), Y.data(), touched.data(),
                                            totals, &over);
                if (rc) { std::printf("harness_line: %d\n", rc); return 1; }
                if (touched[21] != 1 || touched[22] != 0) { std::printf("touched is wrong\n"); return 1; }
                for (int j = 0; j < dim; j++)
                    if (X[(size_t)22 * dim + j] != line_value(line_init_cell(line_seed2(12345), (uint64_t)(22 * dim + j), dim))) { std::printf("an isolated vertex moved\n"); return 1; }
                if (order == 1) for (double y : Y) if (y != 0.0) { std::printf("order 1 wrote Y\n"); return 1; }
                for (double x : X) { uint64_t b; std::memcpy(&b, &x, 8); sum = sum * 31 + b; }
                for (double y : Y) { uint64_t b; std::memcpy(&b, &y, 8); sum = sum * 31 + b; }
            }
    {
        const int dim = 4;
        std::vector<double> init((size_t)n * dim, 255.9), X((size_t)n * dim, 9.0), Y((size_t)n * dim, 7.0);
        int64_t totals[4], over = -1;
        const int rc = harness_line(es.data(), ed.data(), ew.data(), (int64_t)ew.size(), n, dim, 1, 2, 8, 100, 1.0, 1, init.data(), nullptr, X.data(), Y.data(), nullptr, totals, &over);
        if (rc != 2 || over != 0) { std::printf("the bound: rc %d, batch %lld\n", rc, (long long)over); return 1; }
        for (double x : X) if (x != 9.0) { std::printf("an output was written\n"); return 1; }
    }
    std::printf("line_rule_harness ok: %zu edges, checksum %016llx\n", ew.size(), (unsigned long long)sum);
    return 0;
}
#endif
