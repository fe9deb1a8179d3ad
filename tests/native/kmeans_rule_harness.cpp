// Host build of embedding_amd/csrc/kmeans_rule.h and cluster_match.h: the per-element pieces every lane of kmeans.hip runs, and a whole clustering as a plain
// host loop over them, handed to tests/test_kmeans_host.py (and, for a larger case, tests/test_gpu_kmeans.py) through ctypes.  Build with -ffp-contract=off.
// Built as a program (its own main) with -fsanitize=address,undefined it clusters generated tables at block and tile edges, scores them, and prints what it saw.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../embedding_amd/csrc/kmeans_rule.h"
#include "../../embedding_amd/csrc/cluster_match.h"

struct km_result {
    int64_t rows, total_iterations;
    int32_t best_restart, iterations, scale_bits, empty;
    double inertia;
};

static void block_sums(const double* v, int64_t n, std::vector<double>& bs) {
    bs.clear();
    for (int64_t lo = 0; lo < n; lo += KM_BLOCK) bs.push_back(km_block_sum(v, lo, lo + KM_BLOCK < n ? lo + KM_BLOCK : n));
}

static int64_t pick_row(const double* dmin, int64_t n, double u) {
    std::vector<double> bs;
    block_sums(dmin, n, bs);
    int64_t i = km_walk(dmin, bs.data(), n, u * km_sum_blocks(bs.data(), (int64_t)bs.size()));
    if (i < 0) { i = 0; for (int64_t r = 1; r < n; r++) if (dmin[r] > dmin[i]) i = r; }
    return i;
}

// the rule of include/dge.h on n selected rows, one row after another; 0, or 1 for arguments outside the limits
static int kmeans_host(const float* x, int64_t n, int dim, int k, uint64_t seed, int n_init, int max_iter, const float* init, int32_t* labels, float* centres, km_result* res) {
    if (k < 1 || k > KM_MAX_K || dim < 1 || dim > KM_MAX_DIM || n < k || n_init < 1 || max_iter < 1) return 1;
    const size_t kd = (size_t)k * (size_t)dim;
    float max_abs = 0.0f;
    for (size_t e = 0; e < (size_t)n * (size_t)dim; e++) { const float a = fabsf(x[e]); if (!(a <= 3.4028234663852886e38f)) return 1; if (a > max_abs) max_abs = a; }
    const int s = km_scale_bits(max_abs, n);
    std::vector<float> cen(kd);
    std::vector<int32_t> lab((size_t)n);
    std::vector<double> d((size_t)n), dmin((size_t)n), bs;
    std::vector<int64_t> S(kd), count((size_t)k);
    bool have = false;
    res->total_iterations = 0;
    if (init) n_init = 1;
    for (int r = 0; r < n_init; r++) {
        if (init) memcpy(cen.data(), init, kd * sizeof(float));
        else {
            int64_t p = km_first_pick(seed, r, k, n);
            memcpy(cen.data(), x + (size_t)p * dim, (size_t)dim * sizeof(float));
            for (int c = 1; c < k; c++) {
                for (int64_t i = 0; i < n; i++) {
                    const double v = km_dist(x + (size_t)i * dim, cen.data() + (size_t)(c - 1) * dim, dim);
                    if (c == 1 || v < dmin[(size_t)i]) dmin[(size_t)i] = v;
                }
                p = pick_row(dmin.data(), n, km_draw(seed, r, k, c));
                memcpy(cen.data() + (size_t)c * dim, x + (size_t)p * dim, (size_t)dim * sizeof(float));
            }
        }
        std::fill(lab.begin(), lab.end(), -1);
        int iter = 0;
        for (;;) {
            int64_t changed = 0;
            std::fill(S.begin(), S.end(), (int64_t)0);
            std::fill(count.begin(), count.end(), (int64_t)0);
            for (int64_t i = 0; i < n; i++) {
                const float* xi = x + (size_t)i * dim;
                int bc = 0;
                double bd = km_dist(xi, cen.data(), dim);
                for (int c = 1; c < k; c++) { const double v = km_dist(xi, cen.data() + (size_t)c * dim, dim); if (v < bd) { bd = v; bc = c; } }
                if (lab[(size_t)i] != bc) changed++;
                lab[(size_t)i] = bc; d[(size_t)i] = bd;
                count[(size_t)bc]++;
                for (int j = 0; j < dim; j++) S[(size_t)bc * dim + j] += km_quantise(xi[j], s);
            }
            iter++;
            if (changed == 0 || iter == max_iter) break;
            for (int c = 0; c < k; c++)
                if (count[(size_t)c] > 0) for (int j = 0; j < dim; j++) cen[(size_t)c * dim + j] = km_centre_from_sum(S[(size_t)c * dim + j], count[(size_t)c], s);
        }
        res->total_iterations += iter;
        block_sums(d.data(), n, bs);
        const double inertia = km_sum_blocks(bs.data(), (int64_t)bs.size());
        if (!have || inertia < res->inertia) {
            have = true;
            res->inertia = inertia; res->best_restart = r; res->iterations = iter; res->empty = 0;
            for (int c = 0; c < k; c++) if (count[(size_t)c] == 0) res->empty++;
            memcpy(labels, lab.data(), (size_t)n * sizeof(int32_t));
            memcpy(centres, cen.data(), kd * sizeof(float));
        }
    }
    res->rows = n; res->scale_bits = s;
    return 0;
}

extern "C" {
double harness_dist(const float* x, const float* c, int dim) { return km_dist(x, c, dim); }
void harness_dist_all(const float* x, int64_t n, int dim, const float* c, int k, double* out) {
    for (int64_t i = 0; i < n; i++) for (int a = 0; a < k; a++) out[i * k + a] = km_dist(x + (size_t)i * dim, c + (size_t)a * dim, dim);
}
double harness_fma_sq_add(double t, double acc) { return fma(t, t, acc); }
int harness_scale_bits(float max_abs, int64_t n) { return km_scale_bits(max_abs, n); }
void harness_quantise(const float* x, int64_t n, int s, int64_t* out) { for (int64_t i = 0; i < n; i++) out[i] = km_quantise(x[i], s); }
float harness_centre_from_sum(int64_t sum, int64_t count, int s) { return km_centre_from_sum(sum, count, s); }
int64_t harness_first_pick(uint64_t seed, int64_t r, int k, int64_t n) { return km_first_pick(seed, r, k, n); }
double harness_draw(uint64_t seed, int64_t r, int k, int c) { return km_draw(seed, r, k, c); }
double harness_blocked_sum(const double* v, int64_t n) {
    std::vector<double> bs;
    block_sums(v, n, bs);
    return km_sum_blocks(bs.data(), (int64_t)bs.size());
}
// the walk alone (-1: no row exceeds the target) and the pick with its fall-back
int64_t harness_walk(const double* v, int64_t n, double target) {
    std::vector<double> bs;
    block_sums(v, n, bs);
    return km_walk(v, bs.data(), n, target);
}
int64_t harness_pick(const double* dmin, int64_t n, double u) { return pick_row(dmin, n, u); }
int harness_kmeans(const float* x, int64_t n, int dim, int k, uint64_t seed, int n_init, int max_iter, const float* init, int32_t* labels, float* centres, km_result* res) {
    return kmeans_host(x, n, dim, k, seed, n_init, max_iter, init, labels, centres, res);
}
int harness_accuracy(const int32_t* labels, const int32_t* gnd, int64_t n, int32_t k, int64_t* cnt, int32_t* map, double* acc) {
    int64_t n_gnd = 0;
    if (cm_contingency(labels, gnd, n, k, cnt, &n_gnd) >= 0) return 1;
    *acc = cm_accuracy(cm_greedy_map(cnt, k, map), n_gnd);
    return 0;
}
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 12;
    uint64_t st = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    auto next = [&]() { st = st * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(st >> 11) * 0x1.0p-53; };
    int64_t bad = 0, rows_seen = 0;
    const int64_t ns[] = {1, 5, 63, 64, 65, 255, 256, 257, 513};
    for (int round = 0; round < rounds; round++) {
        for (int64_t n : ns) {
            const int dim = 1 + (int)(next() * 9), k = (int)(1 + next() * (double)(n < 8 ? n : 8)), blobs = 1 + (int)(next() * 4);
            const double mag = round % 4 == 3 ? 0x1p120 : (round % 4 == 2 ? 0.0 : 1.0);
            std::vector<float> x((size_t)n * dim), cen((size_t)k * dim);
            for (int64_t i = 0; i < n; i++) for (int j = 0; j < dim; j++) x[(size_t)i * dim + j] = (float)(mag * ((double)(i % blobs) * 4.0 + next()));
            std::vector<int32_t> lab((size_t)n), gnd((size_t)n), map((size_t)k);
            std::vector<int64_t> cnt((size_t)k * k);
            km_result res;
            if (kmeans_host(x.data(), n, dim, k, st, 2, 30, nullptr, lab.data(), cen.data(), &res)) { bad++; continue; }
            rows_seen += n;
            if (!(res.inertia >= 0.0) || res.rows != n || res.iterations < 1 || res.iterations > 30 || res.empty < 0 || res.empty >= k) bad++;
            for (int64_t i = 0; i < n; i++) { if (lab[(size_t)i] < 0 || lab[(size_t)i] >= k) bad++; gnd[(size_t)i] = i % 7 == 0 ? -1 : (int32_t)(i % k); }
            double acc = -1.0;
            if (harness_accuracy(lab.data(), gnd.data(), n, k, cnt.data(), map.data(), &acc)) bad++;
            if (!(acc != acc) && !(acc >= 0.0 && acc <= 1.0)) bad++;
            std::vector<uint8_t> seen((size_t)k, 0);
            for (int c = 0; c < k; c++) { if (map[(size_t)c] < 0 || map[(size_t)c] >= k || seen[(size_t)map[(size_t)c]]) bad++; else seen[(size_t)map[(size_t)c]] = 1; }
        }
    }
    // the quantiser at its extremes and the walk at block edges
    if (km_quantise(3.4028234663852886e38f, km_scale_bits(3.4028234663852886e38f, 1)) <= 0 || km_quantise(0.0f, km_scale_bits(0.0f, 5)) != 0) bad++;
    if (km_quantise(0.5f, 0) != 0 || km_quantise(1.5f, 0) != 2 || km_quantise(-2.5f, 0) != -2) bad++;
    std::vector<double> v(600, 1.0);
    for (int64_t want : {0, 255, 256, 511, 512, 599}) if (harness_walk(v.data(), 600, (double)want + 0.5) != want) bad++;
    if (harness_walk(v.data(), 600, 600.0) != -1 || harness_pick(v.data(), 600, 0.999999999) != 599) bad++;
    std::vector<double> z(300, 0.0);
    if (harness_pick(z.data(), 300, 0.7) != 0) bad++;
    printf("rounds %d rows %lld wrong %lld\n", rounds, (long long)rows_seen, (long long)bad);
    return bad ? 1 : 0;
}
