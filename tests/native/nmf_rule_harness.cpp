// Host build of embedding_amd/csrc/nmf_rule.h: the NMF rule of include/dge.h as a one-thread loop over the pieces every lane of nmf.hip runs, with std::fma.
// tests/test_nmf_host.py holds it to tests/nmf_ref.py bit for bit; tests/test_gpu_nmf.py holds the kernels to it at a size Python cannot reach.
//   g++ -O2 -shared -fPIC -std=c++17 -ffp-contract=off -o libnmf_rule_harness.so nmf_rule_harness.cpp
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -DNMF_HARNESS_MAIN -o nmf_rule_harness nmf_rule_harness.cpp   (a stand-alone program)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../embedding_amd/csrc/nmf_rule.h"

namespace {

// the entries by row (ri, ci, v; columns ascending inside a row) and their order by column (perm; rows ascending inside a column)
struct Entries {
    int64_t n, m, ne;
    const int32_t *ri, *ci;
    const double* v;
    std::vector<int64_t> rptr, cptr, perm;
};

void order(Entries& E) {
    E.rptr.assign((size_t)E.n + 1, 0); E.cptr.assign((size_t)E.m + 1, 0); E.perm.resize((size_t)E.ne);
    for (int64_t e = 0; e < E.ne; e++) { E.rptr[(size_t)E.ri[e] + 1]++; E.cptr[(size_t)E.ci[e] + 1]++; }
    for (int64_t i = 0; i < E.n; i++) E.rptr[(size_t)i + 1] += E.rptr[(size_t)i];
    for (int64_t j = 0; j < E.m; j++) E.cptr[(size_t)j + 1] += E.cptr[(size_t)j];
    std::vector<int64_t> at(E.cptr.begin(), E.cptr.end() - 1);
    for (int64_t e = 0; e < E.ne; e++) E.perm[(size_t)at[(size_t)E.ci[e]]++] = e;      // a counting sort keeps the rows ascending
}

// the blocked sum over x = 0 .. cnt-1 of X[x * sx + a] (dot == false) or of the rounded product X[x * sx + a] * X[x * sx + b]
double blocked(const double* X, int64_t cnt, int64_t sx, int64_t a, int64_t b, bool dot) {
    const int64_t nb = (cnt + NMF_BLOCK - 1) / NMF_BLOCK;
    std::vector<double> bs((size_t)nb);
    for (int64_t k = 0; k < nb; k++) {
        const int64_t lo = k * NMF_BLOCK, hi = lo + NMF_BLOCK < cnt ? lo + NMF_BLOCK : cnt;
        bs[(size_t)k] = dot ? nmf_block_dot(X + a, X + b, sx, lo, hi) : nmf_block_sum(X + a, sx, lo, hi);
    }
    return nmf_sum_blocks(bs.data(), 1, nb);
}

double p_of(const Entries& E, const double* W, const double* H, int rank, int64_t e) { return nmf_p(W + (size_t)E.ri[e] * rank, 1, H + E.ci[e], E.m, rank); }

void iteration(const Entries& E, double* W, double* H, int rank, int update) {
    const int64_t n = E.n, m = E.m;
    std::vector<double> Q((size_t)E.ne), num((size_t)(n > m ? n : m) * rank), den((size_t)rank * rank), old((size_t)rank);
    double part[NMF_LANES];
    // ---- H
    if (update == 0) for (int64_t e = 0; e < E.ne; e++) Q[(size_t)e] = E.v[e] / p_of(E, W, H, rank, e);
    for (int64_t j = 0; j < m; j++)
        for (int r = 0; r < rank; r++) {
            for (int l = 0; l < NMF_LANES; l++) part[l] = 0.0;
            for (int64_t c = E.cptr[(size_t)j], t = 0; c < E.cptr[(size_t)j + 1]; c++, t++) {
                const int64_t e = E.perm[(size_t)c];
                part[t % NMF_LANES] = nmf_seg_step(part[t % NMF_LANES], W[(size_t)E.ri[e] * rank + r], update == 0 ? Q[(size_t)e] : E.v[e]);
            }
            num[(size_t)j * rank + r] = nmf_seg_fold(part);
        }
    if (update == 0) for (int r = 0; r < rank; r++) den[(size_t)r] = blocked(W, n, rank, r, 0, false);
    else for (int r = 0; r < rank; r++) for (int s = 0; s < rank; s++) den[(size_t)r * rank + s] = blocked(W, n, rank, r, s, true);
    for (int64_t j = 0; j < m; j++) {
        for (int s = 0; s < rank; s++) old[(size_t)s] = H[(size_t)s * m + j];
        for (int r = 0; r < rank; r++) {
            double d = update == 0 ? den[(size_t)r] : 0.0;
            if (update == 1) for (int s = 0; s < rank; s++) d = fma(den[(size_t)r * rank + s], old[(size_t)s], d);
            H[(size_t)r * m + j] = nmf_update(old[(size_t)r], num[(size_t)j * rank + r], d);
        }
    }
    // ---- W
    if (update == 0) for (int64_t e = 0; e < E.ne; e++) Q[(size_t)e] = E.v[e] / p_of(E, W, H, rank, e);
    for (int64_t i = 0; i < n; i++)
        for (int r = 0; r < rank; r++) {
            for (int l = 0; l < NMF_LANES; l++) part[l] = 0.0;
            for (int64_t e = E.rptr[(size_t)i], t = 0; e < E.rptr[(size_t)i + 1]; e++, t++)
                part[t % NMF_LANES] = nmf_seg_step(part[t % NMF_LANES], update == 0 ? Q[(size_t)e] : E.v[e], H[(size_t)r * m + E.ci[e]]);
            num[(size_t)i * rank + r] = nmf_seg_fold(part);
        }
    if (update == 0) for (int r = 0; r < rank; r++) den[(size_t)r] = blocked(H, m, 1, (int64_t)r * m, 0, false);
    else for (int r = 0; r < rank; r++) for (int s = 0; s < rank; s++) den[(size_t)r * rank + s] = blocked(H, m, 1, (int64_t)r * m, (int64_t)s * m, true);
    for (int64_t i = 0; i < n; i++) {
        for (int s = 0; s < rank; s++) old[(size_t)s] = W[(size_t)i * rank + s];
        for (int r = 0; r < rank; r++) {
            double d = update == 0 ? den[(size_t)r] : 0.0;
            if (update == 1) for (int s = 0; s < rank; s++) d = fma(old[(size_t)s], den[(size_t)s * rank + r], d);
            W[(size_t)i * rank + r] = nmf_update(old[(size_t)r], num[(size_t)i * rank + r], d);
        }
    }
}

}  // namespace

extern "C" {

double harness_nmf_u(uint64_t seed, uint64_t t) { return nmf_u(seed, t); }
double harness_nmf_floor(double x) { return nmf_floor(x); }
double harness_nmf_update(double x, double num, double den) { return nmf_update(x, num, den); }
double harness_nmf_fma(double a, double b, double c) { return nmf_seg_step(c, a, b); }
double harness_nmf_segment_sum(const double* a, const double* b, int64_t count) {
    double part[NMF_LANES];
    for (int l = 0; l < NMF_LANES; l++) part[l] = 0.0;
    for (int64_t t = 0; t < count; t++) part[t % NMF_LANES] = nmf_seg_step(part[t % NMF_LANES], a[t], b[t]);
    return nmf_seg_fold(part);
}
double harness_nmf_blocked_sum(const double* v, int64_t count) { return blocked(v, count, 1, 0, 0, false); }

// ri, ci, v: the kept entries by row, columns ascending, no duplicate, every v > 0.  init_W / init_H: both or neither.  W [n x rank], H [rank x m].
int harness_nmf(const int32_t* ri, const int32_t* ci, const double* v, int64_t ne, int64_t n, int64_t m, int rank, int max_iter, int update, uint64_t seed, const double* init_W,
                const double* init_H, double* W, double* H, double* vmax_out) {
    if (ne < 1 || n < 1 || m < 1 || rank < 1 || rank > NMF_MAX_RANK || max_iter < 1 || (update != 0 && update != 1)) return 1;
    Entries E{n, m, ne, ri, ci, v, {}, {}, {}};
    for (int64_t e = 0; e < ne; e++) {
        if (ri[e] < 0 || ri[e] >= n || ci[e] < 0 || ci[e] >= m || !(v[e] > 0.0) || !std::isfinite(v[e])) return 2;
        if (e > 0 && (ri[e] < ri[e - 1] || (ri[e] == ri[e - 1] && ci[e] <= ci[e - 1]))) return 3;
    }
    order(E);
    double vmax = 0.0;
    for (int64_t e = 0; e < ne; e++) if (v[e] > vmax) vmax = v[e];
    for (int64_t i = 0; i < n; i++)
        for (int r = 0; r < rank; r++)
            W[(size_t)i * rank + r] = init_W ? nmf_floor(init_W[(size_t)i * rank + r]) : nmf_init(seed, (uint64_t)i * (uint64_t)rank + (uint64_t)r, vmax);
    for (int r = 0; r < rank; r++)
        for (int64_t j = 0; j < m; j++)
            H[(size_t)r * m + j] = init_H ? nmf_floor(init_H[(size_t)r * m + j]) : nmf_init(seed, (uint64_t)n * (uint64_t)rank + (uint64_t)r * (uint64_t)m + (uint64_t)j, vmax);
    for (int it = 0; it < max_iter; it++) iteration(E, W, H, rank, update);
    if (vmax_out) *vmax_out = vmax;
    return 0;
}

}  // extern "C"

#ifdef NMF_HARNESS_MAIN
// a stand-alone run for the sanitizers: a generated matrix with an empty row, an empty column and a full row, both updates; prints a checksum of the bits
int main() {
    const int64_t n = 70, m = 53;
    std::vector<int32_t> ri, ci;
    std::vector<double> v;
    for (int64_t i = 0; i < n; i++)
        for (int64_t j = 0; j < m; j++) {
            if (i == 7 || j == 11) continue;
            const uint64_t h = dge_mix64((uint64_t)(i * m + j));
            if (i == 20 || h % 9 == 0) { ri.push_back((int32_t)i); ci.push_back((int32_t)j); v.push_back((double)(1 + h % 50)); }
        }
    uint64_t sum = 0;
    for (int update = 0; update < 2; update++)
        for (int rank : {1, 3, 32}) {
            std::vector<double> W((size_t)n * rank), H((size_t)rank * m);
            double vmax = 0.0;
            const int rc = harness_nmf(ri.data(), ci.data(), v.data(), (int64_t)v.size(), n, m, rank, 4, update, 12345, nullptr, nullptr, W.data(), H.data(), &vmax);
            if (rc) { std::printf("harness_nmf: %d\n", rc); return 1; }
            for (double x : W) { uint64_t b; std::memcpy(&b, &x, 8); sum = sum * 31 + b; if (!(x >= NMF_EPS)) { std::printf("W below the floor\n"); return 1; } }
            for (double x : H) { uint64_t b; std::memcpy(&b, &x, 8); sum = sum * 31 + b; if (!(x >= NMF_EPS)) { std::printf("H below the floor\n"); return 1; } }
            if (H[11] != NMF_EPS || W[(size_t)7 * rank] != NMF_EPS) { std::printf("an empty row or column is not at the floor\n"); return 1; }
        }
    std::printf("nmf_rule_harness ok: %zu entries, checksum %016llx\n", v.size(), (unsigned long long)sum);
    return 0;
}
#endif
