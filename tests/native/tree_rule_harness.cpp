// Host build of embedding_amd/csrc/tree_rule.h: the per-element pieces every lane of tree.hip runs — the value key, the score, the ONE comparator, the
// threshold, the leaf test and the vote — handed to tests/test_tree_host.py through ctypes.  Build with -ffp-contract=off.
// Built as a program (its own main) with -fsanitize=address,undefined it walks the comparator and the threshold over generated and extreme inputs and prints
// what it saw.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../embedding_amd/csrc/tree_rule.h"

extern "C" {
uint32_t harness_tree_key(float x) { return tr_key(x); }
float harness_tree_unkey(uint32_t k) { return tr_unkey(k); }
void harness_tree_score(int64_t n, int64_t p, int64_t nL, int64_t pL, uint64_t* N, uint64_t* Dn) { tr_score(n, p, nL, pL, N, Dn); }
int harness_tree_score_cmp(uint64_t N1, uint64_t D1, uint64_t N2, uint64_t D2) { return tr_score_cmp(N1, D1, N2, D2); }
// does the cut (nL1, pL1) of feature f1 at key a1 win against (nL2, pL2, f2, a2) in a node of n rows, p of label 1?
int harness_tree_better(int64_t n, int64_t p, int64_t nL1, int64_t pL1, int32_t f1, uint32_t a1, int64_t nL2, int64_t pL2, int32_t f2, uint32_t a2) {
    tr_cand x{0, 0, f1, a1}, y{0, 0, f2, a2};
    tr_score(n, p, nL1, pL1, &x.N, &x.D);
    tr_score(n, p, nL2, pL2, &y.N, &y.D);
    return tr_better(x, y) ? 1 : 0;
}
int harness_tree_better_raw(uint64_t N1, uint64_t D1, int32_t f1, uint32_t a1, uint64_t N2, uint64_t D2, int32_t f2, uint32_t a2) {
    return tr_better(tr_cand{N1, D1, f1, a1}, tr_cand{N2, D2, f2, a2}) ? 1 : 0;
}
double harness_tree_threshold(float a, float b) { return tr_threshold(a, b); }
int harness_tree_goes_left(float x, double m) { return tr_goes_left(x, m) ? 1 : 0; }
int harness_tree_is_leaf(int64_t n, int64_t p, int32_t depth, int32_t max_depth, int32_t min_split, int32_t min_leaf) {
    return tr_is_leaf(n, p, depth, tr_limits{max_depth, min_split, min_leaf}) ? 1 : 0;
}
int harness_tree_valid_cut(int64_t n, int64_t nL, int32_t min_leaf) { return tr_valid_cut(n, nL, tr_limits{0, 2, min_leaf}) ? 1 : 0; }
int harness_tree_vote(int64_t n, int64_t p) { return tr_vote(n, p); }
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 200000;
    uint64_t st = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    auto next = [&]() { st = st * 6364136223846793005ULL + 1442695040888963407ULL; return st >> 11; };
    int64_t bad = 0;
    for (int r = 0; r < rounds; r++) {
        const int64_t n = 2 + (int64_t)(next() % (uint64_t)(r % 3 ? TR_MAX_ROWS - 1 : 40));
        const int64_t p = (int64_t)(next() % (uint64_t)(n + 1));
        tr_cand c[2];
        for (int s = 0; s < 2; s++) {
            const int64_t nL = 1 + (int64_t)(next() % (uint64_t)(n - 1));
            const int64_t lo = p - (n - nL) > 0 ? p - (n - nL) : 0, hi = p < nL ? p : nL;
            const int64_t pL = lo + (int64_t)(next() % (uint64_t)(hi - lo + 1));
            tr_score(n, p, nL, pL, &c[s].N, &c[s].D);
            c[s].f = (int32_t)(next() % 3); c[s].a = (uint32_t)(next() % 3) + 1;
            if (c[s].N > (1ULL << 58) || c[s].D > (1ULL << 38) || c[s].D == 0) bad++;
        }
        const unsigned __int128 l = (unsigned __int128)c[0].N * c[1].D, q = (unsigned __int128)c[1].N * c[0].D;
        const bool want = l != q ? l > q : (c[0].f != c[1].f ? c[0].f < c[1].f : c[0].a < c[1].a);
        if (tr_better(c[0], c[1]) != want) bad++;
        if (tr_better(c[0], c[1]) && tr_better(c[1], c[0])) bad++;
        uint32_t ka = (uint32_t)next(), kb = (uint32_t)next();
        if (ka == kb || !tr_finite_bits(tr_unkey_bits(ka)) || !tr_finite_bits(tr_unkey_bits(kb))) continue;
        if (ka > kb) { const uint32_t t = ka; ka = kb; kb = t; }
        const float a = tr_unkey(ka), b = tr_unkey(kb);
        if (tr_key(a) == tr_key(b)) continue;                    // the two zeros
        const double m = tr_threshold(a, b);
        if (!(a < b) || !((double)a <= m && m < (double)b) || !tr_goes_left(a, m) || tr_goes_left(b, m)) bad++;
    }
    if (tr_key(-0.0f) != tr_key(0.0f) || tr_vote(4, 2) != 0 || tr_vote(5, 3) != 1) bad++;
    printf("rounds %d wrong %lld\n", rounds, (long long)bad);
    return bad ? 1 : 0;
}
