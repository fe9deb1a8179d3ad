// Host build of embedding_amd/csrc/pairwise_rule.h for tests/test_pairwise_host.py: the ground distances, the ground order's ranks and the ideal DCG prefixes of
// the pairwise evaluation's rule (include/dge.h), by plain loops over the header's pieces.  g++ -O2 -ffp-contract=off.
#include <algorithm>
#include <vector>

#include "../../embedding_amd/csrc/pairwise_rule.h"

// dist [n x n] (the diagonal holds dist(a, a), which nothing reads); present may be null
extern "C" int harness_pw_distances(const float* x, const uint8_t* present, int32_t n, int32_t g, double* dist) {
    std::vector<double> ss((size_t)n);
    std::vector<uint8_t> live((size_t)n);
    for (int r = 0; r < n; r++) {
        double s = 0.0;
        for (int j = 0; j < g; j++) s = pw_step(s, x[(size_t)r * g + j], x[(size_t)r * g + j]);
        ss[r] = s;
        live[r] = (!present || present[r]) && pw_live(s);
    }
    for (int a = 0; a < n; a++)
        for (int b = 0; b < n; b++)
            dist[(size_t)a * n + b] = pw_dist_rows(x + (size_t)a * g, x + (size_t)b * g, g, ss[a], ss[b], live[a] != 0, live[b] != 0);
    return 0;
}

// rank int32 [n x n] (-1 on the diagonal), ideal_idx int32 [n x kmax], ideal binary64 [n_k x n]; kmax = ks[n_k - 1] <= n - 1
extern "C" int harness_pw_order(const double* dist, int32_t n, const int32_t* ks, int32_t n_k, int32_t* rank, int32_t* ideal_idx, double* ideal) {
    const int kmax = ks[n_k - 1];
    if (kmax > n - 1 || kmax > PW_MAX_K) return 1;
    std::vector<int32_t> order;
    for (int r = 0; r < n; r++) {
        const double* d = dist + (size_t)r * n;
        order.clear();
        for (int c = 0; c < n; c++) if (c != r) order.push_back(c);
        std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return pw_key_less(d[a], a, d[b], b); });
        rank[(size_t)r * n + r] = -1;
        for (int i = 0; i < n - 1; i++) rank[(size_t)r * n + order[i]] = i;
        double acc = 0.0;
        int j = 0;
        for (int i = 0; i < kmax; i++) {
            ideal_idx[(size_t)r * kmax + i] = order[i];
            acc = pw_gain(acc, d[order[i]], pw_disc_host(i));
            if (j < n_k && i == ks[j] - 1) { ideal[(size_t)j * n + r] = acc; j++; }
        }
    }
    return 0;
}

// ratio of one region from its neighbours' distances: the chain cut at every k, over the given ideal values
extern "C" int harness_pw_ratios(const double* nb_dist, const int32_t* ks, int32_t n_k, const double* ideal, double* ratio) {
    double acc = 0.0;
    int j = 0;
    for (int i = 0; i < ks[n_k - 1]; i++) {
        acc = pw_gain(acc, nb_dist[i], pw_disc_host(i));
        if (j < n_k && i == ks[j] - 1) { ratio[j] = pw_ratio(acc, ideal[j]); j++; }
    }
    return 0;
}
