// cluster_match.h — the clustering accuracy of the reference's evaluation (P/embeddingEvaluation_tract.py:544-571): the contingency table of cluster labels
// against ground labels and the greedy one-to-one map of clusters to labels.  Plain host C++, O(rows + k^2 log k); the rule is written out in include/dge.h.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

// cnt[a * k + g] = rows with labels == a and gnd == g, both >= 0; *n_gnd = rows with gnd >= 0.  Returns -1, or the least row that holds a value outside [-1, k).
inline int64_t cm_contingency(const int32_t* labels, const int32_t* gnd, int64_t n_rows, int32_t k, int64_t* cnt, int64_t* n_gnd) {
    std::fill(cnt, cnt + (size_t)k * (size_t)k, (int64_t)0);
    *n_gnd = 0;
    for (int64_t i = 0; i < n_rows; i++) {
        const int32_t a = labels[i], g = gnd[i];
        if (a < -1 || a >= k || g < -1 || g >= k) return i;
        if (g >= 0) (*n_gnd)++;
        if (a >= 0 && g >= 0) cnt[(size_t)a * (size_t)k + (size_t)g]++;
    }
    return -1;
}

// Clusters by row total of cnt, descending, the larger index first among equals; for each the ground labels by its counts, descending, the larger label first
// among equals; the cluster takes the first label not yet taken.  That is numpy's argsort(..)[::-1] under a stable sort.  Returns the sum of cnt[a][map[a]].
inline int64_t cm_greedy_map(const int64_t* cnt, int32_t k, int32_t* map) {
    std::vector<int64_t> total((size_t)k, 0);
    for (int32_t a = 0; a < k; a++) for (int32_t g = 0; g < k; g++) total[(size_t)a] += cnt[(size_t)a * (size_t)k + (size_t)g];
    std::vector<int32_t> visit((size_t)k), order((size_t)k);
    for (int32_t a = 0; a < k; a++) visit[(size_t)a] = a;
    std::sort(visit.begin(), visit.end(), [&](int32_t a, int32_t b) { return total[(size_t)a] != total[(size_t)b] ? total[(size_t)a] > total[(size_t)b] : a > b; });
    std::vector<uint8_t> taken((size_t)k, 0);
    int64_t hit = 0;
    for (int32_t a : visit) {
        const int64_t* row = cnt + (size_t)a * (size_t)k;
        for (int32_t g = 0; g < k; g++) order[(size_t)g] = g;
        std::sort(order.begin(), order.end(), [&](int32_t g, int32_t h) { return row[g] != row[h] ? row[g] > row[h] : g > h; });
        for (int32_t g : order)
            if (!taken[(size_t)g]) { taken[(size_t)g] = 1; map[a] = g; hit += row[g]; break; }
    }
    return hit;
}

inline double cm_accuracy(int64_t hit, int64_t n_gnd) { return n_gnd > 0 ? (double)hit / (double)n_gnd : (double)NAN; }
