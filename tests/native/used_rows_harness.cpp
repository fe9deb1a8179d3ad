// used_rows_harness.cpp — embedding_amd/csrc/used_rows.h behind a C interface for tests/test_used_rows_host.py (ctypes), and a stand-alone program for the
// sanitizers: `used_rows_harness ROUNDS SEED` runs the intake, the gathers and the scatters on random tables against a plain restatement of the selection rule
// and prints "rounds R wrong W".
#include <stdio.h>
#include <stdlib.h>

#include "../../embedding_amd/csrc/used_rows.h"

// Everything the header gives for one call.  used, fold, yu (n_labels x rows), tu (rows x n_targets), vals_*, out_*: room for `rows` rows; the first n entries
// of vals_* are the used rows' values that go back to out_*.  meta: n, all, kind, bad_row, bad_col, bad_value.
extern "C" void harness_used_rows(int64_t rows, const uint8_t* present, const uint8_t* select, const int32_t* fold, int32_t n_folds, const uint8_t* labels, int n_labels,
                                  const double* targets, int n_targets, int64_t* used, int32_t* fold_out, int64_t* tested, int64_t* meta, uint8_t* yu, double* tu,
                                  const double* vals_d, double* out_d, const int32_t* vals_i, int32_t* out_i) {
    ur_rows u;
    ur_intake(ur_in{rows, present, select, fold, n_folds, labels, n_labels, targets, n_targets}, &u);
    if (!fold) ur_no_folds(&u);
    meta[0] = u.n; meta[1] = u.all ? 1 : 0; meta[2] = u.kind; meta[3] = u.bad_row; meta[4] = u.bad_col; meta[5] = u.bad_value;
    for (int64_t t = 0; t < u.n; t++) { used[t] = u.at(t); fold_out[t] = u.fold[(size_t)t]; }
    for (size_t f = 0; f < u.tested.size(); f++) tested[f] = u.tested[f];
    if (labels) { const std::vector<uint8_t> g = ur_gather_labels(u, labels, n_labels); if (!g.empty()) memcpy(yu, g.data(), g.size()); }
    if (targets) { const std::vector<double> g = ur_gather_targets(u, targets, n_targets); if (!g.empty()) memcpy(tu, g.data(), g.size() * sizeof(double)); }
    if (vals_d) ur_scatter_back(out_d, u, __builtin_nan(""), vals_d);
    if (vals_i) ur_scatter_back<int32_t>(out_i, u, -1, vals_i);
}

extern "C" int harness_outside(const char* who, const char* name, int v, int max, char* msg192) {
    char msg[192] = "";
    const bool out = ur_outside(msg, who, name, v, max);
    memcpy(msg192, msg, sizeof msg);
    return out ? 1 : 0;
}

static uint64_t rnd(uint64_t* s) { *s = *s * 6364136223846793005ULL + 1442695040888963407ULL; return *s >> 33; }

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 4;
    uint64_t seed = argc > 2 ? (uint64_t)atoll(argv[2]) : 1;
    int64_t wrong = 0;
    for (int r = 0; r < rounds; r++)
        for (int mask = 0; mask < 8; mask++) {
            const int64_t rows = (int64_t)(rnd(&seed) % 40);       // 0 rows too
            const int F = 1 + (int)(rnd(&seed) % 3), L = 1 + (int)(rnd(&seed) % 3), T = 2;
            const int drop = (int)(rnd(&seed) % 3);                // 0: every mask keeps every row, 1: some go, 2: all go
            std::vector<uint8_t> pres((size_t)rows), sel((size_t)rows), y((size_t)L * (size_t)rows);
            std::vector<int32_t> fold((size_t)rows);
            std::vector<double> tg((size_t)rows * T);
            for (int64_t i = 0; i < rows; i++) {
                pres[(size_t)i] = drop == 0 ? 1 : (drop == 2 ? 0 : rnd(&seed) % 4 != 0);
                sel[(size_t)i] = drop == 0 ? 3 : (drop == 2 ? 0 : rnd(&seed) % 4 != 0);
                fold[(size_t)i] = drop == 0 ? (int32_t)(rnd(&seed) % F) : (drop == 2 ? -1 : (int32_t)(rnd(&seed) % (F + 1)) - 1);
                for (int l = 0; l < L; l++) y[(size_t)l * (size_t)rows + (size_t)i] = (uint8_t)(rnd(&seed) % 2);
                for (int t = 0; t < T; t++) tg[(size_t)i * T + t] = (double)(rnd(&seed) % 1000) / 8.0;
            }
            const uint8_t* p = (mask & 1) ? pres.data() : nullptr;
            const uint8_t* s = (mask & 2) ? sel.data() : nullptr;
            const int32_t* f = (mask & 4) ? fold.data() : nullptr;
            std::vector<int64_t> want;
            for (int64_t i = 0; i < rows; i++)
                if ((!p || p[i]) && (!s || s[i]) && (!f || f[i] >= 0)) want.push_back(i);
            std::vector<int64_t> used((size_t)rows), tested((size_t)F, 0);
            std::vector<int32_t> fo((size_t)rows), vi((size_t)rows), oi((size_t)rows);
            std::vector<uint8_t> yu((size_t)L * (size_t)rows);
            std::vector<double> tu((size_t)rows * T), vd((size_t)rows), od((size_t)rows);
            for (int64_t i = 0; i < rows; i++) { vi[(size_t)i] = (int32_t)(100 + i); vd[(size_t)i] = 0.5 + (double)i; }
            int64_t meta[6];
            harness_used_rows(rows, p, s, f, F, y.data(), L, tg.data(), T, used.data(), fo.data(), tested.data(), meta, yu.data(), tu.data(), vd.data(), od.data(), vi.data(), oi.data());
            const int64_t n = (int64_t)want.size();
            if (meta[0] != n || meta[1] != (n == rows ? 1 : 0) || meta[2] != UR_NONE) { wrong++; continue; }
            std::vector<int64_t> slot((size_t)rows, -1);
            for (int64_t t = 0; t < n; t++) {
                const int64_t i = want[(size_t)t];
                slot[(size_t)i] = t;
                if (used[(size_t)t] != i || fo[(size_t)t] != (f ? f[i] : -1)) wrong++;
                for (int l = 0; l < L; l++) if (yu[(size_t)l * (size_t)n + (size_t)t] != y[(size_t)l * (size_t)rows + (size_t)i]) wrong++;
                for (int t2 = 0; t2 < T; t2++) if (tu[(size_t)t * T + t2] != tg[(size_t)i * T + t2]) wrong++;
            }
            for (int64_t i = 0; i < rows; i++) {
                const int64_t t = slot[(size_t)i];
                if (oi[(size_t)i] != (t < 0 ? -1 : vi[(size_t)t])) wrong++;
                if (t < 0 ? od[(size_t)i] == od[(size_t)i] : od[(size_t)i] != vd[(size_t)t]) wrong++;
            }
            if (f) for (int k = 0; k < F; k++) { int64_t c = 0; for (int64_t i : want) c += f[i] == k; if (tested[(size_t)k] != c) wrong++; }
        }
    printf("rounds %d wrong %lld\n", rounds, (long long)wrong);
    return wrong ? 1 : 0;
}
