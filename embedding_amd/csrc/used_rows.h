// used_rows.h — the used rows of a call on a table of rows, for k-means, the tree, ridge and the SVM: which rows take part, the check of the per-row values
// that come with them, the gathers that bring those values to the used rows' order, and the way back to the original row numbers.  Plain C++: the tests
// compile it for the host (tests/native/used_rows_harness.cpp).
// A row is used iff it is present, and select is absent or non-zero there, and fold is absent or >= 0 there.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

enum { UR_NONE = 0, UR_FOLD, UR_LABEL, UR_TARGET };      // what the first offence of the walk is

struct ur_in {
    int64_t rows = 0;
    const uint8_t* present = nullptr;      // [rows], nullptr: every row is present
    const uint8_t* select = nullptr;       // [rows], nullptr: no mask
    const int32_t* fold = nullptr;         // [rows] in -1 .. n_folds - 1, nullptr: no folds
    int32_t n_folds = 0;
    const uint8_t* labels = nullptr;       // [n_labels x rows], 0 or 1 on a used row
    int n_labels = 0;
    const double* targets = nullptr;       // [rows x n_targets], finite on a used row
    int n_targets = 0;
};

struct ur_rows {
    int64_t rows = 0, n = 0;
    bool all = false;                      // no row is left out; `used` is then empty
    std::vector<int64_t> used;             // the used rows' original numbers, ascending
    std::vector<int32_t> fold;             // [n]; without a fold array it is empty until ur_no_folds fills it with -1
    std::vector<int64_t> tested;           // [n_folds]: the used rows of every fold
    int kind = UR_NONE;                    // the first offence in row order, then column order:
    int64_t bad_row = -1;                  // its original row number
    int bad_col = 0, bad_value = 0;        // label column or target column; the fold or the label found
    int64_t at(int64_t t) const { return all ? t : used[(size_t)t]; }
};

static inline bool ur_finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }      // false for NaN

// One walk over the rows.  The fold's range is checked on every row, the labels and targets on used rows only, and only the first offence is kept; a row whose
// fold is out of range is not used.  The walk goes on behind an offence, so n is the table's in any case.  Where nothing can leave a row out and there is no
// value to check, there is no walk.
static inline void ur_intake(const ur_in& in, ur_rows* u) {
    *u = ur_rows();
    u->rows = in.rows;
    u->tested.assign(in.fold ? (size_t)in.n_folds : 0, 0);
    const bool plain = !in.present && !in.select && !in.fold;
    if (plain && !in.n_labels && !in.n_targets) { u->n = in.rows; u->all = true; return; }
    for (int64_t i = 0; i < in.rows; i++) {
        const int32_t f = in.fold ? in.fold[i] : -1;
        if (in.fold && (f < -1 || f >= in.n_folds)) {
            if (!u->kind) { u->kind = UR_FOLD; u->bad_row = i; u->bad_value = f; }
            continue;
        }
        if ((in.present && !in.present[i]) || (in.select && !in.select[i]) || (in.fold && f < 0)) continue;
        for (int l = 0; l < in.n_labels && !u->kind; l++)
            if (in.labels[(size_t)l * (size_t)in.rows + (size_t)i] > 1) { u->kind = UR_LABEL; u->bad_row = i; u->bad_col = l; u->bad_value = in.labels[(size_t)l * (size_t)in.rows + (size_t)i]; }
        for (int t = 0; t < in.n_targets && !u->kind; t++)
            if (!ur_finite(in.targets[(size_t)i * (size_t)in.n_targets + (size_t)t])) { u->kind = UR_TARGET; u->bad_row = i; u->bad_col = t; }
        if (!plain) u->used.push_back(i);
        if (in.fold) { u->fold.push_back(f); u->tested[(size_t)f]++; }
        u->n++;
    }
    u->all = u->n == in.rows;
    if (u->all) std::vector<int64_t>().swap(u->used);
}
// the folds of a call without a fold array: every used row trains every problem and tests none
static inline void ur_no_folds(ur_rows* u) { u->fold.assign((size_t)u->n, -1); }

// the used rows' labels [n_labels x n] (column-major per label) and targets [n x T]
static inline std::vector<uint8_t> ur_gather_labels(const ur_rows& u, const uint8_t* y, int n_labels) {
    std::vector<uint8_t> yu((size_t)n_labels * (size_t)u.n);
    for (int l = 0; l < n_labels; l++)
        for (int64_t t = 0; t < u.n; t++) yu[(size_t)l * (size_t)u.n + (size_t)t] = y[(size_t)l * (size_t)u.rows + (size_t)u.at(t)];
    return yu;
}
static inline std::vector<double> ur_gather_targets(const ur_rows& u, const double* y, int T) {
    std::vector<double> yu((size_t)u.n * (size_t)T);
    for (int64_t t = 0; t < u.n; t++) memcpy(yu.data() + (size_t)t * (size_t)T, y + (size_t)u.at(t) * (size_t)T, (size_t)T * sizeof(double));
    return yu;
}

// out [rows]: values[t] at the used row t's original number, fill everywhere else
template <typename T>
static inline void ur_scatter_back(T* out, const ur_rows& u, T fill, const T* values) {
    if (u.all) { if (u.n) memcpy(out, values, (size_t)u.n * sizeof(T)); return; }
    for (int64_t i = 0; i < u.rows; i++) out[i] = fill;
    for (int64_t t = 0; t < u.n; t++) out[u.used[(size_t)t]] = values[t];
}

// true, and the refusal's words in msg, when v is outside 1 .. max
static inline bool ur_outside(char (&msg)[192], const char* who, const char* name, int v, int max) {
    if (v >= 1 && v <= max) return false;
    snprintf(msg, sizeof msg, "%s: %s = %d is outside 1 .. %d", who, name, v, max);
    return true;
}
