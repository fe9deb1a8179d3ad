// flow_rule.h — the per-element pieces of the hour-window and triplet rules of include/dge.h, compiled for host and device: whether an hour lies in a window,
// the three pair predicates and the triple predicate of the triplet search, the ten conditions on thirteen given sums, and the argument checks of windows and
// rule.  Everything is int64 arithmetic: a window sum is below 24 * 2^40 < 2^45, the ratio at most 2^16, so every product stays below 2^62.
#pragma once
#include <stdint.h>

#include "../../include/dge.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FR_HD __host__ __device__ inline
#else
#define FR_HD static inline
#endif

#define FR_MAX_COUNT (1LL << 40)     // the total of one key (hour, s, e), at most; the minima of a rule, at most
#define FR_MAX_RATIO 65536

// the thirteen sums the ten conditions read, in the order of dge_triplet_rule_check: W[x,y] with 1 = residence, 2 = office, 3 = night life
enum { FR_A12 = 0, FR_A21, FR_C21, FR_C12, FR_B31, FR_E31, FR_C13, FR_D13, FR_B13, FR_B23, FR_C23, FR_D23, FR_B32, FR_SUMS };

// is hour h (0 .. 23) one of start, start + 1, .., start + hours - 1, each mod 24?
FR_HD bool fr_window_has(int32_t start, int32_t hours, int32_t h) { return (h - start + 24) % 24 < hours; }

FR_HD bool fr_window_ok(const dge_hour_window& w) { return w.start >= 0 && w.start <= 23 && w.hours >= 0 && w.hours <= 24; }

// 0: the rule is fine; 1 .. 5: window A .. E is not; 6: min_a, 7: min_b, 8: ratio
FR_HD int fr_rule_fault(const dge_triplet_rule& r) {
    const dge_hour_window* w[5] = {&r.A, &r.B, &r.C, &r.D, &r.E};
    for (int k = 0; k < 5; k++) if (!fr_window_ok(*w[k])) return k + 1;
    if (r.min_a < 0 || r.min_a > FR_MAX_COUNT) return 6;
    if (r.min_b < 0 || r.min_b > FR_MAX_COUNT) return 7;
    if (r.ratio < 1 || r.ratio > FR_MAX_RATIO) return 8;
    return 0;
}

// the conditions of one pair of regions, in the reference's numbering (J/Tracts.java:391-400): (t1, t2) holds 1, 4 and 6
FR_HD bool fr_pair12(const dge_triplet_rule& r, int64_t a12, int64_t a21, int64_t c21, int64_t c12) {
    return a12 > r.min_a && a12 > r.ratio * a21 && c21 > r.ratio * c12;
}
// (t2, t3) holds 3 and 7
FR_HD bool fr_pair23(const dge_triplet_rule& r, int64_t b23, int64_t c23, int64_t d23) { return b23 > r.min_b && c23 > r.ratio * d23; }
// (t3, t1) holds 2, 5, 8 and 10
FR_HD bool fr_pair31(const dge_triplet_rule& r, int64_t b31, int64_t e31, int64_t c13, int64_t d13, int64_t b13) {
    return b31 > r.min_b && c13 > r.ratio * d13 && b31 > r.ratio * e31 && b31 > r.ratio * b13;
}
// the ninth needs all three regions
FR_HD bool fr_triple(const dge_triplet_rule& r, int64_t b31, int64_t b32) { return b31 > r.ratio * b32; }

FR_HD bool fr_keep(const dge_triplet_rule& r, const int64_t* s) {
    return fr_pair12(r, s[FR_A12], s[FR_A21], s[FR_C21], s[FR_C12]) && fr_pair23(r, s[FR_B23], s[FR_C23], s[FR_D23]) &&
           fr_pair31(r, s[FR_B31], s[FR_E31], s[FR_C13], s[FR_D13], s[FR_B13]) && fr_triple(r, s[FR_B31], s[FR_B32]);
}
