// pairwise_rule.h — the per-element arithmetic of the per-slice pairwise evaluation (include/dge.h: dge_pairwise_eval_vectors), written once for the
// kernels of pairwise.hip and for the host (tests/native/pairwise_rule_harness.cpp): the ground distance of two regions, the order of the keys
// (distance, region), one step of a DCG chain and the ratio.
//
// Every operation is a rounded binary64 + - * / or sqrt in the order written; compile with -ffp-contract=off and write no fma, so that the device, the
// host harness and tests/pairwise_ref.py give the same bits.  The product of two widened float32 values is exact in binary64, so the chains below are
// what a fused multiply-add would give as well; sqrt and / are correctly rounded on the host and on the device (as spatial_weight.h and line_rule.h
// already rely on).  Outside the build stamp: nothing here is read by a training launch.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PW_HD __host__ __device__ inline
#else
#define PW_HD inline
#endif

#define PW_MAX_K 128          // the longest list
#define PW_MAX_NK 16          // the most cut-offs of a call
#define PW_MAX_SETS 64
#define PW_MAX_DIM 256        // of the ground rows and of the feature rows

// one step of ss[a] (a == b) or dot(a, b): acc + x * y, the product exact
PW_HD double pw_step(double acc, float x, float y) { return acc + (double)x * (double)y; }

// a ground row has a direction iff its sum of squares lies in (0, +inf): a NaN or an infinity anywhere makes the sum NaN or +inf
PW_HD bool pw_live(double ss) { return ss > 0.0 && ss < (double)INFINITY; }

// dist(a, b) of two rows with a direction, from their dot product and sums of squares: one multiply, one sqrt, one divide, one subtract
PW_HD double pw_dist_live(double dot, double ss_a, double ss_b) { return 1.0 - dot / sqrt(ss_a * ss_b); }
#define PW_DIST_ZERO 2.0      /* dist(a, b) where either is a zero vector */

// dist(a, b) from the rows: the chain over the columns in order
PW_HD double pw_dist_rows(const float* a, const float* b, int g, double ss_a, double ss_b, bool live_a, bool live_b) {
    if (!live_a || !live_b) return PW_DIST_ZERO;
    double dot = 0.0;
    for (int j = 0; j < g; j++) dot = pw_step(dot, a[j], b[j]);
    return pw_dist_live(dot, ss_a, ss_b);
}

// key (d, c) < key (d2, c2): the distance ascends, then the region number
PW_HD bool pw_key_less(double d, int32_t c, double d2, int32_t c2) { return d < d2 || (d == d2 && c < c2); }

// one step of a DCG chain: a rounded subtract, a rounded multiply, a rounded add
PW_HD double pw_gain(double acc, double dist, double disc) { return acc + (1.0 - dist) * disc; }

PW_HD double pw_ratio(double dcg, double ideal) { return ideal != 0.0 ? dcg / ideal : 0.0; }

// disc[i] = 1 / log2(i + 2): the host's, uploaded; no device log2 decides a bit
inline double pw_disc_host(int i) { return 1.0 / log2((double)(i + 2)); }
