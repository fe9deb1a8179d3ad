// kmeans_rule.h — the per-element pieces of the k-means rule of include/dge.h, written once for the kernels of kmeans.hip and, compiled for the host, for
// tests/native/kmeans_rule_harness.cpp: the scale of the fixed-point row sums, the quantiser, a centre from its sum, the distance chain, the seeding draw and
// the blocked sum with its walk.  Every fused operation is an explicit fma(); compile with -ffp-contract=off so that nothing else fuses.
#pragma once
#include <math.h>
#include <stdint.h>

#include "dge_algos.h"      // DGE_HD, dge_mix64

#define KM_MAX_K 64
#define KM_MAX_DIM 256
#define KM_BLOCK 256        // rows of one block of the blocked sum

// s = 62 - bitlength(n) - e, where max|x| = m * 2^e with 0.5 <= m < 1 (e = 0 for max|x| = 0): |q| < 2^(62 - bitlength(n)), so n of them stay below 2^62
DGE_HD int km_scale_bits(float max_abs, int64_t n) {
    int e = 0;
    if (max_abs != 0.0f) (void)frexpf(max_abs, &e);
    int b = 0;
    for (uint64_t v = (uint64_t)n; v; v >>= 1) b++;
    return 62 - b - e;
}

// q = x * 2^s rounded to the nearest integer, ties to even: the scaling is exact in binary64, rint is the one rounding
DGE_HD int64_t km_quantise(float x, int s) { return (int64_t)rint(ldexp((double)x, s)); }

// int64 -> binary64 (nearest even), one division, an exact scaling, one rounding to binary32
DGE_HD float km_centre_from_sum(int64_t sum, int64_t count, int s) { return (float)ldexp((double)sum / (double)count, -s); }

// one step of the distance chain: t = x - c (one rounding), acc = fma(t, t, acc) (one rounding)
DGE_HD double km_dist_step(double acc, float x, float c) {
    const double t = (double)x - (double)c;
    return fma(t, t, acc);
}

DGE_HD double km_dist(const float* x, const float* c, int dim) {
    double acc = 0.0;
    for (int j = 0; j < dim; j++) acc = km_dist_step(acc, x[j], c[j]);
    return acc;
}

// the first centre of restart r, and the draw u in [0, 1) of centre c >= 1 (unsigned 64-bit arithmetic, wrapping)
DGE_HD int64_t km_first_pick(uint64_t seed, int64_t r, int k, int64_t n) { return (int64_t)(dge_mix64(seed + (uint64_t)r * (uint64_t)k) % (uint64_t)n); }
DGE_HD double km_draw(uint64_t seed, int64_t r, int k, int c) { return (double)(dge_mix64(seed + (uint64_t)r * (uint64_t)k + (uint64_t)c) >> 11) * 0x1.0p-53; }

// ---- the blocked sum: blocks of KM_BLOCK values, each added sequentially from +0.0; the block sums added sequentially in block order
DGE_HD double km_block_sum(const double* v, int64_t lo, int64_t hi) {
    double s = 0.0;
    for (int64_t i = lo; i < hi; i++) s += v[i];
    return s;
}

DGE_HD double km_sum_blocks(const double* block_sums, int64_t n_blocks) {
    double s = 0.0;
    for (int64_t b = 0; b < n_blocks; b++) s += block_sums[b];
    return s;
}

// the first row at which the running blocked sum exceeds target: the first block whose running total exceeds it, then row by row from the total in front of
// that block.  -1: no row does.
DGE_HD int64_t km_walk(const double* v, const double* block_sums, int64_t n, double target) {
    const int64_t n_blocks = (n + KM_BLOCK - 1) / KM_BLOCK;
    double run = 0.0;
    for (int64_t b = 0; b < n_blocks; b++) {
        const double next = run + block_sums[b];
        if (next > target) {
            const int64_t hi = (b + 1) * KM_BLOCK < n ? (b + 1) * KM_BLOCK : n;
            for (int64_t i = b * KM_BLOCK; i < hi; i++) {
                run += v[i];
                if (run > target) return i;
            }
            return hi - 1;                                    // (front + v0) + v1 .. rounds otherwise than front + (v0 + v1 ..): the block's last row then
        }
        run = next;
    }
    return -1;
}
