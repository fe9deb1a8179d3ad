// nmf_rule.h — the per-element pieces of the NMF rule of include/dge.h, written once for the kernels of nmf.hip and, compiled for the host, for
// tests/native/nmf_rule_harness.cpp: the draw of the initial factors, the floor, the chain of P, one step of a segment sum's partial and the fold of the 16
// partials, the multiplicative update, the blocked sum.  Every fused operation is an explicit fma(); compile with -ffp-contract=off so that nothing else fuses.
#pragma once
#include <math.h>
#include <stdint.h>

#include "dge_algos.h"      // DGE_HD, dge_mix64

#define NMF_MAX_RANK 32
#define NMF_MAX_ITER 10000
#define NMF_LANES 16        // partials of a segment sum: one DPP row
#define NMF_BLOCK 256       // values of one block of the blocked sum
#define NMF_EPS 0x1.0p-52

// u(t) in [0, 1): unsigned 64-bit arithmetic, wrapping
DGE_HD double nmf_u(uint64_t seed, uint64_t t) { return (double)(dge_mix64(seed + t) >> 11) * 0x1.0p-53; }

DGE_HD double nmf_floor(double x) { return x < NMF_EPS ? NMF_EPS : x; }

// the initial W[i][r] is nmf_init(seed, i * rank + r, vmax), the initial H[r][j] nmf_init(seed, n * rank + r * m + j, vmax)
DGE_HD double nmf_init(uint64_t seed, uint64_t t, double vmax) { return nmf_floor(nmf_u(seed, t) * vmax); }

// P of one entry: w = row i of W, h = column j of H, each with its stride
DGE_HD double nmf_p(const double* w, int64_t sw, const double* h, int64_t sh, int rank) {
    double acc = 0.0;
    for (int r = 0; r < rank; r++) acc = fma(w[(int64_t)r * sw], h[(int64_t)r * sh], acc);
    return acc;
}

// one product into its partial: product t of a segment goes to partial t % NMF_LANES
DGE_HD double nmf_seg_step(double partial, double a, double b) { return fma(a, b, partial); }

// the fold of the 16 partials (the host's form; the kernels do the same four steps across the lanes of a DPP row)
DGE_HD double nmf_seg_fold(double* p) {
    for (int s = NMF_LANES / 2; s > 0; s >>= 1)
        for (int l = 0; l < s; l++) p[l] = p[l] + p[l + s];
    return p[0];
}

// x * (num / den): one division, one multiplication, the floor
DGE_HD double nmf_update(double x, double num, double den) { return nmf_floor(x * (num / den)); }

// ---- the blocked sum (k-means' shape): blocks of NMF_BLOCK values, each added sequentially from +0.0; the block sums added sequentially in block order
DGE_HD double nmf_block_sum(const double* v, int64_t stride, int64_t lo, int64_t hi) {
    double s = 0.0;
    for (int64_t i = lo; i < hi; i++) s += v[i * stride];
    return s;
}

DGE_HD double nmf_block_dot(const double* a, const double* b, int64_t stride, int64_t lo, int64_t hi) {      // of the rounded products a * b
    double s = 0.0;
    for (int64_t i = lo; i < hi; i++) s += a[i * stride] * b[i * stride];
    return s;
}

DGE_HD double nmf_sum_blocks(const double* block_sums, int64_t stride, int64_t n_blocks) {
    double s = 0.0;
    for (int64_t b = 0; b < n_blocks; b++) s += block_sums[b * stride];
    return s;
}
