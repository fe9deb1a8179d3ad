// line_rule.h — the per-element pieces of the LINE rule of include/dge.h, written once for the kernels of line.hip and, compiled for the host, for
// tests/native/line_rule_harness.cpp: the limits, the draw of an initial cell, the quantisation, the two inverse-CDF searches, the negative weight of a degree,
// the step size of a batch, the sigmoid table and its look-up, the dot (the SEGMENT SUM of nmf_rule.h) and the quantised gradient term.  Every fused operation is
// an explicit fma(); compile with -ffp-contract=off so that nothing else fuses.
#pragma once
#include <math.h>
#include <stdint.h>

#include "nmf_rule.h"          // DGE_HD, dge_mix64, NMF_LANES, nmf_seg_step, nmf_seg_fold
#include "spatial_weight.h"    // sw_exp_neg: E(x), x <= 0

#define LINE_MAX_N (1LL << 22)
#define LINE_MAX_DIM 256
#define LINE_MAX_NEG 32
#define LINE_MAX_BATCH 65536
#define LINE_MAX_SAMPLES (1LL << 40)
#define LINE_MAX_WEIGHT (1LL << 31)        // one weight stays below it
#define LINE_MAX_TOTAL (1LL << 40)         // the total weight W stays below it
#define LINE_CELL_LIMIT (1LL << 40)        // |P| of a table cell stays below it: |value| < 256
#define LINE_INIT_LIMIT 256.0              // |x| of a supplied initial value stays below it
#define LINE_SIG_N 1000
#define LINE_SIG_BOUND 6.0
#define LINE_FIX 0x1.0p32
#define LINE_UNFIX 0x1.0p-32
#define LINE_SEED_TAG 0x4C494E45ULL        // "LINE"
#define LINE_DRAW_STRIDE 64ULL             // sample s draws from seed + 64 s + d, d = 0 .. K

DGE_HD uint64_t line_seed2(uint64_t seed) { return dge_mix64(seed ^ LINE_SEED_TAG); }

// u(t) in [0, 1) from seed2: unsigned 64-bit arithmetic, wrapping
DGE_HD double line_u(uint64_t seed2, uint64_t t) { return (double)(dge_mix64(seed2 + t) >> 11) * 0x1.0p-53; }

// rint(x * 2^32), ties to even; |x| < 2^31 so that the result fits
DGE_HD int64_t line_quant(double x) { return (int64_t)rint(x * LINE_FIX); }

// the value of a table cell: exact while |P| < 2^53
DGE_HD double line_value(int64_t P) { return (double)P * LINE_UNFIX; }

// the initial PX[v][j], t = v * dim + j
DGE_HD int64_t line_init_cell(uint64_t seed2, uint64_t t, int dim) { return line_quant((line_u(seed2, t) - 0.5) / (double)dim); }

// the least e in [0, cnt) with C[e] > r mod total, C an inclusive prefix sum that ends in total > 0
DGE_HD int64_t line_search(const int64_t* C, int64_t cnt, uint64_t r, int64_t total) {
    const int64_t want = (int64_t)(r % (uint64_t)total);
    int64_t lo = 0, hi = cnt - 1;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (C[mid] > want) hi = mid; else lo = mid + 1; }
    return lo;
}

// nw of a vertex of out-weight d: d^0.75 as two correctly rounded roots and one product, times 1024, truncated
DGE_HD int64_t line_neg_weight(int64_t d) {
    const double x = (double)d;
    const double p = sqrt(x * sqrt(x));
    return (int64_t)(p * 1024.0);
}

// the draws of sample s: d = 0 the edge, d = 1 .. K the negatives
DGE_HD uint64_t line_draw(uint64_t seed, uint64_t s, uint64_t d) { return dge_mix64(seed + LINE_DRAW_STRIDE * s + d); }

// rho of the batch that starts at sample `first`
DGE_HD double line_rho(double rho0, int64_t first, int64_t samples) {
    const double rho = rho0 * (1.0 - (double)first / (double)(samples + 1));
    const double least = rho0 * 0.0001;
    return rho < least ? least : rho;
}

// entry k of the sigmoid table (built on the host and uploaded: one set of bits for every reader)
inline double line_sig_entry(int k) {
    const double x = ((double)k * 12.0) / 1000.0 - 6.0;
    if (x >= 0.0) return 1.0 / (1.0 + sw_exp_neg(-x));
    const double e = sw_exp_neg(x);
    return e / (1.0 + e);
}

DGE_HD double line_sig(const double* T, double f) {
    if (f > LINE_SIG_BOUND) return 1.0;
    if (f < -LINE_SIG_BOUND) return 0.0;
    int k = (int)(((f + LINE_SIG_BOUND) * 1000.0) / 12.0);
    if (k > LINE_SIG_N - 1) k = LINE_SIG_N - 1;
    if (k < 0) k = 0;                       // never taken on a number; keeps a look-up inside the table whatever f is
    return T[k];
}

// dot(a, b) over dim values: the SEGMENT SUM (the host's form; the kernels hold partial l in lane l of a DPP row)
DGE_HD double line_dot(const double* a, const double* b, int dim) {
    double p[NMF_LANES];
    for (int l = 0; l < NMF_LANES; l++) p[l] = 0.0;
    for (int j = 0; j < dim; j++) p[j % NMF_LANES] = nmf_seg_step(p[j % NMF_LANES], a[j], b[j]);
    return nmf_seg_fold(p);
}

// g of one (sample, target)
DGE_HD double line_g(double label, double sig, double rho) { return (label - sig) * rho; }

// what one cell of a delta table takes: rint((g * x) * 2^32)
DGE_HD int64_t line_term(double g, double x) { return line_quant(g * x); }

DGE_HD int line_cell_over(int64_t P) { return P >= LINE_CELL_LIMIT || P <= -LINE_CELL_LIMIT; }
