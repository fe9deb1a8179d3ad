// ridge_rule.h — the per-element pieces of the ridge rule of include/dge.h, written once for the kernels of ridge.hip and, compiled for the host, for
// tests/native/ridge_rule_harness.cpp: the design value, the steps of the moment, factorisation, substitution, leverage and prediction chains, and the whole
// rule as one plain host loop over them (rg_solve_host: what the kernels are held to and what scripts/ridge_rate.py times as the one-thread host figure).
// Every fused operation is an explicit fma(); compile with -ffp-contract=off so that nothing else fuses.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "dge_algos.h"      // DGE_HD

#define RG_MAX_DIM 256
#define RG_MAX_TARGETS 64
#define RG_MAX_LAMBDA 64
#define RG_BLOCK 256        // rows of one block of the blocked sums (k-means' block)

// z[i][j]: the design row of a feature row x
DGE_HD double rg_z(const float* x, int j) { return j == 0 ? 1.0 : (double)x[j - 1]; }

// one row's step of a moment: acc + za * w in one rounding.  For G both factors come from float32, the product is exact in binary64 and this is the rounded
// addition of the rule; for c it is the rule's fma
DGE_HD double rg_moment_step(double acc, double za, double w) { return fma(za, w, acc); }

// A[j][j] of the system of one lambda: the intercept is not penalised
DGE_HD double rg_diag(double g, int j, double lambda) { return j >= 1 ? g + lambda : g; }

// acc = fma(-l, v, acc): the step of both substitutions, and of the factorisation with v = rg_ldl_t
DGE_HD double rg_sub_step(double acc, double l, double v) { return fma(-l, v, acc); }
DGE_HD double rg_ldl_t(double ljk, double dk) { return ljk * dk; }

// h's step: acc = fma(u, u * inv, acc)
DGE_HD double rg_lev_step(double acc, double u, double inv) { return fma(u, u * inv, acc); }

// the prediction of a model beta[0 .. dim] for a feature row
DGE_HD double rg_pred_step(double p, double z, double b) { return fma(z, b, p); }
DGE_HD double rg_predict(const float* x, const double* beta, int dim) {
    double p = beta[0];
    for (int j = 1; j <= dim; j++) p = rg_pred_step(p, (double)x[j - 1], beta[j]);
    return p;
}

// the blocked sum of k-means: blocks of RG_BLOCK values added from +0.0, the block sums added from +0.0 in block order
DGE_HD double rg_blocked_sum_abs(const double* v, int64_t n) {
    double s = 0.0;
    for (int64_t lo = 0; lo < n; lo += RG_BLOCK) {
        const int64_t hi = lo + RG_BLOCK < n ? lo + RG_BLOCK : n;
        double b = 0.0;
        for (int64_t i = lo; i < hi; i++) b += fabs(v[i]);
        s += b;
    }
    return s;
}

enum { RG_FINE = 0, RG_PIVOT = 1, RG_LEVERAGE = 2 };
struct rg_refusal {
    int32_t kind;          // RG_PIVOT: d[index] of lambda is not > 0;  RG_LEVERAGE: 1 - h of used row index under lambda is not > 0
    int32_t lambda;
    int64_t index;
};

// The rule on n used rows, one thread, one row and one element after another.  x [n x dim], y [n x T], lambda [nl].  Outputs, all required:
// M [P x (P + T)]: G (both triangles) beside c, M[a][P + t] = c[t][a];  d [nl x P];  L [nl x P x P] row-major, unit lower, zero above;  beta [nl x T x P];
// h [nl x n];  e [nl x T x n];  mae, mre [nl x T].  Every factorisation comes before the first leverage: a pivot's refusal goes before a leverage's, the
// lower lambda index before the higher.  -> RG_FINE, or the kind of *why.
static inline int rg_solve_host(const float* x, const double* y, int64_t n, int dim, int T, const double* lambda, int nl, double* M, double* d, double* L, double* beta,
                                double* h, double* e, double* mae, double* mre, rg_refusal* why) {
    const int P = dim + 1, W = P + T;
    const size_t PW = (size_t)P * W, PP = (size_t)P * P;
    std::vector<double> part(PW), z((size_t)P), inv((size_t)P);
    for (size_t q = 0; q < PW; q++) M[q] = 0.0;
    for (int64_t lo = 0; lo < n; lo += RG_BLOCK) {
        const int64_t hi = lo + RG_BLOCK < n ? lo + RG_BLOCK : n;
        std::fill(part.begin(), part.end(), 0.0);
        for (int64_t i = lo; i < hi; i++) {
            for (int j = 0; j < P; j++) z[(size_t)j] = rg_z(x + (size_t)i * dim, j);
            const double* yi = y + (size_t)i * T;
            for (int a = 0; a < P; a++) {
                double* pa = part.data() + (size_t)a * W;
                const double za = z[(size_t)a];
                for (int b = a; b < P; b++) pa[b] = rg_moment_step(pa[b], za, z[(size_t)b]);
                for (int t = 0; t < T; t++) pa[P + t] = rg_moment_step(pa[P + t], za, yi[t]);
            }
        }
        for (size_t q = 0; q < PW; q++) M[q] += part[q];
    }
    for (int a = 0; a < P; a++) for (int b = 0; b < a; b++) M[(size_t)a * W + b] = M[(size_t)b * W + a];

    for (int l = 0; l < nl; l++) {
        double* Ll = L + (size_t)l * PP;
        double* dl = d + (size_t)l * P;
        for (size_t q = 0; q < PP; q++) Ll[q] = 0.0;
        for (int j = 0; j < P; j++) {
            const double* Lj = Ll + (size_t)j * P;
            double acc = rg_diag(M[(size_t)j * W + j], j, lambda[l]);
            for (int k = 0; k < j; k++) acc = rg_sub_step(acc, Lj[k], rg_ldl_t(Lj[k], dl[k]));
            dl[j] = acc;
            if (!(acc > 0.0)) { why->kind = RG_PIVOT; why->lambda = l; why->index = j; return RG_PIVOT; }
            Ll[(size_t)j * P + j] = 1.0;
            for (int i = j + 1; i < P; i++) {
                double* Li = Ll + (size_t)i * P;
                acc = M[(size_t)j * W + i];
                for (int k = 0; k < j; k++) acc = rg_sub_step(acc, Li[k], rg_ldl_t(Lj[k], dl[k]));
                Li[j] = acc / dl[j];
            }
        }
        for (int t = 0; t < T; t++) {
            double* w = beta + ((size_t)l * T + t) * P;
            for (int j = 0; j < P; j++) {
                double acc = M[(size_t)j * W + P + t];
                for (int k = 0; k < j; k++) acc = rg_sub_step(acc, Ll[(size_t)j * P + k], w[k]);
                w[j] = acc;
            }
            for (int j = 0; j < P; j++) w[j] = w[j] / dl[j];
            for (int j = P - 1; j >= 0; j--) {
                double acc = w[j];
                for (int k = P - 1; k > j; k--) acc = rg_sub_step(acc, Ll[(size_t)k * P + j], w[k]);
                w[j] = acc;
            }
        }
    }
    for (int l = 0; l < nl; l++) {
        const double* Ll = L + (size_t)l * PP;
        for (int j = 0; j < P; j++) inv[(size_t)j] = 1.0 / d[(size_t)l * P + j];
        for (int64_t i = 0; i < n; i++) {
            const float* xi = x + (size_t)i * dim;
            double hv = 0.0;
            for (int j = 0; j < P; j++) {
                double acc = rg_z(xi, j);
                for (int k = 0; k < j; k++) acc = rg_sub_step(acc, Ll[(size_t)j * P + k], z[(size_t)k]);
                z[(size_t)j] = acc;                           // u
                hv = rg_lev_step(hv, acc, inv[(size_t)j]);
            }
            h[(size_t)l * n + i] = hv;
            const double g = 1.0 - hv;
            if (!(g > 0.0)) { why->kind = RG_LEVERAGE; why->lambda = l; why->index = i; return RG_LEVERAGE; }
            for (int t = 0; t < T; t++) {
                const double r = y[(size_t)i * T + t] - rg_predict(xi, beta + ((size_t)l * T + t) * P, dim);
                e[((size_t)l * T + t) * n + i] = r / g;
            }
        }
        for (int t = 0; t < T; t++) {
            const size_t m = (size_t)l * T + t;
            mae[m] = rg_blocked_sum_abs(e + m * n, n) / (double)n;
            mre[m] = mae[m] / (M[P + t] / (double)n);        // M[0][P + t] = c[t][0]: the blocked sum of y[.][t]
        }
    }
    why->kind = RG_FINE; why->lambda = -1; why->index = -1;
    return RG_FINE;
}
