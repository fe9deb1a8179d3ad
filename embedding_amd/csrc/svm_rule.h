// svm_rule.h — the per-element pieces of the SVM rule of include/dge.h (RBF C-SVC by sequential minimal optimisation), written once for the kernels of svm.hip
// and, compiled for the host, for tests/native/svm_rule_harness.cpp: the kernel entry, the candidate score, the two comparators, the step with its clamps, the
// gradient step, the decision term, and svm_solve_host, the whole rule as one plain one-thread loop over them.  Every fused operation is an explicit fma();
// compile with -ffp-contract=off so that nothing else fuses.  Outside the build stamp: nothing here is read by a training launch.
#pragma once
#include <math.h>
#include <stdint.h>

#include "dge_algos.h"          // DGE_HD
#include "kmeans_rule.h"        // km_dist, km_dist_step: the distance chain
#include "spatial_weight.h"     // sw_exp_neg: E

#define SV_MAX_ROWS 65536       // used rows of one call: the kernel matrix is 8 n^2 bytes and there is no row cache
#define SV_MAX_DIM 4096
#define SV_MAX_LABELS 64
#define SV_MAX_FOLDS 64
#define SV_BLOCK KM_BLOCK       // support rows of one block of the decision's blocked sum
#define SV_TAU 0x1p-40          // the curvature where 2 - 2K is not > 0 (two equal rows)
#define SV_NONE 0x7fffffff      // "no row"

// ---- the kernel matrix: K = E(-(gamma * d2)), one rounded product, an exact negation
DGE_HD double sv_kernel_of(double d2, double gamma) { return sw_exp_neg(-(gamma * d2)); }
DGE_HD double sv_kernel(const float* a, const float* b, int dim, double gamma) { return sv_kernel_of(km_dist(a, b, dim), gamma); }

// ---- the sets: s is +1 or -1, "at a bound" is alpha == 0 or alpha == C exactly
DGE_HD double sv_v(int s, double G) { return s > 0 ? -G : G; }                                    // -s * G, exact
DGE_HD bool sv_in_up(int s, double alpha, double C) { return s > 0 ? alpha < C : alpha > 0.0; }
DGE_HD bool sv_in_low(int s, double alpha, double C) { return s > 0 ? alpha > 0.0 : alpha < C; }

// ---- the two comparators: the greatest value, the least row among equals.  Both orders are total, so any reduction tree gives the same winner.
DGE_HD bool sv_up_better(double v, int32_t t, double best_v, int32_t best_t) { return v > best_v || (v == best_v && t < best_t); }
DGE_HD bool sv_score_better(double sc, int32_t t, double best_sc, int32_t best_t) { return sc > best_sc || (sc == best_sc && t < best_t); }

// step 1 of an iteration as a running triple: (m, i) over I_up, M over I_low.  i == SV_NONE: I_up is empty (m = -inf); M == +inf: I_low is empty.
struct sv_front {
    double m, M;
    int32_t i;
};
DGE_HD sv_front sv_front_none() { return sv_front{-INFINITY, INFINITY, SV_NONE}; }
DGE_HD void sv_front_row(sv_front& f, int32_t t, int s, double alpha, double G, double C) {
    const double v = sv_v(s, G);
    if (sv_in_up(s, alpha, C) && sv_up_better(v, t, f.m, f.i)) { f.m = v; f.i = t; }
    if (sv_in_low(s, alpha, C) && v < f.M) f.M = v;
}
DGE_HD void sv_front_merge(sv_front& f, double m, double M, int32_t i) {
    if (sv_up_better(m, i, f.m, f.i)) { f.m = m; f.i = i; }
    if (M < f.M) f.M = M;
}
// step 2: stop when a set is empty or the gap RN(m - M) is below eps
DGE_HD bool sv_front_closed(const sv_front& f, double eps) { return f.i == SV_NONE || !(f.M < INFINITY) || f.m - f.M < eps; }
// the bias: the midpoint of the last gap; where one set was empty the other value twice
DGE_HD double sv_bias(const sv_front& f) {
    const bool up = f.i != SV_NONE, low = f.M < INFINITY;
    const double a = up ? f.m : f.M, b = low ? f.M : f.m;
    return (a + b) * 0.5;
}

// ---- step 3: the candidate score of row t against the chosen i
DGE_HD double sv_curv(double Kit) {
    const double a = 2.0 - 2.0 * Kit;                          // 2K is exact: one rounding
    return a > 0.0 ? a : SV_TAU;
}
DGE_HD double sv_score(double m, double v, double Kit) {
    const double b = m - v;
    return (b * b) / sv_curv(Kit);
}
struct sv_pick {
    double score;
    int32_t j;
};
DGE_HD sv_pick sv_pick_none() { return sv_pick{-1.0, SV_NONE}; }                                  // a score is >= 0
DGE_HD void sv_pick_row(sv_pick& p, int32_t t, int s, double alpha, double G, double C, double m, double Kit) {
    const double v = sv_v(s, G);
    if (!sv_in_low(s, alpha, C) || !(v < m)) return;
    const double sc = sv_score(m, v, Kit);
    if (sv_score_better(sc, t, p.score, p.j)) { p.score = sc; p.j = t; }
}

// ---- steps 4 and 5: the step size, the clamps, the new alphas and their differences
DGE_HD double sv_clamp(double a, double C) { return a < 0.0 ? 0.0 : (a > C ? C : a); }
struct sv_move {
    double ai, aj, Di, Dj;
};
DGE_HD sv_move sv_step(double m, double vj, double Kij, int si, int sj, double alpha_i, double alpha_j, double C) {
    double delta = (m - vj) / sv_curv(Kij);
    const double lim_i = si > 0 ? C - alpha_i : alpha_i;
    const double lim_j = sj > 0 ? alpha_j : C - alpha_j;
    if (lim_i < delta) delta = lim_i;
    if (lim_j < delta) delta = lim_j;
    sv_move r;
    if (delta == lim_i) r.ai = si > 0 ? C : 0.0;
    else r.ai = sv_clamp(si > 0 ? alpha_i + delta : alpha_i - delta, C);
    if (delta == lim_j) r.aj = sj > 0 ? 0.0 : C;
    else r.aj = sv_clamp(sj > 0 ? alpha_j - delta : alpha_j + delta, C);
    r.Di = r.ai - alpha_i;
    r.Dj = r.aj - alpha_j;
    return r;
}

// ---- step 6: one row's gradient; the sign flips are exact
DGE_HD double sv_grad(double G, int st, int si, int sj, double Kti, double Ktj, double Di, double Dj) {
    const double qi = (st > 0) == (si > 0) ? Kti : -Kti;
    const double qj = (st > 0) == (sj > 0) ? Ktj : -Ktj;
    return fma(qj, Dj, fma(qi, Di, G));
}

// ---- the decision: one term, and f(x) over a support list (sup ascending, Kx[r] = K(row r, x)) in the blocked order
DGE_HD double sv_coef(int s, double alpha) { return alpha > 0.0 ? (s > 0 ? alpha : -alpha) : 0.0; }        // +0.0 on a row that is not support
DGE_HD double sv_term(double coef, double Kux) { return coef * Kux; }
DGE_HD double sv_decide(const double* Kx, const int32_t* sup, const double* coef, int64_t n_sup, double bias) {
    double total = 0.0;
    for (int64_t lo = 0; lo < n_sup; lo += SV_BLOCK) {
        const int64_t hi = lo + SV_BLOCK < n_sup ? lo + SV_BLOCK : n_sup;
        double s = 0.0;
        for (int64_t k = lo; k < hi; k++) s += sv_term(coef[k], Kx[sup[k]]);
        total += s;
    }
    return bias + total;
}

// ---- the whole rule on one thread.  K: the full matrix [n x n] of the rows; sgn[t]: +1 / -1 on a training row, 0 on a row that does not train.
// alpha, G: [n], written (0 and -1 on rows that do not train).  -> the updates made
inline int64_t svm_solve_host(const double* K, int32_t n, const int8_t* sgn, double C, double eps, int64_t max_iter, double* alpha, double* G, double* bias,
                              int32_t* converged) {
    for (int32_t t = 0; t < n; t++) { alpha[t] = 0.0; G[t] = -1.0; }
    int64_t it = 0;
    for (;;) {
        sv_front f = sv_front_none();
        for (int32_t t = 0; t < n; t++) if (sgn[t]) sv_front_row(f, t, sgn[t], alpha[t], G[t], C);
        if (sv_front_closed(f, eps)) { *converged = 1; *bias = sv_bias(f); return it; }
        if (it == max_iter) { *converged = 0; *bias = sv_bias(f); return it; }
        const int32_t i = f.i;
        const double* Ki = K + (size_t)i * (size_t)n;
        sv_pick p = sv_pick_none();
        for (int32_t t = 0; t < n; t++) if (sgn[t]) sv_pick_row(p, t, sgn[t], alpha[t], G[t], C, f.m, Ki[t]);
        if (p.j == SV_NONE) { *converged = 0; *bias = sv_bias(f); return it; }      // cannot happen while G is finite: the row of M is a candidate
        const int32_t j = p.j;
        const double* Kj = K + (size_t)j * (size_t)n;
        const sv_move mv = sv_step(f.m, sv_v(sgn[j], G[j]), Ki[j], sgn[i], sgn[j], alpha[i], alpha[j], C);
        alpha[i] = mv.ai; alpha[j] = mv.aj;
        for (int32_t t = 0; t < n; t++) if (sgn[t]) G[t] = sv_grad(G[t], sgn[t], sgn[i], sgn[j], Ki[t], Kj[t], mv.Di, mv.Dj);
        it++;
    }
}

// the kernel matrix of n rows on one thread
inline void svm_kernel_host(const float* x, int32_t n, int dim, double gamma, double* K) {
    for (int32_t i = 0; i < n; i++)
        for (int32_t j = 0; j < n; j++) K[(size_t)i * (size_t)n + (size_t)j] = sv_kernel(x + (size_t)i * dim, x + (size_t)j * dim, dim, gamma);
}
