"""The SVM rule of include/dge.h (RBF C-SVC by sequential minimal optimisation, its decision function, its cross-validation) read out in Python: binary64
operations in the order the header names, every fused step an explicit fma (nmf_ref.fma_np, correctly rounded).  numpy's elementwise + - * / on float64 are the
rounded operations of the header, so whole rows are taken at once; the reductions are exact comparisons, so their order does not matter.  E is the scalar
spatial_ref.E restated on arrays (E_np; tests/test_svm_host.py holds the two equal).  Shares no code with embedding_amd/csrc.  Not a test module."""
import numpy as np

import kmeans_ref
import spatial_ref as sp
from nmf_ref import fma_np

TAU = 2.0 ** -40
BLOCK = 256
MAX_ROWS = 65536
LDS_ROWS = 3584


def E_np(x):
    """spatial_ref.E on an array of values <= 0"""
    x = np.asarray(x, np.float64)
    out = np.empty(x.shape, np.float64)
    under = x < sp.UNDER
    tiny = x >= -sp.TINY
    out[under] = 0.0
    out[tiny] = 1.0 + x[tiny]
    rest = ~(under | tiny)
    xr = x[rest]
    hi = xr.copy(); lo = np.zeros_like(xr); k = np.zeros(xr.shape, np.int64)
    a = (xr < -sp.HALF_LN2) & (xr > -sp.THREE_HALF_LN2)
    hi[a] = xr[a] + sp.LN2_HI; lo[a] = -sp.LN2_LO; k[a] = -1
    b = (xr < -sp.HALF_LN2) & ~a
    t = np.trunc(sp.INV_LN2 * xr[b] - 0.5)                    # truncation towards zero, as a C cast
    k[b] = t.astype(np.int64); hi[b] = xr[b] - t * sp.LN2_HI; lo[b] = t * sp.LN2_LO
    r = hi - lo
    t = r * r
    c = r - t * (sp.P1 + t * (sp.P2 + t * (sp.P3 + t * (sp.P4 + t * sp.P5))))
    with np.errstate(all="ignore"):
        y0 = 1.0 - ((r * c) / (c - 2.0) - r)
        y1 = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi)
        deep = k < -1021
        res = np.where(k == 0, y0, np.where(deep, (y1 * np.ldexp(1.0, np.where(deep, k + 1000, 0))) * sp.TWOM1000, y1 * np.ldexp(1.0, np.where(deep, 0, k))))
    out[rest] = res
    return out


def kernel_matrix(A, B, gamma):
    """K(a, b) for every row of A and of B: float32 [na x dim], [nb x dim] -> float64 [na x nb]"""
    d2 = kmeans_ref.dist_all(np.asarray(A, np.float32), np.asarray(B, np.float32))
    return E_np(-(float(gamma) * d2))


def kernel_matrix_sym(X, gamma, block=256):
    """kernel_matrix(X, X, gamma) from its upper block triangle, mirrored: K is symmetric bit for bit (tests/test_svm_host.py holds the two equal)"""
    X = np.asarray(X, np.float32)
    n = len(X)
    K = np.empty((n, n))
    for i in range(0, n, block):
        for j in range(i, n, block):
            B = kernel_matrix(X[i:i + block], X[j:j + block], gamma)
            K[i:i + block, j:j + block] = B
            K[j:j + block, i:i + block] = B.T
    return K


def solve(K, sgn, C=1.0, eps=1e-3, max_iter=10_000_000):
    """One problem on the rows of K: sgn[t] = +1 / -1 on a training row, 0 on a row that does not train.
    -> dict(alpha, G, coef, bias, iterations, converged)"""
    sgn = np.asarray(sgn, np.int64)
    n = len(sgn)
    C = float(C); eps = float(eps)
    tr = sgn != 0
    pos = sgn > 0; neg = sgn < 0
    sf = sgn.astype(np.float64)
    alpha = np.zeros(n); G = np.full(n, -1.0)
    it = 0
    while True:
        v = -sf * G                                            # exact
        up = (pos & (alpha < C)) | (neg & (alpha > 0.0))
        low = (pos & (alpha > 0.0)) | (neg & (alpha < C))
        has_up, has_low = bool(up.any()), bool(low.any())
        m = float(v[up].max()) if has_up else None
        M = float(v[low].min()) if has_low else None
        if not has_up or not has_low or m - M < eps:
            converged = 1
            break
        if it == max_iter:
            converged = 0
            break
        i = int(np.flatnonzero(up & (v == m))[0])
        cand = low & (v < m)
        b = m - v
        a = 2.0 - 2.0 * K[i]
        a = np.where(a > 0.0, a, TAU)
        with np.errstate(all="ignore"):
            score = np.where(cand, (b * b) / a, -1.0)
        j = int(np.argmax(score))                              # the first of the greatest: the least row among equals
        delta = float(b[j]) / float(a[j])
        ai, aj = float(alpha[i]), float(alpha[j])
        lim_i = C - ai if sgn[i] > 0 else ai
        lim_j = aj if sgn[j] > 0 else C - aj
        delta = min(delta, lim_i, lim_j)
        if delta == lim_i:
            ni = C if sgn[i] > 0 else 0.0
        else:
            ni = min(max(ai + delta if sgn[i] > 0 else ai - delta, 0.0), C)
        if delta == lim_j:
            nj = 0.0 if sgn[j] > 0 else C
        else:
            nj = min(max(aj - delta if sgn[j] > 0 else aj + delta, 0.0), C)
        Di, Dj = ni - ai, nj - aj
        alpha[i] = ni; alpha[j] = nj
        qi = (sf * sf[i]) * K[i]                               # the sign flips are exact
        qj = (sf * sf[j]) * K[j]
        G = np.where(tr, fma_np(qj, Dj, fma_np(qi, Di, G)), G)
        it += 1
    lo_v = m if has_up else M
    hi_v = M if has_low else m
    bias = (lo_v + hi_v) * 0.5
    return dict(alpha=alpha, G=G, coef=sf * alpha + 0.0, bias=bias, iterations=it, converged=converged, m=m, M=M)


def decision(Kx, coef, bias):
    """f(x) for every row of Kx [nx x n] = K(x, row): the support rows are those with a coefficient that is neither 0 nor NaN, ascending; blocked sum"""
    coef = np.asarray(coef, np.float64)
    sup = np.flatnonzero((coef != 0.0) & ~np.isnan(coef))
    terms = coef[sup][None, :] * Kx[:, sup]
    total = np.zeros(Kx.shape[0])
    for lo in range(0, len(sup), BLOCK):
        s = np.zeros(Kx.shape[0])
        for k in range(lo, min(lo + BLOCK, len(sup))):
            s = s + terms[:, k]
        total = total + s
    return float(bias) + total


def used_rows(n_rows, present=None, select=None):
    use = np.ones(n_rows, bool)
    if present is not None:
        use &= np.asarray(present) != 0
    if select is not None:
        use &= np.asarray(select) != 0
    return np.flatnonzero(use)


def fit(X, Y, present=None, select=None, C=1.0, gamma=None, eps=1e-3, max_iter=10_000_000, K=None):
    """dge_svm_fit*: Y [n_labels x rows] -> dict(coef [n_labels x rows], bias, iterations, converged [n_labels], support, K, used)"""
    X = np.asarray(X, np.float32)
    Y = np.atleast_2d(np.asarray(Y))
    rows, dim = X.shape
    gamma = 1.0 / dim if gamma is None else gamma
    used = used_rows(rows, present, select)
    if K is None:
        K = kernel_matrix_sym(X[used], gamma)
    L = Y.shape[0]
    coef = np.full((L, rows), np.nan); bias = np.zeros(L); its = np.zeros(L, np.int64); conv = np.zeros(L, np.int32); sup = np.zeros(L, np.int64)
    for l in range(L):
        r = solve(K, np.where(Y[l, used] != 0, 1, -1), C, eps, max_iter)
        coef[l, used] = r["coef"]; bias[l] = r["bias"]; its[l] = r["iterations"]; conv[l] = r["converged"]; sup[l] = int((r["alpha"] > 0).sum())
    return dict(coef=coef, bias=bias, iterations=its, converged=conv, support=sup, K=K, used=used, gamma=gamma)


def decide(SV, coef, bias, gamma, X=None, present=None):
    """dge_svm_decision*: coef [n_models x rows(SV)] -> [n_models x rows(X)], NaN on absent rows of X"""
    SV = np.asarray(SV, np.float32)
    X = SV if X is None else np.asarray(X, np.float32)
    coef = np.atleast_2d(np.asarray(coef, np.float64)); bias = np.atleast_1d(bias)
    out = np.full((coef.shape[0], len(X)), np.nan)
    rows = used_rows(len(X), present)
    for l in range(coef.shape[0]):
        sup = np.flatnonzero((coef[l] != 0.0) & ~np.isnan(coef[l]))
        Kx = np.zeros((len(rows), len(SV)))
        if len(sup) and len(rows):
            Kx[:, sup] = kernel_matrix(SV[sup], X[rows], gamma).T
        out[l, rows] = decision(Kx, coef[l], bias[l])
    return out


def cv(X, Y, fold, n_folds, present=None, C=1.0, gamma=None, eps=1e-3, max_iter=10_000_000):
    """dge_svm_cv*: -> dict(correct, iterations, support, converged [n_labels x F], tested [F], decision [n_labels x rows], coef [n_labels x F x rows])"""
    X = np.asarray(X, np.float32)
    Y = np.atleast_2d(np.asarray(Y))
    fold = np.asarray(fold, np.int64)
    rows, dim = X.shape
    gamma = 1.0 / dim if gamma is None else gamma
    used = used_rows(rows, present, fold >= 0)
    K = kernel_matrix_sym(X[used], gamma)
    fu = fold[used]
    L, F = Y.shape[0], int(n_folds)
    correct = np.zeros((L, F), np.int64); its = np.zeros((L, F), np.int64); sup = np.zeros((L, F), np.int64); conv = np.zeros((L, F), np.int32)
    tested = np.array([int((fu == f).sum()) for f in range(F)], np.int64)
    dec = np.full((L, rows), np.nan); coef = np.full((L, F, rows), np.nan)
    for l in range(L):
        yl = Y[l, used]
        for f in range(F):
            test = fu == f
            assert (~test).any(), "fold %d has no training rows" % f
            r = solve(K, np.where(test, 0, np.where(yl != 0, 1, -1)), C, eps, max_iter)
            its[l, f] = r["iterations"]; conv[l, f] = r["converged"]; sup[l, f] = int((r["alpha"] > 0).sum())
            c = np.where(test, np.nan, r["coef"])
            coef[l, f, used] = c
            if test.any():
                fx = decision(K[test], c, r["bias"])
                dec[l, used[test]] = fx
                correct[l, f] = int(((fx > 0.0).astype(np.int64) == (yl[test] != 0)).sum())
            coef[l, f, used[~test]] = r["coef"][~test]
    return dict(correct=correct, tested=tested, iterations=its, support=sup, converged=conv, decision=dec, coef=coef, gamma=gamma)


def dual_objective(K, sgn, alpha):
    """sum alpha - 1/2 sum_ij alpha_i alpha_j s_i s_j K_ij (plain float64: a figure, not a rule)"""
    z = np.asarray(sgn, np.float64) * alpha
    return float(alpha.sum() - 0.5 * z @ (K @ z))


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def table(n, dim, seed, dup=0):
    """n rows of dim float32 columns in two overlapping classes; dup > 0: the last dup rows repeat the first dup with the opposite label"""
    rng = np.random.default_rng(seed)
    y = (np.arange(n) % 2).astype(np.uint8) if n < 8 else (rng.random(n) < 0.45).astype(np.uint8)
    if n >= 2:
        y[0] = 1; y[1] = 0
    X = (rng.standard_normal((n, dim)) + 0.8 * (2.0 * y[:, None] - 1.0)).astype(np.float32)
    if dup:
        X[n - dup:] = X[:dup]; y[n - dup:] = 1 - y[:dup]
    return X, y
