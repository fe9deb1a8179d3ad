"""The ridge rule of include/dge.h read out in Python: moments in the blocked order, the system of every lambda, LDL' without pivoting, the two substitutions,
the leverage, the left-out errors and the two figures.  Test infrastructure: what csrc/ridge_rule.h and the kernels of csrc/ridge.hip are held to, bit for bit.

The fused multiply-add is `fma` below: exact rational arithmetic (fractions.Fraction) and one correctly rounded conversion, as in tests/kmeans_ref.py — this
Python has no math.fma.  Everything else is Python's own binary64 arithmetic, one rounding an operation.  `exact_loo` is no part of the rule: the left-out
predictions of the n refits in rational arithmetic, which the rule's results are compared with."""
from fractions import Fraction

import numpy as np

BLOCK = 256


class Refused(Exception):
    """kind: 'pivot' (index = the column) or 'leverage' (index = the used row); lam: the index of the lambda"""

    def __init__(self, kind, lam, index):
        super().__init__("%s %d under lambda %d" % (kind, index, lam))
        self.kind, self.lam, self.index = kind, lam, index


def fma(a, b, c):
    """a * b + c with one rounding (float(Fraction) is correctly rounded, ties to even); an exact zero takes the sign IEEE 754 gives it"""
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        return a * b + c if (a == 0 or b == 0) else 0.0
    return float(r)


def design(X):
    """float32 [n x dim] -> the rows z as lists of Python floats, z[0] = 1.0"""
    X = np.asarray(X, np.float32)
    return [[1.0] + [float(v) for v in row] for row in X]


def blocked(values):
    """the blocked sum of a sequence of floats"""
    total = 0.0
    for lo in range(0, len(values), BLOCK):
        b = 0.0
        for v in values[lo:lo + BLOCK]:
            b += v
        total += b
    return total


def moments(Z, Y):
    """-> (G [P x P] symmetric, c [T x P], ysum [T])"""
    n, P, T = len(Z), len(Z[0]), len(Y[0])
    G = np.zeros((P, P)); c = np.zeros((T, P))
    for a in range(P):
        for b in range(a, P):
            total = 0.0
            for lo in range(0, n, BLOCK):
                acc = 0.0
                for i in range(lo, min(lo + BLOCK, n)):
                    acc = acc + Z[i][a] * Z[i][b]              # the product of two float32 values is exact
                total += acc
            G[a, b] = G[b, a] = total
        for t in range(T):
            total = 0.0
            for lo in range(0, n, BLOCK):
                acc = 0.0
                for i in range(lo, min(lo + BLOCK, n)):
                    acc = fma(Z[i][a], Y[i][t], acc)
                total += acc
            c[t, a] = total
    ysum = np.array([blocked([Y[i][t] for i in range(n)]) for t in range(T)])
    return G, c, ysum


def factor(G, lam, l=0):
    """-> (d [P], L [P x P] unit lower) of A = G + lam on the diagonal from 1 on"""
    P = len(G)
    L = np.zeros((P, P)); d = np.zeros(P)
    for j in range(P):
        acc = float(G[j, j]) + lam if j >= 1 else float(G[j, j])
        for k in range(j):
            acc = fma(-L[j, k], L[j, k] * d[k], acc)
        d[j] = acc
        if not acc > 0:
            raise Refused("pivot", l, j)
        L[j, j] = 1.0
        for i in range(j + 1, P):
            acc = float(G[i, j])
            for k in range(j):
                acc = fma(-L[i, k], L[j, k] * d[k], acc)
            L[i, j] = acc / d[j]
    return d, L


def coefficients(d, L, c_t):
    P = len(d)
    w = [float(v) for v in c_t]
    for j in range(P):
        for k in range(j):
            w[j] = fma(-L[j, k], w[k], w[j])
    for j in range(P):
        w[j] = w[j] / d[j]
    for j in range(P - 1, -1, -1):
        for k in range(P - 1, j, -1):
            w[j] = fma(-L[k, j], w[k], w[j])
    return w


def leverage(d, L, z):
    P = len(d)
    u = list(z)
    for j in range(P):
        for k in range(j):
            u[j] = fma(-L[j, k], u[k], u[j])
    inv = [1.0 / float(v) for v in d]
    acc = 0.0
    for j in range(P):
        acc = fma(u[j], u[j] * inv[j], acc)
    return acc


def predict(z, beta):
    p = float(beta[0])
    for j in range(1, len(z)):
        p = fma(z[j], float(beta[j]), p)
    return p


def ridge_loo(X, Y, lambdas):
    """The rule on the used rows X float32 [n x dim], targets Y [n x T], penalties.  -> dict(G, c, ysum, d [L x P], L [L x P x P], beta [L x T x P], h [L x n],
    e, loo_pred [L x T x n], mae, mre [L x T]); raises Refused."""
    Z = design(X)
    Y = np.asarray(Y, np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    Yl = [[float(v) for v in row] for row in Y]
    n, P, T, nl = len(Z), len(Z[0]), Y.shape[1], len(lambdas)
    G, c, ysum = moments(Z, Yl)
    d = np.zeros((nl, P)); L = np.zeros((nl, P, P)); beta = np.zeros((nl, T, P))
    for l, lam in enumerate(lambdas):                             # every factorisation before the first leverage
        d[l], L[l] = factor(G, float(lam), l)
        for t in range(T):
            beta[l, t] = coefficients(d[l], L[l], c[t])
    h = np.zeros((nl, n)); e = np.zeros((nl, T, n)); pred = np.zeros((nl, T, n)); mae = np.zeros((nl, T)); mre = np.zeros((nl, T))
    for l in range(nl):
        for i in range(n):
            h[l, i] = leverage(d[l], L[l], Z[i])
            g = 1.0 - h[l, i]
            if not g > 0:
                raise Refused("leverage", l, i)
            for t in range(T):
                r = Yl[i][t] - predict(Z[i], beta[l, t])
                e[l, t, i] = r / g
                pred[l, t, i] = Yl[i][t] - e[l, t, i]
        for t in range(T):
            mae[l, t] = blocked([abs(float(v)) for v in e[l, t]]) / float(n)
            with np.errstate(divide="ignore", invalid="ignore"):
                mre[l, t] = np.float64(mae[l, t]) / (np.float64(ysum[t]) / np.float64(n))
    return dict(G=G, c=c, ysum=ysum, d=d, L=L, beta=beta, h=h, e=e, loo_pred=pred, mae=mae, mre=mre)


def _solve(A, b):
    """Gauss-Jordan on Fractions; A is positive definite or the caller made sure it is regular"""
    n = len(A)
    M = [list(A[i]) + [b[i]] for i in range(n)]
    for col in range(n):
        piv = next(r for r in range(col, n) if M[r][col] != 0)
        M[col], M[piv] = M[piv], M[col]
        pv = M[col][col]
        M[col] = [v / pv for v in M[col]]
        for r in range(n):
            if r != col and M[r][col] != 0:
                f = M[r][col]
                M[r] = [a - f * b_ for a, b_ in zip(M[r], M[col])]
    return [M[i][n] for i in range(n)]


def exact_loo(X, y, lam):
    """For every row i: fit ridge (intercept not penalised) on the other rows, exactly, and predict row i.  X [n x dim], y [n], lam a float -> Fractions [n]"""
    Z = [[Fraction(v) for v in z] for z in design(X)]
    y = [Fraction(float(v)) for v in y]
    n, P = len(Z), len(Z[0])
    lam = Fraction(float(lam))
    out = []
    for i in range(n):
        rows = [r for r in range(n) if r != i]
        A = [[sum(Z[r][a] * Z[r][b] for r in rows) + (lam if a == b and a >= 1 else 0) for b in range(P)] for a in range(P)]
        rhs = [sum(Z[r][a] * y[r] for r in rows) for a in range(P)]
        beta = _solve(A, rhs)
        out.append(sum(Z[i][j] * beta[j] for j in range(P)))
    return out
