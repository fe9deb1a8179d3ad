"""The NMF rule of include/dge.h read out in Python.  Test infrastructure: what csrc/nmf_rule.h and the kernels of csrc/nmf.hip are held to, bit for bit.

The fused multiply-add comes in two forms.  `fma` is exact rational arithmetic (fractions.Fraction) and one correctly rounded conversion — this Python has no
math.fma.  `fma_np` is the same on numpy binary64 arrays, put together from error-free pieces (Veltkamp's split and Dekker's exact product, Knuth's exact
sum, and Boldo and Melquiond's rounding to odd of the low parts, which makes the last addition the one correct rounding).  It is valid where neither the
product's error term nor the product itself under- or overflows; tests/test_nmf_ref.py holds it to `fma` bit for bit.  nmf(..., exact=True) runs the rule on
`fma` with Python loops (small shapes only), exact=False on `fma_np`."""
import math
from fractions import Fraction

import numpy as np

BLOCK = 256
LANES = 16
EPS = 2.0 ** -52
MASK = (1 << 64) - 1
DIVERGENCE, EUCLIDEAN = 0, 1


def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def u(seed, t):
    return float(mix64((seed + t) & MASK) >> 11) * 2.0 ** -53


def fma(a, b, c):
    """a * b + c with one rounding (float(Fraction) is correctly rounded, ties to even)"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _two_sum(a, b):
    s = a + b
    bp = s - a
    ap = s - bp
    return s, (a - ap) + (b - bp)


def _split(a):
    c = 134217729.0 * a                                      # Veltkamp's split at 27 bits
    hi = c - (c - a)
    return hi, a - hi


def fma_np(a, b, c):
    """fma(a, b, c) on binary64 arrays (broadcast), correctly rounded"""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl        # Dekker: p + e == a * b exactly
    hi, lo = _two_sum(c, p)
    v, r = _two_sum(lo, e)                                   # v + r == lo + e exactly; round v to odd
    fix = (r != 0.0) & ((v.view(np.int64) & 1) == 0)
    if fix.any():
        v = np.where(fix, np.nextafter(v, np.where(r > 0.0, np.inf, -np.inf)), v)
    return hi + v


def floor_eps(x):
    return np.where(x < EPS, EPS, x)


def init_factors(n, m, rank, seed, vmax):
    W = np.empty((n, rank)); H = np.empty((rank, m))
    for i in range(n):
        for r in range(rank):
            W[i, r] = u(seed, i * rank + r) * vmax
    for r in range(rank):
        for j in range(m):
            H[r, j] = u(seed, n * rank + r * m + j) * vmax
    return floor_eps(W), floor_eps(H)


def blocked_sum_rows(X):
    """the BLOCKED SUM over the first axis of X [cnt x ...] for every trailing index at once.  A short last block is padded with +0.0, which changes no bit of a
    sum of values that are not -0.0 (here every value is > 0)."""
    X = np.asarray(X, np.float64)
    cnt = X.shape[0]
    nb = (cnt + BLOCK - 1) // BLOCK
    pad = np.zeros((nb * BLOCK,) + X.shape[1:])
    pad[:cnt] = X
    pad = pad.reshape((nb, BLOCK) + X.shape[1:])
    bs = np.zeros((nb,) + X.shape[1:])
    for k in range(BLOCK):
        bs = bs + pad[:, k]
    s = np.zeros(X.shape[1:])
    for b in range(nb):
        s = s + bs[b]
    return s


def blocked_sum(v):
    """the BLOCKED SUM of a list, by Python loops"""
    total = 0.0
    for lo in range(0, len(v), BLOCK):
        s = 0.0
        for x in v[lo:lo + BLOCK]:
            s += float(x)
        total += s
    return total


class Entries:
    """the kept entries of the rule: by row (ri, ci, v) and the permutation that lists them by column"""

    def __init__(self, rows, cols, vals, shape):
        rows = np.asarray(rows, np.int64); cols = np.asarray(cols, np.int64); vals = np.asarray(vals, np.float64)
        n, m = shape
        assert len(rows) == len(cols) == len(vals) >= 1 and n >= 1 and m >= 1
        assert ((rows >= 0) & (rows < n) & (cols >= 0) & (cols < m)).all() and np.isfinite(vals).all() and (vals >= 0).all()
        keep = vals != 0
        self.zeros = int((~keep).sum())
        rows, cols, vals = rows[keep], cols[keep], vals[keep]
        assert len(vals) >= 1 and len(np.unique(rows * m + cols)) == len(vals)
        o = np.argsort(rows * m + cols, kind="stable")
        self.ri, self.ci, self.v = rows[o], cols[o], vals[o]
        self.perm = np.argsort(self.ci * n + self.ri, kind="stable")
        self.n, self.m, self.ne = n, m, len(vals)
        self.vmax = float(vals.max())
        # position of an entry inside its row, and of the t-th entry of the column order inside its column
        self.rt = np.arange(self.ne) - np.searchsorted(self.ri, self.ri, "left")
        cj = self.ci[self.perm]
        self.ct = np.arange(self.ne) - np.searchsorted(cj, cj, "left")


def segment_sums(seg, t, A, b, count, exact=False):
    """SEGMENT SUM for every segment and every r at once: entry x (in the segments' order) belongs to segment seg[x], is its t[x]-th product, and its products are
    A[x][r] * b[x].  -> [count x rank]"""
    rank = A.shape[1]
    p = np.zeros((count, LANES, rank))
    lane = t % LANES
    step = t // LANES
    if exact:
        for x in range(len(seg)):                            # ascending t inside a segment: the order of the arrays
            for r in range(rank):
                p[seg[x], lane[x], r] = fma(A[x, r], b[x], p[seg[x], lane[x], r])
    else:
        for k in range(int(step.max()) + 1 if len(step) else 0):
            sel = np.nonzero(step == k)[0]                   # one product at most per (segment, partial)
            p[seg[sel], lane[sel]] = fma_np(A[sel], b[sel, None], p[seg[sel], lane[sel]])
    s = LANES // 2
    while s:
        p[:, :s] = p[:, :s] + p[:, s:2 * s]
        s //= 2
    return p[:, 0].copy()


def chain(A, B, exact=False):
    """acc = +0.0; for r ascending: acc = fma(A[..., r], B[..., r], acc)"""
    A, B = np.broadcast_arrays(A, B)
    acc = np.zeros(A.shape[:-1])
    for r in range(A.shape[-1]):
        if exact:
            flat = [fma(x, y, z) for x, y, z in zip(A[..., r].ravel(), B[..., r].ravel(), acc.ravel())]
            acc = np.array(flat, np.float64).reshape(acc.shape)
        else:
            acc = fma_np(A[..., r], B[..., r], acc)
    return acc


def P_of(E, W, H, exact=False):
    return chain(W[E.ri], H.T[E.ci], exact)


def iterate(E, W, H, update, exact=False):
    """one iteration of the rule -> the new (W, H)"""
    n, m = E.n, E.m
    cr = E.ri[E.perm]; cc = E.ci[E.perm]
    with np.errstate(all="ignore"):
        if update == DIVERGENCE:
            Q = E.v / P_of(E, W, H, exact)
            N = segment_sums(cc, E.ct, W[cr], Q[E.perm], m, exact)                  # [m x rank]
            d = blocked_sum_rows(W)
            H = floor_eps(H * (N.T / d[:, None]))
            Q = E.v / P_of(E, W, H, exact)
            N2 = segment_sums(E.ri, E.rt, H.T[E.ci], Q, n, exact)                   # [n x rank]
            d2 = blocked_sum_rows(H.T)
            W = floor_eps(W * (N2 / d2[None, :]))
        else:
            A = segment_sums(cc, E.ct, W[cr], E.v[E.perm], m, exact)
            G = blocked_sum_rows(W[:, :, None] * W[:, None, :])                     # [rank x rank]
            B = chain(G[:, None, :], H.T[None, :, :], exact)                        # B[r][j] = chain over s of G[r][s] * H[s][j]
            H = floor_eps(H * (A.T / B))
            A2 = segment_sums(E.ri, E.rt, H.T[E.ci], E.v, n, exact)
            G2 = blocked_sum_rows(H.T[:, :, None] * H.T[:, None, :])
            B2 = chain(W[:, None, :], G2.T[None, :, :], exact)                      # B'[i][r] = chain over s of W[i][s] * G'[s][r]
            W = floor_eps(W * (A2 / B2))
    return W, H


def objective(E, W, H, update):
    """-> (the objective of the rule in plain numpy and math.fsum, A = the sum of the absolute values of its terms)"""
    P = P_of(E, W, H)
    if update == DIVERGENCE:
        terms = [E.v * np.log(E.v / P), -E.v, blocked_sum_rows(W) * blocked_sum_rows(H.T)]
    else:
        d = E.v - P
        terms = [d * d, -(P * P), (blocked_sum_rows(W[:, :, None] * W[:, None, :]) * blocked_sum_rows(H.T[:, :, None] * H.T[:, None, :])).ravel()]
    flat = np.concatenate([np.ravel(t) for t in terms])
    return math.fsum(flat), math.fsum(np.abs(flat))


def objective_bound(E, rank, A):
    return (E.ne + rank * rank + 8) * 2.0 ** -50 * A


def nmf(rows, cols, vals, shape, rank=10, max_iter=30, update=DIVERGENCE, seed=1, init=None, exact=False, trace=None):
    """-> dict of W [n x rank], H [rank x m] and the counters of struct dge_nmf_info (objective and its A included).  trace: a list that receives the
    objective after every iteration."""
    assert 1 <= rank <= 32 and 1 <= max_iter <= 10000 and update in (DIVERGENCE, EUCLIDEAN)
    E = Entries(rows, cols, vals, shape)
    n, m = shape
    if init is None:
        W, H = init_factors(n, m, rank, seed, E.vmax)
    else:
        W = floor_eps(np.array(init[0], np.float64).reshape(n, rank)); H = floor_eps(np.array(init[1], np.float64).reshape(rank, m))
        assert np.isfinite(W).all() and np.isfinite(H).all() and (np.asarray(init[0]) >= 0).all() and (np.asarray(init[1]) >= 0).all()
    for _ in range(max_iter):
        W, H = iterate(E, W, H, update, exact)
        if trace is not None:
            trace.append(objective(E, W, H, update))
    obj, A = objective(E, W, H, update)
    return dict(W=W, H=H, rows=n, cols=m, entries=E.ne, zeros=E.zeros, iterations=max_iter, vmax=E.vmax, objective=obj, A=A, E=E)


def random_sparse(n, m, density, seed, hub=None, vmax=50):
    """integer values, as flows are: about density * n * m distinct cells with values in 1 .. vmax; hub = (row, col): that row and that column are filled
    completely.  -> rows int32, cols int32, vals float64, in a shuffled order"""
    rng = np.random.default_rng(seed)
    cells = set(rng.integers(0, n * m, max(1, int(density * n * m))).tolist())
    if hub is not None:
        cells |= {hub[0] * m + j for j in range(m)} | {i * m + hub[1] for i in range(n)}
    cells = np.array(sorted(cells), np.int64)
    rng.shuffle(cells)
    return (cells // m).astype(np.int32), (cells % m).astype(np.int32), rng.integers(1, vmax + 1, len(cells)).astype(np.float64)


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
