"""The k-means rule of include/dge.h read out in Python, and the numpy transcription of the reference's clusteringAccuracy
(P/embeddingEvaluation_tract.py:544-571, argsort with kind="stable").  Test infrastructure: what csrc/kmeans_rule.h, csrc/cluster_match.h and the kernels of
csrc/kmeans.hip are held to, bit for bit.

The fused multiply-add is `fma` below: exact rational arithmetic (fractions.Fraction) and one correctly rounded conversion — this Python has no math.fma.
`dist` is the chain of the rule on it.  A whole clustering needs n * k * dim of those per pass, which Fraction cannot deliver in a test's time, so the passes
use `dist_all`: the same chain for all rows and centres at once in numpy binary64, each fma put together from error-free pieces (Dekker's exact square,
Knuth's exact sum, and Boldo and Melquiond's rounding to odd of the low parts, which makes the last addition the one correct rounding).  It is valid here
because nothing under- or overflows: |t| is 0 or in [2^-149, 2^129).  tests/test_kmeans_host.py holds dist_all to dist bit for bit.  The blocked sums are
Python loops, the fixed-point sums Python ints."""
import math
from fractions import Fraction

import numpy as np

BLOCK = 256
MASK = (1 << 64) - 1


def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def fma(a, b, c):
    """a * b + c with one rounding (float(Fraction) is correctly rounded, ties to even)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def dist(x, c):
    """d of one row to one centre: float32 sequences of one length"""
    acc = 0.0
    for xv, cv in zip(x, c):
        t = float(xv) - float(cv)
        acc = fma(t, t, acc)
    return acc


def _two_sum(a, b):
    s = a + b
    bp = s - a
    ap = s - bp
    return s, (a - ap) + (b - bp)


def fma_sq_add(t, acc):
    """fma(t, t, acc) on binary64 arrays, correctly rounded"""
    p = t * t
    c = 134217729.0 * t                                      # Veltkamp's split at 27 bits, Dekker's product: p + e == t * t exactly
    th = c - (c - t)
    tl = t - th
    e = ((th * th - p) + 2.0 * th * tl) + tl * tl
    hi, lo = _two_sum(acc, p)
    v, r = _two_sum(lo, e)                                   # v + r == lo + e exactly; round v to odd
    fix = (r != 0.0) & ((v.view(np.int64) & 1) == 0)
    if fix.any():
        v = np.where(fix, np.nextafter(v, np.where(r > 0.0, np.inf, -np.inf)), v)
    return hi + v


def dist_all(X, centres):
    """d(i, c) for every row and centre: float32 [n x dim], float32 [k x dim] -> float64 [n x k]"""
    X = np.asarray(X, np.float32).astype(np.float64)
    Cn = np.asarray(centres, np.float32).astype(np.float64)
    acc = np.zeros((X.shape[0], Cn.shape[0]))
    for j in range(X.shape[1]):
        t = X[:, j:j + 1] - Cn[None, :, j]
        acc = fma_sq_add(np.ascontiguousarray(t), acc)
    return acc


def scale_bits(max_abs, n):
    e = math.frexp(float(max_abs))[1] if max_abs != 0 else 0
    return 62 - int(n).bit_length() - e


def quantise(x, s):
    """x * 2^s to the nearest integer, ties to even (Python's round on a float is that)"""
    return round(math.ldexp(float(x), s))


def centre_from_sum(S, count, s):
    """int -> binary64 (Python rounds to nearest even), one division, an exact scaling, one rounding to binary32"""
    with np.errstate(over="ignore"):
        return np.float32(math.ldexp(float(S) / float(count), -s))


def first_pick(seed, r, k, n):
    return mix64((seed + r * k) & MASK) % n


def draw(seed, r, k, c):
    return float(mix64((seed + r * k + c) & MASK) >> 11) * 2.0 ** -53


def block_sums(v):
    out = []
    for lo in range(0, len(v), BLOCK):
        s = 0.0
        for x in v[lo:lo + BLOCK]:
            s += float(x)
        out.append(s)
    return out


def sum_blocks(bs):
    s = 0.0
    for x in bs:
        s += x
    return s


def blocked_sum(v):
    return sum_blocks(block_sums(v))


def walk(v, bs, target):
    """the first row after which the running sum exceeds target, or -1"""
    run = 0.0
    for b, x in enumerate(bs):
        nxt = run + x
        if nxt > target:
            hi = min(len(v), (b + 1) * BLOCK)
            for i in range(b * BLOCK, hi):
                run += float(v[i])
                if run > target:
                    return i
            return hi - 1
        run = nxt
    return -1


def pick(dmin, u):
    bs = block_sums(dmin)
    i = walk(dmin, bs, u * sum_blocks(bs))
    if i < 0:
        i = int(np.argmax(dmin))                             # the first of the greatest
    return i


def seed_centres(X, k, seed, r, every=None):
    n = len(X)
    rows = [first_pick(seed, r, k, n)]
    dmin = None
    # every (optional): d of every row to every row, formed once for all restarts of a small table — the same chains, fewer numpy calls
    for c in range(1, k):
        d = every[:, rows[-1]] if every is not None else dist_all(X, X[rows[-1]:rows[-1] + 1])[:, 0]
        dmin = d if dmin is None else np.minimum(dmin, d)
        rows.append(pick(dmin, draw(seed, r, k, c)))
    return X[rows].copy(), rows


def kmeans(X, k, seed=1, n_init=10, max_iter=300, init=None):
    """X: the selected rows, float32 [n x dim].  -> dict of labels, centres, inertia, iterations, best_restart, total_iterations, scale_bits, empty"""
    X = np.ascontiguousarray(X, np.float32)
    n, dim = X.shape
    assert 1 <= k <= 64 and 1 <= dim <= 256 and k <= n and n_init >= 1 and max_iter >= 1 and np.isfinite(X).all()
    s = scale_bits(np.abs(X).max(), n)
    Q = np.empty((n, dim), object)
    for i in range(n):
        for j in range(dim):
            Q[i, j] = quantise(X[i, j], s)
    best = None
    total = 0
    every = dist_all(X, X) if init is None and k > 1 and n <= 8 * k else None
    for r in range(1 if init is not None else n_init):
        centres = np.array(init, np.float32).reshape(k, dim).copy() if init is not None else seed_centres(X, k, seed, r, every)[0]
        labels = np.full(n, -1)
        it = 0
        while True:
            D = dist_all(X, centres)
            new = np.argmin(D, axis=1)                       # the least c among equals
            d = D[np.arange(n), new]
            changed = int((new != labels).sum())
            labels = new
            it += 1
            count = [int((labels == c).sum()) for c in range(k)]
            if changed == 0 or it == max_iter:
                break
            for c in range(k):
                if count[c]:
                    S = Q[labels == c].sum(axis=0)           # Python ints
                    centres[c] = [centre_from_sum(S[j], count[c], s) for j in range(dim)]
        total += it
        inertia = blocked_sum(d)
        if best is None or inertia < best["inertia"]:
            best = dict(labels=labels.astype(np.int32), centres=centres.copy(), inertia=inertia, iterations=it, best_restart=r, empty=count.count(0))
    best.update(total_iterations=total, scale_bits=s, rows=n)
    return best


def kmeans_rows(rows, k, present=None, select=None, **kw):
    """the rule on a table with absent and unselected rows: labels of the whole table (-1 where not selected), the rest as kmeans()"""
    rows = np.ascontiguousarray(rows, np.float32)
    take = np.ones(len(rows), bool)
    if present is not None:
        take &= np.asarray(present) != 0
    if select is not None:
        take &= np.asarray(select) != 0
    res = kmeans(rows[take], k, **kw)
    labels = np.full(len(rows), -1, np.int32)
    labels[take] = res["labels"]
    res["labels"] = labels
    return res


def clustering_accuracy(labels, gnd, k):
    """The accuracy rule of include/dge.h as numpy states it: the table from two label arrays (-1: none), clusters and labels visited in the order
    argsort(kind="stable")[::-1] gives, each cluster mapped to the first label still free.  -> (accuracy, cnt int64 [k x k], map int32 [k])"""
    labels = np.asarray(labels); gnd = np.asarray(gnd)
    cnt = np.zeros((k, k))
    both = (labels >= 0) & (gnd >= 0)
    np.add.at(cnt, (labels[both], gnd[both]), 1)
    mapping = np.full(k, -1, np.int32)
    free = np.ones(k, bool)
    hit = 0.0
    for a in np.argsort(cnt.sum(axis=1), kind="stable")[::-1]:
        for g in np.argsort(cnt[a], kind="stable")[::-1]:
            if free[g]:
                free[g] = False
                mapping[a] = g
                hit += cnt[a, g]
                break
    n_gnd = int((gnd >= 0).sum())
    return (hit / n_gnd if n_gnd else float("nan")), cnt.astype(np.int64), mapping


def blobs(n, dim, k, seed=12345, spread=1.0, box=10.0):
    """Gaussian blobs: k centres uniform in [-box, box]^dim, rows dealt to them in turn -> (float32 [n x dim], truth int [n])"""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(-box, box, (k, dim))
    truth = np.arange(n) % k
    return (mu[truth] + spread * rng.standard_normal((n, dim))).astype(np.float32), truth
