"""The LINE rule of include/dge.h read out in Python.  Test infrastructure: what csrc/line_rule.h and the kernels of csrc/line.hip are held to, bit for bit.

The tables are int64 arrays (Python ints in the scalar pieces); every real is a binary64 and every operation rounds once.  The fused multiply-add of the dot is
nmf_ref.fma_np (held to exact rational arithmetic by tests/test_nmf_ref.py); a batch is computed for all its samples and targets at once, which is what
"synchronous" means: every read sees the tables as they stood at the batch's start, and the integer adds commute."""
import numpy as np

import spatial_ref
from nmf_ref import LANES, MASK, fma, fma_np, mix64, same_bits  # noqa: F401  (re-exported for the tests)

FIX = 2.0 ** 32
UNFIX = 2.0 ** -32
CELL_LIMIT = 1 << 40
SEED_TAG = 0x4C494E45
SIG_N = 1000
MAX_N, MAX_DIM, MAX_NEG, MAX_BATCH, MAX_SAMPLES, MAX_WEIGHT, MAX_TOTAL = 1 << 22, 256, 32, 65536, 1 << 40, 1 << 31, 1 << 40


class BoundLeft(Exception):
    """a table cell reached |P| >= 2^40 after batch `batch`"""

    def __init__(self, batch):
        Exception.__init__(self, "batch %d" % batch)
        self.batch = batch


def mix64_np(x):
    x = np.asarray(x, np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def seed2(seed):
    return mix64((seed ^ SEED_TAG) & MASK)


def u(s2, t):
    return float(mix64((s2 + t) & MASK) >> 11) * 2.0 ** -53


def quant(x):
    """rint(x * 2^32), ties to even -> int"""
    return int(np.rint(np.float64(x) * FIX))


def init_cell(s2, t, dim):
    return quant((u(s2, t) - 0.5) / float(dim))


def init_table(n, dim, seed):
    with np.errstate(over="ignore"):
        t = np.uint64(seed2(seed)) + np.arange(n * dim, dtype=np.uint64)
    uu = (mix64_np(t) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return np.rint(((uu - 0.5) / float(dim)) * FIX).astype(np.int64).reshape(n, dim)


def search(C, r, total):
    """the least e with C[e] > r mod total"""
    return int(np.searchsorted(np.asarray(C, np.int64), r % total, side="right"))


def neg_weight(d):
    x = np.float64(d)
    return int(np.sqrt(x * np.sqrt(x)) * 1024.0)


def rho_b(rho0, first, samples):
    rho = rho0 * (1.0 - float(first) / float(samples + 1))
    least = rho0 * 0.0001
    return least if rho < least else rho


def sig_entry(k):
    x = (k * 12.0) / 1000.0 - 6.0
    if x >= 0.0:
        return 1.0 / (1.0 + spatial_ref.E(-x))
    e = spatial_ref.E(x)
    return e / (1.0 + e)


_T = None


def sig_table():
    global _T
    if _T is None:
        _T = np.array([sig_entry(k) for k in range(SIG_N)], np.float64)
    return _T


def sig(f):
    """sig of the rule on a binary64 array (or one value)"""
    f = np.asarray(f, np.float64)
    inside = np.clip(f, -6.0, 6.0)
    k = np.minimum(SIG_N - 1, (((inside + 6.0) * 1000.0) / 12.0).astype(np.int64))
    return np.where(f > 6.0, 1.0, np.where(f < -6.0, 0.0, sig_table()[k]))


def dot(A, B):
    """the SEGMENT SUM over the last axis of A * B (broadcast)"""
    A, B = np.broadcast_arrays(np.asarray(A, np.float64), np.asarray(B, np.float64))
    dim = A.shape[-1]
    p = np.zeros(A.shape[:-1] + (LANES,))
    for lo in range(0, dim, LANES):
        w = min(LANES, dim - lo)
        p[..., :w] = fma_np(A[..., lo:lo + w], B[..., lo:lo + w], p[..., :w])
    s = LANES // 2
    while s:
        p[..., :s] = p[..., :s] + p[..., s:2 * s]
        s //= 2
    return p[..., 0].copy()


def term(g, x):
    """rint((g * x) * 2^32) -> int64 array"""
    return np.rint((np.asarray(g, np.float64) * np.asarray(x, np.float64)) * FIX).astype(np.int64)


class Graph:
    """the kept edges in (src, dst) order with the edge table and the negative table"""

    def __init__(self, src, dst, w, n):
        src = np.asarray(src, np.int64); dst = np.asarray(dst, np.int64); w = np.asarray(w, np.float64)
        assert len(src) == len(dst) == len(w) >= 1 and 1 <= n <= MAX_N
        assert ((src >= 0) & (src < n) & (dst >= 0) & (dst < n)).all()
        assert np.isfinite(w).all() and (w >= 0).all() and (w == np.rint(w)).all() and (w < MAX_WEIGHT).all()
        keep = w != 0
        self.zeros = int((~keep).sum())
        src, dst, w = src[keep], dst[keep], w[keep].astype(np.int64)
        assert len(w) >= 1 and len(np.unique(src * n + dst)) == len(w)
        o = np.argsort(src * n + dst, kind="stable")
        self.es, self.ed, self.ew = src[o], dst[o], w[o]
        self.n, self.ne = n, len(w)
        self.C = np.cumsum(self.ew)
        self.W = int(self.C[-1])
        assert self.W < MAX_TOTAL
        self.d = np.zeros(n, np.int64)
        np.add.at(self.d, self.es, self.ew)
        x = self.d.astype(np.float64)
        self.nw = (np.sqrt(x * np.sqrt(x)) * 1024.0).astype(np.int64)
        self.NC = np.cumsum(self.nw)
        self.N = int(self.NC[-1])
        self.touched = np.zeros(n, bool)
        self.touched[self.es] = True; self.touched[self.ed] = True

    def draws(self, seed, first, count, K):
        """int64 [count x (K + 2)]: u, v, the K negatives of the samples first .. first + count - 1"""
        with np.errstate(over="ignore"):
            base = np.uint64(seed & MASK) + np.uint64(64) * (np.uint64(first) + np.arange(count, dtype=np.uint64))
            r = mix64_np(base[:, None] + np.arange(K + 1, dtype=np.uint64)[None, :])
        e = np.searchsorted(self.C, (r[:, 0] % np.uint64(self.W)).astype(np.int64), side="right")
        out = np.empty((count, K + 2), np.int64)
        out[:, 0] = self.es[e]; out[:, 1] = self.ed[e]
        if K:
            out[:, 2:] = np.searchsorted(self.NC, (r[:, 1:] % np.uint64(self.N)).astype(np.int64), side="right")
        return out


def batch_step(PX, PY, dr, order, rho):
    """one synchronous mini-batch on the int64 tables, in place; dr: the draws of its samples"""
    K = dr.shape[1] - 2
    PB = PX if order == 1 else PY
    U, Tg = dr[:, 0], dr[:, 1:]
    A = PX[U].astype(np.float64) * UNFIX                     # [cnt x dim], exact
    Bt = PB[Tg].astype(np.float64) * UNFIX                   # [cnt x (K + 1) x dim]
    label = np.zeros(K + 1); label[0] = 1.0
    g = (label[None, :] - sig(dot(A[:, None, :], Bt))) * rho
    DX = np.zeros_like(PX); DB = DX if order == 1 else np.zeros_like(PY)
    np.add.at(DB, Tg, term(g[:, :, None], A[:, None, :]))
    np.add.at(DX, U, term(g[:, :, None], Bt).sum(axis=1))
    PX += DX
    if order != 1:
        PY += DB


def line(src, dst, w, n, dim=20, order=2, negative=5, samples=1000, batch=64, rho0=0.025, seed=1, init=None):
    """-> dict of X, Y [n x dim], touched and the counters of struct dge_line_info; BoundLeft when the rule's bound is left"""
    assert 1 <= dim <= MAX_DIM and order in (1, 2) and 0 <= negative <= MAX_NEG and 1 <= batch <= MAX_BATCH and 1 <= samples <= MAX_SAMPLES and 0 < rho0 <= 1
    G = Graph(src, dst, w, n)
    PY = np.zeros((n, dim), np.int64)
    if init is None:
        PX = init_table(n, dim, seed)
    else:
        ix, iy = init if isinstance(init, (tuple, list)) else (init, None)
        ix = np.asarray(ix, np.float64).reshape(n, dim)
        assert np.isfinite(ix).all() and (np.abs(ix) < 256).all()
        PX = np.rint(ix * FIX).astype(np.int64)
        if iy is not None:
            iy = np.asarray(iy, np.float64).reshape(n, dim)
            assert np.isfinite(iy).all() and (np.abs(iy) < 256).all()
            PY = np.rint(iy * FIX).astype(np.int64)
    batches = (samples + batch - 1) // batch
    for b in range(batches):
        first = b * batch
        batch_step(PX, PY, G.draws(seed, first, min(batch, samples - first), negative), order, rho_b(rho0, first, samples))
        if max(int(np.abs(PX).max()), int(np.abs(PY).max())) >= CELL_LIMIT:
            raise BoundLeft(b)
    big = max(int(np.abs(PX).max()), int(np.abs(PY).max()))
    return dict(X=PX.astype(np.float64) * UNFIX, Y=PY.astype(np.float64) * UNFIX, touched=G.touched, vertices=n, entries=G.ne, zeros=G.zeros, batches=batches, samples=samples,
                total_weight=G.W, neg_total=G.N, max_abs=float(big) * UNFIX, G=G)


def three_blocks(seed=7, blocks=3, size=12):
    """the learning test's graph by a fixed generator: `blocks` blocks of `size` vertices, every ordered pair inside a block at weight 20 .. 40, 15 % of the
    ordered pairs across blocks at weight 1.  -> src int32, dst int32, w float64, n"""
    rng = np.random.default_rng(seed)
    n = blocks * size
    src, dst, w = [], [], []
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            if i // size == j // size:
                src.append(i); dst.append(j); w.append(float(rng.integers(20, 41)))
            elif rng.random() < 0.15:
                src.append(i); dst.append(j); w.append(1.0)
    return np.array(src, np.int32), np.array(dst, np.int32), np.array(w, np.float64), n


def random_graph(n, entries, seed, wmax=50, hub=None):
    """about `entries` distinct directed edges with integer weights 1 .. wmax, shuffled; hub: every other vertex also points at it"""
    rng = np.random.default_rng(seed)
    cells = set(rng.integers(0, n * n, entries).tolist())
    if hub is not None:
        cells |= {i * n + hub for i in range(n)}
    cells = np.array(sorted(cells), np.int64)
    rng.shuffle(cells)
    return (cells // n).astype(np.int32), (cells % n).astype(np.int32), rng.integers(1, wmax + 1, len(cells)).astype(np.float64)
