"""Inputs and float64 readings for the cosine-KNN and nDCG tests (tests/test_gpu_knn_exact.py on the device, tests/test_knn_ref.py on the CPU).
Pure numpy; the distance matrix is oracle.quality's.  Not a test module.

LATTICE INPUTS.  Row r has exactly c_r non-zero entries, c_r in {1, 4, 16, 64, 256} and c_r <= D, each +-2^e_r with one exponent per row.  Its norm
2^e_r sqrt(c_r) is a power of two, so the inverse norm is exact, every normalised entry is +-2^-m (m <= 4), every partial sum of every dot product
is an integer multiple of 2^-8 of magnitude <= 1, and the float32 result is exact in ANY accumulation order; so is 1.0f - s, and the float64 reading
gives the same number.  On such rows the device lists must equal the reference lists: no tolerance, no excused row.  Rows come in families (a sign
pattern on a fixed support with some signs flipped: cosine (c - 2 flips) / c), which makes few distinct distances and ties at nearly every list's
k-th place — the (distance, index) order is what these inputs test.

FLOAT INPUTS.  For unit rows x, y of dimension D the float32 dot product, summed in any order (an MFMA's included; padding zeros add nothing), errs
by at most gamma_D sum|x_i y_i| <= about D 2^-24, as sum|x_i y_i| <= |x||y| = 1.  The rows are unit only up to the roundings of the normalisation, at most two per
factor (an inverse norm held in float32, the product; the kernel forms both in binary64 and rounds once): at most 4 2^-24 on the dot product.  The subtraction 1 - s rounds once more and the
reference is cast to float32 for nothing: 2 2^-24 covers both.  tol(D) = (D + 10) 2^-24 bounds the sum with room for the second-order terms.
"""
import math

import numpy as np

from oracle import quality as qo

COUNTS = (1, 4, 16, 64, 256)


def tol(D):
    """The derived bound on |device distance - float64 distance| for finite float32 rows of dimension D (module docstring)."""
    return (D + 10) * 2.0 ** -24


def lattice(n, D, seed, exps=(-3, -2, -1, 0, 1, 2, 3), width=None):
    """n lattice rows of dimension D (float32); only the first `width` columns (default: all) are used."""
    rng = np.random.default_rng(seed)
    W = D if width is None else width
    counts = [c for c in COUNTS if c <= W]
    bases = {}
    for c in counts:                                   # two families per count: a support and a sign pattern
        bases[c] = []
        for start in (0, W - min(W, 2 * c)):           # supports drawn from a window at either end, so families of different counts overlap
            w = min(W, 2 * c)
            bases[c].append((start + rng.choice(w, c, replace=False), rng.choice([-1.0, 1.0], c)))
    f = np.zeros((n, D), np.float32)
    for r in range(n):
        c = counts[rng.integers(len(counts))]
        if rng.random() < 0.75:
            cols, signs = bases[c][rng.integers(2)]
            signs = signs.copy()
            flips = rng.choice(c, rng.integers(0, c // 2 + 1), replace=False)
            signs[flips] = -signs[flips]
        else:
            cols, signs = rng.choice(W, c, replace=False), rng.choice([-1.0, 1.0], c)
        f[r, cols] = (signs * 2.0 ** float(exps[rng.integers(len(exps))])).astype(np.float32)
    return f


def zeroed(f):
    """The rule of include/dge.h: a row with a non-finite entry counts as a zero vector."""
    g = np.array(f, np.float32)
    g[~np.isfinite(g).all(axis=1)] = 0.0
    return g


def distances(f):
    """float64 cosine distances [n x n] of the reference's rule (a zero or non-finite row at distance 2 from everything)."""
    return qo.cosine_distance_matrix(zeroed(f))


def lists_from(d, k):
    """The lists a distance matrix implies: per row the k other rows in a stable sort by (distance, index); slots past n-1 hold -1 / 3.0."""
    n = len(d)
    kk = min(k, n - 1)
    key = d.copy()
    np.fill_diagonal(key, np.inf)
    order = np.argsort(key, axis=1, kind="stable")[:, :kk]
    idx = np.full((n, k), -1, np.int32); dist = np.full((n, k), 3.0, np.float32)
    idx[:, :kk] = order
    dist[:, :kk] = np.take_along_axis(d, order, 1).astype(np.float32)
    return idx, dist


def reference_lists(f, k):
    return lists_from(distances(f), k)


def model_f32(f, reverse=False):
    """A float32 model of the device arithmetic: the inverse norm in binary64, x * inv rounded once to float32, the products accumulated in float32
    one column at a time (forward or backward), 1.0f - s; a zero or non-finite row at distance 2.  -> float32 [n x n]."""
    x = zeroed(f).astype(np.float64)
    s = (x * x).sum(axis=1)
    live = s > 0
    inv = np.zeros(len(x)); inv[live] = 1.0 / np.sqrt(s[live])
    xn = (x * inv[:, None]).astype(np.float32)
    acc = np.zeros((len(x), len(x)), np.float32)
    cols = range(xn.shape[1] - 1, -1, -1) if reverse else range(xn.shape[1])
    for j in cols:
        acc += np.outer(xn[:, j], xn[:, j])            # float32 product, float32 sum
    d = np.float32(1.0) - acc
    d[~live, :] = 2.0; d[:, ~live] = 2.0
    return d


# ---- the lattice cases: name -> (features, k's).  Every one is read by the CPU test of the test as well.
SHAPES = [(1, 4), (2, 1), (63, 16), (64, 32), (65, 33), (128, 64), (129, 65), (257, 128), (193, 129), (200, 255), (321, 256)]
KS = (1, 10, 64)


def shape_case(n, D):
    return lattice(n, D, seed=1000 * n + D)


GROUP = np.arange(5, 5 + 9 * 70, 9)                    # 70 identical rows, stride 9: every 64-column tile and 64-row workgroup up to 626 holds some
ZERO_ROWS = (0, 63, 64, 300, 699)


def planted_case():
    f = lattice(700, 64, seed=7)
    rng = np.random.default_rng(70)
    f[GROUP] = 0.0
    f[GROUP[:, None], rng.choice(64, 16, replace=False)] = rng.choice([-0.5, 0.5], 16).astype(np.float32)   # a direction of its own: no other row is parallel to it
    f[list(ZERO_ROWS)] = 0.0
    return f


SPARSE_LIVE = np.r_[np.arange(1, 700, 31), np.arange(64, 80)]          # 39 rows, fewer than k = 64


def sparse_case():
    """Fewer than k non-zero rows: every list runs out of finite neighbours and goes on through the distance-2 block in index order."""
    f = np.zeros((700, 64), np.float32)
    f[SPARSE_LIVE] = lattice(len(SPARSE_LIVE), 64, seed=8)
    return f


def order_case():
    """(2049, 64): row 0 is a probe with every entry set, two thirds of the rows are the probe with 0..32 signs flipped (cosine (64 - 2 flips) / 64)."""
    rng = np.random.default_rng(9)
    f = lattice(2049, 64, seed=9)
    probe = rng.choice([-1.0, 1.0], 64)
    for r in range(2049):
        if r == 0 or rng.random() < 0.66:
            s = probe.copy()
            if r:
                flips = rng.choice(64, rng.integers(0, 33), replace=False)
                s[flips] = -s[flips]
            f[r] = (s * 2.0 ** float(rng.integers(-3, 4))).astype(np.float32)
    return f


def order_permutations(f):
    """The three row orders: by descending reference distance to the probe (every later column displaces the tail of the lists near the probe), the
    reverse, shuffled.  perm[i] = the original row that becomes row i."""
    d0 = distances(f)[0]
    down = np.argsort(-d0, kind="stable")
    return {"descending": down, "ascending": down[::-1].copy(), "shuffled": np.random.default_rng(10).permutation(len(f))}


def huge_case():
    return lattice(150, 33, seed=11, exps=(-60, 60))


def subnormal_case():
    """Rows whose every entry is a subnormal float32 (2^-140: norm below 2^-128) beside ordinary rows."""
    return lattice(150, 33, seed=12, exps=(-140, -140, -3, 0, 3))


def nonfinite_case():
    f = lattice(150, 20, seed=13)
    f[3, 4] = np.nan
    f[70] = 0.0; f[70, 0] = np.inf
    f[130, 7] = -np.inf                                # the rest of row 130 stays finite
    f[131] = 1.0; f[131, 19] = np.nan
    return f


def absent_case():
    f = lattice(333, 20, seed=14)
    present = np.ones(333, bool); present[[0, 17, 63, 64, 200, 332]] = False
    return f, present


def lattice_cases():
    """Every lattice matrix the device tests use, by name (the planted and ordered ones included)."""
    out = {"shape-%dx%d" % s: shape_case(*s) for s in SHAPES}
    out.update(planted=planted_case(), sparse=sparse_case(), huge=huge_case(), subnormal=subnormal_case(), nonfinite=nonfinite_case(),
               absent=absent_case()[0])
    f = order_case()
    for name, perm in order_permutations(f).items():
        out["order-" + name] = f[perm]
    return out


# ---- the float cases
FLOAT_DIMS = (20, 64, 100, 256)
FLOAT_KINDS = ("cluster", "positive", "near-duplicates")


def float_case(kind, D, n=300):
    rng = np.random.default_rng(D * 10 + FLOAT_KINDS.index(kind))
    if kind == "cluster":                              # every distance near 0: 1 - s cancels
        return (rng.normal(size=D) + 1e-3 * rng.normal(size=(n, D))).astype(np.float32)
    if kind == "positive":                             # no cancellation inside a dot product: sum|x_i y_i| is the dot product itself
        return rng.uniform(0.0, 1.0, size=(n, D)).astype(np.float32)
    f = rng.normal(size=(n, D))                        # n even: row 2i+1 = row 2i perturbed at relative 2^-20
    f[1::2] = f[0::2] * (1.0 + 2.0 ** -20 * rng.uniform(-1, 1, size=(n // 2, D)))
    return f.astype(np.float32)


def check_float_lists(f, k, idx, dist):
    """The assertions of the float legs, excusing nothing.  -> the largest |dist - reference| / tol(D)."""
    n, D = f.shape
    t = tol(D)
    d = distances(f)
    ridx, rdist = lists_from(d, k)
    kk = min(k, n - 1)
    idx, dist = idx[:, :kk], dist[:, :kk].astype(np.float64)
    assert (idx >= 0).all() and (idx < n).all()
    assert not (idx == np.arange(n)[:, None]).any(), "a row in its own list"
    assert all(len(set(row)) == kk for row in idx.tolist()), "an index twice in one list"
    assert (np.diff(dist, axis=1) >= 0).all(), "distances decrease along a list"
    own = np.take_along_axis(d, idx.astype(np.int64), 1)          # float64 distance of the very pair the device reports
    want = np.take_along_axis(d, ridx[:, :kk].astype(np.int64), 1)  # float64 distance of the reference's neighbour in that slot
    err = max(np.abs(dist - own).max(), np.abs(dist - want).max())
    print("knn float leg n=%d D=%d k=%d: max |dist - ref| = %.3g = %.4f tol(D)" % (n, D, k, err, err / t))
    assert err <= t, (err, t)
    kth = want[:, -1:]
    assert (own <= kth + 2 * t).all(), "a returned neighbour lies beyond the reference's k-th distance + 2 tol"
    key = d.copy(); np.fill_diagonal(key, np.inf)
    must = key < kth - 2 * t                                      # clearly inside the list
    got = np.zeros_like(must); np.put_along_axis(got, idx.astype(np.int64), True, 1)
    assert not (must & ~got).any(), "a neighbour closer than the reference's k-th distance - 2 tol is missing"
    return err / t


# ---- nDCG
def ndcg_reference(f, g, k):
    """nDCG@k of the lists of f under the ground features g, read per row in float64, and the bound on |device - this reading| for lattice f and g.

    RULE (include/dge.h): a region whose ideal DCG is exactly 0 contributes ratio 0 (oracle.quality would divide by zero there).

    BOUND.  On lattice inputs the lists, the ground distances and the kernel's own dot products are exact, so device and reading hold the same
    relevances relv_i and differ only in rounding.  u = 2^-53.  A term relv_i / log2(i + 1) carries log2's error (<= 1 ulp, relative 2u) and the
    division's (u); the k-term sum adds (k - 1) u relative to A = sum_i |relv_i| / log2(i + 1).  So each side's DCG errs by <= (k + 2) u A, the
    two sides together by (k + 2) 2^-52 A — for the numerator (A_num) and for the ideal DCG dmax (A_den) alike.  The ratio dcg / dmax then differs
    by <= (k + 2) 2^-52 (A_num + |ratio| A_den) / |dmax| plus one division rounding per side, 2^-52 |ratio| <= 2^-52 |ratio| A_den / |dmax|:
    c = k + 3, and k + 4 with room for the second-order terms.  Per row: (k + 4) 2^-52 (A_num + |ratio| A_den) / |dmax|.  The device's mean is a
    sequential float64 sum of n ratios and a division, (n - 1) u + u relative to sum|ratio|; this reading sums with math.fsum (exact): n 2^-53
    mean|ratio|.  A dmax that cancels to almost nothing would make the bound large: the committed cases are chosen so that it stays below 1e-9
    (tests/test_knn_ref.py holds them to it).
    -> (nDCG, bound, number of regions with ideal DCG 0)"""
    n = len(f)
    est = reference_lists(f, k)[0].astype(np.int64)
    gd = distances(g)
    gdist = lists_from(gd, k)[1].astype(np.float64)
    w = 1.0 / np.log2(np.arange(2, k + 2, dtype=np.float64))
    ratios, bounds, flat = [], [], 0
    for r in range(n):
        num = 1.0 - gd[r, est[r]]
        den = 1.0 - gdist[r]
        dcg, dmax = float(np.sum(num * w)), float(np.sum(den * w))
        a_num, a_den = float(np.sum(np.abs(num) * w)), float(np.sum(np.abs(den) * w))
        if a_den == 0.0:                               # every relevance of the ideal list is 0: the ideal DCG is 0 on any machine
            ratios.append(0.0); bounds.append(0.0); flat += 1
            continue
        if dmax == 0.0:                                # cancelled to 0 here, perhaps not on the device: no bound
            ratios.append(0.0); bounds.append(math.inf)
            continue
        ratio = dcg / dmax
        ratios.append(ratio)
        bounds.append((k + 4) * 2.0 ** -52 * (a_num + abs(ratio) * a_den) / abs(dmax))
    mean_abs = math.fsum(abs(x) for x in ratios) / n
    return math.fsum(ratios) / n, math.fsum(bounds) / n + n * 2.0 ** -53 * mean_abs, flat


NDCG_DIMS = [(20, 7), (64, 64), (33, 100), (128, 256), (256, 129)]
NDCG_N = 300


def ndcg_case(dim, gnd_dim):
    """(features, ground features), both lattice.  (33, 100): three ground rows alone on a column of their own, every other row orthogonal to them
    (ideal DCG exactly 0).  (64, 64): zero and non-finite ground rows, and a zero and a NaN feature row."""
    f = lattice(NDCG_N, dim, seed=100 * dim + gnd_dim)
    if (dim, gnd_dim) == (33, 100):
        g = lattice(NDCG_N, gnd_dim, seed=100 * gnd_dim + dim + 1, width=gnd_dim - 3)
        for i, r in enumerate((2, 150, 299)):
            g[r] = 0.0; g[r, gnd_dim - 3 + i] = 2.0 ** (i - 1)
        return f, g
    g = lattice(NDCG_N, gnd_dim, seed=100 * gnd_dim + dim + 1)
    if (dim, gnd_dim) == (64, 64):
        g[[5, 64, 191]] = 0.0
        g[77, 3] = np.nan
        g[200] = 0.0; g[200, 63] = -np.inf
        f[9] = 0.0
        f[120, 0] = np.nan
    return f, g
