"""A second reading of the three held-out evaluation entries (include/dge.h, "Held-out evaluation": dge_model_score_pairs, dge_model_eval_links,
dge_model_eval_sgns), in plain numpy and Python, written from the header's text and independent of the device.

The lattice.  Planted tables hold small integers times 2^-s (s = `shift`), a few of them in a row: one live column in every 64-float chunk plus the
first and the last column, entries -1 / 0 / +1.  A score is then (an integer of a few units) * 4^-s — quarter steps at s = 1, mostly within -6 .. 6 —
so wins, ties and losses are all plentiful.  The condition for exactness:

    max |entry|^2 * 512 < 2^24                                   (entries as integers; a row has at most 512 floats)

every product is an integer below 2^24 / 512 and every partial sum of at most 512 of them, in ANY association order, fused or not, is an integer
below 2^24: an exact float32.  `check_exact` asserts it on the generated tables, and the sharper per-pair form sum_i |x_i| |y_i| < 2^24 (which is what
the argument needs, and what the column-witness tables — a ramp row 1 .. dim against one-hot rows — meet although the ramp's square does not fit).
Padding columns [dim, stride) are planted as zero: the layout's invariant, which the kernels may assume.

Scores come from int64 matrix products; wins, ties and negatives are Python ints; auc = (wins + 0.5 * ties) / negatives as the header's struct states
it.  The loss: the scores take a few dozen distinct values, so the sum over the terms is formed as sum over the distinct values v of count(v) * softplus(v),
softplus evaluated by np.logaddexp in np.longdouble (eps 1.1e-19), the product with the integer count one more longdouble rounding, and the products —
split into a double head and tail — added by math.fsum: the reference's own error is below 2^-60 relative."""
import math
from collections import namedtuple

import numpy as np

U64 = np.uint64
LD = np.longdouble


def mix64(x):
    """splitmix64 (the header's dge_mix64) on a uint64 array; array arithmetic wraps."""
    x = np.atleast_1d(np.asarray(x, dtype=U64)) + U64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
    return x ^ (x >> U64(31))


def host_map(vid, NV):
    """vertex id -> vocabulary row, -1 outside the vocabulary."""
    remap = -np.ones(NV, np.int64); remap[np.asarray(vid, np.int64)] = np.arange(len(vid))
    return remap


def look(remap, v):
    v = np.asarray(v, np.int64)
    return np.where((v >= 0) & (v < len(remap)), remap[np.clip(v, 0, len(remap) - 1)], -1)


def u64(x):
    return U64(int(x) & 0xFFFFFFFFFFFFFFFF)


# ------------------------------------------------------------------------------------------------ the two draw rules
def links(walks, row0, R, seed, remap):
    """dge_model_eval_links -> (rows of a, rows of b, rows of r) of the scored steps, skipped."""
    n, L = walks.shape
    if L < 2:
        z = np.zeros(0, np.int64)
        return z, z, z, 0
    g = (u64(row0) + np.arange(n, dtype=U64))[:, None]; j = np.arange(L - 1, dtype=U64)[None, :]
    a = walks[:, :-1].astype(np.int64); b = walks[:, 1:].astype(np.int64)
    h = mix64(u64(seed) + g * U64(L) + j).reshape(n, L - 1)
    r = (np.maximum(b, 0) // R) * R + (h % U64(R)).astype(np.int64)
    cand = (a >= 0) & (b >= 0)
    ra, rb, rr = look(remap, a[cand]), look(remap, b[cand]), look(remap, r[cand])
    ok = (ra >= 0) & (rb >= 0) & (rr >= 0)
    return ra[ok], rb[ok], rr[ok], int((~ok).sum())


Pairs = namedtuple("Pairs", "gi i c ctr ctx lens")      # walk index in the call, packed positions, rows of centre and context; packed lengths [n]
Sgns = namedtuple("Sgns", "ctr ctx neg valid")          # rows [P], rows [P], drawn rows [P x K], which of them are scored [P x K]


def sgns_pairs(walks, W, remap):
    """The pairs of dge_model_eval_sgns, by band: the in-vocabulary tokens left-packed, then offsets d = 1 .. min(W, n - 1), each giving (i, i + d) and
    (i + d, i).  Sorted by (walk, centre, context)."""
    n, L = walks.shape
    rows = look(remap, walks)
    keep = rows >= 0
    order = np.argsort(~keep, axis=1, kind="stable")
    packed = np.take_along_axis(rows, order, 1); lens = keep.sum(1)
    G, I, C = [], [], []
    for d in range(1, min(int(W), int(lens.max(initial=0)) - 1) + 1):
        gi, lo = np.nonzero(np.arange(L - d)[None, :] + d < lens[:, None])
        G += [gi, gi]; I += [lo, lo + d]; C += [lo + d, lo]
    if not G:
        z = np.zeros(0, np.int64)
        return Pairs(z, z, z, z, z, lens)
    gi, i, c = np.concatenate(G), np.concatenate(I), np.concatenate(C)
    o = np.lexsort((c, i, gi))
    gi, i, c = gi[o], i[o], c[o]
    return Pairs(gi, i, c, packed[gi, i], packed[gi, c], lens)


def sgns_draws(p, row0, max_len, K, seed, table):
    """The K negatives of every pair: slot = mix64(seed + ((g * max_len + i) * max_len + c) * K + k) % table_size, g = row0 + walk index.
    `max_len` is the corpus's row length (a scalar; an array per pair only in the tests' mutants)."""
    ml = np.broadcast_to(np.asarray(max_len, dtype=U64), p.gi.shape)
    g = u64(row0) + p.gi.astype(U64)
    base = ((g * ml + p.i.astype(U64)) * ml + p.c.astype(U64)) * U64(K)
    slots = mix64(u64(seed) + base[:, None] + np.arange(K, dtype=U64)[None, :]).reshape(len(base), K) % U64(len(table))
    neg = np.asarray(table)[slots.astype(np.int64)].astype(np.int64)
    return Sgns(p.ctr, p.ctx, neg, neg != p.ctr[:, None])


def sgns(walks, row0, W, K, seed, remap, table):
    """dge_model_eval_sgns -> Sgns; skipped = (~valid).sum()."""
    return sgns_draws(sgns_pairs(walks, W, remap), row0, walks.shape[1], K, seed, table)


# ------------------------------------------------------------------------------------------------ the figures
def _softplus_sum(ints, shift):
    """sum of softplus(v * 4^-shift) over the integer scores `ints` -> the correctly rounded double of the longdouble terms' sum."""
    if len(ints) == 0:
        return 0.0
    v, cnt = np.unique(np.asarray(ints, np.int64), return_counts=True)
    t = np.logaddexp(LD(0), v.astype(LD) * LD(4.0) ** -shift) * cnt.astype(LD)
    hi = t.astype(np.float64); lo = (t - hi.astype(LD)).astype(np.float64)
    return math.fsum(list(hi) + list(lo))


def figures(S0, S1, shift, form, pos_ctx, pos_tgt, neg_ctx, neg_tgt, owner):
    """S0 / S1: integer tables [V x dim] (the planted values are these times 2^-shift).  Positives score(ctx row, tgt row) [P]; scored negatives [N], each
    compared with positive owner[N].  form "links": loss = mean softplus(-pos) + mean softplus(neg); "sgns": (both sums) / pairs."""
    assert S0.dtype == np.int64 and S1.dtype == np.int64
    G = S0 @ S1.T                                   # every score of the model, as an integer: score = G * 4^-shift
    pos = G[pos_ctx, pos_tgt]; neg = G[neg_ctx, neg_tgt]
    pairs, negatives = int(len(pos)), int(len(neg))
    wins = int((pos[owner] > neg).sum()); ties = int((pos[owner] == neg).sum())
    s_pos, s_neg = _softplus_sum(-pos, shift), _softplus_sum(neg, shift)
    out = dict(pairs=pairs, negatives=negatives, wins=wins, ties=ties, w2=2 * wins + ties, s_pos=s_pos, s_neg=s_neg, terms=pairs + negatives,
               auc=float("nan"), loss=float("nan"), lo=int(min(pos.min(initial=0), neg.min(initial=0))), hi=int(max(pos.max(initial=0), neg.max(initial=0))))
    if negatives:
        out["auc"] = (float(wins) + 0.5 * float(ties)) / float(negatives)
    if pairs:
        out["loss"] = float(LD(s_pos) / LD(pairs) + LD(s_neg) / LD(negatives)) if form == "links" else float((LD(s_pos) + LD(s_neg)) / LD(pairs))
    return out


def loss_tolerance(terms):
    """Relative bound on |device loss - reference loss| over `terms` softplus terms of EXACT scores (no gamma_D term), in units of 1:

      * a term is log1p(exp(-|x|)) (+ |x|): the device's binary64 exp and log1p.  The HIP documentation installed with the toolchain states no ulp
        bound for either (its math headers declare the functions and say nothing of their error), so 4 ulp a term is an ALLOWANCE, not a documented
        bound — log1p(e) moves by at most the relative error of e, so it covers exp and log1p at 2 ulp each;
      * one rounding (1/2 ulp) for the addition inside softplus;
      * terms * 2^-52 for adding `terms` positive doubles in any order;
      * 2 ulp for what is left: the quotients and the sum behind the two totals (three roundings), and the reference's own rounding to a double.

    An ulp is at most 2^-52 relative, and all terms are positive, so the per-term bounds carry over to the sum."""
    return (4.0 + 0.5 + float(terms) + 2.0) * 2.0 ** -52


# ------------------------------------------------------------------------------------------------ the world of the planted tests
NV, MIN_COUNT, TABLE_SIZE, SHIFT = 640, 2, 20011, 1


def world_counts():
    """Counts of the NV vertex ids: a Zipf head over a shuffled ranking (so that drawn negatives equal the centre at a useful rate), 36 ids below min_count."""
    rng = np.random.default_rng(7)
    c = 30000 // (rng.permutation(NV) + 1) + 2
    c[rng.choice(NV, 36, replace=False)] = 1
    return c.astype(np.int64)


def vocabulary(counts, min_count=MIN_COUNT):
    """dge_model_create's order: descending count, ids ascending inside a tie, count >= min_count -> (vertex ids of the rows, their counts)."""
    ids = np.argsort(-counts, kind="stable")
    ids = ids[counts[ids] >= min_count]
    return ids.astype(np.int32), counts[ids]


def unigram_table(sorted_counts, T=TABLE_SIZE):
    """word2vec.c, InitUnigramTable, as its serial loop: slot a takes the current row, and the row advances (once a slot at most) when a / T has passed the
    cumulative count^0.75 share d1.  (The CPU tests' table; a device test reads the model's own with dge_model_table, which is the one the header names.)"""
    p = np.asarray(sorted_counts, np.float64) ** 0.75
    tot = float(p.sum()); V = len(p)
    table = np.empty(T, np.int32)
    i, d1 = 0, p[0] / tot
    for a in range(T):
        table[a] = i
        if a / float(T) > d1:
            i += 1
            d1 += p[min(i, V - 1)] / tot
        if i >= V:
            i = V - 1
    return table


def live_columns(dim):
    """One column in every 64-float chunk of the row, and the first and the last column."""
    rng = np.random.default_rng(dim)
    return np.unique([0, dim - 1] + [c0 + int(rng.integers(min(64, dim - c0))) for c0 in range(0, dim, 64)])


def lattice(V, dim, seed=0):
    """Integer tables S0, S1 [V x dim] of the lattice (module docstring)."""
    rng = np.random.default_rng([int(seed), V, dim])
    cols = live_columns(dim)
    S0 = np.zeros((V, dim), np.int64); S1 = np.zeros((V, dim), np.int64)
    S0[:, cols] = rng.choice([-1, 0, 0, 1], (V, len(cols))); S1[:, cols] = rng.choice([-1, 0, 0, 1], (V, len(cols)))
    return S0, S1


def witness(V, dim, seed=0):
    """The column witness: syn0 row j = e_j for j < dim, syn1neg row 0 = the ramp 1 .. dim; every other row from the lattice.  score(e_j, ramp) = j + 1."""
    assert V > dim
    S0, S1 = lattice(V, dim, seed)
    S0[:dim] = np.eye(dim, dtype=np.int64); S1[0] = np.arange(1, dim + 1)
    return S0, S1


def check_exact(S0, S1, lattice_only=True):
    if lattice_only:
        assert max(np.abs(S0).max(), np.abs(S1).max()) ** 2 * 512 < 2 ** 24
    assert S0.shape[1] <= 512 and int((np.abs(S0) @ np.abs(S1).T).max()) < 2 ** 24


def make_walks(n, L, seed, counts):
    """n walks of L tokens: ids drawn by count (the Zipf head recurs), 8 % holes (-1), 3 % ids below min_count, 3 % ids >= n_vertices; a third of the
    walks end early (a padded tail), every ninth is mostly holes, and every walk of three tokens or more has a hole in its first half."""
    rng = np.random.default_rng([int(seed), n, L])
    p = counts / counts.sum()
    w = rng.choice(NV, (n, L), p=p).astype(np.int64)
    u = rng.random((n, L))
    below = np.flatnonzero(counts < MIN_COUNT)
    w[u < 0.14] = rng.choice(below, (n, L))[u < 0.14]
    w[u < 0.11] = rng.integers(NV, NV + 6, (n, L))[u < 0.11]
    w[u < 0.08] = -1
    for g in range(n):
        if L >= 3:
            w[g, rng.integers(0, L // 2)] = -1          # no walk is whole: the packed length differs from max_len
        if g % 3 == 1:
            w[g, rng.integers(L // 2, L + 1):] = -1
        if g % 9 == 4:
            w[g, rng.random(L) < 0.7] = -1
    return w.astype(np.int32)


class Case:
    """A named builder: the corpus, the call and — given the vocabulary's ids and the unigram table — the expected figures of one device call."""

    def __init__(self, name, entry, dim=64, L=24, W=5, K=5, n=40, row0=3, seed=3, R=40, wseed=0, tags=()):
        self.name, self.entry, self.dim, self.L, self.W, self.K, self.n, self.row0, self.seed, self.R, self.wseed, self.tags = name, entry, dim, L, W, K, n, row0, seed, R, wseed, set(tags)

    def __repr__(self):
        return self.name

    def walks(self):
        """The evaluated rows [n x L] (corpus rows row0 .. row0 + n - 1)."""
        return make_walks(self.n, self.L, 1000 + self.wseed, world_counts())

    def corpus(self):
        """The whole corpus: row0 rows of holes in front of the evaluated ones (they must not be read, and the draw index must count them)."""
        return np.concatenate([np.full((self.row0, self.L), -1, np.int32), self.walks()])

    def tables(self, V):
        return lattice(V, self.dim, seed=1)

    def reference(self, vid, table, first=0, count=None, detail=False):
        """Expected figures of the call on rows [row0 + first, row0 + first + count)."""
        count = self.n - first if count is None else count
        w = self.walks()[first:first + count]
        remap = host_map(vid, NV)
        S0, S1 = self.tables(len(vid))
        if self.entry == "links":
            ra, rb, rr, skipped = links(w, self.row0 + first, self.R, self.seed, remap)
            f = figures(S0, S1, SHIFT, "links", rb, ra, rr, ra, np.arange(len(ra)))
            d = (ra, rb, rr)
        else:
            d = sgns(w, self.row0 + first, self.W, self.K, self.seed, remap, table)
            f = sgns_figures(S0, S1, d)
            skipped = int((~d.valid).sum())
        f["skipped"] = skipped
        return (f, d) if detail else f


def sgns_figures(S0, S1, d, shift=SHIFT):
    own, k = np.nonzero(d.valid)
    return figures(S0, S1, shift, "sgns", d.ctx, d.ctr, d.ctx[own], d.neg[own, k], own)


def _cases():
    out = []
    for K in (0, 1, 5, 15, 16, 17, 31, 32, 33):
        out.append(Case("sgns-K%d" % K, "sgns", K=K, tags=["K"]))
    for dim in (20, 320, 512):
        out.append(Case("sgns-dim%d" % dim, "sgns", dim=dim, K=17, tags=["dim"]))
    for L in (1, 2, 16, 17, 33, 768, 769, 1537, 3073, 6145, 12288):
        out.append(Case("sgns-L%d" % L, "sgns", L=L, W=1, n=40 if L <= 33 else 24, tags=["L"] + (["empty"] if L == 1 else [])))
    out.append(Case("sgns-L3073-one-row", "sgns", L=3073, W=1, n=1, wseed=1, tags=["L"]))
    out.append(Case("sgns-L6145-one-row", "sgns", L=6145, W=1, n=1, wseed=1, tags=["L"]))
    out.append(Case("sgns-L17-W17", "sgns", L=17, W=17, tags=["W", "wide"]))
    out.append(Case("sgns-L17-W24", "sgns", L=17, W=24, tags=["W", "wide"]))
    for n in (1, 3, 15, 17):
        out.append(Case("sgns-rows%d" % n, "sgns", n=n, wseed=2, tags=["rows"]))
    out.append(Case("sgns-far-row0", "sgns", row0=100_000 - 40, tags=["edge"]))
    out.append(Case("sgns-seed-wraps", "sgns", seed=2 ** 64 - 3, tags=["edge"]))
    for dim in (64, 320, 512):
        out.append(Case("links-dim%d" % dim, "links", dim=dim, n=200, tags=["links"]))
    out.append(Case("links-L1", "links", L=1, n=40, tags=["links", "empty"]))
    out.append(Case("links-L2", "links", L=2, n=400, tags=["links"]))
    out.append(Case("links-R1", "links", R=1, n=200, tags=["links", "all-ties"]))
    out.append(Case("links-R48", "links", R=48, n=200, tags=["links"]))
    out.append(Case("links-R1000", "links", R=1000, n=200, tags=["links"]))
    return {c.name: c for c in out}


CASES = _cases()
