"""A second reading of the graph half — edge store, alias tables, walk sampler — in numpy and Python integers.

Nothing here calls the oracle or a library of the project.  It is written from the rules stated in include/dge.h (edge store: "per-vertex edge order =
insertion order; outDegree = running sum"; the walk sampler's two stream layouts; "a dead end yields a shorter walk") and from the published
specification of java.util.Random:

    seed scramble   s = (seed ^ 0x5DEECE66D) mod 2^48
    next(bits)      s = (s * 0x5DEECE66D + 0xB) mod 2^48;  return the top `bits` bits of s
    nextDouble()    ((next(26) << 27) + next(27)) * 2^-53

What it is for (tests/test_walk_ref.py shows it is sound on its own, tests/test_gpu_graph_exact.py holds the device to it):

  * mass()           what a pair of (prob, alias) arrays ENCODES: the probability mass, in slot units, that lands on every slot.  On lattice weights
                     (lattice_weights) every operation of either alias builder is exact, so the mass has to equal w / 2^m as a float64 equality —
                     whatever the pairing order was.
  * replay_*()       walks from the tables a graph handed back (get_csr + get_source_alias) and the draw -> slot -> neighbour rule, for both stream
                     layouts.  A table that is consistent and a draw that is shifted, or the other way round, shows here.
"""
import math

import numpy as np

JR_MULT = 0x5DEECE66D
JR_ADD = 0xB
JR_MASK = (1 << 48) - 1


def _affine_pow(n):
    """(M, P) with  step^n(s) = (M * s + P) mod 2^48  for the LCG step, by squaring: O(log n)."""
    n = int(n)
    assert n >= 0
    am, ap, cm, cp = 1, 0, JR_MULT, JR_ADD
    while n:
        if n & 1:
            am, ap = (am * cm) & JR_MASK, (ap * cm + cp) & JR_MASK
        cp = ((cm + 1) * cp) & JR_MASK
        cm = (cm * cm) & JR_MASK
        n >>= 1
    return am, ap


class JavaRandom:
    """java.util.Random, from its specification."""

    def __init__(self, seed):
        self.s = (int(seed) ^ JR_MULT) & JR_MASK

    def next(self, bits):
        self.s = (self.s * JR_MULT + JR_ADD) & JR_MASK
        return self.s >> (48 - bits)

    def next_int(self):
        v = self.next(32)
        return v - (1 << 32) if v >= 1 << 31 else v          # (int) of the 32 bits: two's complement

    def next_double(self):
        hi = self.next(26)
        return float((hi << 27) + self.next(27)) * 2.0 ** -53

    def jump(self, n_steps):
        """Advance by n_steps calls of next() (a nextDouble is two)."""
        m, p = _affine_pow(n_steps)
        self.s = (m * self.s + p) & JR_MASK
        return self

    @classmethod
    def before_draw(cls, seed, o):
        """The generator as it stands before its o-th nextDouble (o = 0: fresh)."""
        return cls(seed).jump(2 * int(o))


def _next_double_vec(s):
    """One nextDouble of every stream of the uint64 array `s` (48-bit states), in place -> float64 array."""
    mult, add, mask = np.uint64(JR_MULT), np.uint64(JR_ADD), np.uint64(JR_MASK)
    s *= mult; s += add; s &= mask                      # uint64 wraps mod 2^64; the mask keeps the low 48 bits, which is all the rule reads
    hi = s >> np.uint64(22)
    s *= mult; s += add; s &= mask
    lo = s >> np.uint64(21)
    return ((hi << np.uint64(27)) + lo).astype(np.float64) * 2.0 ** -53        # below 2^53: the conversion is exact


def stream_doubles(seed, first_draw, count):
    """Draws first_draw .. first_draw + count - 1 of java.util.Random(seed) as float64[count]: `lanes` streams a fixed jump apart, stepped side by side."""
    count = int(count)
    if count == 0:
        return np.zeros(0, np.float64)
    lanes = min(count, 1024)
    per = -(-count // lanes)
    m, p = _affine_pow(2 * per)
    st = [JavaRandom.before_draw(seed, first_draw).s]
    for _ in range(lanes - 1):
        st.append((m * st[-1] + p) & JR_MASK)
    s = np.array(st, np.uint64)
    out = np.empty((lanes, per), np.float64)
    for j in range(per):
        out[:, j] = _next_double_vec(s)
    return out.reshape(-1)[:count]


# ------------------------------------------------------------------------------------------- edge store
def csr_of(src, dst, w, V):
    """The store of include/dge.h: edges in stable order by source — inside a vertex the insertion order, duplicates kept — and out_degree as the running
    sum of a vertex's weights in that order -> dict(row_ptr int64[V+1], nbr int32[E], weight float64[E], out_degree float64[V])."""
    src = np.asarray(src, np.int64); dst = np.asarray(dst, np.int32); w = np.asarray(w, np.float64)
    assert len(src) == len(dst) == len(w) and (len(src) == 0 or (src.min() >= 0 and max(src.max(), dst.max()) < V and dst.min() >= 0))
    order = np.argsort(src, kind="stable")
    row_ptr = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=V), out=row_ptr[1:])
    weight = w[order]
    od = [0.0] * V
    for s, x in zip(src[order].tolist(), weight.tolist()):
        od[s] += x                                         # in order, one rounded addition per edge
    return dict(row_ptr=row_ptr, nbr=dst[order], weight=weight, out_degree=np.array(od, np.float64).reshape(V))


# ------------------------------------------------------------------------------------------- lattice weights
LATTICE_SHAPES = ("pareto", "near", "two", "giant")


def lattice_weights(rng, k, m, shape):
    """k integer weights (as float64) that sum to exactly k * 2^m.  Then total = k * 2^m and  p_i = k * w_i / total = w_i / 2^m  without rounding (k * w_i
    and the total are below 2^53, the quotient is a multiple of 2^-m below 2^53 / 2^m), and every (p_l + p_s) - 1 or p_g - (1 - p_s) either builder forms
    is a difference of multiples of 2^-m of magnitude at most k: exact.  Shapes: `pareto` heavy tail; `near` 2^m plus -1, 0 or +1 (slots a hair under, at
    and over 1); `two` values 1 or 37, rescaled; `giant` ones plus one slot that takes the rest.  The conditions are asserted on the result."""
    k, m = int(k), int(m)
    K = k << m
    assert k >= 1 and m >= 1 and shape in LATTICE_SHAPES

    def rescale(v):
        v = [int(x) for x in v]
        tot = sum(v)
        out = [x * K // tot for x in v]
        rest = K - sum(out)
        assert 0 <= rest < k
        for i in range(rest):                              # the floor's remainder, a unit each to the first slots
            out[i] += 1
        return out

    if shape == "pareto":
        w = rescale(np.floor(rng.pareto(1.1, k) * 3) + 1)
    elif shape == "two":
        w = rescale(np.where(rng.random(k) < 0.9, 1, 37))
    elif shape == "near":
        d = rng.integers(-1, 2, k)
        e = int(d.sum())
        if e > 0:
            d[np.flatnonzero(d > -1)[:e]] -= 1             # at least e slots hold +1
        elif e < 0:
            d[np.flatnonzero(d < 1)[:-e]] += 1
        w = [(1 << m) + int(x) for x in d]
    else:
        w = [1] * k
        w[k // 3] = K - (k - 1)
    assert len(w) == k and min(w) >= 1 and sum(w) == K, "lattice weights must be positive integers that sum to k * 2^m"
    assert K < 1 << 53 and k * max(w) < 1 << 53, "k * w_i or the total leaves the exactly representable integers"
    return np.array(w, np.float64)


# ------------------------------------------------------------------------------------------- what a table encodes
def mass(prob, alias):
    """Per slot i:  prob_i + sum over the slots j with alias_j == i of (1 - prob_j)  — the mass, in slot units, a uniform draw over the slots sends to
    slot i's neighbour.  A slot with alias -1 keeps its own remainder ("no alias": stay in the slot)."""
    prob = np.asarray(prob, np.float64); alias = np.asarray(alias, np.int64)
    k = len(prob)
    assert len(alias) == k and (k == 0 or (alias.min() >= -1 and alias.max() < k)), "alias outside [-1, k)"
    to = np.where(alias < 0, np.arange(k), alias)
    out = prob.copy()
    np.add.at(out, to, 1.0 - prob)
    return out


def assert_lattice_table(prob, alias, out_degree, w, m, what=None):
    """The assertions of a table built from lattice_weights(.., m, ..): it encodes w / 2^m exactly."""
    k = len(w)
    prob = np.asarray(prob, np.float64); alias = np.asarray(alias, np.int64)
    assert len(prob) == len(alias) == k, what
    assert out_degree == float(k << m), what
    assert alias.min() >= -1 and alias.max() < k, what
    assert (prob >= 0).all() and (prob <= 1).all(), what
    assert not ((prob < 1) & (alias < 0)).any(), what                       # no slot is left with a remainder and nowhere to send it
    got, want = mass(prob, alias), np.asarray(w, np.float64) / float(1 << m)
    bad = np.flatnonzero(got != want)                                        # float64 equality
    assert len(bad) == 0, (what, "%d of %d slots carry another mass; first: slot %d holds %r, its weight says %r" % (
        len(bad), k, bad[0], got[bad[0]], want[bad[0]]))


def mass_total_error(prob):
    """|sum of mass() - k| with the sum taken exactly (math.fsum).  Every slot hands on prob_i + (1 - prob_i), so in exact arithmetic the total is k for
    ANY table whose aliases are in range: what is left is the rounding of the k differences 1 - prob_i and of the final sum."""
    prob = np.asarray(prob, np.float64)
    return abs(math.fsum(prob.tolist() + (1.0 - prob).tolist()) - len(prob))


def float_table_checks(prob, alias):
    """What holds for a table of ARBITRARY weights: alias in [-1, k), prob >= 0 -> (|sum of mass - k|, its bound 2k * 2^-53 * max prob; derived in
    tests/test_walk_ref.py for max prob >= 3/4, asserted here).  Per-slot mass is not held to a bound on such tables: the reconstruction error chains
    through the donors."""
    prob = np.asarray(prob, np.float64); alias = np.asarray(alias, np.int64)
    k = len(prob)
    assert len(alias) == k and alias.min() >= -1 and alias.max() < k
    assert (prob >= 0).all()
    pmax = float(prob.max())
    assert pmax >= 0.75
    return mass_total_error(prob), 2 * k * 2.0 ** -53 * pmax


# ------------------------------------------------------------------------------------------- walks from tables
def tables_of(g):
    """What the replays need, read once from a graph object with get_csr() and get_source_alias() (the device's or the oracle's)."""
    c = g.get_csr(); s = g.get_source_alias()
    return dict(row_ptr=np.asarray(c["row_ptr"], np.int64), nbr=np.asarray(c["nbr"], np.int64), prob=np.asarray(c["prob"], np.float64),
                alias=np.asarray(c["alias"], np.int64), src=np.asarray(s["src"], np.int64), src_prob=np.asarray(s["prob"], np.float64),
                src_alias=np.asarray(s["alias"], np.int64))


def _pick(x, base, k, prob, alias, ids):
    """One draw per lane: x in [0, 1) over the k slots that start at `base` -> ids of the chosen slots.
    i = min(int(x * k), k - 1);  y = x * k - i;  slot i if y < prob[i] or it has no alias, else slot alias[i]."""
    xk = x * k.astype(np.float64)
    i = np.minimum(xk.astype(np.int64), k - 1)             # the cast truncates
    y = xk - i.astype(np.float64)
    a = alias[base + i]
    own = (y < prob[base + i]) | (a < 0)
    return ids[base + np.where(own, i, a)]


def _walk_from(t, s, L):
    """Walks of the streams whose uint64 states are `s` (one walk per stream) -> int32 [n x L], pad -1."""
    n = len(s)
    out = np.full((n, L), -1, np.int32)
    S = len(t["src"])
    if n == 0 or S == 0 or L == 0:
        return out
    deg = np.diff(t["row_ptr"])
    x = _next_double_vec(s)
    cur = _pick(x, np.zeros(n, np.int64), np.full(n, S, np.int64), t["src_prob"], t["src_alias"], t["src"])
    out[:, 0] = cur
    live = np.arange(n)
    for j in range(1, L):
        keep = deg[cur] > 0                                # a vertex without out-edges ends the walk before drawing
        live, cur = live[keep], cur[keep]
        if len(live) == 0:
            break
        st = s[live]
        x = _next_double_vec(st)
        s[live] = st
        cur = _pick(x, t["row_ptr"][cur], deg[cur], t["prob"], t["alias"], t["nbr"])
        out[live, j] = cur
    return out


def replay_strided(tables, n, L, seed, first_index=0):
    """rng_mode 1: walk i owns the draws that start at draw (first_index + i) * L of java.util.Random(seed) -> int32 [n x L], pad -1."""
    n, L = int(n), int(L)
    m, p = _affine_pow(2 * L)
    st = [JavaRandom.before_draw(seed, int(first_index) * L).s] if n else []
    for _ in range(n - 1):
        st.append((m * st[-1] + p) & JR_MASK)
    return _walk_from(tables, np.array(st, np.uint64), L)


def replay_sequential(tables, n, L, seed, first_draw=0):
    """rng_mode 0: ONE java.util.Random(seed) stream, `first_draw` draws already taken, consumed walk after walk, one draw per vertex of a walk
    -> (int32 [n x L] pad -1, draws consumed)."""
    n, L = int(n), int(L)
    out = np.full((n, L), -1, np.int32)
    S = len(tables["src"])
    if n == 0 or S == 0 or L == 0:
        return out, 0
    xs = stream_doubles(seed, first_draw, n * L).tolist()   # no walk takes more than L
    row_ptr = tables["row_ptr"].tolist(); nbr = tables["nbr"].tolist(); prob = tables["prob"].tolist(); alias = tables["alias"].tolist()
    src = tables["src"].tolist(); sp = tables["src_prob"].tolist(); sa = tables["src_alias"].tolist()
    rows = []
    o = 0
    for _ in range(n):
        xk = xs[o] * S; o += 1
        i = min(int(xk), S - 1)
        v = src[i] if (xk - i < sp[i] or sa[i] < 0) else src[sa[i]]
        row = [v]
        while len(row) < L:
            b = row_ptr[v]; k = row_ptr[v + 1] - b
            if k == 0:
                break
            xk = xs[o] * k; o += 1
            i = min(int(xk), k - 1)
            v = nbr[b + i] if (xk - i < prob[b + i] or alias[b + i] < 0) else nbr[b + alias[b + i]]
            row.append(v)
        rows.append(row)
    for r, row in enumerate(rows):
        out[r, :len(row)] = row
    return out, o
