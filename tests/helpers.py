"""Shared builders for the parity tests: the same seeded inputs go to the oracle and to libdge."""
import numpy as np


def layered_graph(R=40, T=4, deg=6, seed=0, shuffle=True, duplicates=True, dead_ends=0.0):
    """Small cross-time graph in INSERTION order that is not sorted by source (as J/CrossTimeGraph.java:33-41
    would produce it, then shuffled) with duplicate (src,dst) pairs kept (J/LayeredGraph.java:157-174)."""
    rng = np.random.default_rng(seed)
    src, dst, w = [], [], []
    for h in range(T):
        for s in range(R):
            if dead_ends > 0 and h > 0 and rng.random() < dead_ends:
                continue
            k = int(rng.integers(1, deg + 1))
            for d in rng.integers(0, R, k):
                src.append(h * R + s); dst.append(((h + 1) % T) * R + int(d)); w.append(float(rng.integers(1, 60)))
            if duplicates and rng.random() < 0.3:
                src.append(h * R + s); dst.append(dst[-1]); w.append(float(rng.integers(1, 60)))
    src = np.array(src, np.int32); dst = np.array(dst, np.int32); w = np.array(w, np.float64)
    if shuffle:
        p = rng.permutation(len(src))
        src, dst, w = src[p], dst[p], w[p]
    present = np.zeros(R * T, bool); present[src] = True; present[dst] = True
    sources = np.array([v for v in range(R) if present[v]], np.int32)
    return src, dst, w, sources


def build_both(O, E, src, dst, w, sources, exact=True, stream_sum=False, top_k=None):
    og = O.Graph(); og.add_edges(src, dst, w)
    dg = E.DeviceGraph(0); dg.add_edges(src, dst, w)
    if top_k is not None:
        og.keep_top_k(top_k); dg.keep_top_k(top_k)
    og.set_sources(sources, stream_sum); dg.set_sources(sources, stream_sum)
    og.build_alias(exact); dg.build_alias(exact)
    return og, dg


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def cosine_rows(a, b):
    num = (a.astype(np.float64) * b.astype(np.float64)).sum(1)
    den = np.linalg.norm(a.astype(np.float64), axis=1) * np.linalg.norm(b.astype(np.float64), axis=1)
    return num / np.maximum(den, 1e-300)


def simulate_block_schedule(models, train_fn, serial=False):
    """The multi-GPU block schedule (embedding_amd/distributed.py: block_schedule_step) with all ranks on ONE device:
    models[g] plays rank g; the all-gather between episodes becomes direct export/import between the models."""
    import torch
    N = len(models)
    pf = models[0].partition_floats(N)
    bufs = [torch.empty(pf, dtype=torch.float32, device=models[0].torch_device) for _ in range(N)]
    for e in range(N):
        for g, m in enumerate(models):
            m.set_partition(N, g, (g + e) % N)
            if train_fn.__code__.co_argcount >= 2:
                train_fn(m, e)              # (the episode number: learning-rate position by progress)
            else:
                train_fn(m)
            if serial:
                m.stats()                   # drains this model's stream: the ranks' launches of an episode run one after the other, as they would on N devices of their own
        for table in ((1, 2) if getattr(getattr(models[0], "cfg", None), "use_hs", 0) else (1,)):      # syn1 partitions travel with the syn1neg partitions (use_hs)
            for g, m in enumerate(models):
                m.export_partition(table, N, (g + e) % N, bufs[g])
            for g, m in enumerate(models):
                for r in range(N):
                    if r != g:
                        m.import_partition(table, N, (r + e) % N, bufs[r])
    for g, m in enumerate(models):
        m.set_partition(1)


def simulate_gather_syn0(models):
    import torch
    N = len(models)
    pf = models[0].partition_floats(N)
    bufs = [torch.empty(pf, dtype=torch.float32, device=models[0].torch_device) for _ in range(N)]
    for g, m in enumerate(models):
        m.export_partition(0, N, g, bufs[g])
    for g, m in enumerate(models):
        for r in range(N):
            if r != g:
                m.import_partition(0, N, r, bufs[r])


def link_auc(syn0, syn1neg, vocab_ids, test_walks, R, seed=3):
    """Link prediction on held-out walk steps: AUC of syn0[next] . syn1neg[current] for true next vertices against a random region of
    the same slice (the statistical parity measure of scripts/quality_scale.py, on the host)."""
    rng = np.random.default_rng(seed)
    NV = int(max(int(vocab_ids.max()), int(test_walks.max())) + 1)
    remap = -np.ones(NV + R, np.int64); remap[vocab_ids.astype(np.int64)] = np.arange(len(vocab_ids))
    a = test_walks[:, :-1].reshape(-1).astype(np.int64); b = test_walks[:, 1:].reshape(-1).astype(np.int64)
    ok = (a >= 0) & (b >= 0); a, b = a[ok], b[ok]
    rnd = (b // R) * R + rng.integers(0, R, len(b))
    ra, rb, rr = remap[a], remap[b], remap[np.minimum(rnd, NV - 1)]
    ok = (ra >= 0) & (rb >= 0) & (rr >= 0); ra, rb, rr = ra[ok], rb[ok], rr[ok]
    pos = (syn0[rb].astype(np.float64) * syn1neg[ra]).sum(1); neg = (syn0[rr].astype(np.float64) * syn1neg[ra]).sum(1)
    return float((pos > neg).mean() + 0.5 * (pos == neg).mean())


# ---- device-side helpers of the full-size statistical tests (tables of a million rows never visit the host)
def device_table(model, table, n_parts=1, part=0):
    """Rows of partition `part` (row % n_parts == part; n_parts = 1: the whole table) of syn0 (0) / syn1neg (1) as a torch tensor
    [rows x stride] on the model's device — through the C ABI's partition export, device to device."""
    import torch
    pf = model.partition_floats(n_parts)
    buf = torch.empty(pf, dtype=torch.float32, device=model.torch_device)
    model.export_partition(table, n_parts, part, buf)
    stride = -(-model.cfg.dim // 64) * 64
    return buf.view(-1, stride)


def link_scores_device(model, vocab_ids, test_walks, R, NV, seed=3):
    """Scores syn0[next] . syn1neg[current] of the held-out walk steps of `test_walks` (torch int64 [n x L] on the device) and of a random
    region of the next vertex's slice instead of it -> (pos, neg) score tensors."""
    import torch
    dev = model.torch_device
    s0 = device_table(model, 0); s1 = device_table(model, 1)
    vid = torch.from_numpy(vocab_ids.astype(np.int64)).to(dev)
    remap = -torch.ones(NV, dtype=torch.int64, device=dev); remap[vid] = torch.arange(len(vid), device=dev)
    a = test_walks[:, :-1].reshape(-1); b = test_walks[:, 1:].reshape(-1)
    ok = (a >= 0) & (b >= 0); a, b = a[ok], b[ok]
    gen = torch.Generator(device=dev); gen.manual_seed(seed)
    rnd = torch.div(b, R, rounding_mode="floor") * R + torch.randint(0, R, (len(b),), generator=gen, device=dev)
    ra, rb, rr = remap[a], remap[b], remap[rnd]
    ok = (ra >= 0) & (rb >= 0) & (rr >= 0); ra, rb, rr = ra[ok], rb[ok], rr[ok]
    pos = torch.empty(len(ra), dtype=torch.float32, device=dev); neg = torch.empty_like(pos)
    for i in range(0, len(ra), 1 << 20):                      # in slices: the gathered rows of 4.6 M steps would be gigabytes
        j = slice(i, i + (1 << 20))
        x = s1[ra[j]]
        pos[j] = (s0[rb[j]] * x).sum(1); neg[j] = (s0[rr[j]] * x).sum(1)
    return pos, neg


def link_auc_device(model, vocab_ids, test_walks, R, NV, seed=3):
    """Link-prediction AUC on held-out walk steps (helpers.link_auc, scripts/quality_scale.py) computed on the device, and the mean
    negative-sampling loss of the same (positive, random-region) score pairs."""
    import torch
    pos, neg = link_scores_device(model, vocab_ids, test_walks, R, NV, seed)
    auc = float((pos > neg).float().mean() + 0.5 * (pos == neg).float().mean())
    loss = float(torch.nn.functional.softplus(-pos.double()).mean() + torch.nn.functional.softplus(neg.double()).mean())
    return auc, loss


# ---- the saturated, exactly summable regime (tests/test_oracle_kats.py, tests/test_gpu_conservation.py)
# Column 0 of every row saturates the score: syn0[:, 0] = 4 and syn1neg[:, 0] = 2 * sign, so f = 8 * sign (+ something tiny) for every pair, beyond
# MAX_EXP = 6, and word2vec's clamp gives g = (label - 1) * alpha for sign +1 (positives 0, negatives exactly -alpha) and g = label * alpha for sign -1
# (positives exactly +alpha, negatives 0).  With alpha = min_alpha = 2^-40 and small integers in the columns of the table that stands still, the other
# table accumulates 2^-40 x (a sum of small integers): every product and partial sum is exact while |sum| < 2^24, whatever the order of the additions.
SAT_ALPHA = 2.0 ** -40
SAT_CAP = 1 << 24


def saturated_state(V, D, side, sign, seed, mag=3, use_hs=False):
    """Initial tables of the saturated regime -> {"syn0", "syn1neg"[, "syn1"]}, float32 [V x D] (syn1: [V-1 x D]).
    side "A": syn0[:, 1:] holds the integer codes (column 1 = 1, the count channel; the others +/- 1 .. mag, never 0) and syn1neg[:, 1:] = 0 accumulates;
    side "B": the mirror image — syn1neg holds the codes, syn0[:, 1:] = 0 accumulates.  With use_hs, syn1[:, 0] = 2 and the rest zero: the tree step
    is skipped on every node (|f| >= 6) and syn1 has to come back unchanged."""
    assert side in ("A", "B") and sign in (1, -1) and D >= 2 and mag >= 1
    rng = np.random.default_rng([int(seed), V, D])
    codes = (rng.integers(1, mag + 1, (V, D)) * rng.choice([-1, 1], (V, D))).astype(np.float32)
    codes[:, 1] = 1.0
    s0 = np.zeros((V, D), np.float32); s1 = np.zeros((V, D), np.float32)
    (s0 if side == "A" else s1)[:] = codes
    s0[:, 0] = 4.0; s1[:, 0] = 2.0 * sign
    out = {"syn0": s0, "syn1neg": s1}
    if use_hs:
        s2 = np.zeros((max(V - 1, 0), D), np.float32); s2[:, 0] = 2.0
        out["syn1"] = s2
    return out


# ---- the balanced, exactly summable regime (tests/test_oracle_kats.py, tests/test_gpu_conservation_balanced.py)
# Column 0 of every row puts every score into the middle bin of the sigmoid table: syn0[:, 0] = 1/4 and syn1neg[:, 0] = syn1[:, 0] = 1/8, so f = 2^-5 (+ something
# tiny) for every term; idx = (int)((f + 6) * 83) = 500 for f in [0.024096, 0.036145) and exp_table[500] is exactly 0.5f.  The tree term is then
# g = (1 - code - 0.5) * alpha = +/- alpha/2 and the negative-sampling term g = (label - 0.5) * alpha = +/- alpha/2: no clamp, no skip, the table look-up on every
# term.  With alpha = min_alpha = 2^-60 the accumulating table holds 2^-61 x (a signed sum of small integers) — exact in any order below 2^24 — and what flows back
# into the standing table (~2^-122 x integers) is absorbed by its entries, none of which is 0; a score moves by less than 1.2e-8, the bin has 0.0048 to spare.
BAL_ALPHA = 2.0 ** -60


def balanced_state(V, D, side, seed, mag=3, use_hs=False):
    """Initial tables of the balanced regime -> {"syn0", "syn1neg"[, "syn1"]}, float32 [V x D] (syn1: [V-1 x D]).
    side "A": syn0[:, 1:] holds the integer codes (column 1 = 1, the net-count channel; the others +/- 1 .. mag, never 0), syn1neg[:, 1:] and syn1[:, 1:] = 0 accumulate;
    side "B": the mirror image — syn1neg and syn1 hold codes (different ones), syn0[:, 1:] = 0 accumulates through a pair's neu1e."""
    assert side in ("A", "B") and D >= 2 and mag >= 1
    rng = np.random.default_rng([int(seed), V, D, 60])

    def codes(rows):
        c = (rng.integers(1, mag + 1, (rows, D)) * rng.choice([-1, 1], (rows, D))).astype(np.float32)
        c[:, 1] = 1.0
        return c
    s0 = np.zeros((V, D), np.float32); s1 = np.zeros((V, D), np.float32); s2 = np.zeros((max(V - 1, 0), D), np.float32)
    if side == "A":
        s0[:] = codes(V)
    else:
        s1[:] = codes(V); s2[:] = codes(len(s2))
    s0[:, 0] = 0.25; s1[:, 0] = 0.125; s2[:, 0] = 0.125
    out = {"syn0": s0, "syn1neg": s1}
    if use_hs:
        out["syn1"] = s2
    return out


class Balanced:
    """What balanced_diff returns: per row `diff`, the largest |got - want| over the row's columns in units of alpha/2, and `whole`, whether the row of `got` holds
    whole multiples of alpha/2 only."""

    def __init__(self, diff, whole, net_want, net_got):
        self.diff, self.whole, self.net_want, self.net_got = diff, whole, net_want, net_got

    @property
    def exact(self):
        return not self.diff.any()

    def worst(self):
        r = int(np.argmax(self.diff))
        return "row %d: off by %.3f units of alpha/2 (net count %.3f, expected %d); %d of %d rows differ, %d hold a fraction of a unit" % (
            r, self.diff[r], self.net_got[r], self.net_want[r], int((self.diff != 0).sum()), len(self.diff), int((~self.whole).sum()))


def balanced_diff(got, want, init, bound, alpha=BAL_ALPHA):
    """Trained table `got` against the expected one `want` (both [rows x D], an ACCUMULATING table of a balanced run that began as `init`) -> Balanced.
    Asserts first, on `want` alone, the conditions of the method: column 0 is unchanged, every accumulated value is a whole multiple of alpha/2, and `bound` — the
    largest code magnitude times an upper bound on the terms one row can take, from host quantities — is below 2^24, so that every partial sum in ANY order is
    exact (and the reference's own sums are inside it)."""
    unit = alpha / 2
    assert 0 <= bound < SAT_CAP, "a row can take %d units: partial sums may leave the exactly summable range (2^24) — shorten the corpus or lower `mag`" % bound
    assert np.array_equal(bits(want[:, 0]), bits(init[:, 0])), "the reference's column 0 moved: it is outside the balanced regime"
    w = want[:, 1:].astype(np.float64) / unit
    assert (w == np.rint(w)).all(), "the expected table is not a table of whole multiples of alpha/2: the reference is outside the balanced regime"
    assert np.abs(w).max(initial=0.0) <= bound, "the expected table exceeds the stated term bound: |sum| = %.0f > %d" % (np.abs(w).max(initial=0.0), bound)
    g = got[:, 1:].astype(np.float64) / unit
    diff = np.maximum(np.abs(g - w).max(1), np.abs(got[:, 0].astype(np.float64) - init[:, 0]) / unit)
    return Balanced(diff, (g == np.rint(g)).all(1), np.rint(w[:, 0]).astype(np.int64), g[:, 0])


def device_rows(a, stride, rows=None):
    """[V x D] -> the C ABI's import shape [rows x stride] (rows: the table's V; zero padding columns, zero rows behind a shorter table such as syn1)."""
    out = np.zeros((a.shape[0] if rows is None else rows, stride), np.float32)
    out[:a.shape[0], :a.shape[1]] = a
    return out


class Conservation:
    """What conservation_diff returns: per row, `expected` / `got` — the count channel in whole updates (signed: negatives count -1, positives +1) —,
    `deficit` = |expected| - |got| (> 0: updates lost, < 0: a surplus), `other` = the largest |difference| of the remaining columns in units of alpha."""

    def __init__(self, expected, got, other):
        self.expected, self.got, self.other = expected, got, other
        self.deficit = np.abs(expected) - np.abs(got)

    @property
    def exact(self):
        return bool((self.got == self.expected).all() and (self.other == 0).all())

    def worst(self):
        r = int(np.argmax(np.abs(self.deficit) + self.other))
        return "row %d: expected %d updates, got %.3f (other columns off by %.3f alpha); %d rows differ, %d updates of %d missing" % (
            r, self.expected[r], self.got[r], self.other[r], int(((self.got != self.expected) | (self.other != 0)).sum()),
            int(self.deficit.sum()), int(np.abs(self.expected).sum()))


def conservation_diff(got, want, alpha=SAT_ALPHA):
    """Trained table `got` against the expected one `want` (both [V x D], the ACCUMULATING table of a saturated run) -> Conservation.
    Asserts first, on `want`, the condition of the method: every accumulated |value| / alpha is an integer below 2^24 (beyond it float32 sums stop being
    exact and the comparison would depend on the order of the additions — choose a shorter corpus or smaller codes)."""
    w = want[:, 1:].astype(np.float64) / alpha
    assert np.abs(w).max(initial=0.0) < SAT_CAP, "the expected table leaves the exactly summable range: |sum| = %.0f >= 2^24 — shorten the corpus or lower `mag`" % np.abs(w).max()
    assert (w == np.rint(w)).all(), "the expected table is not a table of whole multiples of alpha: the reference is outside the saturated regime"
    assert np.array_equal(bits(got[:, 0]), bits(want[:, 0])), "the saturating column moved"
    g = got[:, 1:].astype(np.float64) / alpha
    other = np.abs(g[:, 1:] - w[:, 1:]).max(1) if w.shape[1] > 1 else np.zeros(len(w))
    return Conservation(np.rint(w[:, 0]).astype(np.int64), g[:, 0], other)


# ---- graded rates: the per-walk learning rate on an exact dyadic lattice (tests/test_oracle_kats.py, tests/test_gpu_conservation_rates.py)
# alpha0 = 2^-e, min_alpha = 2^-(e+2) and a vocabulary whose token sum T has epochs * T + 1 = 2^m: a walk that `done` tokens precede trains at
# 2^-e * (2^m - done) / 2^m — every step of the formula exact in binary64, the cast exact in float32 — a whole multiple of u = 2^-(e+b) wherever 2^(m-b) divides
# every `done` that occurs.  In the saturated state a live term is then +/- level x code units of u, in the balanced state units of u/2: sums still do not depend on
# the order of the additions, but they do depend on the rate each term carried.
def rate_level(wb, words_before, epoch, T, epochs, b, words_scale=(1, 1), clamp=2):
    """The learning rate, in units of alpha0 / 2^b, of a walk that `wb` in-vocabulary tokens of its launch precede: `words_before` tokens of the epoch lie before the
    launch, `T` tokens make an epoch (epochs * T + 1 must be a power of two, 2^m, m >= b), words_scale = (numerator, denominator) is the launch's scale on wb
    (truncated, as the cast to int64 truncates), clamp = c puts the floor at alpha0 / 2^c (None: no floor).  Integers only."""
    wb, words_before, epoch, T, epochs, b = int(wb), int(words_before), int(epoch), int(T), int(epochs), int(b)
    num, den = int(words_scale[0]), int(words_scale[1])
    full = epochs * T + 1
    m = full.bit_length() - 1
    assert full == 1 << m and 0 <= b <= m and num > 0 and den > 0 and wb >= 0 and words_before >= 0 and 0 <= epoch
    done = epoch * T + words_before + (wb * num) // den
    left, step = full - done, 1 << (m - b)
    assert 0 < left < 1 << 24, "2^m - done = %d does not fit a float32 significand (or the schedule has run out)" % left
    assert left % step == 0, "%d tokens done: the rate is no whole multiple of alpha0 / 2^%d" % (done, b)
    level = left // step
    if clamp is not None:
        assert 0 <= clamp <= b
        level = max(level, 1 << (b - clamp))
    return level


class Graded:
    """What graded_diff returns: per row `diff`, the largest |got - want| over the row's columns in lattice units, `whole`, whether the row of `got` holds whole
    multiples of the unit only, and column 1 — the sum of the levels of the row's terms, signed — as `level_want` / `level_got`."""

    def __init__(self, diff, whole, level_want, level_got):
        self.diff, self.whole, self.level_want, self.level_got = diff, whole, level_want, level_got

    @property
    def exact(self):
        return not self.diff.any()

    def worst(self):
        r = int(np.argmax(self.diff))
        return "row %d: off by %.3f lattice units (sum of its terms' levels: expected %d, got %.3f); %d of %d rows differ, %d hold a fraction of a unit" % (
            r, self.diff[r], self.level_want[r], self.level_got[r], int((self.diff != 0).sum()), len(self.diff), int((~self.whole).sum()))


def graded_diff(got, want, init, unit, levels, bound):
    """Trained table `got` against the expected one `want` (both [rows x D], an ACCUMULATING table of a graded-rates run that began as `init`) -> Graded.
    `unit`: what one lattice unit is worth in the table (saturated: alpha0 / 2^b, balanced: alpha0 / 2^(b+1)); `levels`: the largest level a walk can train at (2^b);
    `bound`: the largest code magnitude times an upper bound on the terms one row can take, from host quantities.  Asserts first, on `want` alone, the conditions of
    the method: bound x levels < 2^24 (every partial sum in ANY order is exact), column 0 unchanged, every accumulated value a whole multiple of the unit and inside
    the bound."""
    assert levels >= 1 and 0 <= bound * levels < SAT_CAP, "a row can take %d x %d units: partial sums may leave the exactly summable range (2^24) — shorten the corpus, coarsen the lattice or lower `mag`" % (bound, levels)
    assert np.array_equal(bits(want[:, 0]), bits(init[:, 0])), "the reference's column 0 moved: it is outside the regime"
    w = want[:, 1:].astype(np.float64) / unit
    assert (w == np.rint(w)).all(), "the expected table is not a table of whole multiples of the lattice unit: the reference is outside the graded regime"
    assert np.abs(w).max(initial=0.0) <= bound * levels, "the expected table exceeds the stated term bound: |sum| = %.0f > %d" % (np.abs(w).max(initial=0.0), bound * levels)
    g = got[:, 1:].astype(np.float64) / unit
    diff = np.maximum(np.abs(g - w).max(1), np.abs(got[:, 0].astype(np.float64) - init[:, 0]) / unit)
    return Graded(diff, (g == np.rint(g)).all(1), np.rint(w[:, 0]).astype(np.int64), g[:, 0])
