"""CPU: the test of the exact held-out evaluation tests (tests/eval_ref.py, tests/test_gpu_eval_exact.py).  What the device tests claim must not rest on the
device run: the reading of include/dge.h in eval_ref.py equals the mesh restatement of tests/test_gpu_eval.py and scalar loops written out here; the
planted tables meet the exactness condition; every named builder's input meets the conditions that make its case worth running (skips, ties, wins and
losses all present, every lane of a negative batch used, a skip inside a full batch); and every builder tells the true reading from each of eight
plausible slips of a kernel — in a count, in 2 wins + ties, or in the loss by more than the device test's tolerance."""
import math

import numpy as np
import pytest

import eval_ref as ref
from test_gpu_eval import sgns_restate

M64 = (1 << 64) - 1


def mix64_int(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


@pytest.fixture(scope="module")
def world():
    counts = ref.world_counts()
    vid, sorted_counts = ref.vocabulary(counts)
    return dict(counts=counts, vid=vid, table=ref.unigram_table(sorted_counts), remap=ref.host_map(vid, ref.NV))


@pytest.fixture(scope="module")
def readings(world):
    """name -> (figures, detail) of every builder, computed once."""
    return {name: c.reference(world["vid"], world["table"], detail=True) for name, c in ref.CASES.items()}


# ------------------------------------------------------------------------------------------------ soundness
def test_mix64_and_the_world(world):
    for x in (0, 1, M64 - 5, 2 ** 63):
        assert int(ref.mix64(x)[0]) == mix64_int(x)
    assert int(ref.mix64(0)[0]) == 0xE220A8397B1DCDAF                  # splitmix64's first output from state 0
    V = len(world["vid"])
    assert 512 < V < ref.NV and (world["counts"] < ref.MIN_COUNT).sum() == ref.NV - V
    c = world["counts"][world["vid"]]
    assert (np.diff(c) <= 0).all() and (np.diff(world["vid"])[np.diff(c) == 0] > 0).all()
    t = world["table"]
    assert len(t) == ref.TABLE_SIZE and t[0] == 0 and t[-1] == V - 1 and (np.diff(t) >= 0).all() and len(np.unique(t)) == V


@pytest.mark.parametrize("L,W", [(8, 1), (8, 3), (8, 8), (8, 15), (24, 1), (24, 24), (24, 31)])
@pytest.mark.parametrize("K", [0, 1, 5, 17])
def test_sgns_by_band_equals_the_mesh_and_a_scalar_loop(world, L, W, K):
    w = ref.make_walks(7, L, 50 + L + W, world["counts"])
    w[5] = -1                                                            # a walk with nothing in the vocabulary
    row0, seed, table, remap = 12345, 2 ** 64 - 9, world["table"], world["remap"]
    got = ref.sgns(w, row0, W, K, seed, remap, table)
    want = sgns_restate(w, row0, W, K, seed, remap, table)
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.array_equal(a, b)
    ctr, ctx, neg = [], [], []
    for gi in range(len(w)):
        t = [int(remap[v]) for v in w[gi] if 0 <= v < ref.NV and remap[v] >= 0]
        for i in range(len(t)):
            for c in range(len(t)):
                if 0 < abs(i - c) <= W:
                    ctr.append(t[i]); ctx.append(t[c])
                    base = ((((row0 + gi) * L + i) * L + c) * K) & M64
                    neg.append([int(table[mix64_int((seed + base + k) & M64) % len(table)]) for k in range(K)])
    assert len(ctr) > 0
    assert got.ctr.tolist() == ctr and got.ctx.tolist() == ctx and got.neg.tolist() == neg
    assert np.array_equal(got.valid, got.neg != got.ctr[:, None])


@pytest.mark.parametrize("L,R", [(1, 40), (2, 40), (9, 40), (9, 1), (9, 48), (9, 1000)])
def test_links_equals_a_scalar_loop(world, L, R):
    w = ref.make_walks(60, L, 70 + L + R, world["counts"])
    row0, seed, remap = 99, 2 ** 64 - 2, world["remap"]
    ra, rb, rr, skipped = ref.links(w, row0, R, seed, remap)
    A, B, RR, sk = [], [], [], 0
    row = lambda v: int(remap[v]) if 0 <= v < ref.NV else -1
    for i in range(len(w)):
        for j in range(L - 1):
            a, b = int(w[i, j]), int(w[i, j + 1])
            if a < 0 or b < 0:
                continue
            r = (b // R) * R + mix64_int((seed + (row0 + i) * L + j) & M64) % R
            if min(row(a), row(b), row(r)) < 0:
                sk += 1
                continue
            A.append(row(a)); B.append(row(b)); RR.append(row(r))
    assert (ra.tolist(), rb.tolist(), rr.tolist(), skipped) == (A, B, RR, sk)
    assert L == 1 or (sk > 0 and len(A) > 0)


def test_figures_against_a_float_loop():
    """figures() on a handful of pairs against softplus and comparisons written out in Python floats."""
    S0, S1 = ref.lattice(30, 70, seed=5)
    rng = np.random.default_rng(3)
    pc, pt = rng.integers(0, 30, 40), rng.integers(0, 30, 40)
    own = rng.integers(0, 40, 100); nc, nt = pc[own], rng.integers(0, 30, 100)
    score = lambda c, t: sum(float(x) * float(y) for x, y in zip(S0[c], S1[t])) / 4.0
    sp = lambda x: math.log1p(math.exp(-abs(x))) + max(x, 0.0)
    pos = [score(c, t) for c, t in zip(pc, pt)]; neg = [score(c, t) for c, t in zip(nc, nt)]
    wins = sum(pos[o] > n for o, n in zip(own, neg)); ties = sum(pos[o] == n for o, n in zip(own, neg))
    for form, loss in (("links", sum(sp(-x) for x in pos) / 40 + sum(sp(x) for x in neg) / 100), ("sgns", (sum(sp(-x) for x in pos) + sum(sp(x) for x in neg)) / 40)):
        f = ref.figures(S0, S1, 1, form, pc, pt, nc, nt, own)
        assert (f["pairs"], f["negatives"], f["wins"], f["ties"]) == (40, 100, wins, ties) and wins > 0 and ties > 0
        assert f["auc"] == (wins + 0.5 * ties) / 100
        assert abs(f["loss"] - loss) <= 140 * 2.0 ** -50 * loss


# ------------------------------------------------------------------------------------------------ the planted tables
@pytest.mark.parametrize("dim", [1, 20, 64, 65, 128, 200, 256, 257, 320, 448, 512])
def test_the_planted_tables_are_exact_in_any_order(dim):
    V = 604
    S0, S1 = ref.lattice(V, dim, seed=1)
    ref.check_exact(S0, S1)
    cols = ref.live_columns(dim)
    assert cols[0] == 0 and cols[-1] == dim - 1 and set(cols // 64) == set(range(-(-dim // 64)))      # every chunk of the row carries weight
    assert (S0[:, cols] != 0).any(0).all() and (S1[:, cols] != 0).any(0).all()
    W0, W1 = ref.witness(V, dim, seed=2)
    ref.check_exact(W0, W1, lattice_only=False)
    G = W0 @ W1.T
    assert np.array_equal(G[:dim, 0], np.arange(1, dim + 1))
    # a float32 model of the sum in two opposite orders, fused-free: the same bits as the integer product
    x = (W0[dim:dim + 40] * 0.5).astype(np.float32); y = (W1[:40] * 0.5).astype(np.float32)
    want = (W0[dim:dim + 40] * W1[:40]).sum(1) / 4.0
    for order in (slice(None), slice(None, None, -1)):
        acc = np.zeros(40, np.float32)
        for k in np.arange(dim)[order]:
            acc = acc + x[:, k] * y[:, k]
        assert np.array_equal(acc.astype(np.float64), want)


# ------------------------------------------------------------------------------------------------ conditions on the inputs
def test_the_case_list_is_the_one_the_device_file_runs():
    names = set(ref.CASES)
    for K in (0, 1, 5, 15, 16, 17, 31, 32, 33):
        assert "sgns-K%d" % K in names
    for L in (1, 2, 16, 17, 33, 768, 769, 1537, 3073, 6145, 12288):
        assert ref.CASES["sgns-L%d" % L].L == L and ref.CASES["sgns-L%d" % L].W == 1
    assert all(c.row0 > 0 for c in ref.CASES.values())


@pytest.mark.parametrize("name", list(ref.CASES))
def test_input_conditions(readings, name):
    c = ref.CASES[name]
    f, d = readings[name]
    print(name, {k: f[k] for k in ("pairs", "negatives", "skipped", "wins", "ties", "lo", "hi", "loss")})
    if "empty" in c.tags:
        assert (f["pairs"], f["negatives"], f["skipped"]) == (0, 0, 0) and math.isnan(f["auc"]) and math.isnan(f["loss"])
        return
    assert f["pairs"] > 0 and -16 <= f["lo"] < 0 < f["hi"] <= 16                 # scores in a narrow range around 0, in quarter steps
    if c.entry == "sgns":
        assert f["pairs"] * c.K == f["negatives"] + f["skipped"]
        lens = ref.sgns_pairs(c.walks(), c.W, ref.host_map(ref.vocabulary(ref.world_counts())[0], ref.NV)).lens
        assert (lens < c.L).any() or c.L == 1                                     # the packed length differs from max_len somewhere
        if c.K == 0:
            assert f["negatives"] == 0 and math.isnan(f["auc"]) and f["loss"] == f["s_pos"] / f["pairs"]
            return
    if "all-ties" in c.tags:
        assert f["ties"] == f["negatives"] > 0 and f["auc"] == 0.5 and f["skipped"] > 0
        return
    assert f["skipped"] > 0 and f["ties"] > 0 and f["wins"] > 0 and f["negatives"] - f["wins"] - f["ties"] > 0
    if c.entry == "sgns":
        lanes = {int(k) % 16 for k in np.flatnonzero(d.valid.any(0))}
        assert lanes == set(range(min(c.K, 16)))                                   # every lane of a batch takes a scored negative somewhere
        if c.K >= 16:
            assert (~d.valid)[:, :16 * (c.K // 16)].any()                         # a skip inside a full batch
        if "L" in c.tags and c.L > 16:
            assert len(np.unique(lens)) > 1 or c.n == 1                           # uneven packed lengths across the 16-token rounds


def test_the_odd_slice_width_reaches_beyond_n_vertices(world):
    for name, some_inside in (("links-R48", True), ("links-R1000", True)):
        c = ref.CASES[name]
        w = c.walks().astype(np.int64)
        a, b = w[:, :-1], w[:, 1:]
        g = (np.uint64(c.row0) + np.arange(c.n, dtype=np.uint64))[:, None]; j = np.arange(c.L - 1, dtype=np.uint64)[None, :]
        r = (np.maximum(b, 0) // c.R) * c.R + (ref.mix64(np.uint64(c.seed) + g * np.uint64(c.L) + j).reshape(c.n, c.L - 1) % np.uint64(c.R)).astype(np.int64)
        cand = (a >= 0) & (b >= 0) & (ref.look(world["remap"], a) >= 0) & (ref.look(world["remap"], b) >= 0)
        assert (r[cand] >= ref.NV).any() and (r[cand] < ref.NV).any()
    assert ref.NV % 48 != 0 and 1000 > ref.NV


# ------------------------------------------------------------------------------------------------ sensitivity
def differs(c, f, g):
    """Would the device test of builder c, expecting f, fail on a device that returned g?"""
    if any(f[k] != g[k] for k in ("pairs", "negatives", "skipped", "w2")):
        return True
    if math.isnan(f["loss"]) or math.isnan(g["loss"]):
        return math.isnan(f["loss"]) != math.isnan(g["loss"])
    return abs(f["loss"] - g["loss"]) > ref.loss_tolerance(f["terms"]) * f["loss"]


def _with(f, **kw):
    g = dict(f); g.update(kw)
    g["w2"] = 2 * g["wins"] + g["ties"]
    if g["pairs"]:
        g["loss"] = g["s_pos"] / g["pairs"] + g["s_neg"] / g["negatives"] if kw.get("form") == "links" else (g["s_pos"] + g["s_neg"]) / g["pairs"]
    return g


def mutants(c, f, d, world):
    """name -> the figures a device with that slip would return; only the slips that can touch this builder's call (the reasons stand beside each)."""
    vid, table, remap = world["vid"], world["table"], world["remap"]
    out = {}
    if c.entry == "links":
        out["a tie counted as a win"] = dict(f, w2=2 * (f["wins"] + f["ties"]))
        if c.R > 1:                                      # regions_per_slice = 1: the draw is mix64(..) % 1 = 0 whatever g is
            ra, rb, rr, sk = ref.links(c.walks(), 0, c.R, c.seed, remap)
            S0, S1 = c.tables(len(vid))
            g = ref.figures(S0, S1, ref.SHIFT, "links", rb, ra, rr, ra, np.arange(len(ra))); g["skipped"] = sk
            out["g taken without row0"] = g
        return out
    S0, S1 = c.tables(len(vid))
    w = c.walks()

    def fig(dd):
        g = ref.sgns_figures(S0, S1, dd); g["skipped"] = int((~dd.valid).sum())
        return g
    if "wide" not in c.tags:                             # cfg.window >= max_len - 1: the header's rule gives the pairs of every smaller window >= n - 1 too
        out["window one short"] = fig(ref.sgns(w, c.row0, c.W - 1, c.K, c.seed, remap, table))
    if c.K % 16 == 0:                                    # (K = 0 included: the same trailing branch takes the positive's term)
        out["the positive's term dropped when K % 16 == 0"] = _with(f, s_pos=0.0)
        out["the positive's term added twice when K % 16 == 0"] = _with(f, s_pos=2.0 * f["s_pos"])
    if c.K == 0:                                         # no draw, no negative: nothing else to slip on
        return out
    out["the row == row(t_i) skip dropped"] = fig(d._replace(valid=np.ones_like(d.valid)))
    out["a tie counted as a win"] = dict(f, w2=2 * (f["wins"] + f["ties"]))
    if c.K >= 16:
        neg = d.neg.copy()
        for k0 in range(0, c.K - 15, 16):
            neg[:, k0 + 15] = neg[:, k0]
        out["the last negative of a full batch scored against the first's row"] = fig(d._replace(neg=neg, valid=neg != d.ctr[:, None]))
    out["g taken without row0"] = fig(ref.sgns(w, 0, c.W, c.K, c.seed, remap, table))
    if c.L == 2:                                         # a walk of two tokens that forms a pair is whole: its packed length IS max_len
        return out
    p = ref.sgns_pairs(w, c.W, remap)
    out["max_len replaced by the packed length in the draw index"] = fig(ref.sgns_draws(p, c.row0, p.lens[p.gi], c.K, c.seed, table))
    return out


@pytest.mark.parametrize("name", [n for n, c in ref.CASES.items() if "empty" not in c.tags])
def test_every_builder_tells_every_slip_apart(readings, world, name):
    c = ref.CASES[name]
    f, d = readings[name]
    ms = mutants(c, f, d, world)
    assert ms
    missed = [m for m, g in ms.items() if not differs(c, f, g)]
    assert not missed, (name, missed)
    assert not differs(c, f, dict(f))


def test_every_slip_is_tried_somewhere(readings, world):
    seen = {}
    for name, c in ref.CASES.items():
        if "empty" not in c.tags and c.L <= 33:
            for m in mutants(c, *readings[name], world):
                seen.setdefault(m, []).append(name)
    print({m: len(v) for m, v in seen.items()})
    assert len(seen) == 8
    assert "sgns-K0" in seen["the positive's term dropped when K % 16 == 0"] and "sgns-K32" in seen["the positive's term added twice when K % 16 == 0"]
    assert "sgns-far-row0" in seen["g taken without row0"] and "links-R48" in seen["g taken without row0"]


def test_wide_windows_are_told_from_narrow_ones(readings, world):
    """W = L and W = L + 7 give the figures of W = L - 1 by the rule itself; what those two cases pin is that the window is not cut short."""
    for name in ("sgns-L17-W17", "sgns-L17-W24"):
        c = ref.CASES[name]
        f, _ = readings[name]
        S0, S1 = c.tables(len(world["vid"]))
        short = ref.sgns(c.walks(), c.row0, 10, c.K, c.seed, world["remap"], world["table"])
        assert ref.sgns_figures(S0, S1, short)["pairs"] < f["pairs"]
        assert readings["sgns-L17-W17"][0]["pairs"] == readings["sgns-L17-W24"][0]["pairs"]
