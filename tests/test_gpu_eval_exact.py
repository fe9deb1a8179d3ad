"""GPU: held-out evaluation (csrc/eval.hip) on PLANTED tables — exact figures across K, row widths, walk lengths and the geometry's edges.

Models are created from a synthetic count vector and never trained; both tables are written whole through dge_model_import_partition with the lattice of
tests/eval_ref.py (small integers times 2^-1, a few to a row), on which every dot product is an exact float32 in any association order.  The expected
figures come from the named builders of eval_ref.CASES, whose inputs tests/test_eval_ref.py has shown to be sensitive: scores from int64 matrix
products, wins / ties / skips as Python ints, the loss by math.fsum over longdouble softplus terms.  The unigram table is the model's own
(dge_model_table), as the header names it.

Every integer figure is compared with ==, and so is auc as a double.  The ONLY tolerance of this file is eval_ref.loss_tolerance (derived there: scores
are exact, so no gamma_D term; 4 ulp a term for the device's exp and log1p — an allowance, the installed HIP documentation states no bound —, half an
ulp for softplus's own addition, terms * 2^-52 for the summation, 2 ulp for the final quotients and the reference's rounding).  Every case prints the
observed |dev - ref| / ref beside that bound.  No test asserts a time."""
import math

import numpy as np
import pytest

import eval_ref as ref
import helpers

pytestmark = pytest.mark.gpu


class World:
    def __init__(self, dge):
        import torch
        self.dge = dge
        self.counts_host = ref.world_counts()
        self.counts = torch.from_numpy(self.counts_host).to("cuda:0")
        self.vid, _ = ref.vocabulary(self.counts_host)
        self.V = len(self.vid)
        self.models = {}

    def plant(self, m, S0, S1, shift):
        import torch
        stride = m.partition_floats(1) // self.V
        assert stride % 64 == 0 and stride >= S0.shape[1] and m.partition_floats(1) == self.V * stride
        for t, S in ((0, S0), (1, S1)):
            buf = np.zeros((self.V, stride), np.float32)
            buf[:, :S.shape[1]] = S * 2.0 ** -shift
            m.import_partition(t, 1, 0, torch.from_numpy(buf).to(m.torch_device))
        return stride

    def model(self, dim, W=5, K=5, use_hs=False, tables="lattice"):
        """A model of this world's vocabulary, planted (tables = "lattice": eval_ref.lattice(V, dim, 1), what Case.tables gives) fresh (None), or fresh for the caller to plant ("witness"); kept."""
        key = (dim, W, K, use_hs, tables)
        if key not in self.models:
            cfg = self.dge.make_config(dim, W, ref.NV, negative=K, min_count=ref.MIN_COUNT, seed=1, table_size=ref.TABLE_SIZE, use_hs=use_hs)
            m = self.dge.SgnsModel.create(cfg, self.counts, 0)
            _, vid = m.vectors()
            assert np.array_equal(vid, self.vid)                      # the vocabulary's order is the one eval_ref.vocabulary states
            if tables == "lattice":
                S0, S1 = ref.lattice(self.V, dim, seed=1)
                ref.check_exact(S0, S1)
                self.plant(m, S0, S1, ref.SHIFT)
            self.models[key] = m
        return self.models[key]


@pytest.fixture(scope="module")
def world(dge):
    w = World(dge)
    yield w
    for m in w.models.values():
        m.close()


def w2(r):
    return int(np.rint(2.0 * r["auc"] * r["negatives"]))             # 2 x wins + ties: an integer


def check(name, res, exp):
    """One device result against the expected figures: integers and auc with ==, the loss within the derived tolerance."""
    print(name, {k: res[k] for k in ("pairs", "negatives", "skipped", "auc", "loss")}, "kernel %.3f ms" % res["kernel_ms"])
    assert (res["pairs"], res["negatives"], res["skipped"]) == (exp["pairs"], exp["negatives"], exp["skipped"]), name
    if exp["negatives"] == 0:
        assert math.isnan(res["auc"]), name
    else:
        assert w2(res) == exp["w2"], name
        assert res["auc"] == exp["auc"], name
    if exp["pairs"] == 0:
        assert math.isnan(res["loss"]), name
        return
    tol = ref.loss_tolerance(exp["terms"])
    rel = abs(res["loss"] - exp["loss"]) / exp["loss"]
    print("%s: loss dev %.17g ref %.17g  |dev - ref| / ref = %.3g  (bound %.3g over %d terms)" % (name, res["loss"], exp["loss"], rel, tol, exp["terms"]))
    assert rel <= tol, name


def run(world, c, first=0, count=None, use_hs=False):
    m = world.model(c.dim, c.W, c.K, use_hs=use_hs)
    corpus = world.dge.WalkCorpus.from_host(c.corpus(), 0)
    count = c.n - first if count is None else count
    if c.entry == "links":
        res = m.eval_links(corpus, c.R, seed=c.seed, row0=c.row0 + first, n_rows=count)
    else:
        res = m.eval_sgns(corpus, seed=c.seed, row0=c.row0 + first, n_rows=count)
    exp = c.reference(world.vid, m.table(), first, count)
    corpus.close()
    return res, exp


# ------------------------------------------------------------------------------------------------ the planting itself
@pytest.mark.parametrize("dim", [20, 64, 320, 512])
def test_planted_tables_are_what_the_device_holds(world, dim):
    import torch
    m = world.model(dim)
    S0, S1 = ref.lattice(world.V, dim, seed=1)
    stride = m.partition_floats(1) // world.V
    assert stride == {20: 64, 64: 64, 320: 384, 512: 512}[dim]
    for t, S in ((0, S0), (1, S1)):
        if stride == -(-dim // 64) * 64:
            got = helpers.device_table(m, t).cpu().numpy()
        else:                                                            # (helpers.device_table takes the stride for dim rounded up to 64: 320 floats lie in rows of 384)
            buf = torch.empty(world.V * stride, dtype=torch.float32, device=m.torch_device)
            m.export_partition(t, 1, 0, buf)
            got = buf.view(-1, stride).cpu().numpy()
        assert got.shape == (world.V, stride)
        assert np.array_equal(got[:, :dim], (S * 0.5).astype(np.float32)) and not got[:, dim:].any()
    table = m.table()
    mine = ref.unigram_table(ref.vocabulary(world.counts_host)[1])
    print("dim %d: the model's unigram table and numpy's differ in %d of %d slots" % (dim, int((table != mine).sum()), len(table)))
    assert len(table) == ref.TABLE_SIZE and table.min() == 0 and table.max() == world.V - 1 and (np.diff(table) >= 0).all()


# ------------------------------------------------------------------------------------------------ score_pairs: a column witness for every width
@pytest.mark.parametrize("dim", [1, 20, 64, 65, 128, 200, 256, 257, 320, 448, 512])
def test_column_witness_and_lattice_scores(world, dim):
    import torch
    m = world.model(dim, tables="witness")
    S0, S1 = ref.witness(world.V, dim, seed=2)
    ref.check_exact(S0, S1, lattice_only=False)
    world.plant(m, S0, S1, 0)
    G = S0 @ S1.T
    vid = world.vid.astype(np.int64)

    def scores(ctx, tgt):
        c = torch.from_numpy(np.ascontiguousarray(ctx, np.int32)).to(m.torch_device); t = torch.from_numpy(np.ascontiguousarray(tgt, np.int32)).to(m.torch_device)
        return m.score_pairs(c, t).cpu().numpy()
    got = scores(vid[:dim], np.full(dim, vid[0]))
    wrong = np.flatnonzero(got != np.arange(1, dim + 1, dtype=np.float32))
    assert len(wrong) == 0, "score(e_j, ramp) != j + 1 at columns %s: got %s" % (wrong[:16], got[wrong[:16]])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(dim)
    below = np.flatnonzero(world.counts_host < ref.MIN_COUNT)
    for n in (1, 17, 8 * cus * 16 * 2 + 333):                          # the last: every group of the grid takes a third pair (the stride loop runs twice and more)
        rc, rt = rng.integers(0, world.V, n), rng.integers(0, world.V, n)
        ctx, tgt = vid[rc], vid[rt]
        bad = np.zeros(n, bool)
        if n >= 17:
            ctx[2:7] = (-1, ref.NV, ref.NV + 3, below[0], 2 ** 31 - 1); tgt[9:12] = (-1, ref.NV, below[-1]); bad[2:7] = bad[9:12] = True
            ctx[n - 1] = -7; bad[n - 1] = True
        got = scores(ctx, tgt)
        assert got.shape == (n,) and np.array_equal(np.isnan(got), bad), n
        assert np.array_equal(got[~bad], G[rc, rt][~bad].astype(np.float32)), n        # bit-equal to the integer product (no -0.0: the sums start from +0)
        assert not np.signbit(got[~bad][got[~bad] == 0]).any()


# ------------------------------------------------------------------------------------------------ eval_sgns and eval_links by named builder
@pytest.mark.parametrize("name", list(ref.CASES))
def test_builder(world, name):
    res, exp = run(world, ref.CASES[name])
    check(name, res, exp)
    c = ref.CASES[name]
    if "all-ties" in c.tags:
        # regions_per_slice = 1: r = b, pos == neg on every step.  The loss of a step is softplus(-s) + softplus(s) = |s| + 2 log1p(exp(-|s|)): 2 ln 2 where the
        # score is 0 (test_a_fresh_model_ties_every_score asserts that value) and more on a planted model, whose exact figure `check` has just compared
        assert res["auc"] == 0.5 and w2(res) == res["negatives"] > 0 and res["loss"] > 2.0 * math.log(2.0)
    if c.entry == "sgns" and c.K == 0:
        assert res["negatives"] == 0 and res["pairs"] > 0


def test_walks_beyond_12288_tokens_are_refused(world, dge):
    m = world.model(64, 1, 5)
    corpus = dge.WalkCorpus.from_host(np.zeros((2, 12289), np.int32), 0)
    with pytest.raises(dge.DgeError) as ei:
        m.eval_sgns(corpus)
    assert ei.value.code == 1 and "12288" in str(ei.value)


@pytest.mark.parametrize("name", ["sgns-K17", "sgns-K32", "links-dim64"])
def test_halves_add_up(world, name):
    c = ref.CASES[name]
    h = c.n // 2 + 1
    (a, ea), (p, ep), (q, eq) = run(world, c), run(world, c, 0, h), run(world, c, h, c.n - h)
    for tag, r, e in (("whole", a, ea), ("first", p, ep), ("second", q, eq)):
        check("%s %s" % (name, tag), r, e)
    for k in ("pairs", "negatives", "skipped"):
        assert a[k] == p[k] + q[k] and p[k] > 0 and q[k] > 0, k
    assert w2(a) == w2(p) + w2(q)
    if c.entry == "sgns":                                                 # loss * pairs is the sum of the terms
        whole, parts = a["loss"] * a["pairs"], p["loss"] * p["pairs"] + q["loss"] * q["pairs"]
        bound = ref.loss_tolerance(ea["terms"]) * whole + ref.loss_tolerance(ep["terms"]) * p["loss"] * p["pairs"] + ref.loss_tolerance(eq["terms"]) * q["loss"] * q["pairs"]
        print("%s: sum of halves off by %.3g relative (bound %.3g)" % (name, abs(whole - parts) / whole, bound / whole))
        assert abs(whole - parts) <= bound


# ------------------------------------------------------------------------------------------------ special models
def test_a_fresh_model_ties_every_score(world):
    """Not planted: syn1neg = 0, every score is +0 whatever syn0 holds."""
    m = world.model(64, tables=None, K=17)
    assert not helpers.device_table(m, 1).any().item() and helpers.device_table(m, 0).any().item()
    ln2 = math.log(2.0)
    for name in ("links-dim64", "links-R1", "sgns-K17"):
        c = ref.CASES[name]
        exp = c.reference(world.vid, m.table())
        corpus = world.dge.WalkCorpus.from_host(c.corpus(), 0)
        res = m.eval_links(corpus, c.R, seed=c.seed, row0=c.row0) if c.entry == "links" else m.eval_sgns(corpus, seed=c.seed, row0=c.row0)
        corpus.close()
        assert (res["pairs"], res["negatives"], res["skipped"]) == (exp["pairs"], exp["negatives"], exp["skipped"]) and res["pairs"] > 0
        assert res["auc"] == 0.5 and w2(res) == res["negatives"]
        want = 2.0 * ln2 if c.entry == "links" else (res["pairs"] + res["negatives"]) * ln2 / res["pairs"]
        rel = abs(res["loss"] - want) / want
        print("%s, fresh: loss dev %.17g ref %.17g  |dev - ref| / ref = %.3g  (bound %.3g)" % (name, res["loss"], want, rel, ref.loss_tolerance(exp["terms"])))
        assert rel <= ref.loss_tolerance(exp["terms"])


def test_a_hierarchical_softmax_model_gives_its_plain_twin_s_figures(world):
    """include/dge.h: a use_hs model is evaluated on syn0 / syn1neg like any other; the tree term is not scored."""
    for name in ("links-dim64", "sgns-K17", "sgns-dim320"):
        c = ref.CASES[name]
        (plain, exp), (hs, _) = run(world, c), run(world, c, use_hs=True)
        check(name + " use_hs", hs, exp)
        for k in ("pairs", "negatives", "skipped", "auc", "loss"):
            assert np.float64(plain[k]).view(np.int64) == np.float64(hs[k]).view(np.int64), (name, k)
