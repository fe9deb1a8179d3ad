"""GPU: held-out evaluation on the device (include/dge.h: dge_model_score_pairs, dge_model_eval_links, dge_model_eval_sgns; csrc/eval.hip).

Models are trained on the device; the references are float64 numpy over the tables read back with vectors() / syn1neg(), and restatements of the
header's draw rules (splitmix64 in wrapping uint64 arithmetic).  Bounds:
  * a score: |dev - ref| <= gamma_D * sum_i |x_i y_i|, gamma_D = D u / (1 - D u), u = 2^-24 — an f32 dot product in any association order, fused or not;
  * counts, and the AUC (integer wins and ties over the f32 scores the device itself returns through score_pairs): exact;
  * a loss over n softplus terms of those same f32 scores: relative 2 n 2^-52 (n positive doubles summed in any order, doubled for the few-ulp log1p(exp)).
No test asserts a time."""
import math

import numpy as np
import pytest

import helpers
from eval_ref import host_map, look, mix64      # the draw rules' plain-numpy pieces live in tests/eval_ref.py

pytestmark = pytest.mark.gpu

U64 = np.uint64


def softplus(x):
    return np.logaddexp(0.0, np.asarray(x, np.float64))


def gamma(D):
    u = 2.0 ** -24
    return D * u / (1.0 - D * u)


def dev_scores(m, ctx, tgt):
    import torch
    c = torch.from_numpy(np.ascontiguousarray(ctx, np.int32)).to(m.torch_device); t = torch.from_numpy(np.ascontiguousarray(tgt, np.int32)).to(m.torch_device)
    return m.score_pairs(c, t).cpu().numpy()


def auc_of(wins, ties, n):
    return (float(wins) + 0.5 * float(ties)) / float(n)


def links_restate(walks, row0, R, seed, remap):
    """include/dge.h, dge_model_eval_links -> (a, b, r) of the scored steps, skipped."""
    n, L = walks.shape
    g = (U64(row0) + np.arange(n, dtype=U64))[:, None]; j = np.arange(L - 1, dtype=U64)[None, :]
    a = walks[:, :-1].astype(np.int64); b = walks[:, 1:].astype(np.int64)
    h = mix64(U64(seed) + g * U64(L) + j).reshape(n, L - 1)
    r = (np.maximum(b, 0) // R) * R + (h % U64(R)).astype(np.int64)
    cand = (a >= 0) & (b >= 0)
    a, b, r = a[cand], b[cand], r[cand]
    ok = (look(remap, a) >= 0) & (look(remap, b) >= 0) & (look(remap, r) >= 0)
    return a[ok], b[ok], r[ok], int((~ok).sum())


def sgns_restate(walks, row0, W, K, seed, remap, table):
    """include/dge.h, dge_model_eval_sgns -> centre rows [P], context rows [P], negative rows [P x K], which negatives are scored [P x K]."""
    n, L = walks.shape
    rows = look(remap, walks)
    keep = rows >= 0
    order = np.argsort(~keep, axis=1, kind="stable")                     # left-pack, order kept
    packed = np.take_along_axis(rows, order, 1); lens = keep.sum(1)
    gi, ii, cc = np.meshgrid(np.arange(n), np.arange(L), np.arange(L), indexing="ij")
    ok = (ii < lens[gi]) & (cc < lens[gi]) & (ii != cc) & (np.abs(ii - cc) <= W)
    gi, ii, cc = gi[ok], ii[ok], cc[ok]
    ctr = packed[gi, ii]; ctx = packed[gi, cc]
    base = (((U64(row0) + gi.astype(U64)) * U64(L) + ii.astype(U64)) * U64(L) + cc.astype(U64)) * U64(K)
    slots = mix64(U64(seed) + base[:, None] + np.arange(K, dtype=U64)[None, :]).reshape(len(base), K) % U64(len(table))
    neg = table[slots.astype(np.int64)].astype(np.int64)
    return ctr, ctx, neg, neg != ctr[:, None]


class Small:
    """A layered graph with dead ends (walks are padded) and a min_count that drops the rarest vertices (held-out walks carry tokens outside the vocabulary)."""
    R, T = 40, 4

    def __init__(self, dge, L, n_train=4000, n_test=2000):
        import torch
        self.dge, self.L, self.NV = dge, L, self.R * self.T
        src, dst, w, sources = helpers.layered_graph(self.R, self.T, deg=6, seed=11, dead_ends=0.2)
        g = dge.DeviceGraph(0); g.add_edges(src, dst, w); g.set_sources(sources); g.build_alias(True)
        self.n_train, self.n_test = n_train, n_test
        self.walks = np.concatenate([g.sample_walks(n_train, L, seed=5, rng_mode=1), g.sample_walks(n_test, L, seed=99, rng_mode=1)])
        self.corpus = dge.WalkCorpus.from_host(self.walks, 0)
        self.counts = torch.zeros(self.NV, dtype=torch.int64, device="cuda:0")
        self.corpus.count_tokens(self.NV, self.counts, 0, n_train)
        c = self.counts.cpu().numpy()
        self.min_count = int(np.percentile(c[c > 0], 15)) + 1
        assert 0 < (c >= self.min_count).sum() < (c > 0).sum() and (self.walks < 0).any()

    def model(self, dim, window=None, workers=0, train=True, negative=5, seed=1):
        cfg = self.dge.make_config(dim, window or self.L, self.NV, negative=negative, min_count=self.min_count, workers=workers, seed=seed, table_size=1_000_000)
        m = self.dge.SgnsModel.create(cfg, self.counts, 0)
        if train:
            for _ in range(3):      # a few passes: scores well away from zero
                m.train(self.corpus, 0, self.n_train, total_walks=self.n_train)
        return m

    @property
    def test_walks(self):
        return self.walks[self.n_train:]


@pytest.fixture(scope="module")
def small8(dge):
    return Small(dge, 8)


@pytest.fixture(scope="module")
def small24(dge):
    return Small(dge, 24)


def test_mix64_restatement(oracle):
    for x in (0, 1, 0xFFFFFFFFFFFFFFFF - 5):
        assert int(mix64(x)[0]) == oracle.mix64(x)


# ------------------------------------------------------------------------------------------------ 1. scores
@pytest.mark.parametrize("dim", [20, 64, 128, 200, 256])
def test_scores_against_float64(small8, dim):
    s = small8
    m = s.model(dim)
    s0, vid = m.vectors(); s1 = m.syn1neg()
    remap = host_map(vid, s.NV)
    rng = np.random.default_rng(dim)
    ctx = rng.integers(-2, s.NV + 6, 4000); tgt = rng.integers(-2, s.NV + 6, 4000)
    ctx[:4] = (-1, s.NV, 0, 2 ** 31 - 1); tgt[:4] = (0, 0, -1, 0)
    below = np.flatnonzero(remap < 0)
    assert len(below)
    ctx[4:4 + len(below)] = below                   # ids below min_count
    got = dev_scores(m, ctx, tgt)
    rc, rt = look(remap, ctx), look(remap, tgt)
    bad = (rc < 0) | (rt < 0)
    assert bad.any() and not bad.all()
    assert np.array_equal(np.isnan(got), bad)
    x = s0[rc[~bad]].astype(np.float64); y = s1[rt[~bad]].astype(np.float64)
    ref = (x * y).sum(1); mag = np.abs(x * y).sum(1)
    err = np.abs(got[~bad].astype(np.float64) - ref)
    print("dim %d: max |dev - ref| / (gamma sum|xy|) = %.3f, largest |score| %.3f" % (dim, (err / np.maximum(gamma(dim) * mag, 1e-300)).max(), np.abs(ref).max()))
    assert np.abs(ref).max() > 0.01                 # a trained model: the scores are not all zero
    assert (err <= gamma(dim) * mag).all()


# ------------------------------------------------------------------------------------------------ 2. links
def _links_host(m, s, walks, row0, seed):
    _, vid = m.vectors()
    a, b, r, skipped = links_restate(walks, row0, s.R, seed, host_map(vid, s.NV))
    pos = dev_scores(m, b, a); neg = dev_scores(m, r, a)
    return pos, neg, skipped


@pytest.mark.parametrize("dim", [64, 200])
def test_links_against_the_restatement(small8, dim):
    s = small8
    m = s.model(dim)
    res = m.eval_links(s.corpus, s.R, seed=3, row0=s.n_train)
    pos, neg, skipped = _links_host(m, s, s.test_walks, s.n_train, 3)
    n = len(pos)
    print(res, n, skipped)
    assert skipped > 0 and n > 1000
    assert (res["pairs"], res["negatives"], res["skipped"]) == (n, n, skipped)
    assert res["auc"] == auc_of((pos > neg).sum(), (pos == neg).sum(), n)
    ref = math.fsum(softplus(-pos)) / n + math.fsum(softplus(neg)) / n
    print("loss dev %.17g ref %.17g rel %.3g" % (res["loss"], ref, abs(res["loss"] - ref) / ref))
    assert abs(res["loss"] - ref) <= 2 * (2 * n) * 2.0 ** -52 * ref


# ------------------------------------------------------------------------------------------------ 3. determinism, additivity
def _strip(r):
    return {k: v for k, v in r.items() if k != "kernel_ms"}


def test_two_calls_agree_bit_for_bit_and_halves_add_up(small24):
    s = small24
    m = s.model(128)
    n = s.n_test; h = n // 2
    for name, call in (("links", lambda r0, k: m.eval_links(s.corpus, s.R, seed=7, row0=r0, n_rows=k)),
                       ("sgns", lambda r0, k: m.eval_sgns(s.corpus, seed=7, row0=r0, n_rows=k))):
        a, b = call(s.n_train, n), call(s.n_train, n)
        assert np.array_equal(np.array(list(_strip(a).values()), np.float64).view(np.int64), np.array(list(_strip(b).values()), np.float64).view(np.int64)), (a, b)
        assert isinstance(a["pairs"], int) and a["pairs"] > 1000
        p, q = call(s.n_train, h), call(s.n_train + h, n - h)
        for k in ("pairs", "negatives", "skipped"):
            assert a[k] == p[k] + q[k], (name, k)
        w2 = lambda r: int(np.rint(2.0 * r["auc"] * r["negatives"]))          # 2 x wins + ties: an integer
        assert w2(a) == w2(p) + w2(q), name
        terms = a["pairs"] + a["negatives"]
        whole, parts = a["loss"] * a["pairs"], p["loss"] * p["pairs"] + q["loss"] * q["pairs"]
        print(name, a, "sum of halves off by %.3g relative" % (abs(whole - parts) / whole))
        assert abs(whole - parts) <= 2 * terms * 2.0 ** -52 * whole, name


# ------------------------------------------------------------------------------------------------ 4. against helpers.link_auc_device, 7. it measures learning
@pytest.fixture(scope="module")
def big(dge):
    import torch
    from embedding_amd import synth
    R, T, L, D = 2000, 24, 24, 128
    NV = R * T
    G = synth.flow_graph_torch(R, T, 30, "cuda:0", dst="community")
    g = dge.DeviceGraph(0); g.add_edges_device(G["src"], G["dst"], G["w"]); g.set_sources(G["sources"]); del G
    g.build_alias(False)
    n_train, n_test = 200_000, 10_000
    corpus = g.sample_walks_device(n_train, L, seed=5)
    test = g.sample_walks_device(n_test, L, seed=99)
    counts = torch.zeros(NV, dtype=torch.int64, device="cuda:0"); corpus.count_tokens(NV, counts)
    cfg = dge.make_config(D, L, NV, negative=5, workers=0, seed=1, table_size=10_000_000)
    fresh = dge.SgnsModel.create(cfg, counts, 0)
    m = dge.SgnsModel.create(cfg, counts, 0)
    m.train(corpus, 0, n_train, total_walks=n_train)
    return dict(R=R, NV=NV, L=L, m=m, fresh=fresh, test=test, corpus=corpus)


def test_links_agree_with_the_torch_yardstick(big):
    import torch
    m, test, R, NV = big["m"], big["test"], big["R"], big["NV"]
    res = m.eval_links(test, R, seed=3)
    _, vid = m.vectors()
    tw_host = test.to_host()
    tw = torch.from_numpy(tw_host.astype(np.int64)).to(m.torch_device)
    auc_t, loss_t = helpers.link_auc_device(m, vid, tw, R, NV, seed=3)
    steps = res["pairs"]
    assert steps >= 200_000
    # the variance of a step's loss term, from the scores of this entry's own draws
    a, b, r, _ = links_restate(tw_host, 0, R, 3, host_map(vid, NV))
    assert len(a) == steps
    term = softplus(-dev_scores(m, b, a)) + softplus(dev_scores(m, r, a))
    tol_auc = 5.0 * math.sqrt(0.5 / steps); tol_loss = 5.0 * math.sqrt(2.0 * term.var() / steps)
    print("steps %d: auc %.5f vs %.5f (tolerance %.5f), loss %.5f vs %.5f (tolerance %.5f), kernel %.3f ms" % (steps, res["auc"], auc_t, tol_auc, res["loss"], loss_t, tol_loss, res["kernel_ms"]))
    assert abs(res["auc"] - auc_t) < tol_auc
    assert abs(res["loss"] - loss_t) < tol_loss


def test_training_lowers_the_held_out_loss_and_raises_the_auc(big):
    m, fresh, test, R = big["m"], big["fresh"], big["test"], big["R"]
    before, after = fresh.eval_sgns(test, seed=3, n_rows=2000), m.eval_sgns(test, seed=3, n_rows=2000)
    lb, la = fresh.eval_links(test, R, seed=3), m.eval_links(test, R, seed=3)
    print("sgns loss %.4f -> %.4f (auc %.4f -> %.4f); link auc %.4f -> %.4f" % (before["loss"], after["loss"], before["auc"], after["auc"], lb["auc"], la["auc"]))
    assert before["pairs"] == after["pairs"] > 0
    assert after["loss"] < before["loss"]
    assert la["auc"] > lb["auc"]


# ------------------------------------------------------------------------------------------------ 5. the SGNS objective
@pytest.mark.parametrize("L,window", [(8, 3), (24, 24)])
def test_sgns_objective_against_the_restatement(small8, small24, L, window):
    s = small8 if L == 8 else small24
    D, K = 64, 5
    m = s.model(D, window=window, negative=K)
    s0, vid = m.vectors(); s1 = m.syn1neg()
    table = m.table()
    assert len(table) == 1_000_000
    res = m.eval_sgns(s.corpus, seed=3, row0=s.n_train)
    ctr, ctx, neg, valid = sgns_restate(s.test_walks, s.n_train, window, K, 3, host_map(vid, s.NV), table)
    P = len(ctr)
    print(res, P, int(valid.sum()), int((~valid).sum()))
    assert P > 10_000 and (~valid).any()
    assert (res["pairs"], res["negatives"], res["skipped"]) == (P, int(valid.sum()), int((~valid).sum()))
    # the device's own f32 scores: a table of every (context row, target row) through score_pairs
    V = len(vid)
    cc, tt = np.meshgrid(np.arange(V), np.arange(V), indexing="ij")
    S = dev_scores(m, vid[cc.reshape(-1)], vid[tt.reshape(-1)]).reshape(V, V)
    pos = S[ctx, ctr]; ng = S[ctx[:, None], neg]
    wins = ((pos[:, None] > ng) & valid).sum(); ties = ((pos[:, None] == ng) & valid).sum()
    assert res["auc"] == auc_of(wins, ties, valid.sum())
    # float64 over the tables read back; a term moves by at most its score's error (softplus is 1-Lipschitz)
    X, Y = s0.astype(np.float64), s1.astype(np.float64)
    S64 = X @ Y.T; A64 = np.abs(X) @ np.abs(Y).T
    ref = (softplus(-S64[ctx, ctr]).sum() + (softplus(S64[ctx[:, None], neg]) * valid).sum()) / P
    slack = gamma(D) * (A64[ctx, ctr].sum() + (A64[ctx[:, None], neg] * valid).sum()) / P + 2 * (P + int(valid.sum())) * 2.0 ** -52 * ref
    print("loss dev %.12g ref %.12g |diff| %.3g bound %.3g" % (res["loss"], ref, abs(res["loss"] - ref), slack))
    assert abs(res["loss"] - ref) <= slack


# ------------------------------------------------------------------------------------------------ 6. reads only
def _state(m):
    return [helpers.device_table(m, t).clone().view(-1).view(__import__("torch").int32) for t in (0, 1)], m.stats(), m.schedule()


def test_the_entries_only_read(small8):
    import torch
    s = small8
    m = s.model(64)
    ids = torch.arange(-1, s.NV + 1, dtype=torch.int32, device=m.torch_device)
    for call in (lambda: m.score_pairs(ids, ids.flip(0)), lambda: m.eval_links(s.corpus, s.R, row0=s.n_train), lambda: m.eval_sgns(s.corpus, row0=s.n_train)):
        tabs, st, sch = _state(m)
        call()
        tabs2, st2, sch2 = _state(m)
        assert torch.equal(tabs[0], tabs2[0]) and torch.equal(tabs[1], tabs2[1])
        assert st == st2 and sch == sch2


def test_an_evaluation_between_two_launches_leaves_the_training_as_it_was(small8):
    """The trainer keeps the compacted form of the corpus rows it trained last and skips the compaction when the same rows come again: an evaluation
    that borrowed those buffers would make the second launch train the held-out rows.  workers = 1: the in-order schedule, bit-reproducible."""
    import torch
    s = small8
    out = []
    for evaluate in (True, False):
        m = s.model(64, workers=1, train=False)
        m.train(s.corpus, 0, s.n_train, total_walks=s.n_train)
        if evaluate:
            a = m.eval_sgns(s.corpus, row0=s.n_train); b = m.eval_links(s.corpus, s.R, row0=s.n_train)
            assert a["pairs"] > 0 and b["pairs"] > 0
        m.train(s.corpus, 0, s.n_train, total_walks=s.n_train)
        out.append([helpers.device_table(m, t).clone().view(-1).view(torch.int32) for t in (0, 1)])
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_cpp_mirror_prints_a_held_out_figure(tmp_path, dge):
    """embedding_amd/host/embedding_host.hpp: DeepWalk::learnEmbedding with held-out .seq files (tests/native/host_eval_test.cpp)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "embedding_amd")
    exe = str(tmp_path / "host_eval_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", os.path.join(root, "tests", "native", "host_eval_test.cpp"), "-o", exe,
                           "-L" + libdir, "-l:libdge.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "HOST EVAL OK" in out.stdout


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_and_empty_calls(small8, dge):
    import torch
    s = small8
    m = s.model(64)
    ids = torch.zeros(8, dtype=torch.int32, device=m.torch_device)
    calls = (lambda: m.score_pairs(ids, ids), lambda: m.eval_links(s.corpus, s.R), lambda: m.eval_sgns(s.corpus))
    m.set_partition(2, 0, 0)
    for call in calls:
        with pytest.raises(dge.DgeError) as ei:
            call()
        assert ei.value.code == 5 and "partition" in str(ei.value)
    m.set_partition(1)
    for call in calls:
        call()
    for r in (m.eval_links(s.corpus, s.R, n_rows=0), m.eval_sgns(s.corpus, n_rows=0)):
        assert (r["pairs"], r["negatives"], r["skipped"]) == (0, 0, 0) and math.isnan(r["auc"]) and math.isnan(r["loss"])
    assert m.score_pairs(ids[:0], ids[:0]).numel() == 0
    with pytest.raises(dge.DgeError) as ei:
        m.eval_links(s.corpus, s.R, row0=0, n_rows=s.corpus.shape[0] + 1)
    assert ei.value.code == 1
    with pytest.raises(dge.DgeError) as ei:
        m.eval_links(s.corpus, 0)
    assert ei.value.code == 1
