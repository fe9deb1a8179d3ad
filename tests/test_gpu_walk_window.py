"""GPU: the walk-window pair loop of k_sgns_train_locked<relaxed> (embedding_amd/csrc/sgns_kernels.h: k_sgns_train_window) — a walk's syn0 updates parked in LDS, written once at walk end.

The loop is what auto launches on a flat vocabulary; on the small vocabularies here it is reached by forcing update_policy 5 with watchdog_ms = 0 (sgns_plan.h: wd_ticks
0 selects the instantiation without the watchdog; with the watchdog left on the same shape runs the per-pair loop, which gives a comparison inside one build).  Which
loop ran is asked of the library (dge_model_pair_loop); the kernel's name is the same for both.

Everything runs in the saturated regime of tests/helpers.py (a table is an exact integer count of updates whatever the order — tests/test_gpu_conservation.py's
docstring), the per-walk learning rates in the graded regime of tests/test_gpu_conservation_rates.py.  With several workers BOTH tables are under the relaxed commit now
(syn0 rows at walk end): per row never a surplus, untouched rows untouched, a shortfall of at most max(2, 10 % of the row's updates) — the bound the project states for
that protocol (test_gpu_conservation._assert_conserved).  Pairs and words are counted exactly.

Corpora: ragged walks of up to 24 tokens with holes, a token repeated inside every fourth walk, walks of length 0 and 1 among them."""
import concurrent.futures as cf
import types

import numpy as np
import pytest

from helpers import SAT_ALPHA, bits, saturated_state
from test_gpu_conservation import MAG, RUNS, SEED, _assert_conserved, _import_state, _knobs_in_force, _read_tables

pytestmark = pytest.mark.gpu

L, W = 24, 5
NAME = "k_sgns_train_locked<relaxed>"
WINDOW = dict(watchdog_ms=0)          # forced policy 5 without the watchdog: the instantiation auto launches
LDS_BYTES, FIXED_BYTES, WG_WORKERS = 163840, 32768, 48          # sgns_plan.h: window_slots


def _slots(D, walk_len=L):
    stride = -(-D // 64) * 64
    return min(16, (LDS_BYTES - FIXED_BYTES - WG_WORKERS * 2 * stride * 4) // (walk_len * stride * 4 + ((walk_len + 3) & ~3) * 4))


def _walks(NV, n, seed, walk_len=L):
    """ragged walks of up to walk_len tokens with holes; every fourth walk repeats a token (positions 3 and 7) and, where walks are longer than 32 tokens, is of full
    length and repeats that token once more at position 35: one row behind two words of position bits; a walk of length 0 and one of length 1 among them"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, NV, (n, walk_len)).astype(np.int32)
    rep = np.arange(n) % 4 == 0
    if walk_len > 7:
        ids[rep, 7] = ids[rep, 3]                                 # the same token twice in a walk: two positions, one row
    lens = rng.integers(min(2, walk_len), walk_len + 1, n)
    if walk_len > 35:
        ids[rep, 35] = ids[rep, 3]
        lens[rep] = walk_len
    ids[np.arange(walk_len)[None, :] >= lens[:, None]] = -1
    ids[rng.random(ids.shape) < 0.05] = -1                       # holes
    if n >= 8:
        ids[5] = -1                                               # length 0
        ids[6] = -1; ids[6, min(11, walk_len - 1)] = rng.integers(0, NV)          # length 1
    return ids


_CASES = {}
_POOL = []


@pytest.fixture(scope="module", autouse=True)
def _release_module_state():
    yield
    while _POOL:
        _POOL.pop().shutdown()
    _CASES.clear()


def _case(oracle, NV, n, D, K, table, walk_len=L, window=W, epochs=1):
    """-> namespace(ids, cnt, V, exp {(side, sign): (state, oracle tables)}): one corpus (walks of up to walk_len tokens) and the sequential oracle's four saturated runs
    from it (window radius `window`, `epochs` passes in one call), computed once a module.
    Every vertex is in the vocabulary (counts = occurrences + 2) so that the vocabulary has NV rows whatever the corpus touches.  The premise is asserted on the
    reference alone: the standing table unchanged, the accumulating one whole multiples of alpha below 2^24."""
    k = (NV, n, D, K, table, walk_len, window, epochs)
    if k not in _CASES:
        if not _POOL:
            _POOL.append(cf.ThreadPoolExecutor(max_workers=4))
        ids = _walks(NV, n, NV + n, walk_len)
        cnt = np.bincount(ids[ids >= 0], minlength=NV).astype(np.int64) + 2
        fut = {}
        for side, sign in RUNS:
            st = saturated_state(NV, D, side, sign, seed=SEED, mag=MAG)
            fut[side, sign] = (st, _POOL[0].submit(oracle.train_sgns, ids, NV, D, window, negative=K, min_count=1, epochs=epochs, seed=SEED, table_size=table, alpha=SAT_ALPHA,
                                                   min_alpha=SAT_ALPHA, arith=1, counts=cnt, syn0_init=st["syn0"], syn1neg_init=st["syn1neg"]))
        exp = {}
        for (side, sign), (st, f) in fut.items():
            om = f.result()
            moving, standing = ("syn1neg", "syn0") if side == "A" else ("syn0", "syn1neg")
            assert np.array_equal(bits(getattr(om, standing)), bits(st[standing]))
            units = getattr(om, moving)[:, 1:].astype(np.float64) / SAT_ALPHA
            assert (units == np.rint(units)).all() and np.abs(units).max() < 2 ** 24
            exp[side, sign] = (st, types.SimpleNamespace(syn0=om.syn0, syn1neg=om.syn1neg, pairs=om.pairs, vocab_ids=om.vocab_ids, V=om.V))
        _CASES[k] = types.SimpleNamespace(ids=ids, cnt=cnt, V=NV, exp=exp, table=table, words=epochs * int((ids >= 0).sum()), walk_len=walk_len, window=window, epochs=epochs)
    return _CASES[k]


def _model(dge, c, NV, D, K, workers, window=W, epochs=1):
    import torch
    cfg = dge.make_config(D, window, NV, negative=K, min_count=1, epochs=epochs, workers=workers, alpha=SAT_ALPHA, min_alpha=SAT_ALPHA, seed=SEED, table_size=c.table, update_policy=5)
    return dge.SgnsModel.create(cfg, torch.from_numpy(c.cnt).to("cuda:0"), 0)


def _launch(dge, m, corpus, c, D, run, knobs, loop, label, launch=None):
    """one launch (`launch(m, corpus)`: the case's own way to train the corpus, an epoch a launch for instance) from the run's saturated state -> the tables; pairs,
    words, the kernel's name, the reported policy and the pair loop — with the slots the corpus' walk length leaves room for — asserted"""
    st, om = c.exp[run]
    assert np.array_equal(m.vectors()[1], om.vocab_ids)
    _import_state(dge, m, st, -(-D // 64) * 64)
    m.reset_stats()
    with dge.tuning(**knobs):
        _knobs_in_force(dge, knobs)
        m.train(corpus) if launch is None else launch(m, corpus)
        stats, sch, name, pl = m.stats(), m.schedule(), m.kernel(), m.pair_loop()
    label = "%s -> %s, %d workers, pair loop %s" % (label, name, sch["workers"], pl)
    assert name == NAME and sch["update_policy"] == 5, label
    assert pl == ({"loop": 1, "slots": _slots(D, corpus.shape[1])} if loop else {"loop": 0, "slots": 0}), label
    assert stats["pairs"] == om.pairs and stats["words"] == c.words, (label, stats, om.pairs, c.words)
    return _read_tables(m, D, False), sch, label


def _conserved(tables, c, run, label, exact):
    side, _ = run
    st, om = c.exp[run]
    moving, standing = ("syn1neg", "syn0") if side == "A" else ("syn0", "syn1neg")
    assert np.array_equal(bits(tables[standing]), bits(st[standing])), "%s: %s moved" % (label, standing)
    return _assert_conserved(tables[moving], getattr(om, moving), st[moving], label, exact_rows=None if exact else slice(0, 0))


# ------------------------------------------------------------------------------------------ conservation of both tables, many workers
@pytest.mark.parametrize("NV,D,n,workers", [(6000, 128, 3, 0), (6000, 128, 2 * 6, 96), (6000, 128, 3000, 0), (6000, 64, 3000, 0), (250_000, 64, 4000, 0)],
                         ids=["3-walks", "slots-x-workgroups-walks", "6000-rows-D128", "6000-rows-D64", "250000-rows-D64"])
def test_window_conserves_both_tables(dge, oracle, NV, D, n, workers):
    """3 walks (fewer than slots), exactly slots x workgroups walks (96 workers: two workgroups of six slots at D = 128), a few thousand walks; a 6 000-row and a
    250 000-row vocabulary; D = 64 and 128"""
    if workers == 96:
        assert n == _slots(D) * (96 // WG_WORKERS)
    c = _case(oracle, NV, n, D, 5, 100_003 if NV < 100_000 else 10_000_000)
    corpus = dge.WalkCorpus.from_host(c.ids, 0)
    m = _model(dge, c, NV, D, 5, workers)
    for run in RUNS:
        tables, sch, label = _launch(dge, m, corpus, c, D, run, WINDOW, True, "window NV=%d D=%d %d walks run %s" % (NV, D, n, run))
        assert sch["workers"] > 1, label
        _conserved(tables, c, run, label, exact=False)
    m.close(); corpus.close()


@pytest.mark.parametrize("K", [0, 13])
def test_window_positive_only_and_two_lock_chunks(dge, oracle, K):
    """K = 0: the positive-only pair (one round, no negative); K = 13: two lock chunks (10 + 3)"""
    c = _case(oracle, 6000, 2000, 64, K, 100_003)
    corpus = dge.WalkCorpus.from_host(c.ids, 0)
    m = _model(dge, c, 6000, 64, K, 0)
    for run in RUNS:
        tables, sch, label = _launch(dge, m, corpus, c, 64, run, WINDOW, True, "window K=%d run %s" % (K, run))
        _conserved(tables, c, run, label, exact=False)
    m.close(); corpus.close()


# ------------------------------------------------------------------------------------------ which loop runs
def test_form_selection(dge, oracle):
    """L = 24 at D = 128 with several workers: the window; with the watchdog left on: the per-pair loop; one worker: the per-pair loop, bit-identical to the oracle;
    L = 64 at D = 128 (a slot would take 33 KB: fewer than four fit): the per-pair loop.  The kernel's name is the same throughout."""
    c = _case(oracle, 6000, 3000, 128, 5, 100_003)
    corpus = dge.WalkCorpus.from_host(c.ids, 0)
    run = ("B", 1)
    for workers, knobs, loop in ((0, WINDOW, True), (0, {}, False), (1, WINDOW, False)):
        m = _model(dge, c, 6000, 128, 5, workers)
        tables, sch, label = _launch(dge, m, corpus, c, 128, run, knobs, loop, "workers=%d %s" % (workers, knobs))
        _conserved(tables, c, run, label, exact=workers == 1)
        m.close()
    corpus.close()
    assert _slots(128, 64) < 4 <= _slots(128, 24)
    rng = np.random.default_rng(64)
    ids = rng.integers(0, 6000, (500, 64)).astype(np.int32)
    corpus = dge.WalkCorpus.from_host(ids, 0)
    m = _model(dge, types.SimpleNamespace(cnt=np.bincount(ids.reshape(-1), minlength=6000).astype(np.int64) + 2, table=100_003), 6000, 128, 5, 0)
    with dge.tuning(**WINDOW):
        m.train(corpus)
        assert m.kernel() == NAME and m.pair_loop() == {"loop": 0, "slots": 0} and m.schedule()["workers"] > 1
    m.close(); corpus.close()


# ------------------------------------------------------------------------------------------ the two loops of one build against each other
def test_window_and_per_pair_loop_agree(dge, oracle):
    """the same corpus on the 250 000-row vocabulary under the forced watchdog instantiation (the per-pair loop) and under the window: the conservation tables — the
    updates every row took, every column — agree exactly"""
    NV, D = 250_000, 64
    c = _case(oracle, NV, 4000, D, 5, 10_000_000)
    corpus = dge.WalkCorpus.from_host(c.ids, 0)
    m = _model(dge, c, NV, D, 5, 0)
    for run in RUNS:
        old, _, label_old = _launch(dge, m, corpus, c, D, run, {}, False, "per-pair loop run %s" % (run,))
        new, _, label_new = _launch(dge, m, corpus, c, D, run, WINDOW, True, "window run %s" % (run,))
        for t in ("syn0", "syn1neg"):
            assert np.array_equal(bits(old[t]), bits(new[t])), "%s / %s: %s differs in %d rows" % (label_old, label_new, t, int((old[t] != new[t]).any(1).sum()))
    m.close(); corpus.close()


# ------------------------------------------------------------------------------------------ per-walk learning rates
@pytest.mark.parametrize("static", [0, 1])
def test_window_per_walk_learning_rate(dge, oracle, static):
    """the graded regime of tests/test_gpu_conservation_rates.py on the window: every walk's terms carry the walk's own rate, whichever worker trains the centre —
    walks from the launch-wide counter (48 workers: 4 096 >= 32 x 48) and by the workgroup's stride"""
    from test_gpu_conservation_rates import _check
    loops = []

    def launch(m, corpus, c):
        m.train(corpus)
        loops.append(m.pair_loop()["loop"])
    _check(dge, oracle, "uniform16", 64, 5, (48, 0), NAME, knobs=dict(watchdog_ms=0, static_walks=static), reported=5, relaxed=True, launch=launch, many_walks=True)
    assert loops and all(x == 1 for x in loops), loops
