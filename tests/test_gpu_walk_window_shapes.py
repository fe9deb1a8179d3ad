"""GPU: the walk-window pair loop (embedding_amd/csrc/sgns_kernels.h: k_sgns_train_window) away from the corner tests/test_gpu_walk_window.py stands in — rows with
padding, walks longer than one word of position bits, window radii up to and beyond the walk, full lock chunks, workgroups most of whose workers leave after the
prologue, the negative-sampling table with and without its run form, a second epoch — and its arithmetic outside the saturated regime.

1. Saturated conservation (the regime and the bound of tests/test_gpu_walk_window.py: pairs and words exact, the standing table bit-unchanged, the accumulating one per
   row never a surplus and short by at most max(2, 10 % of the row's updates)) with ONE axis at a time moved from D = 128, L = 24, W = 5, K = 5, workers = 0.  The
   tables are also read stride-wide, device to device: the padding columns [D, stride) of every row are bit-zero after training.
2. Where the window starts and stops: the last walk length and the widest row that select it, asked of the library (no oracle).
3. The balanced regime of tests/test_gpu_conservation_balanced.py on the window: every term through the kernel's own LDS copy of the sigmoid table, g = +/- alpha/2.
4. The linear regime of tests/test_gpu_sgns.py::test_hierarchical_softmax_wave_per_centre_linear_regime: real-valued tables at a vanishing learning rate against the
   sequential oracle, term by term, with the per-pair loop of the same build as a control.

Every launch asserts through dge_model_pair_loop which loop ran and with how many slots (a shape that fell back to the per-pair loop fails), and reads its knobs back.
Vocabularies are flat: uniform tokens over 6 000 rows, counts = occurrences + 2 (forced policy 5 is accepted).  Oracle runs go on the host thread pool of
tests/test_gpu_walk_window.py."""
import concurrent.futures as cf
import types

import numpy as np
import pytest

import test_gpu_conservation_balanced as bal
import test_gpu_walk_window as ww
from helpers import bits, cosine_rows, device_table
from test_gpu_conservation import RUNS, SEED, _knobs_in_force, _read_tables
from test_gpu_walk_window import NAME, WINDOW, _case, _conserved, _launch, _model, _slots, _walks

pytestmark = pytest.mark.gpu

NV, TABLE = 6000, 100_003
BASE = dict(D=128, L=24, W=5, K=5, workers=0, n=2000)


@pytest.fixture(scope="module", autouse=True)
def _release_module_state():
    """the host threads and the cached expected tables of the two modules whose machinery runs here live as long as this module's tests"""
    yield
    for mod in (ww, bal):
        while mod._POOL:
            mod._POOL.pop().shutdown(wait=True, cancel_futures=True)
    ww._CASES.clear(); bal._EXPECTED.clear(); bal._PAIRS.clear(); _LINEAR.clear()


def _padding_bit_zero(m, D, label):
    """both tables as they lie in device memory, [V x stride]: every padding column of every row holds +0.0 (_read_tables compares values: -0.0 would pass there)"""
    for t, name in ((0, "syn0"), (1, "syn1neg")):
        full = device_table(m, t)
        assert full.shape[1] == -(-D // 64) * 64, (label, full.shape)
        pad = full[:, D:].cpu().numpy()
        assert not bits(pad).any(), "%s: %s padding columns [%d, %d) not bit-zero in %d rows" % (label, name, D, full.shape[1], int(bits(pad).any(1).sum()))


def _run_case(dge, oracle, label, D, L, W, K, workers, n, knobs=WINDOW, model_knobs=None, launch=None, epochs=1):
    """one case of the matrix: the corpus and the oracle's four saturated runs (the premise asserted on the reference by _case before any launch), a model, per run one
    launch with the window and its slots asserted, both tables conserved, the padding bit-zero -> the schedule the last launch reported"""
    c = _case(oracle, NV, n, D, K, TABLE, walk_len=L, window=W, epochs=epochs)
    assert c.ids.shape == (n, L) and 1500 <= n <= 3000
    if L > 32:
        full = c.ids[:, L - 1] >= 0          # (tokens up to the last position: positions 32 .. L-1 are trained)
        twice = full & (c.ids[:, 3] >= 0) & (c.ids[:, 3] == c.ids[:, 35])
        assert full.sum() >= n // 5 and twice.sum() >= n // 6, "too few walks of full length / with one row at a position below and one above 32"
    corpus = dge.WalkCorpus.from_host(c.ids, 0)
    with dge.tuning(**(model_knobs or {})):
        m = _model(dge, c, NV, D, K, workers, window=W, epochs=epochs)
    sch = None
    for run in RUNS:
        tables, sch, lab = _launch(dge, m, corpus, c, D, run, knobs, True, "%s run %s" % (label, run), launch=launch)
        assert sch["workers"] > 1, lab
        _conserved(tables, c, run, lab, exact=False)
        _padding_bit_zero(m, D, lab)
    return m, corpus, c, sch


# ------------------------------------------------------------------------------------------ 1. saturated conservation, one axis at a time
MATRIX = {
    # rows with padding: D = 100 and 65 at stride 128, D = 40 at stride 64
    "D100": dict(D=100), "D65": dict(D=65), "D40": dict(D=40),
    # walks behind two words of position bits: 6 slots; an odd length, tokens padded to 40: 11 slots; the floor of four slots
    "L64-D64": dict(L=64, D=64, n=1500), "L37-D64": dict(L=37, D=64), "L39-D128": dict(L=39, D=128, n=1500),
    "L2": dict(L=2, n=3000),
    # the radius: 1; cfg3's 24 (every centre's context is the whole walk), also on a padded row; wider than the walk
    "W1": dict(W=1), "W24": dict(W=24, n=1500), "W24-D100": dict(W=24, D=100, n=1500), "W30": dict(W=30, n=1500),
    # one negative; one exactly full lock chunk; two full chunks
    "K1": dict(K=1), "K10": dict(K=10), "K20": dict(K=20, n=1500),
}
SLOTS = {"L64-D64": 6, "L37-D64": 11, "L39-D128": 4}


@pytest.mark.parametrize("name", list(MATRIX))
def test_window_conserves_over_shapes(dge, oracle, name):
    """D in {100, 65, 40}; (L, D) in {(64, 64), (37, 64), (39, 128)} — every fourth walk of full length with one token at positions 3 and 35 — and a corpus of
    two-token walks; W in {1, 24, 30} and W = 24 at D = 100; K in {1, 10, 20}"""
    p = dict(BASE, **MATRIX[name])
    if name in SLOTS:
        assert _slots(p["D"], p["L"]) == SLOTS[name]
    m, corpus, c, sch = _run_case(dge, oracle, name, **p)
    m.close(); corpus.close()


@pytest.mark.parametrize("workers", [2, 49])
def test_window_conserves_with_few_workers(dge, oracle, workers):
    """2 workers: one workgroup, 46 of whose 48 workers return behind the prologue; 49: a second workgroup with a single worker.  The worker count the schedule
    reports is printed, not fixed in advance."""
    m, corpus, c, sch = _run_case(dge, oracle, "workers=%d" % workers, **dict(BASE, workers=workers))
    print("workers asked %d, the schedule reports %d" % (workers, sch["workers"]))
    assert sch["workers"] > 1
    m.close(); corpus.close()


def test_window_one_token_walks(dge, oracle):
    """L = 1: neither the library nor the oracle refuses a corpus of one-token walks (no refusal to assert).  The plan still selects the window (16 slots; asserted as
    the library reports it), every walk is loaded, counted and completed without a pair: zero pairs, exact words, both tables bit-unchanged."""
    D = 128
    c = _case(oracle, NV, 2000, D, 5, TABLE, walk_len=1)
    assert all(om.pairs == 0 for _, om in c.exp.values()) and c.words > 1500
    corpus = dge.WalkCorpus.from_host(c.ids, 0)
    m = _model(dge, c, NV, D, 5, 0)
    for run in RUNS:
        st, om = c.exp[run]
        tables, sch, lab = _launch(dge, m, corpus, c, D, run, WINDOW, True, "L=1 run %s" % (run,))
        assert m.pair_loop() == {"loop": 1, "slots": 16} and m.stats()["pairs"] == 0 and m.stats()["words"] == c.words, lab
        for t in ("syn0", "syn1neg"):
            assert np.array_equal(bits(tables[t]), bits(st[t])), "%s: %s moved" % (lab, t)
        _padding_bit_zero(m, D, lab)
    m.close(); corpus.close()


@pytest.mark.parametrize("cap", [0, 3])
def test_window_draws_the_tables_rows(dge, oracle, cap):
    """table_runs = 0: the kernel's use_runs == false branch, every draw a look-up in the table; 3: the mixed form — the last three runs of equal counts in LDS, the
    head rows in front of them on the table.  The same corpus and the same oracle tables as the default (D = 64, K = 5): the rows drawn must be the table's."""
    p = dict(BASE, D=64)
    knobs = dict(WINDOW, table_runs=cap)
    m, corpus, c, sch = _run_case(dge, oracle, "table_runs=%d" % cap, knobs=knobs, model_knobs=dict(table_runs=cap), **p)
    runs, exc = m.table_runs()
    assert runs == cap, (cap, runs, exc)
    m.close()
    if cap == 3:          # (what the default is on this vocabulary: more runs than the mixed form keeps)
        m = _model(dge, c, NV, 64, 5, 0)
        assert m.table_runs()[0] > 3, m.table_runs()
        m.close()
    corpus.close()


def test_window_two_epochs(dge, oracle):
    """cfg.epochs = 2, a launch an epoch, as tests/test_gpu_conservation_rates.py launches tiny3: the second launch starts with a non-zero gidx_base (its draws are
    the second epoch's) and a non-zero words_done_base; the oracle runs its two epochs in one call"""
    def launch(m, corpus):
        for ep in range(2):
            m.train(corpus, epoch=ep)
    m, corpus, c, sch = _run_case(dge, oracle, "two epochs", launch=launch, epochs=2, **BASE)
    one = _case(oracle, NV, BASE["n"], 128, 5, TABLE)
    assert c.exp["A", 1][1].pairs > one.exp["A", 1][1].pairs and c.words == 2 * one.words
    assert not np.array_equal(c.exp["A", 1][1].syn1neg[:, 1] - c.exp["A", 1][0]["syn1neg"][:, 1], 2 * (one.exp["A", 1][1].syn1neg[:, 1] - one.exp["A", 1][0]["syn1neg"][:, 1])), \
        "the second epoch drew the first one's negatives: the case proves nothing about gidx_base"
    m.close(); corpus.close()


# ------------------------------------------------------------------------------------------ 2. where the window starts and stops
@pytest.mark.parametrize("D,L,loop", [(128, 39, True), (128, 40, False), (64, 64, True), (64, 65, False), (129, 24, False)])
def test_window_selection_edges(dge, D, L, loop):
    """D = 128: L = 39 is the last walk length that selects the window (4 slots, the floor), L = 40 runs the per-pair loop.  D = 64 under forced policy 5: L = 64
    selects it (6 slots), L = 65 does not.  D = 129 (stride 192) never does.  (D = 64 under AUTO cannot be reached here: auto takes the commit locks on flat
    vocabularies of 131 072 rows and more, these have 6 000.)  Python's _slots against what the library reports at each window shape."""
    if loop:
        assert _slots(D, L) >= 4 > _slots(D, L + 1) or L == 64
    elif D <= 128:
        assert _slots(D, L) < 4 or L > 64
    rng = np.random.default_rng(D * 100 + L)
    ids = rng.integers(0, NV, (500, L)).astype(np.int32)
    corpus = dge.WalkCorpus.from_host(ids, 0)
    m = _model(dge, types.SimpleNamespace(cnt=np.bincount(ids.reshape(-1), minlength=NV).astype(np.int64) + 2, table=TABLE), NV, D, 5, 0)
    with dge.tuning(**WINDOW):
        _knobs_in_force(dge, WINDOW)
        m.train(corpus)
        pl, sch, st = m.pair_loop(), m.schedule(), m.stats()
    print("D=%d L=%d -> %s, %d workers, pair loop %s" % (D, L, m.kernel(), sch["workers"], pl))
    assert m.kernel() == NAME and sch["update_policy"] == 5 and sch["workers"] > 1 and st["words"] == ids.size and st["pairs"] > ids.size
    assert pl == ({"loop": 1, "slots": _slots(D, L)} if loop else {"loop": 0, "slots": 0}), pl
    m.close(); corpus.close()


# ------------------------------------------------------------------------------------------ 3. the balanced regime on the window
@pytest.mark.parametrize("D,K", [(128, 5), (100, 5), (128, 0), (100, 0)])
def test_window_balanced_regime(dge, oracle, D, K):
    """every score in the bin of exp_table[500]: the window reads its own LDS copy of the sigmoid table on every term and takes the label inside sgns_g — the only
    exact test that does.  Both tables are under the relaxed commit with several workers (`loose`): whole multiples of alpha/2, idle rows untouched, the standing
    table and column 0 bit-unchanged, padding zero; the device-filling count and 48 workers."""
    loops = []

    def launch(m, corpus):
        m.train(corpus)
        loops.append(m.pair_loop())
    if not bal._POOL:          # (an empty pool makes _expected send every case that module registers ahead: only this one is wanted here)
        bal._POOL.append(cf.ThreadPoolExecutor(max_workers=4))
    bal._check(dge, oracle, "flat", D, K, policy=5, workers=(0, 48), knobs=dict(watchdog_ms=0), kernel=NAME, reported=5, loose=("syn0", "syn1neg"), launch=launch)
    L = bal._bal_corpus("flat")[0].shape[1]
    print("pair loop %s" % loops)
    assert len(loops) == 4 and all(pl == {"loop": 1, "slots": _slots(D, L)} for pl in loops), loops


# ------------------------------------------------------------------------------------------ 4. the linear regime, real arithmetic
LIN_ALPHA = 1e-5
_LINEAR = {}


def _linear(oracle, D, W, n):
    """-> namespace(ids, cnt, init, starts {name: (state, the sequential oracle's trained tables)}): computed once a module, on the host threads.  `init`: the tables
    of an alpha = 0 oracle run.  Start "library": those tables (syn1neg zero).  Start "seeded": syn0 = init.syn0 scaled to uniform +/- 0.36, syn1neg = the same rows
    moved on by one — scores of 0.3 .. 0.45 standard deviation, so that the sigmoid table is read over a hundred of its bins and BOTH tables move in first order."""
    k = (D, W, n)
    if k not in _LINEAR:
        if not ww._POOL:
            ww._POOL.append(cf.ThreadPoolExecutor(max_workers=4))
        ids = _walks(NV, n, NV + n + D)
        cnt = np.bincount(ids[ids >= 0], minlength=NV).astype(np.int64) + 2
        kw = dict(negative=5, min_count=1, epochs=1, seed=SEED, table_size=TABLE, threads=1, arith=1, counts=cnt)
        init = oracle.train_sgns(ids[:1], NV, D, W, alpha=0.0, min_alpha=0.0, **kw)
        assert init.V == NV and not init.syn1neg.any() and np.abs(init.syn0).max() <= 0.5 / D
        s0 = (init.syn0 * np.float32(0.72 * D)).astype(np.float32)
        starts = {"library": {"syn0": init.syn0, "syn1neg": init.syn1neg}, "seeded": {"syn0": s0, "syn1neg": np.roll(s0, 1, axis=0).copy()}}
        fut = {name: ww._POOL[0].submit(oracle.train_sgns, ids, NV, D, W, alpha=LIN_ALPHA, min_alpha=LIN_ALPHA, syn0_init=st["syn0"], syn1neg_init=st["syn1neg"], **kw)
               for name, st in starts.items()}
        _LINEAR[k] = types.SimpleNamespace(ids=ids, cnt=cnt, init=init, starts=starts, fut=fut)
    return _LINEAR[k]


def _linear_figures(got, want, init):
    """table - init of the device against the oracle's -> (cosine min, cosine median, largest |norm ratio - 1|) over the rows whose oracle update norm is above the
    20th percentile of the non-zero ones, whether every row the oracle leaves untouched is bit-untouched, and how many those are"""
    da, db = (got - init).astype(np.float64), (want - init).astype(np.float64)
    nb = np.linalg.norm(db, axis=1)
    busy = nb > np.percentile(nb[nb > 0], 20)
    cos = cosine_rows(da[busy], db[busy])
    idle = nb == 0
    return float(cos.min()), float(np.median(cos)), float(np.abs(np.linalg.norm(da[busy], axis=1) / nb[busy] - 1).max()), bool(np.array_equal(bits(got[idle]), bits(init[idle]))), int(idle.sum())


@pytest.mark.parametrize("D,W", [(128, 5), (100, 24), (64, 5)])
def test_window_linear_regime(dge, oracle, D, W):
    """alpha = min_alpha = 1e-5, K = 5, 4 000 ragged walks of up to 24 tokens on 6 000 rows, device-filling, the oracle sequential: table - init of the device against
    the oracle's under the bounds of test_hierarchical_softmax_wave_per_centre_linear_regime — on the rows above the 20th percentile of the oracle's non-zero update
    norms cosine min > 0.99, median > 0.9995, norm within 5 %; rows the oracle leaves untouched bit-untouched.  Per start first the per-pair loop of the same build
    (the watchdog left on) on the same inputs as a control, then the window; the figures of both are printed before anything is asserted.

    Start "library": the tables as the library initialises them, bit-equal to an alpha = 0 oracle run (asserted).  syn1neg starts at zero and moves in first order:
    under the bounds.  syn0 moves by g x syn1neg, SECOND order: ~1e-11 an element against a spacing of 2.3e-10 around its values of up to 1/256 — the oracle's own
    syn0 update is what rounding lets through (a median of 3 non-zero elements a row) and depends on how far syn1neg has come when a pair trains.  Measured on an
    MI355X: cosine median 0.42 (per-pair loop, the control) and 0.59 (window) at D = 128, W = 5, minima of -1; no corpus of a size a test can train changes the
    order of magnitude (a syn1neg element would have to grow 50-fold).  There syn0 is held to its order of magnitude only: no element moves by more than the second-
    order terms and the roundings its row can take.
    Start "seeded" (both tables random, imported into the oracle and the device alike): both tables move in first order and BOTH are under the bounds, in both loops."""
    import torch
    from test_gpu_conservation import _import_state
    K = 5
    c = _linear(oracle, D, W, 4000)
    corpus = dge.WalkCorpus.from_host(c.ids, 0)
    cfg = dge.make_config(D, W, NV, negative=K, min_count=1, epochs=1, workers=0, alpha=LIN_ALPHA, min_alpha=LIN_ALPHA, seed=SEED, table_size=TABLE, update_policy=5)
    figures, second_order = {}, {}
    for start, st in c.starts.items():
        om = c.fut[start].result()
        for loop, knobs in (("per-pair", {}), ("window", WINDOW)):
            m = dge.SgnsModel.create(cfg, torch.from_numpy(c.cnt).to("cuda:0"), 0)
            assert np.array_equal(m.vectors()[1], om.vocab_ids)
            if start == "library":
                t0 = _read_tables(m, D, False)
                assert np.array_equal(bits(t0["syn0"]), bits(c.init.syn0)) and np.array_equal(bits(t0["syn1neg"]), bits(c.init.syn1neg)), "the library's initial tables are not the oracle's"
            else:
                _import_state(dge, m, st, -(-D // 64) * 64)
            m.reset_stats()
            with dge.tuning(**knobs):
                _knobs_in_force(dge, knobs)
                m.train(corpus)
                stats, sch, name, pl = m.stats(), m.schedule(), m.kernel(), m.pair_loop()
            lab = "linear D=%d W=%d %s start, %s loop -> %s, %d workers, pair loop %s" % (D, W, start, loop, name, sch["workers"], pl)
            assert name == NAME and sch["update_policy"] == 5 and sch["workers"] > 1 and stats["pairs"] == om.pairs, lab
            assert pl == ({"loop": 1, "slots": _slots(D)} if loop == "window" else {"loop": 0, "slots": 0}), lab
            tables = _read_tables(m, D, False)
            _padding_bit_zero(m, D, lab)
            for t in ("syn0", "syn1neg"):
                f = figures[start, loop, t] = _linear_figures(tables[t], getattr(om, t), st[t])
                print("%s: %s cosine min %.6f median %.6f, norm ratio off by %.4f, the oracle's %d untouched rows untouched: %s" % ((lab, t) + f[:3] + (f[4], f[3])))
            if start == "library":
                # a row is context to at most (its tokens) x 2W pairs of K + 1 terms, each at most alpha x (twice the oracle's largest syn1neg element), and every
                # addition to a value below 2^-8 rounds by at most 2^-33
                terms = (np.bincount(c.ids[c.ids >= 0], minlength=NV)[om.vocab_ids] * 2 * W * (K + 1)).astype(np.float64)
                second_order[loop] = float((np.abs(tables["syn0"].astype(np.float64) - st["syn0"]).max(1) / np.maximum(terms * (LIN_ALPHA * 2 * np.abs(om.syn1neg).max() + 2.0 ** -33), 1e-300)).max())
                print("%s: syn0 moved by at most %.3g of its second-order bound" % (lab, second_order[loop]))
            m.close()
    corpus.close()
    for (start, loop, t), (cmin, cmed, ratio, idle_ok, _) in figures.items():
        if (start, t) == ("library", "syn0"):
            assert second_order[loop] <= 1.0, (loop, second_order[loop])
            continue
        assert cmin > 0.99 and cmed > 0.9995, (start, loop, t, cmin, cmed)
        assert ratio < 0.05, (start, loop, t, ratio)
        assert idle_ok, (start, loop, t)
