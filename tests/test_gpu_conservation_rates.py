"""GPU: the per-walk learning rate of every kernel form of the SGNS trainer, exact at every worker count.

tests/test_gpu_conservation.py and tests/test_gpu_conservation_balanced.py hold every form to "every update exactly once, on the right row, with the right sign and
rate" — with alpha == min_alpha, so the rate is one constant and never at stake.  In a real run every form computes the rate per walk (per mini-batch under
owner-computes) from the tokens that precede the walk, each form with its own copy of the formula, and takes that token count from wherever the walk came from: a
static stride, the launch-wide walk counter, or the block schedule's prefetch of the next walk.  Here the rates are GRADED (helpers.rate_level): alpha0 = 2^-e,
min_alpha = alpha0 / 4, and counts whose sum T has epochs * T + 1 = 2^m, so that the rate of a walk is alpha0 * (2^m - done) / 2^m exactly — a whole number of
lattice units alpha0 / 2^b, b = m where `done` moves a token at a time and b = m - a where every walk holds 2^a tokens; the last quarter of the schedule sits on the
floor.  In the saturated state (helpers.saturated_state) every live term is +/- level x code units, in the balanced state (helpers.balanced_state) +/- level x code
half units: while (terms a row can take) x 2^b x (largest code) < 2^24 every partial sum in any order is exact, so the trained tables do not depend on the order of
the additions or on the number of workers — but they do depend on the rate every single term carried.  A walk trained at its neighbour's rate, a dropped
epoch * total_words, an ignored floor, words_scale on the wrong side of the truncation: each moves named rows by whole units
(tests/test_oracle_kats.py::test_graded_rates_equal_int64_sums shows it on the witness).

Expected tables: the sequential oracle from the same state; its schedule is pinned to integers by that CPU test.  Where the oracle has no counterpart (words_scale
with a truncation) the expectation is the int64 witness itself.  Before anything is compared the conditions of the method are asserted on the reference alone
(_reference): the term bound from host quantities (per row, the live terms counted by the count channel of the oracle's constant-rate saturated runs) times 2^b
below 2^24, whole multiples of the unit, standing tables and column 0 bit-unchanged, and a result that differs from the constant-rate run.

On every table of every case ("always"): pairs equal, the kernel named, the knobs read back, standing tables and column 0 bit-unchanged, rows the oracle leaves
untouched untouched, whole lattice units on every row, padding columns and the spare row behind syn1 zero.  Bit equality with the oracle on everything a form's
design makes exact.  NOT exact by design: rows under the RELAXED commit locks with several workers — a lost re-lock race drops the update; there
the "always" list and, in the saturated state, the bound of test_gpu_conservation.py in lattice units: never a surplus, a deficit of at most
max(2, 10 % of the row's terms) x 2^b.  One worker is exact there too.

Corpora (4 000 vertices instead of 6 000 rows: below 4 096 rows the device-filling launch runs V / 2 workers, so that on 4 096 walks a worker trains more than one
walk under the static stride as well; asserted): uniform16 — 4 096 full walks of 16 tokens, m = 16, b = 12; ragged — ragged walks of 2 .. 24 tokens cut behind the
16 383rd token, m = b = 14; long — walks of 100 tokens (the kernels' memory token path), m = b = 14; tiny / tiny3 — ragged, 4 095 tokens (m = 12) and 1 365 tokens
an epoch of three (3 T + 1 = 2^12); tree — 256 walks of 16 tokens, m = 12, b = 8, on Fibonacci counts whose longest Huffman code (13) is longer than the 12 path
nodes a wave of k_sgns_train_hsw keeps in registers at 256 floats a row.  Codes are +/- 1 (mag = 1)."""
import types

import numpy as np
import pytest

from helpers import SAT_CAP, balanced_state, bits, graded_diff, layered_graph, rate_level, saturated_state, simulate_block_schedule, simulate_gather_syn0
from test_gpu_conservation import NEVER, SEED, TABLE, _import_state, _knobs_in_force, _read_tables

pytestmark = pytest.mark.gpu

A0 = {"sat": 2.0 ** -40, "bal": 2.0 ** -60}          # alpha0 per state; min_alpha = alpha0 / 4
RUNS = [("sat", "A", 1), ("sat", "A", -1), ("sat", "B", 1), ("sat", "B", -1), ("bal", "A", 0), ("bal", "B", 0)]
QUICK = [("sat", "A", 1), ("bal", "B", 0)]           # what one or two workers run on the corpora of more than 8 000 tokens (one worker trains 2e5 .. 4e5 pairs a second)
BAL = [("bal", "A", 0), ("bal", "B", 0)]
ACC = {"A": ("syn1neg", "syn1"), "B": ("syn0",)}
PAIR_BY_PAIR = "k_sgns_train<atomics, hierarchical softmax pair by pair>"
IN_ORDER_HS = "k_sgns_train<in-order, hierarchical softmax pair by pair>"

_CORPORA, _REF = {}, {}


def _cut(ids, T):
    """the corpus cut behind its T-th token, empty walks at the end dropped"""
    seen = np.cumsum((ids >= 0).reshape(-1)).reshape(ids.shape)
    assert seen[-1, -1] > T
    ids = np.where(seen > T, -1, ids).astype(np.int32)
    return ids[:int(np.flatnonzero((ids >= 0).any(1)).max()) + 1]


def _ragged(rng, NV, n, L):
    ids = rng.integers(0, NV, (n, L)).astype(np.int32)
    ids[np.arange(L)[None, :] >= rng.integers(2, L + 1, n)[:, None]] = -1
    return ids


def _corpus(key):
    """-> namespace(ids, NV, cnt — the counts the models and the oracle are made from, every token in the vocabulary (min_count 1) —, T, EP, m, b, W, K)"""
    if key not in _CORPORA:
        rng = np.random.default_rng(sum(map(ord, key)) + 1)
        EP, cnt = 1, None
        if key == "uniform16":
            NV, W, m, b = 4000, 2, 16, 12
            ids = rng.integers(0, NV, (4096, 16)).astype(np.int32)
        elif key == "ragged":
            NV, W, m, b = 4000, 5, 14, 14
            ids = _cut(_ragged(rng, NV, 1400, 24), (1 << m) - 1)
        elif key == "long":
            NV, W, m, b = 2000, 5, 14, 14
            ids = _cut(rng.integers(0, NV, (170, 100)).astype(np.int32), (1 << m) - 1)
        elif key == "tiny":
            NV, W, m, b = 1000, 5, 12, 12
            ids = _cut(_ragged(rng, NV, 400, 24), (1 << m) - 1)
        elif key == "tiny3":
            NV, W, m, b, EP = 1000, 5, 12, 12, 3
            ids = _cut(_ragged(rng, NV, 160, 24), ((1 << m) - 1) // 3)
        elif key == "tree":
            NV, W, m, b = 115, 2, 12, 8
            ids = rng.integers(0, NV, (256, 16)).astype(np.int32)
            fib = [1, 1]
            while len(fib) < 15:
                fib.append(fib[-1] + fib[-2])
            tail = np.full(100, (4095 - sum(fib)) // 100, np.int64)
            tail[:4095 - sum(fib) - int(tail.sum())] += 1
            cnt = rng.permutation(np.concatenate([np.array(fib, np.int64), tail]))
        if cnt is None:
            cnt = np.bincount(ids[ids >= 0], minlength=NV).astype(np.int64)
            if key == "uniform16":
                cnt[int(np.argmax(cnt))] -= 1          # 65 536 tokens are trained, the schedule has 2^16 - 1: T + 1 = 2^m
        T = int(cnt.sum())
        assert EP * T + 1 == 1 << m and (cnt[np.unique(ids[ids >= 0])] >= 1).all()
        _CORPORA[key] = types.SimpleNamespace(key=key, ids=ids, NV=NV, cnt=cnt, T=T, EP=EP, m=m, b=b, W=W, K=5, V=int((cnt >= 1).sum()),
                                              wb=np.concatenate([[0], np.cumsum((ids >= 0).sum(1))[:-1]]).astype(np.int64))
    return _CORPORA[key]


@pytest.fixture(scope="module", autouse=True)
def _release_module_state():
    yield
    _REF.clear(); _CORPORA.clear()


def _state(kind, V, D, side, sign, use_hs):
    return saturated_state(V, D, side, sign, seed=SEED, mag=1, use_hs=use_hs) if kind == "sat" else balanced_state(V, D, side, seed=SEED, mag=1, use_hs=use_hs)


def _reference(oracle, c, D, use_hs=False, part_n=0, sorted_=None, n_rows=None, total_words=0, b=None, witness=None):
    """{(state, side, sign): namespace(st, want {table: [rows x D]}, pairs, bound {table}, unit, levels)} of one (corpus, D, tree term, ranks, mini-batch rule, rows
    trained, total_words the oracle is told, lattice bits): the same for every schedule, computed once a module.  `witness`: None — the sequential oracle — or
    (terms with (epoch, walk), levels [epochs x walks]): the int64 sums of tests/test_oracle_kats.py.  The conditions of the method are asserted here, on the
    reference alone."""
    from test_oracle_kats import _graded_sums
    k = (c.key, D, use_hs, part_n, sorted_, n_rows, total_words, b, None if witness is None else witness[1].tobytes())
    if k in _REF:
        return _REF[k]
    b = c.b if b is None else b
    ids = c.ids if n_rows is None else c.ids[:n_rows]
    longest = int(oracle.huffman(np.sort(c.cnt[c.cnt >= 1])[::-1])[0].max()) if use_hs else 0
    assert not use_hs or longest > 12
    kw = dict(negative=c.K, min_count=1, epochs=c.EP, seed=SEED, table_size=TABLE, arith=1, counts=c.cnt, total_walks=len(c.ids), total_words=total_words, part_n=part_n)
    batches = dict(sorted_chunk=sorted_[0], sorted_walks=sorted_[1]) if sorted_ else {}

    def run(kind, side, sign, a0, amin, hs):
        """(a constant-rate run has one result under every schedule: only the graded runs go through the oracle's slower mini-batch path)"""
        st = _state(kind, c.V, D, side, sign, hs)
        return st, oracle.train_sgns(ids, c.NV, D, c.W, alpha=a0, min_alpha=amin, syn0_init=st["syn0"], syn1neg_init=st["syn1neg"], syn1_init=st.get("syn1"), use_hs=hs, **kw,
                                     **(batches if a0 != amin else {}))
    # the live terms a row takes, from the count channel of constant-rate saturated runs (the negatives: sign +1; the positives: sign -1) — host quantities
    live, pairs = {}, None
    for side in "AB":
        for sign in (1, -1):
            st, om = run("sat", side, sign, A0["sat"], A0["sat"], False)
            t = "syn1neg" if side == "A" else "syn0"
            n = getattr(om, t)[:, 1].astype(np.float64) / A0["sat"]
            assert (n == np.rint(n)).all() and np.abs(n).max() < SAT_CAP
            live[side, sign] = np.abs(n).astype(np.int64)
            pairs = om.pairs
    assert int(live["B", -1].sum()) == pairs == int(live["A", -1].sum())          # every positive pair once, on its context's / its centre's row
    out = {}
    for kind, side, sign in RUNS if not use_hs else BAL:
        a0 = A0[kind]
        unit = a0 / (1 << b) / (2 if kind == "bal" else 1)
        st, flat = run(kind, side, sign, a0 / 2, a0 / 2, use_hs)
        if witness is None:
            st, om = run(kind, side, sign, a0, a0 / 4, use_hs)
            want = {t: getattr(om, t) for t in st}
            assert om.pairs == pairs == flat.pairs
        else:
            sums = _graded_sums(st, side, {"bal": 0}.get(kind, sign), *witness)
            moving = "syn1neg" if side == "A" else "syn0"
            want = dict(st)
            want[moving] = np.concatenate([st[moving][:, :1], (sums.astype(np.float64) * unit).astype(np.float32)], 1)
            assert int(witness[0][2].sum()) == pairs and not use_hs
        if kind == "sat":
            bound = {"syn1neg": int(live["A", sign].max()), "syn0": int(live["B", sign].max())}
        else:
            bound = {"syn1neg": int((live["A", 1] + live["A", -1]).max()), "syn0": int((live["B", 1] + live["B", -1] + longest * live["B", -1]).max()), "syn1": pairs}
        for t in st:
            if t in ACC[side]:
                d = graded_diff(want[t], want[t], st[t], unit, 1 << b, bound[t])
                assert d.exact and d.whole.all() and np.abs(d.level_want).max() > 0
                assert not np.array_equal(bits(want[t]), bits(getattr(flat, t))), "%s: the graded run leaves the constant-rate run's %s: the case proves nothing" % ((kind, side, sign), t)
            else:
                assert np.array_equal(bits(want[t]), bits(st[t])), "the reference's standing %s moved" % t
        out[kind, side, sign] = types.SimpleNamespace(st=st, want=want, pairs=pairs, bound=bound, unit=unit, levels=1 << b, live=live, vocab_ids=flat.vocab_ids, V=flat.V)
    _REF[k] = out
    return out


def _compare(tables, ref, run, label, relaxed=False):
    """the "always" list on every table; bit equality with the reference unless `relaxed` (rows under the relaxed commit with several workers: the module's docstring)"""
    kind, side, sign = run
    for t, init in ref.st.items():
        got, want = tables[t], ref.want[t]
        if t not in ACC[side]:
            assert np.array_equal(bits(got), bits(init)), "%s: the standing %s moved" % (label, t)
            continue
        assert np.array_equal(bits(got[:, 0]), bits(init[:, 0])), "%s: column 0 of %s moved" % (label, t)
        d = graded_diff(got, want, init, ref.unit, ref.levels, ref.bound[t])
        print("%s: %s %d of %d rows differ, the worst by %g lattice units" % (label, t, int((d.diff != 0).sum()), len(d.diff), d.diff.max()))
        assert d.whole.all(), "%s: %s holds a fraction of a lattice unit — %s" % (label, t, d.worst())
        idle = ~(want[:, 1:] != 0).any(1)
        assert np.array_equal(bits(got[idle]), bits(init[idle])), "%s: a row of %s the oracle leaves untouched moved" % (label, t)
        if not relaxed:
            assert d.exact, "%s: %s — %s" % (label, t, d.worst())
            assert np.array_equal(bits(got), bits(want)), "%s: %s" % (label, t)
        elif kind == "sat":          # never a surplus; a lost update loses at most 2^b units
            terms = ref.live[side, sign]
            assert (np.abs(d.level_got) <= np.abs(d.level_want)).all() and (d.level_got * np.sign(d.level_want) >= 0).all(), "%s: %s a surplus — %s" % (label, t, d.worst())
            assert (d.diff <= np.maximum(2, np.floor(0.10 * terms)) * ref.levels).all(), "%s: %s beyond max(2, 10 %%) of a row's terms — %s" % (label, t, d.worst())


def _model(dge, c, D, policy, workers, kind, use_hs=False):
    """a model from the corpus' counts at the state's rates: alpha0 and the floor at a quarter of it"""
    import torch
    cfg = dge.make_config(D, c.W, c.NV, negative=c.K, min_count=1, epochs=c.EP, workers=workers, alpha=A0[kind], min_alpha=A0[kind] / 4, seed=SEED, table_size=TABLE,
                          update_policy=policy, use_hs=use_hs)
    return dge.SgnsModel.create(cfg, torch.from_numpy(c.cnt).to("cuda:0"), 0)


def _launch_whole(m, corpus, c):
    m.train(corpus)


def _check(dge, oracle, key, D, policy, workers, kernel, knobs=None, reported=None, use_hs=False, relaxed=False, launch=_launch_whole, ref_kw=None, quick_below=3,
           many_walks=False):
    """One row of the matrix: per worker count and state a model from the corpus' counts, the state imported, `launch` (one launch of the whole corpus unless the
    case says otherwise), the tables compared.  One or two workers run QUICK; `relaxed`: what is not exact by design with several workers."""
    c = _corpus(key)
    ref = _reference(oracle, c, D, use_hs=use_hs, **(ref_kw or {}))
    corpus = dge.WalkCorpus.from_host(c.ids, 0)
    stride = -(-D // 64) * 64
    knobs = knobs or {}
    for w in workers:
        runs = [r for r in (QUICK if 0 < w < quick_below and c.T > 8000 else RUNS) if r in ref]
        for kind in sorted({r[0] for r in runs}):          # (the rate is part of the model's configuration: a model per state)
            m = _model(dge, c, D, policy, w, kind, use_hs)
            for run in [r for r in runs if r[0] == kind]:
                r = ref[run]
                assert np.array_equal(m.vectors()[1], r.vocab_ids)
                _import_state(dge, m, r.st, stride)
                m.reset_stats()
                with dge.tuning(**knobs):
                    _knobs_in_force(dge, knobs)
                    launch(m, corpus, c)
                    stats, sch, name = m.stats(), m.schedule(), m.kernel()
                label = "%s D=%d policy=%d workers=%d (%d) %s run %s [%s, %.0f ms]" % (key, D, policy, w, sch["workers"], knobs or "", run, name, stats["kernel_ms"])
                assert stats["pairs"] == r.pairs, label
                in_order = w == 1 and policy == 0
                if in_order:
                    assert name == (IN_ORDER_HS if use_hs else "k_sgns_train<in-order>"), label
                else:
                    assert kernel in name, label
                    assert reported is None or sch["update_policy"] == reported, (label, sch)
                    assert "hot_rows" not in knobs or sch["hot_rows"] == min(knobs["hot_rows"], r.V), (label, sch)
                assert w == 1 or policy == 8 or sch["workers"] > 1, (label, sch)
                if many_walks and w == 0:
                    assert 1 < sch["workers"] < len(c.ids), (label, sch)          # device-filling, and still more than one walk for some worker
                _compare(_read_tables(m, D, use_hs), r, run, label, relaxed=relaxed if w != 1 else False)
            m.close()
    corpus.close()


ALL_W = (1, 2, 48, 0)


# ------------------------------------------------------------------------------------------ atomics: k_sgns_train<.., 2, ..>
@pytest.mark.parametrize("key,D", [("uniform16", 64), ("ragged", 130), ("long", 64)])
def test_atomics_graded(dge, oracle, key, D):
    """2 and 48 workers on uniform16 take their walks from the launch-wide counter (4 096 >= 32 x workers), the device-filling launch and every count on the shorter
    corpora by the static stride"""
    _check(dge, oracle, key, D, 2, ALL_W, "k_sgns_train<atomics>", reported=2, many_walks=key == "uniform16")


# ------------------------------------------------------------------------------------------ small rows: k_sgns_train_small
@pytest.mark.parametrize("key,D", [("uniform16", 17), ("ragged", 32)])
def test_small_rows_graded(dge, oracle, key, D):
    """(small_rows = 1: half a wave a worker with ONE worker as well, where the plan would otherwise take k_sgns_train)"""
    _check(dge, oracle, key, D, 2, ALL_W, "k_sgns_train_small<atomics, 32 lanes a worker>", knobs=dict(small_rows=1), reported=2, many_walks=key == "uniform16")


# ------------------------------------------------------------------------------------------ owner-computes: sgns_sorted.hip
@pytest.mark.parametrize("key,D,chunk,walks", [("uniform16", 64, 7, 37), ("ragged", 100, 64, 1000), ("ragged", 64, 3, 37)])
def test_owner_computes_graded(dge, oracle, key, D, chunk, walks):
    """a mini-batch of sorted_walks walks trains at the rate of its FIRST walk (the items carry no rate); sorted_chunk 7 and 3 split a row's items over work units"""
    _check(dge, oracle, key, D, 8, (0,), "k_sorted_phase (owner-computes:", knobs=dict(sorted_chunk=chunk, sorted_walks=walks), reported=8, ref_kw=dict(sorted_=(chunk, walks)))


# ------------------------------------------------------------------------------------------ strict commit locks: k_sgns_train_locked<strict>
@pytest.mark.parametrize("static", [0, 1])
@pytest.mark.parametrize("key,D", [("uniform16", 64), ("ragged", 256)])
def test_strict_commit_locks_graded(dge, oracle, key, D, static):
    """static_walks 1: the static stride at every worker count; 0: the launch-wide counter where the launch has 32 walks a worker"""
    _check(dge, oracle, key, D, 6, ALL_W, "k_sgns_train_locked<strict>", knobs=dict(static_walks=static), reported=6, many_walks=key == "uniform16")


# ------------------------------------------------------------------------------------------ relaxed commit locks: exact with one worker, bounded with many
@pytest.mark.parametrize("static", [0, 1])
def test_relaxed_commit_locks_graded(dge, oracle, static):
    _check(dge, oracle, "uniform16", 64, 5, (1, 48, 0), "k_sgns_train_locked<relaxed>", knobs=dict(static_walks=static), reported=5, relaxed=True, many_walks=True)


# ------------------------------------------------------------------------------------------ the mixed kernel, the head covering the table
@pytest.mark.parametrize("acc,drain,static", [(0, 1, 0), (16, 1, 0), (0, NEVER, 0), (16, NEVER, 0), (16, NEVER, 1)])
def test_mixed_kernel_head_graded(dge, oracle, acc, drain, static):
    """hot_rows = V: every row through the workgroup's atomics wave and its LDS accumulator banks — exact at every worker count"""
    V = _corpus("uniform16").V
    _check(dge, oracle, "uniform16", 64, 7, ALL_W, "k_sgns_train_locked<relaxed, head rows by atomics>", knobs=dict(hot_rows=V, acc_rows=acc, acc_drain=drain, static_walks=static),
           reported=7, many_walks=True)


# ------------------------------------------------------------------------------------------ the tree forms, balanced state
def _hsw_name(centre, D):
    if centre == 0:
        return PAIR_BY_PAIR
    if centre == 1:
        return "k_sgns_train_hsw<atomics, 3 waves>"
    return "k_sgns_train_hsw<negatives under commit locks, head rows by atomics" + (", 7 waves>" if centre == 3 and D <= 128 else ", 3 waves>")


@pytest.mark.parametrize("D", [64, 256])
@pytest.mark.parametrize("centre", [0, 1, 2, 3])
def test_tree_forms_graded(dge, oracle, centre, D):
    """pair by pair and the three wave-per-centre forms (2 / 3 with hot_rows = V: syn1neg by atomics, so that all three tables are exact, as
    tests/test_gpu_conservation_balanced.py claims them); hs_cold = 0: no read-modify-write class.  The root takes a term a pair: pairs x 2^8 < 2^24.  One worker
    under auto runs in order."""
    _check(dge, oracle, "tree", D, 0, ALL_W, _hsw_name(centre, D), knobs=dict(hs_centre=centre, hs_cold=0, **({"hot_rows": 115} if centre >= 2 else {})),
           reported=(7 if centre >= 2 else 2), use_hs=True)


# ------------------------------------------------------------------------------------------ the block schedule (PART): the prefetched tokens-before
@pytest.mark.parametrize("key,policy,D,workers,knobs,kernel", [
    ("uniform16", 2, 64, 0, {}, "k_sgns_train<atomics, one block>"),
    ("uniform16", 7, 64, 0, dict(hot_rows=1 << 20, acc_rows=16, acc_drain=4), "k_sgns_train_locked<relaxed, head rows by atomics, one block>"),
    ("uniform16", 7, 128, 0, dict(hot_rows=1 << 20, acc_rows=0), "k_sgns_train_locked<relaxed, head rows by atomics, one block>"),
    ("uniform16", 8, 100, 0, dict(sorted_chunk=64, sorted_walks=1000), "k_sorted_phase (owner-computes, one block"),
    ("ragged", 5, 64, 1, {}, "k_sgns_train_locked<relaxed, one block>"),
    ("ragged", 5, 128, 1, dict(watchdog_ms=0), "k_sgns_train_locked<relaxed, one block>"),
    ("uniform16", 2, 64, 0, dict(force_segments=1, segment_shift=3), "k_sgns_train<atomics, one block>"),
    ("uniform16", 7, 64, 0, dict(hot_rows=1 << 20, acc_rows=16, acc_drain=NEVER, force_segments=1, segment_shift=3), "k_sgns_train_locked<relaxed, head rows by atomics, one block>")])
def test_block_schedule_graded(dge, oracle, key, policy, D, workers, knobs, kernel):
    """three models on one device play the ranks; the one-block forms carry the NEXT walk's tokens and tokens-before one walk ahead (walk_fetch): every block trains
    a walk at the walk's own rate, as the oracle's nine blocks do (part_n = 3)"""
    N = 3
    c = _corpus(key)
    ref = _reference(oracle, c, D, part_n=N, sorted_=(knobs["sorted_chunk"], knobs["sorted_walks"]) if policy == 8 else None)
    corpus = dge.WalkCorpus.from_host(c.ids, 0)
    stride = -(-D // 64) * 64
    for kind in ("sat", "bal"):
        ms = [_model(dge, c, D, policy, workers, kind) for _ in range(N)]
        for run in [r for r in (QUICK if workers == 1 else RUNS) if r[0] == kind]:
            r = ref[run]
            names = set()
            for m in ms:
                _import_state(dge, m, r.st, stride); m.reset_stats()

            def train(m):
                m.train(corpus); names.add(m.kernel())
            with dge.tuning(**knobs):
                _knobs_in_force(dge, knobs)
                simulate_block_schedule(ms, train)
                simulate_gather_syn0(ms)
            label = "blocks %s policy=%d D=%d workers=%d %s run %s %s" % (key, policy, D, workers, knobs, run, sorted(names))
            assert len(names) == 1 and kernel in names.pop(), label
            assert sum(m.stats()["pairs"] for m in ms) == r.pairs, label
            for m in ms:
                if "hot_rows" in knobs:
                    assert m.schedule()["hot_rows"] == min(knobs["hot_rows"], r.V), (label, m.schedule())
                _compare(_read_tables(m, D, False), r, run, label)          # every rank ends with the whole of both tables
        for m in ms:
            m.close()
    corpus.close()


# ------------------------------------------------------------------------------------------ the launch parameters
FORMS = [(2, "k_sgns_train<atomics>", {}, (48, 0)), (6, "k_sgns_train_locked<strict>", {}, (48, 0)),
         (8, "k_sorted_phase (owner-computes:", dict(sorted_chunk=7, sorted_walks=37), (0,))]
FORM_IDS = ["atomics", "strict-locks", "owner-computes"]


def _sorted_of(knobs):
    return (knobs["sorted_chunk"], knobs["sorted_walks"]) if knobs else None


@pytest.mark.parametrize("policy,kernel,knobs,workers", FORMS, ids=FORM_IDS)
def test_two_launches_equal_one(dge, oracle, policy, kernel, knobs, workers):
    """the corpus in two launches — row0, words_before and walk_index_base set for the second (cut on a mini-batch boundary: 55 x 37 walks) — against the expected
    tables of the ONE launch: bit for bit"""
    h = 55 * 37

    def launch(m, corpus, c):
        m.train(corpus, 0, h)
        m.train(corpus, h, len(c.ids) - h, walk_index_base=h, words_before=int(c.wb[h]))
    _check(dge, oracle, "uniform16", 64, policy, workers, kernel, knobs=knobs, reported=policy, launch=launch, ref_kw=dict(sorted_=_sorted_of(knobs)))


@pytest.mark.parametrize("policy,kernel,knobs,workers", FORMS, ids=FORM_IDS)
def test_three_epochs(dge, oracle, policy, kernel, knobs, workers):
    """cfg.epochs = 3, a launch an epoch: words_done_base = epoch * total_words, all_words = 3 * total_words = 2^12 - 1; the oracle runs its three epochs in one call"""
    def launch(m, corpus, c):
        for ep in range(3):
            m.train(corpus, epoch=ep)
    _check(dge, oracle, "tiny3", 64, policy, workers if policy == 8 else workers + (2,), kernel, knobs=knobs, reported=policy, launch=launch, ref_kw=dict(sorted_=_sorted_of(knobs)))


@pytest.mark.parametrize("policy,kernel,knobs,workers", FORMS, ids=FORM_IDS)
def test_words_scale_two(dge, oracle, policy, kernel, knobs, workers):
    """words_scale = 2.0 on the first half of the corpus: done = 2 wb against 2^16 is the oracle's wb against 2^15 (total_words = 2^15 - 1 told to it) — the same
    dyadic rate exactly; every walk holds 16 tokens: 11 lattice bits"""
    c = _corpus("uniform16")
    half = len(c.ids) // 2

    def launch(m, corpus, c):
        m.train(corpus, 0, half, words_scale=2.0)
    _check(dge, oracle, "uniform16", 64, policy, workers, kernel, knobs=knobs, reported=policy, launch=launch,
           ref_kw=dict(sorted_=_sorted_of(knobs), n_rows=half, total_words=(1 << (c.m - 1)) - 1, b=c.b - 1))


_WITNESS = {}


@pytest.mark.parametrize("policy,kernel,knobs,workers", FORMS, ids=FORM_IDS)
def test_words_scale_half_truncates(dge, oracle, policy, kernel, knobs, workers):
    """words_scale = 0.5 on a ragged corpus: wb is odd for half the walks and (int64)(wb * 0.5) truncates.  The oracle has no words_scale: the expectation is the int64
    witness — enumerate_terms with each term's walk, helpers.rate_level with words_scale = (1, 2) (under owner-computes: of the mini-batch's first walk)."""
    from test_oracle_kats import enumerate_terms
    c = _corpus("tiny")
    assert (c.wb % 2 == 1).sum() > len(c.wb) // 4
    if "terms" not in _WITNESS:
        m0 = oracle.train_sgns(c.ids, c.NV, 8, c.W, negative=c.K, min_count=1, epochs=0, seed=SEED, table_size=TABLE, counts=c.cnt)
        _WITNESS["terms"] = enumerate_terms(c.ids, m0.vocab_ids.tolist(), m0.table(TABLE), c.W, c.K, SEED, with_walk=True)
    per = knobs.get("sorted_walks", 1)
    first = (np.arange(len(c.ids)) // per) * per
    if per not in _WITNESS:
        _WITNESS[per] = (_WITNESS["terms"], np.array([[rate_level(c.wb[w], 0, 0, c.T, 1, c.b, words_scale=(1, 2)) for w in first]], np.int64))
    assert (_WITNESS[per][1] != np.array([[rate_level(c.wb[w], 0, 0, c.T, 1, c.b) for w in first]])).any()

    def launch(m, corpus, c):
        m.train(corpus, words_scale=0.5)
    _check(dge, oracle, "tiny", 64, policy, workers if policy == 8 else workers + (2,), kernel, knobs=knobs, reported=policy, launch=launch, ref_kw=dict(sorted_=_sorted_of(knobs), witness=_WITNESS[per]))


@pytest.mark.parametrize("policy,kernel,knobs,workers", FORMS, ids=FORM_IDS)
def test_walk_and_train_graded(dge, oracle, policy, kernel, knobs, workers):
    """dge_model_walk_and_train samples the walks into the corpus and trains them in one call; the rows are read back afterwards, and the rates are those of the walks
    it sampled: 1 024 full walks of 4 tokens over a 4-slice graph without dead ends (m = 12, b = 10), the counts those of the walks (one lowered by one)."""
    key, n, L, R, D = "walked", 1024, 4, 40, 64
    src, dst, w, sources = layered_graph(R=R, T=L, deg=5, seed=2)
    g = dge.DeviceGraph(0); g.add_edges(src, dst, w); g.set_sources(sources); g.build_alias(True)
    corpus = g.sample_walks_device(n, L, seed=5)
    ids = corpus.to_host()
    assert ids.shape == (n, L) and (ids >= 0).all()
    if key not in _CORPORA:
        cnt = np.bincount(ids.reshape(-1), minlength=R * L).astype(np.int64); cnt[int(np.argmax(cnt))] -= 1
        _CORPORA[key] = types.SimpleNamespace(key=key, ids=ids, NV=R * L, cnt=cnt, T=int(cnt.sum()), EP=1, m=12, b=10, W=3, K=5, V=int((cnt >= 1).sum()),
                                              wb=np.arange(n, dtype=np.int64) * L)
    c = _corpus(key)
    assert np.array_equal(c.ids, ids) and c.T + 1 == 1 << c.m
    ref = _reference(oracle, c, D, sorted_=_sorted_of(knobs))
    for wk in workers:
        for kind in ("sat", "bal"):
            m = _model(dge, c, D, policy, wk, kind)
            for run in [r for r in RUNS if r[0] == kind]:
                r = ref[run]
                _import_state(dge, m, r.st, 64)
                m.reset_stats()
                with dge.tuning(**knobs):
                    _knobs_in_force(dge, knobs)
                    m.walk_and_train(g, corpus, 0, n, walk_seed=5, walk_index_base=0)
                    stats, name = m.stats(), m.kernel()
                label = "walk_and_train policy=%d workers=%d run %s [%s]" % (policy, wk, run, name)
                assert np.array_equal(corpus.to_host(), ids), label          # the walks it trained
                assert stats["pairs"] == r.pairs and kernel in name, label
                _compare(_read_tables(m, D, False), r, run, label)
            m.close()
    corpus.close(); g.close()
