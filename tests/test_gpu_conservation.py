"""GPU: exact update conservation for every kernel form of the SGNS trainer, at every worker count.

The other parity tests compare Hogwild launches with the oracle at "1e-4 cosine on every row" (an angle of 0.014 rad, and blind to a row's norm) or statistically:
a row that takes a few hundred updates can lose one and stay inside.  Here every launch runs in the SATURATED regime (helpers.saturated_state): column 0 of both
tables pushes every score beyond MAX_EXP, so word2vec's clamp makes every negative term exactly -alpha (sign +1) or every positive term exactly +alpha (sign -1),
alpha = min_alpha = 2^-40, and the table that does not stand still accumulates 2^-40 x (a sum of small integers).  All products and partial sums are exact below
2^24, so the trained table DOES NOT DEPEND on the order of the additions, on atomics against locks, on LDS accumulators or on the number of workers — unless an
update is lost, doubled, sent to the wrong row, or applied with the wrong sign or learning rate.  Column 1 (the count channel), divided by alpha, is the number of
updates the row took.  Run A lets syn1neg accumulate, run B syn0 (the path through a pair's neu1e, the centre deltas, the syn0 atomics of the mixed kernels).

Expected tables: the sequential oracle from the same state (its own witness is the int64 enumeration of tests/test_oracle_kats.py::test_saturated_regime_equals_int64_sums).
Every case asserts the kernel / schedule that ran, so that each instantiation plan_train can choose (sgns_kernels.h: launch_train_b; sgns_sorted.hip) is reached.
With use_hs, syn1 saturates too: the tree step is skipped and syn1 must come back unchanged.  The tree term's own arithmetic, and the sigmoid-table path that
saturation never takes, are held to the same exactness in the balanced regime of tests/test_gpu_conservation_balanced.py.
SGNS half of the oracle: a restatement of word2vec.c / DL4J (J/DeepWalk.java:73-79), parity unpinned — DESIGN.md §3."""
import concurrent.futures as cf
import ctypes
import types

import numpy as np
import pytest

from helpers import SAT_ALPHA, bits, conservation_diff, device_rows, device_table, saturated_state, simulate_block_schedule, simulate_gather_syn0

pytestmark = pytest.mark.gpu

SEED, TABLE = 7, 100_003
RUNS = [(side, sign) for side in "AB" for sign in (1, -1)]
NEVER = 1 << 20          # acc_drain: the LDS accumulators are flushed when the workgroup ends only
MAG = 3                  # largest code magnitude of the standing table (helpers.saturated_state)


def _ragged(rng, ids, L, holes=0.05):
    ids = ids.astype(np.int32)
    ids[np.arange(L)[None, :] >= rng.integers(0, L + 1, len(ids))[:, None]] = -1
    ids[rng.random(ids.shape) < holes] = -1
    return ids


_CORPORA = {}


def _corpus(key):
    """(walks int32 [n x L], NV).  zipf: 300 vertices, a quarter of all tokens on one of them, ragged walks of up to 24 tokens with holes; flat: 6 000 vertices
    (device-filling launches get thousands of workers; the forced commit locks are accepted); long: walks of 100 tokens (the kernels' memory token path);
    l3 / l64: walks of 3 and of exactly 64 tokens; wide: a 17-bit row count."""
    if key not in _CORPORA:
        rng = np.random.default_rng(sum(map(ord, key)))
        if key == "zipf":
            NV, n, L = 300, 2500, 24
            ids = np.minimum(rng.zipf(1.25, size=(n, L)) - 1, NV - 1)
            ids[rng.random(ids.shape) < 0.25] = 0
            ids = _ragged(rng, ids, L)
        elif key == "flat":
            NV, n, L = 6000, 12000, 12
            ids = _ragged(rng, rng.integers(0, NV, (n, L)), L, holes=0.02)
        elif key == "long":
            NV, n, L = 300, 400, 100
            ids = _ragged(rng, np.minimum(rng.zipf(1.3, size=(n, L)) - 1, NV - 1), L)
            ids[:40] = rng.integers(0, NV, (40, L))                 # full-length walks among them
        elif key == "l3":
            NV, n, L = 200, 6000, 3
            ids = _ragged(rng, rng.integers(0, NV, (n, L)), L)
        elif key == "l64":
            NV, n, L = 300, 1000, 64
            ids = np.minimum(rng.zipf(1.3, size=(n, L)) - 1, NV - 1).astype(np.int32)
        elif key == "wide":
            NV, n, L = 140_000, 20000, 12
            ids = rng.integers(0, NV, (n, L)).astype(np.int32)
            ids[:, 0] = rng.integers(0, 40, n)                      # a few busy rows whose item lists span work units
        _CORPORA[key] = (ids, NV)
    return _CORPORA[key]


_EXPECTED = {}
_POOL = []


def _pool():
    if not _POOL:
        _POOL.append(cf.ThreadPoolExecutor(max_workers=4))
    return _POOL[0]


@pytest.fixture(scope="module", autouse=True)
def _release_module_state():
    """the host threads and the cached expected tables live as long as this module's tests, not the session"""
    yield
    while _POOL:
        _POOL.pop().shutdown()
    _EXPECTED.clear(); _CORPORA.clear()


def _slim(om):
    """what the comparisons need of an oracle model, as plain arrays (the model and its C memory are released)"""
    return types.SimpleNamespace(syn0=om.syn0, syn1neg=om.syn1neg, syn1=om.syn1, pairs=om.pairs, vocab_ids=om.vocab_ids, V=om.V)


def _expected(oracle, key, D, W, K, use_hs=False, part_n=0):
    """{(side, sign): (initial state, oracle model)} of one (corpus, D, W, K, tree term, ranks): the same for every schedule, computed once a module (the four
    sequential runs side by side on host threads)."""
    k = (key, D, W, K, use_hs, part_n)
    if k not in _EXPECTED:
        ids, NV = _corpus(key)
        cnt = np.bincount(ids[ids >= 0], minlength=NV).astype(np.int64)
        V = int((cnt >= 1).sum())
        fut = {}
        for side, sign in RUNS:
            st = saturated_state(V, D, side, sign, seed=SEED, mag=MAG, use_hs=use_hs)
            fut[side, sign] = (st, _pool().submit(oracle.train_sgns, ids, NV, D, W, negative=K, min_count=1, epochs=1, seed=SEED, table_size=TABLE, alpha=SAT_ALPHA,
                                                min_alpha=SAT_ALPHA, arith=1, counts=cnt, syn0_init=st["syn0"], syn1neg_init=st["syn1neg"], syn1_init=st.get("syn1"),
                                                use_hs=use_hs, part_n=part_n))
        _EXPECTED[k] = {r: (st, _slim(f.result())) for r, (st, f) in fut.items()}
        for (side, sign), (st, om) in _EXPECTED[k].items():          # the premise, on the reference: one table stands still, the other is inside the summable range
            standing = "syn0" if side == "A" else "syn1neg"
            assert np.array_equal(bits(getattr(om, standing)), bits(st[standing]))
            assert conservation_diff(getattr(om, "syn1neg" if side == "A" else "syn0"), getattr(om, "syn1neg" if side == "A" else "syn0")).exact
            assert not use_hs or np.array_equal(bits(om.syn1), bits(st["syn1"]))
    return _EXPECTED[k]


def _import_state(dge, m, st, stride):
    import torch
    V = st["syn0"].shape[0]
    for t, name in ((0, "syn0"), (1, "syn1neg"), (2, "syn1")):
        if name in st:
            m.import_partition(t, 1, 0, torch.from_numpy(device_rows(st[name], stride, rows=V)).to(m.torch_device).view(-1))


def _read_tables(m, D, use_hs):
    """the tables as they lie in device memory, [V x stride]: the padding columns (and, behind syn1's V-1 rows, the first spare row) must be zero"""
    out = {}
    for t, name in ((0, "syn0"), (1, "syn1neg")) + (((2, "syn1"),) if use_hs else ()):
        full = device_table(m, t).cpu().numpy()
        assert not full[:, D:].any(), "%s: padding columns moved" % name
        if name == "syn1":
            assert not full[-1].any(), "syn1: the spare row behind the table is not zero after the launch"
            full = full[:-1]
        out[name] = full[:, :D]
    return out


def _assert_conserved(got, want, init, label, exact_rows=None):
    """The assertions every comparison of an accumulating table shares.  On ALL rows: whole updates only, never a surplus or a wrong sign, a row the oracle leaves
    untouched is untouched, and — the bound the project states for the relaxed commit (test_commit_lock_protocol_conservation) — a deficit of at most
    max(2, 10 % of the row's expected count), the other columns within the largest code magnitude times that.  On `exact_rows` (None: every row): zero deficit and
    every column bit-equal to the oracle.  -> Conservation"""
    c = conservation_diff(got, want)
    exp = np.abs(c.expected)
    worst = int(np.argmax(c.deficit))
    print("%s: %d updates expected, %d lost (%.3g), %d rows short, worst row %d: %d of %d; %d rows differ" % (
        label, int(exp.sum()), int(c.deficit.sum()), c.deficit.sum() / max(int(exp.sum()), 1), int((c.deficit != 0).sum()), worst, int(c.deficit[worst]), int(exp[worst]),
        int(((c.got != c.expected) | (c.other != 0)).sum())))
    assert (c.got == np.rint(c.got)).all(), "%s: a fraction of an update — %s" % (label, c.worst())
    assert (c.deficit >= 0).all() and (c.got * np.sign(c.expected) >= 0).all(), "%s: a surplus — %s" % (label, c.worst())
    assert np.array_equal(bits(got[exp == 0]), bits(init[exp == 0])), "%s: a row the oracle leaves untouched moved" % label
    allowed = np.maximum(2, np.floor(0.10 * exp))
    assert (c.deficit <= allowed).all() and (c.other <= MAG * allowed).all(), "%s: beyond max(2, 10 %%) of a row's updates — %s" % (label, c.worst())
    rows = slice(None) if exact_rows is None else exact_rows
    assert (c.deficit[rows] == 0).all() and (c.other[rows] == 0).all(), "%s: %s" % (label, c.worst())
    assert np.array_equal(bits(got[rows]), bits(want[rows])), label
    return c


def _compare(tables, st, om, side, use_hs, label, exact_rows=None):
    """the standing table (and a saturated syn1) bit-unchanged, the accumulating one through _assert_conserved"""
    moving, standing = ("syn1neg", "syn0") if side == "A" else ("syn0", "syn1neg")
    assert np.array_equal(bits(tables[standing]), bits(st[standing])), "%s: %s moved" % (label, standing)
    if use_hs:
        assert np.array_equal(bits(tables["syn1"]), bits(st["syn1"])), "%s: syn1 moved (the tree step is skipped at |f| >= 6)" % label
    return _assert_conserved(tables[moving], getattr(om, moving), st[moving], label, exact_rows)


def _knobs_in_force(dge, knobs):
    """the tuning knobs read back from the library while they are set: a misspelt or ignored knob must not leave a case green on another path"""
    for k, v in knobs.items():
        got = ctypes.c_int64(-12345)
        assert dge.lib.dge_get_tuning(dge.engine.TUNING_KNOBS[k], ctypes.byref(got)) == 0 and got.value == int(v), (k, v, got.value)


def _check(dge, oracle, key, D, K, W=5, policy=0, workers=(0,), use_hs=False, knobs=None, kernel=None, reported=None, exact_head=None, runs=RUNS):
    """One row of the matrix: a model from the corpus' counts, per (run, sign) and worker count the saturated state imported, one launch, the tables compared.
    `kernel`: what dge_model_kernel must name (a substring), `reported`: the policy dge_model_schedule must report.  exact_head = (rows, rows): with several workers
    only syn1neg rows [0, rows[0]) / syn0 rows [0, rows[1]) are claimed exact — the rest is under the relaxed commit: bounded per row as _assert_conserved says."""
    import torch
    ids, NV = _corpus(key)
    exp = _expected(oracle, key, D, W, K, use_hs)
    corpus = dge.WalkCorpus.from_host(ids, 0)
    counts = torch.zeros(NV, dtype=torch.int64, device="cuda:0"); corpus.count_tokens(NV, counts)
    stride = -(-D // 64) * 64
    for w in workers:
        cfg = dge.make_config(D, W, NV, negative=K, min_count=1, epochs=1, workers=w, alpha=SAT_ALPHA, min_alpha=SAT_ALPHA, seed=SEED, table_size=TABLE,
                              update_policy=policy, use_hs=use_hs)
        m = dge.SgnsModel.create(cfg, counts, 0)
        for side, sign in runs:
            st, om = exp[side, sign]
            assert np.array_equal(m.vectors()[1], om.vocab_ids)
            _import_state(dge, m, st, stride)
            m.reset_stats()
            with dge.tuning(**(knobs or {})):
                _knobs_in_force(dge, knobs or {})
                m.train(corpus)
                stats, sch, name = m.stats(), m.schedule(), m.kernel()
            label = "%s D=%d K=%d policy=%d workers=%d %s run %s sign %+d [%s]" % (key, D, K, policy, w, knobs or "", side, sign, name)
            assert stats["pairs"] == om.pairs, label
            if kernel is not None:
                assert kernel in name, label
            if reported is not None:
                assert sch["update_policy"] == reported, (label, sch)
            assert w == 1 or policy == 8 or sch["workers"] > 1, (label, sch)
            if "hot_rows" in (knobs or {}):
                assert sch["hot_rows"] == min(knobs["hot_rows"], om.V), (label, sch)          # the head the case names is the head that ran
            rows = None
            if exact_head is not None and w != 1:
                rows = slice(0, exact_head[0] if side == "A" else exact_head[1])
            _compare(_read_tables(m, D, use_hs), st, om, side, use_hs, label, rows)
        m.close()
    corpus.close()


# ------------------------------------------------------------------------------------------ atomics: k_sgns_train<.., 2, ..>
@pytest.mark.parametrize("key,D,K", [("zipf", 64, 5), ("zipf", 100, 17), ("zipf", 130, 0), ("flat", 256, 5), ("zipf", 500, 5), ("long", 64, 5), ("long", 130, 17)])
def test_atomics_exact(dge, oracle, key, D, K):
    _check(dge, oracle, key, D, K, policy=2, workers=(0, 48), kernel="k_sgns_train<atomics>", reported=2)


# ------------------------------------------------------------------------------------------ small rows: k_sgns_train_small
@pytest.mark.parametrize("key,D,K", [("l3", 17, 0), ("zipf", 20, 30), ("l64", 32, 5), ("l3", 32, 30)])
def test_small_rows_exact(dge, oracle, key, D, K):
    _check(dge, oracle, key, D, K, policy=2, workers=(0, 48), kernel="k_sgns_train_small<atomics, 32 lanes a worker>", reported=2)


# ------------------------------------------------------------------------------------------ owner-computes: sgns_sorted.hip
@pytest.mark.parametrize("key,D,K,knobs", [("flat", 64, 5, dict(sorted_chunk=64, sorted_walks=1000)), ("zipf", 100, 17, dict(sorted_chunk=7, sorted_walks=37)),
                                           ("wide", 20, 5, dict(sorted_chunk=64, sorted_walks=1000)), ("long", 256, 0, dict(sorted_chunk=16, sorted_walks=50)),
                                           ("flat", 130, 5, dict(sorted_chunk=256))])
def test_owner_computes_exact(dge, oracle, key, D, K, knobs):
    """several mini-batches a launch: within one the context rows are frozen — in this regime nothing reads what another term wrote, so the sequential oracle is the reference"""
    _check(dge, oracle, key, D, K, W=4 if key == "wide" else 5, policy=8, workers=(0,), knobs=knobs, kernel="k_sorted_phase (owner-computes:", reported=8)


# ------------------------------------------------------------------------------------------ strict commit locks: k_sgns_train_locked<strict>
@pytest.mark.parametrize("D", [64, 128, 256])
def test_strict_commit_locks_exact(dge, oracle, D):
    _check(dge, oracle, "flat", D, 5, policy=6, workers=(0, 48), kernel="k_sgns_train_locked<strict>", reported=6)


# ------------------------------------------------------------------------------------------ the mixed kernel: k_sgns_train_locked<relaxed, head rows by atomics>
@pytest.mark.parametrize("key,D,hot,acc,drain", [("zipf", 64, "V", 0, 16), ("zipf", 64, "V", 16, 1), ("zipf", 128, "V", 16, 16), ("zipf", 256, "V", 16, NEVER),
                                                 ("flat", 64, "V", 16, NEVER), ("zipf", 64, "V/2", 16, 16), ("flat", 128, "V/2", 0, 16), ("zipf", 100, 4, 16, NEVER)])
def test_mixed_kernel_head_exact(dge, oracle, key, D, hot, acc, drain):
    """The head [0, hot_rows) goes through the workgroup's atomics wave and its LDS accumulator banks: exact at every worker count (hot_rows = V: the whole table).
    A tail row — under the relaxed commit — is exact with one worker and may only ever lose with many (bounded in test_relaxed_commit_*)."""
    ids, NV = _corpus(key)
    V = int((np.bincount(ids[ids >= 0], minlength=NV) >= 1).sum())
    hot_rows = {"V": V, "V/2": V // 2}.get(hot, hot)
    _check(dge, oracle, key, D, 5, policy=7, workers=(0, 48) if hot == "V" else (0, 1), knobs=dict(hot_rows=hot_rows, acc_rows=acc, acc_drain=drain),
           kernel="k_sgns_train_locked<relaxed, head rows by atomics>", reported=7, exact_head=(hot_rows, hot_rows))


# ------------------------------------------------------------------------------------------ relaxed commit, one worker: exact like the rest
@pytest.mark.parametrize("key,D,knobs", [("zipf", 64, {}), ("long", 256, {}), ("zipf", 128, dict(watchdog_ms=0)), ("zipf", 64, dict(force_segments=1, segment_shift=3))])
def test_relaxed_commit_one_worker_exact(dge, oracle, key, D, knobs):
    """forced policy 5 runs the watchdog's instantiation of the kernel; watchdog_ms = 0 switches the watchdog OFF (sgns_plan.h: wd_ticks 0), which is the instantiation
    auto launches — one worker waits for nobody"""
    _check(dge, oracle, key, D, 5, policy=5, workers=(1,), knobs=knobs, kernel="k_sgns_train_locked<relaxed>", reported=5)


# ------------------------------------------------------------------------------------------ the tree kernels' negative-sampling part
@pytest.mark.parametrize("D", [64, 256])
@pytest.mark.parametrize("centre,hot", [(0, None), (1, None), (2, None), (2, "V"), (3, None), (3, "V")])
def test_tree_kernels_negative_sampling_part_exact(dge, oracle, D, centre, hot):
    """use_hs with a saturated syn1: the tree step is skipped, 20 negatives (two draw rounds) remain.  hs_centre 0: k_sgns_train<atomics, hierarchical softmax pair by
    pair>; 1: k_sgns_train_hsw<atomics>; 2 / 3: the negatives under commit locks in workgroups of three / seven waves (relaxed: exact where the head covers the table —
    hot_rows = V; without a head the syn1neg rows are bounded per row as _assert_conserved says, syn0 — never locked by these kernels — is exact)."""
    ids, NV = _corpus("flat")
    V = int((np.bincount(ids[ids >= 0], minlength=NV) >= 1).sum())
    knobs = dict(hs_centre=centre, **({"hot_rows": V} if hot else {}))
    if centre == 0:
        kernel = "k_sgns_train<atomics, hierarchical softmax pair by pair>"
    elif centre == 1:
        kernel = "k_sgns_train_hsw<atomics, 3 waves>"
    else:
        kernel = "k_sgns_train_hsw<negatives under commit locks" + (", head rows by atomics" if hot else "") + (", 7 waves>" if centre == 3 and D <= 128 else ", 3 waves>")
    locked_tail = centre >= 2 and not hot
    _check(dge, oracle, "flat", D, 20, policy=0, workers=(0, 48) if D == 64 else (0,), use_hs=True, knobs=knobs, kernel=kernel, exact_head=(0, V) if locked_tail else None)


# ------------------------------------------------------------------------------------------ BIG: per-segment table descriptors
@pytest.mark.parametrize("policy,D,kernel,extra", [(2, 130, "k_sgns_train<atomics>", {}), (6, 128, "k_sgns_train_locked<strict>", {}),
                                                   (7, 64, "k_sgns_train_locked<relaxed, head rows by atomics>", dict(hot_rows=1 << 20, acc_rows=16, acc_drain=NEVER)),
                                                   (2, 64, "k_sgns_train<atomics, hierarchical softmax pair by pair>", {})])
def test_segmented_addressing_exact(dge, oracle, policy, D, kernel, extra):
    """force_segments with 8 rows a segment: the rows of one pair lie in different segments (the knobs are read back while set: _knobs_in_force; the kernel's name
    does not say which addressing it was built with)"""
    hs = "hierarchical" in kernel
    _check(dge, oracle, "flat", D, 20 if hs else 5, policy=policy, workers=(0,), use_hs=hs, knobs=dict(force_segments=1, segment_shift=3, **extra), kernel=kernel)


# ------------------------------------------------------------------------------------------ the block schedule (PART)
@pytest.mark.parametrize("policy,D,workers,knobs,kernel", [
    (2, 64, 0, {}, "k_sgns_train<atomics, one block>"),
    (7, 64, 0, dict(hot_rows=1 << 20, acc_rows=16, acc_drain=4), "k_sgns_train_locked<relaxed, head rows by atomics, one block>"),
    (7, 128, 0, dict(hot_rows=1 << 20, acc_rows=0), "k_sgns_train_locked<relaxed, head rows by atomics, one block>"),
    (8, 100, 0, dict(sorted_chunk=64, sorted_walks=1000), "k_sorted_phase (owner-computes, one block"),
    (5, 64, 1, {}, "k_sgns_train_locked<relaxed, one block>"),
    (5, 128, 1, dict(watchdog_ms=0), "k_sgns_train_locked<relaxed, one block>"),
    (2, 64, 0, dict(force_segments=1, segment_shift=3), "k_sgns_train<atomics, one block>"),
    (7, 64, 0, dict(hot_rows=1 << 20, acc_rows=16, acc_drain=NEVER, force_segments=1, segment_shift=3), "k_sgns_train_locked<relaxed, head rows by atomics, one block>")])
def test_block_schedule_exact(dge, oracle, policy, D, workers, knobs, kernel):
    """three models on one device play the ranks of the block schedule; the oracle runs the same nine blocks (part_n = 3: negatives moved into the target partition)"""
    import torch
    key, K, W, N = "flat", 5, 5, 3
    ids, NV = _corpus(key)
    exp = _expected(oracle, key, D, W, K, part_n=N)
    corpus = dge.WalkCorpus.from_host(ids, 0)
    counts = torch.zeros(NV, dtype=torch.int64, device="cuda:0"); corpus.count_tokens(NV, counts)
    stride = -(-D // 64) * 64
    cfg = dge.make_config(D, W, NV, negative=K, min_count=1, epochs=1, workers=workers, alpha=SAT_ALPHA, min_alpha=SAT_ALPHA, seed=SEED, table_size=TABLE, update_policy=policy)
    ms = [dge.SgnsModel.create(cfg, counts, 0) for _ in range(N)]
    for side, sign in RUNS:
        st, om = exp[side, sign]
        names = set()
        for m in ms:
            _import_state(dge, m, st, stride); m.reset_stats()

        def train(m):
            m.train(corpus); names.add(m.kernel())
        with dge.tuning(**knobs):
            _knobs_in_force(dge, knobs)
            simulate_block_schedule(ms, train)
            simulate_gather_syn0(ms)
        label = "blocks policy=%d D=%d workers=%d %s run %s sign %+d %s" % (policy, D, workers, knobs, side, sign, sorted(names))
        assert len(names) == 1 and kernel in names.pop(), label
        assert sum(m.stats()["pairs"] for m in ms) == om.pairs, label
        for m in ms:
            if "hot_rows" in knobs:
                assert m.schedule()["hot_rows"] == min(knobs["hot_rows"], om.V), (label, m.schedule())
            ls = m.lock_stats()
            assert 0 <= ls["rounds_short"] <= ls["rounds"] and ls["pairs_put_back"] >= 0, (label, ls)
            if workers == 1:
                assert ls["pairs_put_back"] == 0, (label, ls)          # one worker never finds its context row taken (a round can still be short: a draw repeats a row it holds)
            _compare(_read_tables(m, D, False), st, om, side, False, label)          # every rank ends with the whole of both tables
    for m in ms:
        m.close()
    corpus.close()


# ------------------------------------------------------------------------------------------ relaxed commit at device-filling concurrency: bounded, and counted
T_SLICES, L_WALK, D_BIG, K_BIG, W_BIG = 24, 24, 64, 5, 5
N_COUNT, N_TRAIN = 400_000, 40_000
NV_UNIFORM = 250_000


@pytest.fixture(scope="module")
def relaxed(dge, oracle):
    """Three vocabularies on which auto itself picks the relaxed commit, a short corpus each (the counts of 400 000 walks of 24 tokens make the vocabulary, the first
    40 000 are trained, window 5), device-filling:
      uniform   — 250 000 vertices drawn uniformly: no busy row, auto takes the commit locks on EVERY row (policy 5, the headline kernel as auto launches it: no watchdog);
      community — the flat 480 000-vertex community graph of tests/test_gpu_quality.py: a handful of busy source rows, so auto takes policy 5 or the mixed kernel with those
                  few rows as its head (as that file finds it);
      zipf      — its Zipf 348 000-vertex community graph: the mixed kernel (7), a head of tens of thousands of rows by atomics, the tail under the relaxed commit.
    Per (run, sign) only the accumulating table and the pair count of the oracle are kept."""
    import torch
    from embedding_amd import synth
    dev = "cuda:0"
    out = {}
    pool = cf.ThreadPoolExecutor(max_workers=8)
    try:
        for name, R, dst in (("uniform", 0, None), ("community", 20000, "community"), ("zipf", 14500, "community_zipf")):
            g = None
            if name == "uniform":
                NV = NV_UNIFORM
                corpus = dge.WalkCorpus.from_host(np.random.default_rng(11).integers(0, NV, (N_COUNT, L_WALK)).astype(np.int32), 0)
            else:
                NV = R * T_SLICES
                G = synth.flow_graph_torch(R, T_SLICES, 30, dev, dst=dst)
                g = dge.DeviceGraph(0); g.add_edges_device(G["src"], G["dst"], G["w"]); g.set_sources(G["sources"]); del G
                g.build_alias(False)
                corpus = g.sample_walks_device(N_COUNT, L_WALK, seed=5)
            counts = torch.zeros(NV, dtype=torch.int64, device=dev); corpus.count_tokens(NV, counts)
            cnt = counts.cpu().numpy()
            V = int((cnt >= 2).sum())
            sl = corpus.to_host()[:N_TRAIN]
            fut = {}
            for side, sign in RUNS:
                st = saturated_state(V, D_BIG, side, sign, seed=SEED, mag=MAG)
                fut[side, sign] = (st, pool.submit(oracle.train_sgns, sl, NV, D_BIG, W_BIG, negative=K_BIG, min_count=2, epochs=1, seed=SEED, table_size=10_000_000,
                                                   alpha=SAT_ALPHA, min_alpha=SAT_ALPHA, arith=1, counts=cnt, syn0_init=st["syn0"], syn1neg_init=st["syn1neg"],
                                                   total_walks=N_COUNT))
            m = dge.SgnsModel.create(dge.make_config(D_BIG, W_BIG, NV, negative=K_BIG, min_count=2, epochs=1, workers=0, alpha=SAT_ALPHA, min_alpha=SAT_ALPHA, seed=SEED,
                                                     table_size=10_000_000), counts, 0)
            runs = {}
            for (side, sign), (st, _) in fut.items():
                moving, standing = ("syn1neg", "syn0") if side == "A" else ("syn0", "syn1neg")
                _import_state(dge, m, st, 64)
                m.reset_stats()
                m.train(corpus, 0, N_TRAIN, total_walks=N_COUNT)
                tables = _read_tables(m, D_BIG, False)
                runs[side, sign] = dict(stats=m.stats(), sch=m.schedule(), kernel=m.kernel(), got=tables[moving], init=st[moving],
                                        standing_unchanged=np.array_equal(bits(tables[standing]), bits(st[standing])))
            m.close(); corpus.close()
            if g is not None:
                g.close()
            torch.cuda.empty_cache()
            for r, (st, f) in fut.items():
                om = f.result()
                runs[r].update(want=getattr(om, "syn1neg" if r[0] == "A" else "syn0"), pairs=om.pairs)
            fut.clear()
            out[name] = dict(V=V, runs=runs)
        yield out
    finally:
        pool.shutdown()
        out.clear()


@pytest.mark.parametrize("name", ["uniform", "community", "zipf"], ids=["uniform-auto5-k_sgns_train_locked<relaxed>", "community-auto5-or-7-with-a-head-below-64-rows",
                                                                         "zipf-auto7-k_sgns_train_locked<relaxed, head rows by atomics>"])
def test_relaxed_commit_loss_is_bounded_and_counted(relaxed, name):
    """The relaxed commit loses a re-lock race now and then, by design.  Per row and sign (_assert_conserved): never a surplus, untouched rows untouched, a deficit of at
    most max(2, 10 % of the row's expected count), the other columns within the largest code (3) times that; under the mixed kernel the head [0, hot_rows) is exact.
    The measured totals are printed (DESIGN.md §5.1 holds one run's)."""
    o = relaxed[name]
    mixed = "k_sgns_train_locked<relaxed, head rows by atomics>"
    for (side, sign), d in o["runs"].items():
        sch = d["sch"]
        label = "%s vocabulary (%d rows), auto -> %s, %d workers, hot_rows %d; run %s (%s accumulates), sign %+d (%s)" % (
            name, o["V"], d["kernel"], sch["workers"], sch["hot_rows"], side, "syn1neg" if side == "A" else "syn0", sign, "negatives" if sign > 0 else "positives")
        if name == "uniform":        # the headline kernel, as auto launches it
            assert sch["update_policy"] == 5 and d["kernel"] == "k_sgns_train_locked<relaxed>" and sch["hot_rows"] == 0, label
        elif name == "community":
            assert (sch["update_policy"], d["kernel"]) in ((5, "k_sgns_train_locked<relaxed>"), (7, mixed)) and sch["hot_rows"] < 64, label
        else:
            assert sch["update_policy"] == 7 and d["kernel"] == mixed and 1000 < sch["hot_rows"] < o["V"] // 4, label
        assert sch["workers"] > 1000, label
        assert d["stats"]["pairs"] == d["pairs"] and d["standing_unchanged"], label
        _assert_conserved(d["got"], d["want"], d["init"], label, exact_rows=slice(0, sch["hot_rows"]))
