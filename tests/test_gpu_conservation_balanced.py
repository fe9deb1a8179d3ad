"""GPU: exact update conservation for the tree term and for the sigmoid-table path of every kernel form, at every worker count.

tests/test_gpu_conservation.py holds the kernels to "every update exactly once, on the right row, with the right sign and rate" in the SATURATED regime, where every
score is clamped: the table look-up is never taken and the tree step is skipped.  Here every launch runs in the BALANCED regime (helpers.balanced_state): column 0 puts
every score at 2^-5, inside the bin of exp_table[500] = 0.5 exactly (idx = (int)((f + 6) * 83): f in [0.024096, 0.036145)), so every tree term is
g = (1 - code - 0.5) * alpha = +/- alpha/2 and every negative-sampling term g = (label - 0.5) * alpha = +/- alpha/2 — through s_exp[idx], no clamp, no skip.  With
alpha = min_alpha = 2^-60 the accumulating tables hold 2^-61 x (a signed sum of small integers), exact in any order below 2^24 units (balanced_diff asserts the bound
from host quantities: a syn1 row takes at most `pairs` terms, a syn1neg row pairs * (K + 1), a syn0 row (its token count) * 2W * (K + 1 + longest code); codes up to 3
where that fits, +/- 1 where it does not), and what flows back into the standing tables is absorbed.  So the trained tables DO NOT DEPEND on the order of the
additions, on atomics against locks, on registers, copies or LDS accumulators, or on the number of workers — unless a (pair, node) or (pair, target) term is lost,
doubled, sent to the wrong row, given the wrong code bit or the wrong rate.  Run A lets syn1 and syn1neg accumulate (syn0 stands), run B syn0 (through a pair's neu1e:
tree nodes and negative-sampling targets together).  Column 1 is a NET count (terms with g > 0 minus terms with g < 0), so messages speak of rows and units of alpha/2.

Expected tables: the sequential oracle from the same state (its own witness, and the proof that balanced_diff catches one dropped / doubled / bit-flipped / misrouted
term: tests/test_oracle_kats.py::test_balanced_regime_equals_int64_sums).  Every case asserts the kernel that ran and reads every set knob back.

On every table of every case ("always"): pairs equal, the standing tables and column 0 bit-unchanged, rows the oracle leaves untouched untouched (a row whose D-1
oracle sums are all zero counts as untouched), whole multiples of alpha/2 on every row, padding columns and the spare row behind syn1 zero.  Bit equality with the
oracle on every table the form's design makes exact — everything but (a) syn1neg under the RELAXED commit locks of k_sgns_train_hsw<negatives under commit locks>
without a head by atomics and with several workers (a lost re-lock race drops the update: by design, bounded in tests/test_gpu_conservation.py), and (b) syn1 rows of
the hs_cold class with several workers (plain read-modify-write: a concurrent update of the same row can be lost, by design, on nodes the counts call rare).  Those
keep the "always" list and are exact with one worker."""
import concurrent.futures as cf

import numpy as np
import pytest

from helpers import BAL_ALPHA, SAT_CAP, balanced_diff, balanced_state, bits, simulate_block_schedule, simulate_gather_syn0
from test_gpu_conservation import NEVER, SEED, TABLE, _corpus, _import_state, _knobs_in_force, _read_tables, _slim

pytestmark = pytest.mark.gpu

ACC = {"A": ("syn1neg", "syn1"), "B": ("syn0",)}          # the tables that accumulate in a run (syn1: with the tree term)
PAIR_BY_PAIR = "k_sgns_train<atomics, hierarchical softmax pair by pair>"
IN_ORDER_HS = "k_sgns_train<in-order, hierarchical softmax pair by pair>"


def _bal_corpus(key):
    """(walks, NV, counts that make the vocabulary and the tree).  The saturated file's corpora with their own token counts, and "deep": 300 vertices, 6 000 ragged
    walks of up to 24 tokens, counts[:27] = 2^(36 - i) above a bushy tail — the longest Huffman code is 37, longer than the 24 (D <= 128) or 12 (D > 128) path nodes a
    wave of k_sgns_train_hsw holds in registers (the corpus of test_hierarchical_softmax_wave_per_centre_linear_regime)."""
    if key == "deep600":
        ids, NV, counts = _bal_corpus("deep")
        return ids[:600], NV, counts
    if key != "deep":
        ids, NV = _corpus(key)
        return ids, NV, np.bincount(ids[ids >= 0], minlength=NV).astype(np.int64)
    if key not in _DEEP:
        rng = np.random.default_rng(1311)
        NV, n, L = 300, 6000, 24
        ids = rng.integers(0, NV, (n, L)).astype(np.int32)
        ids[np.arange(L)[None, :] >= rng.integers(2, L + 1, n)[:, None]] = -1
        counts = rng.integers(1, 5, NV).astype(np.int64)
        counts[:27] = 2 ** (36 - np.arange(27, dtype=np.int64))
        _DEEP[key] = (ids, NV, counts)
    return _DEEP[key]


_DEEP, _EXPECTED, _PAIRS, _POOL, _KEYS = {}, {}, {}, [], []


def _case(key, D, W, K, use_hs=False, part_n=0):
    """registers one (corpus, D, W, K, tree term, ranks) of the matrix below: its expected tables are computed ahead, on host threads"""
    k = (key, D, W, K, use_hs, part_n)
    if k not in _KEYS:
        _KEYS.append(k)
    return k


@pytest.fixture(scope="module", autouse=True)
def _release_module_state():
    """the host threads and the cached expected tables live as long as this module's tests, not the session"""
    yield
    while _POOL:
        _POOL.pop().shutdown(wait=True, cancel_futures=True)
    _EXPECTED.clear(); _DEEP.clear(); _PAIRS.clear()


def _oracle_runs(oracle, k):
    """runs A and B of the sequential oracle for one registered case; codes up to 3 where the term bound fits, +/- 1 where it does not.  The premises are asserted on
    the reference here."""
    key, D, W, K, use_hs, part_n = k
    ids, NV, cnt = _bal_corpus(key)
    V = int((cnt >= 1).sum())
    tokens = int(np.bincount(ids[ids >= 0], minlength=NV).max())
    longest = int(oracle.huffman(np.sort(cnt[cnt >= 1])[::-1])[0].max()) if use_hs else 0
    assert not (use_hs and key.startswith("deep")) or longest == 37          # longer than the register-resident part of a path

    def terms(pairs):
        t = {"syn1neg": pairs * (K + 1), "syn0": tokens * 2 * W * (K + 1 + longest)}
        return dict(t, syn1=pairs) if use_hs else t
    for mag in (3, 1):
        if (key, W) in _PAIRS and mag > 1 and mag * max(terms(_PAIRS[key, W]).values()) >= SAT_CAP:
            continue          # (the pair count of a corpus and window is known from an earlier case: it does not depend on D, K or the codes)
        runs = {}
        for side in "AB":
            st = balanced_state(V, D, side, seed=SEED, mag=mag, use_hs=use_hs)
            runs[side] = (st, _slim(oracle.train_sgns(ids, NV, D, W, negative=K, min_count=1, epochs=1, seed=SEED, table_size=TABLE, alpha=BAL_ALPHA, min_alpha=BAL_ALPHA,
                                                      arith=1, counts=cnt, syn0_init=st["syn0"], syn1neg_init=st["syn1neg"], syn1_init=st.get("syn1"), use_hs=use_hs,
                                                      part_n=part_n)))
            _PAIRS[key, W] = runs[side][1].pairs
            if mag * max(terms(_PAIRS[key, W]).values()) >= SAT_CAP:
                break
        else:
            break
    bound = {t: mag * n for t, n in terms(_PAIRS[key, W]).items()}
    for side, (st, om) in runs.items():
        assert om.V == V and om.pairs == _PAIRS[key, W]
        for t in st:
            if t in ACC[side]:          # (asserts column 0, whole multiples and the term bound on the reference)
                d = balanced_diff(getattr(om, t), getattr(om, t), st[t], bound[t])
                assert d.exact and d.whole.all() and np.abs(d.net_want).max() > 0
            else:
                assert np.array_equal(bits(getattr(om, t)), bits(st[t])), "the reference's standing %s moved" % t
    assert set(runs) == {"A", "B"}
    return dict(runs=runs, bound=bound, mag=mag)


def _expected(oracle, key, D, W, K, use_hs=False, part_n=0):
    """{"runs": {side: (initial state, oracle model)}, "bound": {table: mag x the most terms a row can take}, "mag"} of one registered case: the same for every
    schedule, computed once a module.  The first call sends every registered case to four host threads, so that the oracle works while the device does."""
    k = (key, D, W, K, use_hs, part_n)
    if not _POOL:
        for kk in _KEYS + [k]:
            _bal_corpus(kk[0])          # (the corpora are made here, not on the threads)
        _POOL.append(cf.ThreadPoolExecutor(max_workers=4))
        for kk in _KEYS:
            _EXPECTED[kk] = _POOL[0].submit(_oracle_runs, oracle, kk)
    if k not in _EXPECTED:
        _EXPECTED[k] = _POOL[0].submit(_oracle_runs, oracle, k)
    return _EXPECTED[k].result()


def _compare(tables, st, om, side, bound, label, loose=()):
    """the standing tables bit-unchanged; every accumulating table through the "always" list, and bit-equal to the oracle unless it is named in `loose`"""
    for t in st:
        got, want = tables[t], getattr(om, t)
        if t not in ACC[side]:
            assert np.array_equal(bits(got), bits(st[t])), "%s: the standing %s moved" % (label, t)
            continue
        assert np.array_equal(bits(got[:, 0]), bits(st[t][:, 0])), "%s: column 0 of %s moved" % (label, t)
        d = balanced_diff(got, want, st[t], bound[t])
        print("%s: %s %d of %d rows differ, the worst by %g units of alpha/2" % (label, t, int((d.diff != 0).sum()), len(d.diff), d.diff.max()))
        assert d.whole.all(), "%s: %s holds a fraction of a term — %s" % (label, t, d.worst())
        idle = ~(want[:, 1:] != 0).any(1)
        assert np.array_equal(bits(got[idle]), bits(st[t][idle])), "%s: a row of %s the oracle leaves untouched moved" % (label, t)
        if t not in loose:
            assert d.exact, "%s: %s — %s" % (label, t, d.worst())
            assert np.array_equal(bits(got), bits(want)), "%s: %s" % (label, t)


def _model_counts(dge, key, corpus):
    import torch
    ids, NV, cnt = _bal_corpus(key)
    if key.startswith("deep"):
        return torch.from_numpy(cnt).to("cuda:0")
    counts = torch.zeros(NV, dtype=torch.int64, device="cuda:0"); corpus.count_tokens(NV, counts)
    return counts


def _check(dge, oracle, key, D, K, W=5, policy=0, workers=(0, 48), use_hs=False, knobs=None, kernel=None, reported=None, loose=(), launch=None):
    """One row of the matrix: a model from the corpus' counts, per worker count the two balanced states imported, one launch each, the tables compared.
    `kernel`: what dge_model_kernel must name with several workers (one worker under policy 0 runs in order), `reported`: the policy dge_model_schedule must report,
    `loose`: the tables that are not exact by design with several workers (the module's docstring) — exact with one.  `launch(m, corpus)`: trains the corpus in
    the model's place (one launch of the whole corpus, and whatever the case asks of the model while the knobs are still set)."""
    ids, NV, _ = _bal_corpus(key)
    exp = _expected(oracle, key, D, W, K, use_hs)
    corpus = dge.WalkCorpus.from_host(ids, 0)
    counts = _model_counts(dge, key, corpus)
    stride = -(-D // 64) * 64
    knobs = knobs or {}
    for w in workers:
        cfg = dge.make_config(D, W, NV, negative=K, min_count=1, epochs=1, workers=w, alpha=BAL_ALPHA, min_alpha=BAL_ALPHA, seed=SEED, table_size=TABLE,
                              update_policy=policy, use_hs=use_hs)
        m = dge.SgnsModel.create(cfg, counts, 0)
        for side in "AB":
            st, om = exp["runs"][side]
            assert np.array_equal(m.vectors()[1], om.vocab_ids)
            _import_state(dge, m, st, stride)
            m.reset_stats()
            with dge.tuning(**knobs):
                _knobs_in_force(dge, knobs)
                m.train(corpus) if launch is None else launch(m, corpus)
                stats, sch, name = m.stats(), m.schedule(), m.kernel()
            label = "%s D=%d K=%d W=%d mag=%d policy=%d workers=%d %s run %s [%s, %.0f ms]" % (key, D, K, W, exp["mag"], policy, w, knobs or "", side, name, stats["kernel_ms"])
            assert stats["pairs"] == om.pairs, label
            in_order = w == 1 and policy == 0
            if in_order:
                assert name == (IN_ORDER_HS if use_hs else "k_sgns_train<in-order>"), label
            elif kernel is not None:
                assert kernel in name, label
            if reported is not None and not in_order:
                assert sch["update_policy"] == reported, (label, sch)
            assert w == 1 or policy == 8 or sch["workers"] > 1, (label, sch)
            if "hot_rows" in knobs and not in_order:
                assert sch["hot_rows"] == min(knobs["hot_rows"], om.V), (label, sch)
            _compare(_read_tables(m, D, use_hs), st, om, side, exp["bound"], label, loose=() if w == 1 else loose)
        m.close()
    corpus.close()


def _hsw_name(centre, D, head):
    if centre == 0:
        return PAIR_BY_PAIR
    if centre == 1:
        return "k_sgns_train_hsw<atomics, 3 waves>"
    return "k_sgns_train_hsw<negatives under commit locks" + (", head rows by atomics" if head else "") + (", 7 waves>" if centre == 3 and D <= 128 else ", 3 waves>")


# ====================================================================================================== the tree term
DEEP = {20: (5, 8), 64: (20, 5), 100: (0, 24), 128: (5, 24), 256: (5, 24)}          # D -> (K, W): K = 20 (two draw rounds a pair) on 64, no negatives on 100
TREE = dict(use_hs=True, policy=0)


# ------------------------------------------------------------------------------------------ every tree form on the deep tree
for _D, (_K, _W) in DEEP.items():
    _case("deep", _D, _W, _K, True)
# (measured: the pair-by-pair form takes 4.5 s a case at 128 floats and 48 workers, a locked tail — 300 rows under heavy contention — 10 s at 128 floats and 28 s with
#  20 negatives: those forms run on one dim per row width (1, 2 and 4 chunks of 64 floats), the locked tails on 20, 100 and 256 floats — 5, 0 and 5 negatives — and
#  with 48 workers next to the device-filling count only where there is no negative to wait for; pair by pair at 256 floats with the device-filling count only)
FORMS = [(D, centre, head, (0, 48)) for centre, head in ((1, False), (2, True), (3, True)) for D in sorted(DEEP)] + [(D, 0, False, (0, 48) if D < 256 else (0,)) for D in (64, 100, 256)] + \
        [(D, centre, False, (0, 48) if D == 100 else (0,)) for centre in (2, 3) for D in (20, 100, 256)]


@pytest.mark.parametrize("D,centre,head,workers", FORMS)
def test_tree_forms_on_the_deep_tree(dge, oracle, D, centre, head, workers):
    """hs_centre 0: k_sgns_train<atomics, hierarchical softmax pair by pair>; 1: k_sgns_train_hsw<atomics, 3 waves>; 2 / 3: the negatives under commit locks in workgroups
    of three / seven waves (rows of more than 128 floats have no seven-wave form: the plan reports 3 waves), with hot_rows = V the whole of syn1neg by atomics.  Paths of
    up to 37 nodes: beyond the register-resident part of a path the nodes go pair by pair.  syn0 and syn1 are exact in every form.  syn1neg is exact under atomics
    (centre 0 / 1, or the head covering the table); on a locked tail with several workers it is under the RELAXED commit (not exact by design): the "always" list there
    (one worker: test_tree_one_worker_exact)."""
    K, W = DEEP[D]
    locked_tail = centre >= 2 and not head
    _check(dge, oracle, "deep", D, K, W=W, workers=workers, knobs=dict(hs_centre=centre, hs_cold=0, **({"hot_rows": 300} if head else {})),
           kernel=_hsw_name(centre, D, head), reported=(7 if head else 5) if centre >= 2 else 2, loose=("syn1neg",) if locked_tail else (), **TREE)


# ------------------------------------------------------------------------------------------ the busiest inner nodes in copies, folded after the launch
_case("zipf", 64, 5, 5, True); _case("zipf", 256, 5, 5, True)


@pytest.mark.parametrize("copies", [1, 2, 16])
@pytest.mark.parametrize("key,D,centre", [(key, D, centre) for key in ("zipf", "deep") for D in (64, 256) for centre in (1, 3)])
def test_tree_copies_fold_exactly(dge, oracle, key, D, centre, copies):
    """k_sgns_train_hsw keeps the inner nodes on a tenth of all paths and more in up to hs_copies copies (the root, which takes every pair, in all of them) behind
    syn1's rows; k_hs_rep_fold adds them up after the launch: row + the sum of its copies is exact, and the spare row behind the table is zero again (_read_tables).
    Centre 3 carries hot_rows = V: syn1neg by atomics, so that all three tables are exact.  (On these 300-row vocabularies the device-filling launch has V/8 = 37
    waves in flight; 48 next to it says nothing new about the copies, and is left to the forms above.)"""
    K, W = DEEP[D] if key == "deep" else (5, 5)
    V = int((_bal_corpus(key)[2] >= 1).sum())
    _check(dge, oracle, key, D, K, W=W, workers=(0,), knobs=dict(hs_centre=centre, hs_cold=0, hs_copies=copies, **({"hot_rows": V} if centre == 3 else {})),
           kernel=_hsw_name(centre, D, centre == 3), **TREE)


# ------------------------------------------------------------------------------------------ LDS accumulators instead of copies
@pytest.mark.parametrize("drain", [1, 64, 10**9])
@pytest.mark.parametrize("centre,kb", [(1, 15), (1, 30), (3, 15), (3, 30)])
def test_tree_lds_accumulators_exact(dge, oracle, centre, kb, drain):
    """hs_hot_kb > 0: the nodes nearest the root add up in LDS (hot_add) and are drained every hs_drain additions — "never" (10^9): by the block-wide drain at the
    kernel's end only"""
    K, W = DEEP[64]
    _check(dge, oracle, "deep", 64, K, W=W, workers=(0,), knobs=dict(hs_centre=centre, hs_cold=0, hs_hot_kb=kb, hs_drain=drain, **({"hot_rows": 300} if centre == 3 else {})),
           kernel=_hsw_name(centre, 64, centre == 3), **TREE)


# ------------------------------------------------------------------------------------------ pair by pair: with and without the workgroup's atomics wave
@pytest.mark.parametrize("wave", [0, 1])
def test_tree_pair_by_pair_atomics_wave(dge, oracle, wave):
    K, W = DEEP[64]
    _check(dge, oracle, "deep", 64, K, W=W, knobs=dict(hs_centre=0, hs_cold=0, hs_wave=wave), kernel=PAIR_BY_PAIR, reported=2, **TREE)


# ------------------------------------------------------------------------------------------ BIG: per-segment table descriptors
@pytest.mark.parametrize("centre", [0, 1])
def test_tree_segmented_addressing(dge, oracle, centre):
    """force_segments with 8 rows a segment: a path's nodes lie in different segments.  The wave-per-centre kernels have no segmented build (sgns_plan.h: `!big`), so
    hs_centre = 1 falls to the pair-by-pair form too — the name the plan reports is asserted."""
    K, W = DEEP[64]
    _check(dge, oracle, "deep", 64, K, W=W, knobs=dict(hs_centre=centre, hs_cold=0, force_segments=1, segment_shift=3), kernel=PAIR_BY_PAIR, reported=2, **TREE)


# ------------------------------------------------------------------------------------------ the DeepWalk default path: the schedule auto picks
AUTO = [("flat", 256, 20), ("zipf", 128, 5), ("long", 130, 17)]
for _key, _D, _K in AUTO:
    _case(_key, _D, 5, _K, True)


@pytest.mark.parametrize("key,D,K", AUTO)
def test_tree_auto_schedule(dge, oracle, key, D, K):
    """no hs_centre: below 65 536 vocabulary rows auto trains the tree pair by pair under atomics, the nodes nearest the root in LDS accumulators"""
    _check(dge, oracle, key, D, K, knobs=dict(hs_cold=0), kernel=PAIR_BY_PAIR, reported=2, **TREE)


# ------------------------------------------------------------------------------------------ the cold class
@pytest.mark.parametrize("key,D,centre", [("zipf", 64, None), ("deep", 64, 0), ("deep", 64, 1)])
def test_tree_default_hs_cold(dge, oracle, key, D, centre):
    """hs_cold left to the plan: inner nodes on fewer than 2e-5 of the paths BY THE COUNTS are updated by plain read-modify-write — NOT exact by design with several
    workers (two updates of one row in flight: one is lost).  zipf: the corpus' own counts (the default path; on 28 710 tokens 2e-5 of the paths is less than one, so the class is empty).  deep:
    counts of 2^37 in all make the whole bushy tail cold while the corpus visits it all the time, so the class is really reached.  syn1 with several workers: the
    "always" list; syn0 and syn1neg (no cold class there) exact; one worker: test_tree_one_worker_exact."""
    K, W = DEEP[D] if key == "deep" else (5, 5)
    knobs = {} if centre is None else dict(hs_centre=centre)
    _check(dge, oracle, key, D, K, W=W, knobs=knobs, kernel=PAIR_BY_PAIR if not centre else _hsw_name(centre, D, False), reported=2, loose=("syn1",), **TREE)


# ------------------------------------------------------------------------------------------ what is not exact by design with many workers is exact with one
_case("deep600", 64, 5, 20, True); _case("deep600", 256, 24, 5, True)


@pytest.mark.parametrize("D", [64, 256])
def test_tree_one_worker_exact(dge, oracle, D):
    """One worker under auto runs the tree in order (k_sgns_train<in-order, ..>) whatever hs_centre says, with the commit locks and the cold class out of the picture:
    with the knobs of the two classes above in force (negatives under commit locks; hs_cold left to the plan, the bushy tail cold by the counts), every table is
    bit-equal to the oracle.  The first 600 walks of the deep corpus: one worker trains 1e5 pairs of 40 terms a second."""
    K, W = DEEP[D]
    _check(dge, oracle, "deep600", D, K, W=W, workers=(1,), knobs=dict(hs_centre=3), kernel=IN_ORDER_HS, reported=0, **TREE)


# ------------------------------------------------------------------------------------------ the block schedule (PART)
_case("flat", 64, 5, 5, True, 3)


def _check_blocks(dge, oracle, D, K, policy, workers, knobs, kernel, use_hs):
    """three models on one device play the ranks of the block schedule; the oracle runs the same nine blocks (part_n = 3: negatives moved into the target partition,
    inner nodes split by node % 3)"""
    key, W, N = "flat", 5, 3
    ids, NV, _ = _bal_corpus(key)
    exp = _expected(oracle, key, D, W, K, use_hs, part_n=N)
    corpus = dge.WalkCorpus.from_host(ids, 0)
    counts = _model_counts(dge, key, corpus)
    stride = -(-D // 64) * 64
    cfg = dge.make_config(D, W, NV, negative=K, min_count=1, epochs=1, workers=workers, alpha=BAL_ALPHA, min_alpha=BAL_ALPHA, seed=SEED, table_size=TABLE,
                          update_policy=policy, use_hs=use_hs)
    ms = [dge.SgnsModel.create(cfg, counts, 0) for _ in range(N)]
    for side in "AB":
        st, om = exp["runs"][side]
        names = set()
        for m in ms:
            _import_state(dge, m, st, stride); m.reset_stats()

        def train(m):
            m.train(corpus); names.add(m.kernel())
        with dge.tuning(**knobs):
            _knobs_in_force(dge, knobs)
            simulate_block_schedule(ms, train)
            simulate_gather_syn0(ms)
        label = "blocks policy=%d D=%d K=%d workers=%d hs=%d %s run %s %s" % (policy, D, K, workers, use_hs, knobs, side, sorted(names))
        assert len(names) == 1 and kernel in names.pop(), label
        assert sum(m.stats()["pairs"] for m in ms) == om.pairs, label
        for m in ms:          # every rank ends with the whole of every table
            _compare(_read_tables(m, D, use_hs), st, om, side, exp["bound"], label)
    for m in ms:
        m.close()
    corpus.close()


@pytest.mark.parametrize("workers,kernel", [(1, "k_sgns_train<in-order, hierarchical softmax pair by pair, one block>"),
                                            (0, "k_sgns_train<atomics, hierarchical softmax pair by pair, one block>")])
def test_tree_block_schedule(dge, oracle, workers, kernel):
    """the form test_block_schedule_bit_exact_with_oracle runs with the tree term (one in-order worker a rank), and the Hogwild form the library accepts with it:
    atomics on all three tables.  Commit locks with the tree term are refused when the model is made."""
    _check_blocks(dge, oracle, 64, 5, 0, workers, dict(hs_cold=0), kernel, True)
    if workers == 0:
        import torch
        for pol in (5, 7):
            with pytest.raises(dge.DgeError):
                dge.SgnsModel.create(dge.make_config(64, 5, 6000, negative=5, min_count=1, workers=0, update_policy=pol, use_hs=True), torch.ones(6000, dtype=torch.int64, device="cuda:0"), 0)


# ====================================================================================================== negative sampling through the sigmoid table
NS = dict(use_hs=False)
for _k in (("zipf", 100, 5, 17), ("zipf", 500, 5, 5), ("zipf", 20, 5, 30), ("l64", 32, 5, 5), ("flat", 130, 5, 5), ("flat", 128, 5, 5), ("zipf", 64, 5, 5), ("zipf", 256, 5, 5),
           ("long", 256, 5, 5)):
    _case(*_k)
_case("flat", 64, 5, 5, False, 3); _case("flat", 100, 5, 5, False, 3)


@pytest.mark.parametrize("key,D,K", [("zipf", 100, 17), ("zipf", 500, 5)])
def test_table_path_atomics(dge, oracle, key, D, K):
    _check(dge, oracle, key, D, K, policy=2, kernel="k_sgns_train<atomics>", reported=2, **NS)


@pytest.mark.parametrize("key,D,K", [("zipf", 20, 30), ("l64", 32, 5)])
def test_table_path_small_rows(dge, oracle, key, D, K):
    _check(dge, oracle, key, D, K, policy=2, kernel="k_sgns_train_small<atomics, 32 lanes a worker>", reported=2, **NS)


@pytest.mark.parametrize("key,D,K,knobs", [("flat", 130, 5, dict(sorted_chunk=256)), ("zipf", 100, 17, dict(sorted_chunk=7, sorted_walks=37))])
def test_table_path_owner_computes(dge, oracle, key, D, K, knobs):
    """several mini-batches a launch: within one the context rows are frozen — in this regime nothing a term reads depends on what another wrote"""
    _check(dge, oracle, key, D, K, policy=8, workers=(0,), knobs=knobs, kernel="k_sorted_phase (owner-computes:", reported=8, **NS)


def test_table_path_strict_commit_locks(dge, oracle):
    _check(dge, oracle, "flat", 128, 5, policy=6, kernel="k_sgns_train_locked<strict>", reported=6, **NS)


@pytest.mark.parametrize("D", [64, 256])
def test_table_path_mixed_kernel_head(dge, oracle, D):
    """hot_rows = V: the whole of both tables through the workgroup's atomics wave and its LDS accumulator banks, flushed when the workgroup ends only"""
    V = int((_bal_corpus("zipf")[2] >= 1).sum())
    _check(dge, oracle, "zipf", D, 5, policy=7, knobs=dict(hot_rows=V, acc_rows=16, acc_drain=NEVER), kernel="k_sgns_train_locked<relaxed, head rows by atomics>", reported=7, **NS)


def test_table_path_relaxed_commit_one_worker(dge, oracle):
    """the relaxed commit loses a re-lock race now and then with several workers (by design; bounded in tests/test_gpu_conservation.py) — one worker waits for nobody"""
    _check(dge, oracle, "long", 256, 5, policy=5, workers=(1,), kernel="k_sgns_train_locked<relaxed>", reported=5, **NS)


@pytest.mark.parametrize("policy,D,knobs,kernel", [(2, 64, {}, "k_sgns_train<atomics, one block>"),
                                                   (8, 100, dict(sorted_chunk=64, sorted_walks=1000), "k_sorted_phase (owner-computes, one block")])
def test_table_path_block_schedule(dge, oracle, policy, D, knobs, kernel):
    _check_blocks(dge, oracle, D, 5, policy, 0, knobs, kernel, False)
