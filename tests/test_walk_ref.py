"""tests/walk_ref.py on its own: the second reading of the graph half is sound, stays inside its own conditions and is sensitive to the faults it is
meant to see — before any device is asked (tests/test_gpu_graph_exact.py).  CPU only.

The oracle appears here as the thing under test, not as the reference: its tables have to encode w / 2^m exactly on lattice weights, and its walks have
to be the ones the witness replays from those tables."""
import json
import os

import numpy as np
import pytest

import walk_ref as W
from helpers import layered_graph

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KS = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025)
M = 20


# ------------------------------------------------------------------------------------------- java.util.Random
def test_java_random_known_answers_and_jump():
    for case in json.load(open(os.path.join(GOLD, "java_random_kats.json")))["cases"]:
        r = W.JavaRandom(case["seed"])
        if "next_int" in case:
            assert r.next_int() == case["next_int"]
        else:
            assert r.next_double() == case["next_double"]
    for seed in (0, 12345, -1, -(1 << 63), (1 << 40) + 3):
        a = W.JavaRandom(seed)
        seq = [a.next_double() for _ in range(300)]
        assert all(0.0 <= x < 1.0 for x in seq)
        for o in (0, 1, 2, 7, 63, 64, 255, 299):                       # the jump equals stepping
            assert W.JavaRandom.before_draw(seed, o).next_double() == seq[o]
        assert W.stream_doubles(seed, 0, 300).tolist() == seq            # and so does the many-lane form, at lane counts that do and do not divide
        assert W.stream_doubles(seed, 17, 283).tolist() == seq[17:]
        assert W.stream_doubles(seed, 299, 1).tolist() == seq[299:]
    big = (1 << 40) + 5                                                  # far jumps compose: o + 3 is o, then three draws
    r = W.JavaRandom.before_draw(-7, big)
    for _ in range(3):
        r.next_double()
    assert r.s == W.JavaRandom.before_draw(-7, big + 3).s
    assert W.stream_doubles(-7, big, 2500)[-1] == W.JavaRandom.before_draw(-7, big + 2499).next_double()


# ------------------------------------------------------------------------------------------- the edge store
def test_csr_of_keeps_insertion_order_and_running_sums():
    src = [2, 0, 2, 2, 0, 4]; dst = [1, 1, 1, 3, 0, 4]; w = [0.1, 0.2, 0.3, 1e16, 0.4, 5.0]
    c = W.csr_of(src, dst, w, 6)
    assert c["row_ptr"].tolist() == [0, 2, 2, 5, 5, 6, 6]
    assert c["nbr"].tolist() == [1, 0, 1, 1, 3, 4] and c["weight"].tolist() == [0.2, 0.4, 0.1, 0.3, 1e16, 5.0]
    assert c["out_degree"].tolist() == [0.2 + 0.4, 0.0, (0.1 + 0.3) + 1e16, 0.0, 5.0, 0.0]
    e = W.csr_of([], [], [], 3)
    assert e["row_ptr"].tolist() == [0, 0, 0, 0] and len(e["nbr"]) == 0 and e["out_degree"].tolist() == [0.0, 0.0, 0.0]


# ------------------------------------------------------------------------------------------- replays against the oracle's walks
@pytest.fixture(scope="module")
def walk_graphs(oracle):
    out = {}
    for dead in (0.0, 0.25):
        src, dst, w, sources = layered_graph(R=50, T=6, deg=7, seed=3, dead_ends=dead)
        g = oracle.Graph(); g.add_edges(src, dst, w); g.set_sources(sources); g.build_alias(False)
        out[dead] = (g, W.tables_of(g))
    return out


@pytest.mark.parametrize("L", [1, 2, 7, 63])
@pytest.mark.parametrize("dead", [0.0, 0.25])
def test_replay_strided_equals_the_oracle(walk_graphs, dead, L):
    g, t = walk_graphs[dead]
    for seed, first in ((-5, 0), (42, (1 << 40) + 5), ((1 << 40) + 3, 1234)):
        want = g.sample_walks(1000, L, seed=seed, rng_mode=1, first_index=first)
        assert np.array_equal(W.replay_strided(t, 1000, L, seed, first), want), (seed, first)
        if dead and L > 2:
            assert (want[:, -1] == -1).any() and (want[:, 0] >= 0).all()


@pytest.mark.parametrize("L", [1, 2, 7, 63])
@pytest.mark.parametrize("dead", [0.0, 0.25])
def test_replay_sequential_equals_the_oracle(walk_graphs, dead, L):
    g, t = walk_graphs[dead]
    for seed, first in ((-5, 0), (42, 3 * L), (7, 3 * L + 1), (99, (1 << 40) + 5)):     # aligned and unaligned streams
        want, draws = g.sample_walks(700, L, seed=seed, rng_mode=0, first_index=first, return_draws=True)
        got, d = W.replay_sequential(t, 700, L, seed, first)
        assert np.array_equal(got, want) and d == draws == int((want >= 0).sum()), (seed, first)
        nxt, d2 = W.replay_sequential(t, 50, L, seed, first + d)                        # the stream continues where the call left it
        assert np.array_equal(nxt, g.sample_walks(50, L, seed=seed, rng_mode=0, first_index=first + draws))


def test_replays_see_a_shifted_stream_and_a_dead_end_that_draws(walk_graphs):
    g, t = walk_graphs[0.25]
    n, L = 400, 7
    want, draws = g.sample_walks(n, L, seed=11, rng_mode=0, first_index=9, return_draws=True)
    assert np.array_equal(W.replay_sequential(t, n, L, 11, 9)[0], want)
    assert not np.array_equal(W.replay_sequential(t, n, L, 11, 10)[0], want)             # one draw late
    assert not np.array_equal(W.replay_sequential(t, n, L, 11, 8)[0], want)              # one draw early
    # a walk that took its L draws although it dead-ended is the strided layout: the rows differ from the first short walk on
    aligned = g.sample_walks(n, L, seed=11, rng_mode=0, first_index=0)
    drawn = W.replay_strided(t, n, L, 11, 0)
    first_short = int(np.argmax((aligned == -1).any(1)))
    assert draws < n * L and np.array_equal(drawn[:first_short + 1], aligned[:first_short + 1]) and not np.array_equal(drawn, aligned)
    s = g.sample_walks(n, L, seed=11, rng_mode=1, first_index=5)
    assert np.array_equal(W.replay_strided(t, n, L, 11, 5), s) and not np.array_equal(W.replay_strided(t, n, L, 11, 6), s)
    # the slot rule: a table whose probabilities moved gives other walks
    t2 = dict(t, prob=t["prob"] * 0.5)
    assert not np.array_equal(W.replay_strided(t2, n, L, 11, 5), s)


# ------------------------------------------------------------------------------------------- what the tables encode, exactly
def _oracle_tables(oracle, ws, exact):
    """One oracle graph whose vertex v has the weights ws[v] -> [(prob, alias, out_degree)]."""
    g = oracle.Graph()
    nv = len(ws)
    for v, w in enumerate(ws):
        g.add_edges(np.full(len(w), v, np.int32), ((v + 1 + np.arange(len(w))) % nv).astype(np.int32), w)
    g.set_sources([0]); g.build_alias(exact)
    out = []
    for v in range(nv):
        a = g.get_alias(v)
        out.append((a["prob"], a["alias"], a["out_degree"]))
    return out


def _harness_tables(H, ws, exact):
    """The product's own builders (csrc/dge_algos.h, host build) on the same weights."""
    fn = H.harness_alias_reference if exact else H.harness_alias_vose
    out = []
    for w in ws:
        k = len(w)
        tot = 0.0
        for x in w.tolist():
            tot += x
        prob = np.zeros(k); alias = np.zeros(k, np.int32)
        fn(w.ctypes.data, k, tot, prob.ctypes.data, alias.ctypes.data)
        out.append((prob, alias, tot))
    return out


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("shape", W.LATTICE_SHAPES)
def test_mass_is_exact_on_the_lattice(oracle, algos_harness, shape, exact):
    rng = np.random.default_rng([len(shape), int(exact)])
    ks = KS + (() if exact else (5000,))
    ws = [W.lattice_weights(rng, k, M, shape) for k in ks]
    ot = _oracle_tables(oracle, ws, exact)
    ht = _harness_tables(algos_harness, ws, exact)
    for w, o, h in zip(ws, ot, ht):
        W.assert_lattice_table(*o, w, M, ("oracle", shape, exact, len(w)))
        W.assert_lattice_table(*h, w, M, ("dge_algos.h", shape, exact, len(w)))


def test_lattice_weights_hold_their_conditions():
    rng = np.random.default_rng(1)
    for shape in W.LATTICE_SHAPES:
        for k in (1, 2, 3, 65, 4097, 40_000):
            w = W.lattice_weights(rng, k, M, shape)
            assert w.dtype == np.float64 and (w == np.rint(w)).all() and (w >= 1).all()
            assert sum(int(x) for x in w) == k << M and k * int(w.max()) < 1 << 53
    assert len(set(W.lattice_weights(rng, 1000, M, "near").tolist())) == 3 and W.lattice_weights(rng, 999, M, "giant").max() == (999 << M) - 998
    with pytest.raises(AssertionError):
        W.lattice_weights(rng, 1 << 20, 33, "giant")                        # k * 2^m itself leaves 2^53


def test_mass_check_sees_wrong_tables(oracle):
    rng = np.random.default_rng(2)
    for exact in (True, False):
        w = W.lattice_weights(rng, 65, M, "pareto")
        (prob, alias, od), = _oracle_tables(oracle, [w], exact)
        want = w / float(1 << M)
        assert np.array_equal(W.mass(prob, alias), want)
        donors = np.flatnonzero((alias >= 0) & (prob < 1))
        a, b = next((int(i), int(j)) for i in donors for j in donors if alias[i] != alias[j] and prob[i] != prob[j])
        sw = alias.copy(); sw[a], sw[b] = alias[b], alias[a]                # two donors swap their receivers
        assert not np.array_equal(W.mass(prob, sw), want)
        p2 = prob.copy(); p2[a] += 2.0 ** -20                               # one threshold a lattice step off
        assert not np.array_equal(W.mass(p2, alias), want)
        nb = alias.copy(); nb[a] = (alias[a] + 1) % 65                      # one alias points at the slot next door
        assert not np.array_equal(W.mass(prob, nb), want)
        with pytest.raises(AssertionError):
            W.mass(prob, np.where(np.arange(65) == a, 65, alias))           # an alias outside the table


# ------------------------------------------------------------------------------------------- float weights: structure only
def test_float_tables_structure_on_the_oracle(oracle):
    """Tables of non-lattice weights: alias in [-1, k), prob >= 0, and |sum of mass - k| <= 2k * 2^-53 * max(prob).

    The bound: every slot hands on prob_i + (1 - prob_i), so the exact total is k for any table with aliases in range; walk_ref.mass_total_error sums the 2k
    terms exactly (math.fsum), which leaves k roundings of 1 - prob_i — none for prob_i in [1/2, 2] (Sterbenz), at most 2^-54 for prob_i < 1/2, at most
    2^-53 * prob_i above 2 — and the one rounding of the sum, at most 2^-53 * k: together at most k * 2^-53 * (1 + max(1/2, max prob)) <= 2k * 2^-53 * max prob
    for max prob >= 3/4 (asserted).  It is a check of the witness's own arithmetic and of the alias range, not of the table's values.
    Worst err / bound seen on the oracle over the cases below: 0.0 at every size (every prob of these tables lies in [0, 2], so each difference is exact or
    rounds below what the exact sum resolves)."""
    rng = np.random.default_rng(3)
    worst = 0.0
    for exact, ks in ((True, (1, 2, 40, 801, 5000)), (False, (1, 2, 40, 801, 5000, 40_000))):
        ws = [rng.random(k) * rng.choice([1.0, 1e-3, 1e3], k) + 1e-9 for k in ks]
        for (prob, alias, od), w in zip(_oracle_tables(oracle, ws, exact), ws):
            err, bound = W.float_table_checks(prob, alias)
            print("float table k=%d exact=%d: |sum mass - k| = %.3g, bound %.3g, max prob - 1 = %.3g" % (len(w), exact, err, bound, prob.max() - 1))
            assert err <= bound, (exact, len(w), err, bound)
            worst = max(worst, err / bound)
    print("worst ratio %.3g" % worst)
