"""GPU: edge store, alias tables and walk sampler of libdge.so against tests/walk_ref.py — a reading that is not the oracle — through the C ABI.

Every case builds its graph, reads the tables back once (dge_graph_get_csr, dge_graph_get_source_alias) and compares with the witness:
  * the store against walk_ref.csr_of, weights and degrees by their bits;
  * tables of lattice weights against the weights themselves: mass == w / 2^m as float64 equality, for both builders, whatever the pairing order;
  * walks against a replay from the tables the device returned, for both stream layouts.
Where the oracle has the same table, bit-equality with it is asserted too.  tests/test_walk_ref.py shows on the CPU that the witness is sound and
sees the faults it is meant to see.  Sizes are the smallest that cross a seam of the kernels."""
import numpy as np
import pytest

import walk_ref as W
from helpers import bits, layered_graph

pytestmark = pytest.mark.gpu

M = 20
HUB_KS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4095, 4096, 4097)      # in this order: adjacent tables share scratch boundaries
VOSE_HUB = 40_000


# ------------------------------------------------------------------------------------------- the edge store
def _store_edges(V, trailing, seed):
    """Edges of vertex 0 and of the last source vertex interleaved in insertion order, duplicates and self-loops among them, other sources in between;
    `trailing` vertices at the end appear as destinations only."""
    rng = np.random.default_rng([V, trailing, seed])
    last = V - 1 - trailing                                         # the last vertex that has out-edges
    assert last >= 0
    src, dst = [], []
    for j in range(12):
        src += [0, last]; dst += [int(rng.integers(0, V)), int(rng.integers(0, V))]
        if j % 4 == 0:
            src += [last, 0, 0]; dst += [last, 0, dst[-2]]          # self-loops, and a duplicate of vertex 0's latest edge
    if trailing:
        src += [0] * trailing; dst += list(range(V - trailing, V))
    else:
        src.append(0); dst.append(V - 1)
    n_mid = min(4 * V, 3000)
    total = len(src) + n_mid
    head = np.zeros(total, bool); head[rng.choice(total, len(src), replace=False)] = True      # the interleaved edges keep their relative order
    s = np.empty(total, np.int32); d = np.empty(total, np.int32)
    s[head] = src; d[head] = dst
    s[~head] = rng.integers(0, last + 1, n_mid); d[~head] = rng.integers(0, V, n_mid)
    src, dst = s, d
    w = rng.random(len(src)) * rng.choice([1e-3, 1.0, 1e6], len(src)) + 2.0 ** -30      # sums that round: the order of the additions shows
    return src, dst, w


@pytest.mark.parametrize("V", [2, 3, 4, 5, 1024, 1025, 65_536, 65_537])
def test_store_is_the_csr_of_the_insertion_order(dge, V):
    """V on and past a power of two: the width of the radix sort's key."""
    for trailing in (0, 1) if V < 4 else (0, 1, 3):
        src, dst, w = _store_edges(V, trailing, 0)
        assert int(max(src.max(), dst.max())) == V - 1 and int(src.max()) == V - 1 - trailing
        g = dge.DeviceGraph(0)
        half = len(src) // 2                                         # appended in two calls: one insertion order
        g.add_edges(src[:half], dst[:half], w[:half]); g.add_edges(src[half:], dst[half:], w[half:])
        got, want = g.get_csr(tables=False), W.csr_of(src, dst, w, V)
        assert g.num_vertices == V and g.num_edges == len(src)
        assert np.array_equal(got["row_ptr"], want["row_ptr"]), (V, trailing)
        assert np.array_equal(got["nbr"], want["nbr"]), (V, trailing)
        assert np.array_equal(bits(got["weight"]), bits(want["weight"])), (V, trailing)
        assert np.array_equal(bits(got["out_degree"]), bits(want["out_degree"])), (V, trailing)
        for v in (0, V - 1 - trailing, V - 1):                       # the per-vertex view reads the same store
            a = g.get_alias(v, tables=False); lo, hi = want["row_ptr"][v], want["row_ptr"][v + 1]
            assert np.array_equal(a["nbr"], want["nbr"][lo:hi]) and a["out_degree"] == want["out_degree"][v]


def test_empty_store(dge):
    g = dge.DeviceGraph(0)
    c = g.get_csr(tables=False)
    assert g.num_vertices == 0 and g.num_edges == 0 and c["row_ptr"].tolist() == [0] and len(c["nbr"]) == 0 and len(c["out_degree"]) == 0
    g = dge.DeviceGraph(0)
    g.reserve_vertices(5)                                            # vertices without a single edge
    c = g.get_csr(tables=False)
    assert c["row_ptr"].tolist() == [0] * 6 and np.array_equal(bits(c["out_degree"]), bits(np.zeros(5)))
    g.set_sources([1, 4]); g.build_alias(False)
    s = g.get_source_alias()
    assert s["src"].tolist() == [1, 4] and s["weight_sum"] == 0.0
    w = g.sample_walks(9, 3, seed=1)
    assert np.isin(w[:, 0], [1, 4]).all() and (w[:, 1:] == -1).all()
    assert np.array_equal(w, W.replay_strided(W.tables_of(g), 9, 3, 1))


# ------------------------------------------------------------------------------------------- tables, exact on the lattice
def _lattice_graph(shape, ks, seed=0):
    """Vertex v has len(ks[v]) slots of lattice weights, v = 0 .. len(ks) - 1 in that order; slot j of v leads to vertex (v + 1 + j) mod len(ks), so every
    walk keeps moving among the tables.  Edges in a shuffled insertion order (the per-vertex order is the slot order)."""
    rng = np.random.default_rng([len(shape), len(ks), seed])
    ws = [W.lattice_weights(rng, k, M, shape) for k in ks]
    nv = len(ks)
    src = np.concatenate([np.full(len(w), v, np.int32) for v, w in enumerate(ws)])
    dst = np.concatenate([((v + 1 + np.arange(len(w))) % nv).astype(np.int32) for v, w in enumerate(ws)])
    w = np.concatenate(ws)
    # edges of one vertex keep their slot order: shuffle WHICH vertex the next edge belongs to, not the slots
    pick = rng.permutation(np.repeat(np.arange(nv), [len(x) for x in ws]))
    start = np.concatenate([[0], np.cumsum([len(x) for x in ws])])
    nxt = start[:-1].copy()
    order = np.empty(len(src), np.int64)
    for i, v in enumerate(pick.tolist()):
        order[i] = nxt[v]; nxt[v] += 1
    return src[order], dst[order], w[order], ws


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("shape", W.LATTICE_SHAPES)
def test_vertex_tables_encode_the_lattice_weights(dge, oracle, shape, exact):
    ks = HUB_KS + (() if exact else (VOSE_HUB,))                    # one table of 40 000 slots more for the Vose order
    src, dst, w, ws = _lattice_graph(shape, ks)
    og, dg = oracle.Graph(), dge.DeviceGraph(0)
    for g in (og, dg):
        g.add_edges(src, dst, w); g.set_sources(np.arange(len(ks), dtype=np.int32)); g.build_alias(exact)
    c, want = dg.get_csr(), W.csr_of(src, dst, w, len(ks))
    assert np.array_equal(c["row_ptr"], want["row_ptr"]) and np.array_equal(c["nbr"], want["nbr"])
    assert np.array_equal(bits(c["weight"]), bits(want["weight"])) and np.array_equal(bits(c["out_degree"]), bits(want["out_degree"]))
    for v, wv in enumerate(ws):
        lo, hi = c["row_ptr"][v], c["row_ptr"][v + 1]
        assert np.array_equal(c["weight"][lo:hi], wv), v                 # the slot order is the insertion order
        W.assert_lattice_table(c["prob"][lo:hi], c["alias"][lo:hi], c["out_degree"][v], wv, M, (shape, exact, "vertex %d, %d slots" % (v, len(wv))))
    oc = og.get_csr()
    assert np.array_equal(oc["alias"], c["alias"]) and np.array_equal(bits(oc["prob"]), bits(c["prob"]))


@pytest.mark.parametrize("stream_sum", [0, 1])
@pytest.mark.parametrize("S", [1, 2, 1023, 1024, 1025, 3000])
def test_source_table_encodes_the_lattice_weights(dge, oracle, S, stream_sum):
    """S sources, each with one out-edge of lattice weight: out_degree and the total are exact, so the source table has to encode the weights."""
    for exact in (True, False):
        for shape in W.LATTICE_SHAPES:
            rng = np.random.default_rng([S, stream_sum, int(exact), len(shape)])
            w = W.lattice_weights(rng, S, M, shape)
            order = rng.permutation(S).astype(np.int32)              # slot i of the table is source order[i]
            src = np.arange(S, dtype=np.int32); dst = np.full(S, S, np.int32)
            wv = np.empty(S); wv[order] = w
            og, dg = oracle.Graph(), dge.DeviceGraph(0)
            for g in (og, dg):
                g.add_edges(src, dst, wv); g.set_sources(order, bool(stream_sum)); g.build_alias(exact)
            s = dg.get_source_alias()
            assert np.array_equal(s["src"], order)
            W.assert_lattice_table(s["prob"], s["alias"], s["weight_sum"], w, M, (S, stream_sum, exact, shape))
            o = og.get_source_alias()
            assert np.array_equal(o["alias"], s["alias"]) and np.array_equal(bits(o["prob"]), bits(s["prob"])) and o["weight_sum"] == s["weight_sum"]


def test_float_tables_structure(dge):
    """Tables of arbitrary weights (their values stay with the bit-equality against the oracle, tests/test_gpu_graph.py): structure only — see
    test_walk_ref.test_float_tables_structure_on_the_oracle for the bound and why nothing per slot is asserted."""
    rng = np.random.default_rng(3)
    for exact, ks in ((True, (1, 2, 40, 801, 5000)), (False, (1, 2, 40, 801, 1024, 5000, 40_000))):
        ws = [rng.random(k) * rng.choice([1.0, 1e-3, 1e3], k) + 1e-9 for k in ks]
        src = np.concatenate([np.full(len(w), v, np.int32) for v, w in enumerate(ws)])
        dst = np.concatenate([(np.arange(len(w)) % len(ks)).astype(np.int32) for w in ws])
        g = dge.DeviceGraph(0)
        g.add_edges(src, dst, np.concatenate(ws)); g.set_sources(np.arange(len(ks), dtype=np.int32)); g.build_alias(exact)
        c = g.get_csr()
        for v in range(len(ks)):
            lo, hi = c["row_ptr"][v], c["row_ptr"][v + 1]
            err, bound = W.float_table_checks(c["prob"][lo:hi], c["alias"][lo:hi])
            assert err <= bound, (exact, v, err, bound)


# ------------------------------------------------------------------------------------------- walks
class Sampled:
    """A device graph with its tables read back once."""

    def __init__(self, g):
        self.g = g
        self.t = W.tables_of(g)


@pytest.fixture(scope="module")
def graphs(dge):
    out = {}
    src, dst, w, sources = layered_graph(R=50, T=6, deg=7, seed=3, dead_ends=0.25)
    g = dge.DeviceGraph(0); g.add_edges(src, dst, w); g.set_sources(sources); g.build_alias(True)
    out["dead"] = Sampled(g)
    src, dst, w, sources = layered_graph(R=50, T=6, deg=7, seed=4)
    g = dge.DeviceGraph(0); g.add_edges(src, dst, w); g.set_sources(sources); g.build_alias(False)
    out["full"] = Sampled(g)
    ks = HUB_KS + (VOSE_HUB,)
    src, dst, w, _ = _lattice_graph("pareto", ks)
    g = dge.DeviceGraph(0); g.add_edges(src, dst, w); g.set_sources(np.arange(len(ks), dtype=np.int32)); g.build_alias(False)
    out["lattice"] = Sampled(g)
    # every source is a sink: vertices 30 .. 49 have no out-edge (their source weights are 0: the table's probabilities are 0/0, its aliases -1)
    rng = np.random.default_rng(9)
    g = dge.DeviceGraph(0)
    g.reserve_vertices(50)
    g.add_edges(rng.integers(0, 30, 200).astype(np.int32), rng.integers(0, 50, 200).astype(np.int32), rng.integers(1, 9, 200).astype(np.float64))
    g.set_sources(np.arange(30, 50, dtype=np.int32)); g.build_alias(True)
    out["sinks"] = Sampled(g)
    assert (out["sinks"].t["src_alias"] == -1).all() and (np.diff(out["sinks"].t["row_ptr"])[30:] == 0).all()
    return out


BIG = (1 << 40) + 5
STRIDED_CASES = [                       # (graph, n, L, seed, first_index): every value of each list at least once, the seams of n and L on every graph
    ("dead", 1, 1, 0, 0), ("dead", 255, 2, -1, 1234), ("dead", 256, 7, (1 << 40) + 3, BIG), ("dead", 257, 8, 0, BIG), ("dead", 4097, 62, -1, 0),
    ("dead", 4097, 63, (1 << 40) + 3, 1234), ("dead", 257, 63, -1, BIG), ("dead", 1, 63, 0, 1234),
    ("lattice", 4097, 7, 0, 0), ("lattice", 257, 63, -1, BIG), ("lattice", 256, 62, (1 << 40) + 3, 1234), ("lattice", 255, 8, -1, 0),
    ("lattice", 4097, 2, (1 << 40) + 3, BIG), ("lattice", 1, 7, 0, BIG),
    ("sinks", 1, 2, -1, 0), ("sinks", 255, 63, 0, BIG), ("sinks", 256, 1, (1 << 40) + 3, 1234), ("sinks", 257, 7, -1, 1234), ("sinks", 4097, 8, 0, BIG),
    ("full", 4097, 63, -1, BIG), ("full", 256, 8, 0, 1234),
]


@pytest.mark.parametrize("name,n,L,seed,first", STRIDED_CASES)
def test_strided_walks_are_the_replay_of_the_tables(graphs, name, n, L, seed, first):
    s = graphs[name]
    got = s.g.sample_walks(n, L, seed=seed, rng_mode=1, first_index=first)
    want = W.replay_strided(s.t, n, L, seed, first)
    assert got.shape == (n, L) and np.array_equal(got, want)
    if name == "sinks":
        assert (got[:, 0] >= 30).all() and (got[:, 1:] == -1).all()                  # one token per walk
    if name == "dead" and n >= 255 and L >= 7:
        assert (got[:, -1] == -1).any() and (got[:, 6] >= 0).any()                   # short walks and walks of 7 tokens and more
    if name == "lattice" and n == 4097 and L == 7:                                    # the hubs are entered and left through their far slots
        nv = len(HUB_KS) + 1
        for v in (len(HUB_KS) - 1, len(HUB_KS)):                                      # 4097 and 40 000 slots: slot j leads to (v + 1 + j) mod nv
            assert (got == v).any()
        assert len(np.unique(got)) == nv


def test_shards_reproduce_the_corpus(graphs):
    for name, L in (("dead", 7), ("lattice", 63)):
        s = graphs[name]
        whole = s.g.sample_walks(1000, L, seed=-3, rng_mode=1, first_index=BIG)
        parts = np.concatenate([s.g.sample_walks(n, L, seed=-3, rng_mode=1, first_index=BIG + r0) for r0, n in ((0, 255), (255, 1), (256, 257), (513, 487))])
        assert np.array_equal(whole, parts) and np.array_equal(whole, W.replay_strided(s.t, 1000, L, -3, BIG))


def test_sample_walks_into_writes_its_rows_only(dge, graphs):
    """Rows [1, 258) of a corpus of 600: a first block that starts at an odd row and a last block of one row, stored coalesced — the rows around stay."""
    s = graphs["dead"]
    for L in (7, 8, 63):
        before = (np.arange(600 * L, dtype=np.int32).reshape(600, L) * 7 + 1_000_000)
        c = dge.WalkCorpus.from_host(before, 0)
        s.g.sample_walks_into(c, 1, 257, seed=21, first_index=BIG)
        after = c.to_host()
        assert np.array_equal(after[1:258], W.replay_strided(s.t, 257, L, 21, BIG)), L
        assert np.array_equal(after[:1], before[:1]) and np.array_equal(after[258:], before[258:]), L
        s.g.sample_walks_into(c, 599, 1, seed=21, first_index=0)                      # the last row, nothing behind it
        s.g.sample_walks_into(c, 300, 0, seed=21, first_index=0)                      # no rows: nothing written
        last = c.to_host()
        assert np.array_equal(last[599:], W.replay_strided(s.t, 1, L, 21, 0)) and np.array_equal(last[:599], after[:599]), L


SEQ_CASES = [(2047, 6), (2048, 6), (2048, 8), (2341, 7), (2048, 63), (4681, 7)]
#             one lane | resolver from here on; n * L = 4 blocks of 4096 | 4 blocks + 3 | long rows | 8 blocks - 1


@pytest.mark.parametrize("n,L", SEQ_CASES)
def test_sequential_stream_is_the_replay_of_the_tables(graphs, n, L):
    """rng_mode 0: walks and draws_consumed, aligned and unaligned first_index, with dead ends, without (unaligned: the resolver still runs) and with
    one-token walks; then the stream continues at first_index + draws."""
    off = BIG if BIG % L else BIG + 1                                                 # far into the stream and not a multiple of L
    assert off % L != 0 and (5 * L + 1) % L != 0
    for name, firsts in (("dead", (0, 5 * L, 5 * L + 1, off)), ("full", (5 * L + 1, off)), ("sinks", (0, 3 * L, 3 * L + 2))):
        s = graphs[name]
        for first in firsts:
            got, draws = s.g.sample_walks(n, L, seed=77, rng_mode=0, first_index=first, return_draws=True)
            want, d = W.replay_sequential(s.t, n, L, 77, first)
            assert np.array_equal(got, want), (name, first)
            assert draws == d == int((want >= 0).sum()), (name, first)
            if name == "sinks":
                assert draws == n
            if name == "full":
                assert draws == n * L
            more = s.g.sample_walks(300, L, seed=77, rng_mode=0, first_index=first + draws)
            assert np.array_equal(more, W.replay_sequential(s.t, 300, L, 77, first + d)[0]), (name, first)


# ------------------------------------------------------------------------------------------- the walk-length limit
def test_walks_longer_than_63_are_refused_everywhere(dge, graphs):
    """include/dge.h: max_len <= DGE_MAX_WALK_LEN (63) — DGE_ERR_ARG on the host, before anything is launched, in both modes, aligned or not, short corpus or
    long, and through dge_sample_walks_into.  The graph samples correctly at 63 straight afterwards."""
    s = graphs["dead"]
    for L in (64, 100):
        for mode in (0, 1):
            for first in (0, 3 * L, 3 * L + 1):
                for n in (0, 10, 5000):
                    with pytest.raises(dge.DgeError) as ei:
                        s.g.sample_walks(n, L, seed=1, rng_mode=mode, first_index=first)
                    assert ei.value.code == 1 and "walk length %d too long (max 63)" % L in str(ei.value), (L, mode, first, n)
        with pytest.raises(dge.DgeError) as ei:
            s.g.sample_walks_device(10, L, seed=1, rng_mode=0, first_index=1)
        assert ei.value.code == 1
        c = dge.WalkCorpus.from_host(np.full((12, L), 5, np.int32), 0)                # a corpus may hold longer rows; the sampler does not fill them
        for n in (0, 10):
            with pytest.raises(dge.DgeError) as ei:
                s.g.sample_walks_into(c, 1, n, seed=1, first_index=0)
            assert ei.value.code == 1 and "too long (max 63)" in str(ei.value)
        assert (c.to_host() == 5).all()
    for mode, first in ((1, 2), (0, 63), (0, 64)):
        got, draws = s.g.sample_walks(300, 63, seed=1, rng_mode=mode, first_index=first, return_draws=True)
        want = W.replay_strided(s.t, 300, 63, 1, first) if mode else W.replay_sequential(s.t, 300, 63, 1, first)[0]
        assert np.array_equal(got, want), (mode, first)
