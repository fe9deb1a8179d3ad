"""GPU parity: edge store, alias tables and walk sampler of libdge.so vs the CPU oracle, through the C ABI.

Integer/index outputs and the double-precision tables must be BIT-EXACT.
Reference behaviour under test: J/LayeredGraph.java:54-82,104-116,157-252, J/SpatialGraph.java:29-35,105-108;
golden vector: T/LayeredGraphTest.java:12-44.
"""
import numpy as np
import pytest

from helpers import bits, build_both, layered_graph

pytestmark = pytest.mark.gpu


def test_layered_graph_test_golden_vector(dge):
    """T/LayeredGraphTest.java:12-44 through the device path."""
    g = dge.DeviceGraph(0)
    g.add_edges([0, 0, 0], [1, 2, 3], [2.0, 10.0, 8.0])
    g.set_sources([0])
    g.build_alias(exact=True)
    a = g.get_alias(0)
    assert a["alias"].tolist() == [1, 2, -1]
    assert a["prob"].tolist() == [0.3, 0.8, 1.0]          # exact double equality, as assertEquals does
    assert a["out_degree"] == 20.0
    assert [g.sample_next(0, x) for x in (0.05, 0.3, 0.4, 0.65, 0.9)] == [1, 2, 2, 3, 3]
    assert g.sample_next(1, 0.5) == -1                     # no out-edges -> null (J/LayeredGraph.java:106-107)


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("seed", [0, 1])
def test_alias_tables_bit_exact(dge, oracle, exact, seed):
    src, dst, w, sources = layered_graph(R=60, T=5, deg=9, seed=seed)
    og, dg = build_both(oracle, dge, src, dst, w, sources, exact=exact)
    assert dg.num_vertices == og.num_vertices and dg.num_edges == og.num_edges
    for v in range(og.num_vertices):
        a, b = og.get_alias(v), dg.get_alias(v)
        assert np.array_equal(a["nbr"], b["nbr"]), v                 # insertion order kept per vertex
        assert np.array_equal(bits(a["weight"]), bits(b["weight"])), v
        assert a["out_degree"] == b["out_degree"], v
        assert np.array_equal(a["alias"], b["alias"]), v
        assert np.array_equal(bits(a["prob"]), bits(b["prob"])), v
    sa, sb = og.get_source_alias(), dg.get_source_alias()
    assert sa["weight_sum"] == sb["weight_sum"]
    assert np.array_equal(sa["src"], sb["src"]) and np.array_equal(sa["alias"], sb["alias"])
    assert np.array_equal(bits(sa["prob"]), bits(sb["prob"]))


def test_alias_hub_vertex_exact_order(dge, oracle):
    """A 5000-edge hub: the bit-set restatement of the reference's O(k^2) pairing must give identical arrays."""
    rng = np.random.default_rng(5)
    k = 5000
    w = np.floor(rng.pareto(1.1, k) * 3) + 1
    src = np.zeros(k, np.int32); dst = np.arange(1, k + 1, dtype=np.int32)
    og, dg = build_both(oracle, dge, src, dst, w, [0], exact=True)
    a, b = og.get_alias(0), dg.get_alias(0)
    assert np.array_equal(a["alias"], b["alias"]) and np.array_equal(bits(a["prob"]), bits(b["prob"]))


@pytest.mark.parametrize("shape", ["pareto", "near_uniform", "two_values", "one_giant"])
def test_alias_vose_tables_of_thousands_of_slots(dge, oracle, shape):
    """Vose order on big tables (hub vertices, the source table) is built by a whole wave with register windows over the two stacks
    (alias_vose_wave): the same arrays as the serial loop, bit for bit — hubs of 1023 / 1024 / 1025 / 5000 / 40 000 slots, 3000 sources."""
    rng = np.random.default_rng(len(shape))
    ks = [1023, 1024, 1025, 5000, 40_000]
    src, dst, w = [], [], []
    nxt = len(ks)
    for h, k in enumerate(ks):
        if shape == "pareto": wk = np.floor(rng.pareto(1.1, k) * 3) + 1
        elif shape == "near_uniform": wk = 1000.0 + rng.integers(-1, 2, k)            # slots a hair under, at and over 1: long alternations
        elif shape == "two_values": wk = np.where(rng.random(k) < 0.9, 1.0, 37.0)
        else: wk = np.ones(k); wk[k // 3] = 50.0 * k                               # one large serves nearly every small
        src.append(np.full(k, h, np.int32)); dst.append(np.arange(nxt, nxt + k, dtype=np.int32)); w.append(wk)
    src = np.concatenate(src); dst = np.concatenate(dst); w = np.concatenate(w).astype(np.float64)
    # give 3000 of the leaves an out-edge each so that the source table has 3000 slots of varied weight
    leaves = np.arange(len(ks), len(ks) + 3000, dtype=np.int32)
    src = np.concatenate([src, leaves]); dst = np.concatenate([dst, np.zeros(3000, np.int32)])
    w = np.concatenate([w, np.floor(rng.pareto(1.3, 3000) * 5) + 1])
    og, dg = build_both(oracle, dge, src, dst, w, leaves, exact=False)
    for v in range(len(ks)):
        a, b = og.get_alias(v), dg.get_alias(v)
        assert np.array_equal(a["alias"], b["alias"]) and np.array_equal(bits(a["prob"]), bits(b["prob"])), (shape, v)
    sa, sb = og.get_source_alias(), dg.get_source_alias()
    assert np.array_equal(sa["alias"], sb["alias"]) and np.array_equal(bits(sa["prob"]), bits(sb["prob"])), shape
    # and the walk slots built from them
    n = 4000
    wo = og.sample_walks(n, 3, seed=11, rng_mode=1); wd = dg.sample_walks(n, 3, seed=11, rng_mode=1)
    assert np.array_equal(wo, wd)


@pytest.mark.parametrize("exact", [True, False])
def test_walks_strided_bit_exact(dge, oracle, exact):
    src, dst, w, sources = layered_graph(R=50, T=6, deg=7, seed=3)
    og, dg = build_both(oracle, dge, src, dst, w, sources, exact=exact)
    for first in (0, 1234):
        a = og.sample_walks(3000, 6, seed=42, rng_mode=1, first_index=first)
        b = dg.sample_walks(3000, 6, seed=42, rng_mode=1, first_index=first)
        assert np.array_equal(a, b)
    # shards of one corpus reproduce the corpus
    whole = dg.sample_walks(1000, 6, seed=7, rng_mode=1)
    parts = np.concatenate([dg.sample_walks(250, 6, seed=7, rng_mode=1, first_index=250 * r) for r in range(4)])
    assert np.array_equal(whole, parts)


def test_walks_java_sequential_stream(dge, oracle):
    """rng_mode 0 = what the reference yields after LayeredGraph.rnd = new Random(seed) (J/LayeredGraph.java:14)."""
    src, dst, w, sources = layered_graph(R=50, T=6, deg=7, seed=4)
    og, dg = build_both(oracle, dge, src, dst, w, sources)
    a, da = og.sample_walks(2000, 6, seed=99, rng_mode=0, return_draws=True)
    b, db = dg.sample_walks(2000, 6, seed=99, rng_mode=0, return_draws=True)
    assert np.array_equal(a, b) and da == db == 2000 * 6
    assert np.array_equal(a, dg.sample_walks(2000, 6, seed=99, rng_mode=1))   # no dead ends: both layouts agree
    # continuing the stream: draws already consumed
    c = og.sample_walks(500, 6, seed=99, rng_mode=0, first_index=da)
    d = dg.sample_walks(500, 6, seed=99, rng_mode=0, first_index=db)
    assert np.array_equal(c, d)


def test_walks_dead_ends_are_short_not_errors(dge, oracle):
    """J/LayeredGraph.java:247-248: a vertex without out-edges ends the walk; the draw count becomes data dependent."""
    src, dst, w, sources = layered_graph(R=40, T=6, deg=4, seed=8, dead_ends=0.25)
    og, dg = build_both(oracle, dge, src, dst, w, sources)
    a1 = og.sample_walks(4000, 6, seed=5, rng_mode=1); b1 = dg.sample_walks(4000, 6, seed=5, rng_mode=1)
    assert np.array_equal(a1, b1)
    assert (a1 == -1).any() and (a1[:, 0] >= 0).all()
    a0, da = og.sample_walks(1500, 6, seed=5, rng_mode=0, return_draws=True)
    b0, db = dg.sample_walks(1500, 6, seed=5, rng_mode=0, return_draws=True)
    assert np.array_equal(a0, b0) and da == db and da < 1500 * 6
    assert da == int((a0 >= 0).sum())                    # one draw per node of the walk
    # unaligned continuation of the sequential stream
    c = og.sample_walks(300, 6, seed=5, rng_mode=0, first_index=da)
    d = dg.sample_walks(300, 6, seed=5, rng_mode=0, first_index=db)
    assert np.array_equal(c, d)
    # long corpora go through the parallel resolver of the sequential stream (block exits + chain): still the exact walks
    for n, first in ((2048, 0), (50_000, 0), (30_001, da)):
        a2, d2 = og.sample_walks(n, 6, seed=77, rng_mode=0, first_index=first, return_draws=True)
        b2, e2 = dg.sample_walks(n, 6, seed=77, rng_mode=0, first_index=first, return_draws=True)
        assert np.array_equal(a2, b2) and d2 == e2 and d2 == int((a2 >= 0).sum())


def test_keep_nearest_k_vertices(dge, oracle):
    """J/SpatialGraph.java:29-35 incl. ties (stable sort keeps insertion order) and the self-loop of weight 1."""
    rng = np.random.default_rng(11)
    R = 30
    pts = rng.random((R, 2)) * 0.05
    src, dst, w = [], [], []
    for i in range(R):
        for j in range(R):
            d = float(np.hypot(*(pts[i] - pts[j])))
            src.append(i); dst.append(j); w.append(float(np.round(np.exp(-d * 100), 2)))   # rounding forces ties
    og, dg = build_both(oracle, dge, np.array(src, np.int32), np.array(dst, np.int32), np.array(w), np.arange(R, dtype=np.int32),
                        exact=True, stream_sum=True, top_k=10)
    assert dg.num_edges == R * 10
    for v in range(R):
        a, b = og.get_alias(v), dg.get_alias(v)
        assert np.array_equal(a["nbr"], b["nbr"]) and np.array_equal(bits(a["weight"]), bits(b["weight"]))
        assert a["out_degree"] == b["out_degree"]
        assert b["weight"][0] == 1.0 and (np.diff(b["weight"]) <= 0).all()
        assert np.array_equal(a["alias"], b["alias"]) and np.array_equal(bits(a["prob"]), bits(b["prob"]))
    assert og.get_source_alias()["weight_sum"] == dg.get_source_alias()["weight_sum"]
    wa = og.sample_walks(2000, 8, seed=1, rng_mode=1); wb = dg.sample_walks(2000, 8, seed=1, rng_mode=1)
    assert np.array_equal(wa, wb)
    with pytest.raises(dge.DgeError) as ei:      # subList(0,k) throws when a vertex has fewer than k edges
        dg.keep_top_k(11)
    assert ei.value.code == 3


def test_position_prefix_rule(dge):
    """J/SpatialGraph.java:105-108: token j becomes "j-name" -> id j*R + name."""
    walks = np.array([[3, 1, 2, -1], [0, 0, 0, 0]], np.int32)
    c = dge.WalkCorpus.from_host(walks, 0)
    c.add_position_prefix(5)
    assert c.to_host().tolist() == [[3, 6, 12, -1], [0, 5, 10, 15]]


def test_error_behaviour_and_empty_inputs(dge):
    g = dge.DeviceGraph(0)
    g.add_edges([0, 1], [1, 2], [1.0, 1.0])
    with pytest.raises(dge.DgeError) as ei:
        g.sample_walks(4, 3, seed=1)
    assert ei.value.code == 5                         # alias tables not built yet
    with pytest.raises(dge.DgeError) as ei:
        g.set_sources([7])
    assert ei.value.code == 2
    with pytest.raises(dge.DgeError):
        g.add_edges([-1], [0], [1.0])
    g.set_sources([])
    g.build_alias(True)
    assert (g.sample_walks(5, 3, seed=1) == -1).all()  # no sources: nothing to start from
    g.set_sources([2]); g.build_alias(True)           # source without out-edges: one-node walks
    w = g.sample_walks(5, 3, seed=1)
    assert (w[:, 0] == 2).all() and (w[:, 1:] == -1).all()
    assert g.sample_walks(0, 3, seed=1).shape == (0, 3)
    with pytest.raises(dge.DgeError) as ei:
        dge.DeviceGraph(99)
    assert ei.value.code == 6


def test_full_size_walk_properties(dge):
    """cfg2-sized store (100k vertices, ~5M edges): size-independent properties instead of an oracle replay."""
    import torch
    from embedding_amd import synth
    R, T = 25_000, 4
    G = synth.flow_graph_torch(R, T, 50, "cuda:0")
    g = dge.DeviceGraph(0)
    g.add_edges_device(G["src"], G["dst"], G["w"])
    g.set_sources(G["sources"])
    g.build_alias(exact=False)
    assert g.num_vertices == R * T and g.num_edges == G["n_edges"]
    n = 400_000
    walks = g.sample_walks(n, T, seed=9, rng_mode=1)
    assert (walks >= 0).all()                                   # every vertex has out-edges here
    assert (walks // R == np.arange(T)[None, :]).all()          # step j reads slice j (J/CrossTimeGraph.java:36-39)
    # every step is an edge of the store
    key = G["src"].to(torch.int64) * (R * T) + G["dst"].to(torch.int64)
    key = torch.unique(key)
    wt = torch.from_numpy(walks).to("cuda:0").to(torch.int64)
    step = (wt[:, :-1] * (R * T) + wt[:, 1:]).reshape(-1)
    pos = torch.searchsorted(key, step).clamp_(max=key.numel() - 1)
    assert bool((key[pos] == step).all())
    # transition frequencies out of the most visited source follow the edge weights (chi-square, 5 sigma)
    v0 = int(np.bincount(walks[:, 0]).argmax())
    a = g.get_alias(v0, tables=False)
    nxt = walks[walks[:, 0] == v0, 1]
    exp = {}
    for d, ww in zip(a["nbr"], a["weight"]):
        exp[int(d)] = exp.get(int(d), 0.0) + ww / a["out_degree"]
    obs = np.array([np.sum(nxt == d) for d in exp]); e = np.array(list(exp.values())) * len(nxt)
    chi2 = float(((obs - e) ** 2 / e).sum()); dof = len(e) - 1
    assert chi2 < dof + 5 * np.sqrt(2 * dof) + 10, (chi2, dof)
    # source choice follows out-degree (J/LayeredGraph.java:199-204)
    sa = g.get_source_alias()
    assert abs(sa["prob"].mean() - 1.0) < 0.5 and sa["weight_sum"] > 0


@pytest.mark.parametrize("exact", [True, False])
def test_host_held_public_fields_are_honoured(dge, oracle, exact):
    """The reference's Vertex.outDegree and LayeredGraph.sourceWeightSum are fields that callers assign (J/LayeredGraph.java:35,146;
    J/SpatialGraph.java:33,57), and addSourceVertex may create vertices no edge names (:182-183).  A host that keeps those fields
    hands them over (dge_graph_reserve_vertices / set_out_degree / set_source_weight_sum) and reads every table back in one piece
    (dge_graph_get_csr): bit-exact against the oracle fed the same values, walks included."""
    src, dst, w, sources = layered_graph(R=50, T=4, deg=7, seed=11)
    rng = np.random.default_rng(3)
    V = int(max(src.max(), dst.max())) + 1
    og, dg = oracle.Graph(), dge.DeviceGraph(0)
    for g in (og, dg):
        g.add_edges(src, dst, w)
        g.reserve_vertices(V + 3)                                    # three isolated vertices (unregistered sources)
    od = og.get_csr(tables=False)["out_degree"].copy()
    assert len(od) == V + 3 and np.array_equal(bits(od), bits(dg.get_csr(tables=False)["out_degree"]))
    od[:V] *= rng.choice([1.0, 1.0, 1.0 + 2.0 ** -40, 0.5, 3.0], V)  # fields as a caller left them, not the running sums
    srcs = np.concatenate([sources, [V + 1, V]]).astype(np.int32)
    for g in (og, dg):
        g.set_out_degree(od)
        g.set_sources(srcs)
        g.set_source_weight_sum(float(od[srcs].sum()) * 1.25)
        g.build_alias(exact)
    a, b = og.get_csr(), dg.get_csr()
    assert np.array_equal(a["row_ptr"], b["row_ptr"]) and np.array_equal(a["nbr"], b["nbr"]) and np.array_equal(a["alias"], b["alias"])
    for k in ("weight", "prob", "out_degree"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert np.array_equal(bits(b["out_degree"]), bits(od))
    for v in (0, 7, V - 1, V + 2):                                    # the per-vertex view agrees with the bulk one
        x = dg.get_alias(v); lo, hi = b["row_ptr"][v], b["row_ptr"][v + 1]
        assert np.array_equal(bits(x["prob"]), bits(b["prob"][lo:hi])) and np.array_equal(x["alias"], b["alias"][lo:hi])
    sa, sb = og.get_source_alias(), dg.get_source_alias()
    assert sa["weight_sum"] == sb["weight_sum"] == float(od[srcs].sum()) * 1.25
    assert np.array_equal(sa["alias"], sb["alias"]) and np.array_equal(bits(sa["prob"]), bits(sb["prob"]))
    for mode in (0, 1):
        assert np.array_equal(og.sample_walks(3000, 4, seed=9, rng_mode=mode), dg.sample_walks(3000, 4, seed=9, rng_mode=mode))
    # refreshed source weights when the fields change after set_sources; a later set_sources drops the fixed sum
    od2 = od * 2.0
    for g in (og, dg):
        g.set_sources(srcs); g.set_out_degree(od2); g.build_alias(exact)
    sa, sb = og.get_source_alias(), dg.get_source_alias()
    assert sa["weight_sum"] == sb["weight_sum"] and np.array_equal(bits(sa["prob"]), bits(sb["prob"]))
    with pytest.raises(dge.DgeError):
        dg.set_out_degree(od[:-1])                                    # one value per vertex


# ------------------------------------------------------------------------------------------ the handle's state: refusals, sequences, builders, waits
def snapshot(g, L=3):
    """everything a host can read of a built graph, doubles as bits: the CSR with its tables, the source table, walks of both stream layouts."""
    c, s = g.get_csr(), g.get_source_alias()
    out = [np.int64([g.num_vertices, g.num_edges])] + [c[k] for k in ("row_ptr", "nbr", "weight", "out_degree", "prob", "alias")]
    out += [s["prob"], s["alias"], s["src"], np.float64([s["weight_sum"]])] + [g.sample_walks(64, L, seed=2, rng_mode=m) for m in (0, 1)]
    return [(a.shape, a.dtype, np.ascontiguousarray(a).tobytes()) for a in (np.asarray(x) for x in out)]


def refused(dge, code, call):
    with pytest.raises(dge.DgeError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)


def test_every_reachable_refusal_leaves_the_graph_as_it_was(dge):
    """A refused call changes nothing a host can read: CSR, tables, source table and the walks of both modes are the bytes they were.  The builders are aimed at the
    used handle through the C entries (the classes only ever hand them a new one).  The pruned copy keeps min(2, least degree) edges a vertex: this graph has
    vertices with one edge, which keep_top_k(2) itself refuses."""
    import ctypes as C
    from embedding_amd._native import check
    from embedding_amd.engine import _text_args
    lib, p = dge.lib, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    src, dst, w, sources = layered_graph(R=12, T=3, deg=3, seed=5)

    def built():
        g = dge.DeviceGraph(0); g.add_edges(src, dst, w); g.set_sources(sources); g.build_alias(True)
        return g
    g = built()
    V = g.num_vertices
    least = int(np.diff(g.get_csr()["row_ptr"]).min())
    assert V == 36 and least >= 1
    before = snapshot(g)
    rg = dge.Regions.from_arrays([7], [0, 1], [0, 5], [(0, 0), (0, 1), (1, 1), (1, 0), (0, 0)])
    flows = dge.Flows(rg); flows.add_entries([0], [0], [0], [1])
    _keep, texts, sizes, n = _text_args([b"1 2 3"])
    ids, xy = np.arange(3, dtype=np.int64), np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    for code, call in [(2, lambda: g.set_sources([V])), (2, lambda: g.add_edges([-1], [0], [1.0])), (2, lambda: g.add_edges([0], [0x7fffffff], [1.0])),
                       (1, lambda: g.set_out_degree(np.ones(V - 1))), (3, lambda: g.keep_top_k(least + 1)),
                       (1, lambda: g.sample_walks(4, 64, seed=1, rng_mode=0)), (1, lambda: g.sample_walks(4, 64, seed=1, rng_mode=1)),
                       (5, lambda: check(lib.dge_graph_add_od_texts(g._h, texts, sizes, n, None, None))),
                       (5, lambda: check(lib.dge_graph_add_flows(g._h, flows._h, 1, 0, None, None))),
                       (5, lambda: check(lib.dge_graph_add_spatial_points(g._h, p(ids), p(xy), 3, 2, 100.0, None, None)))]:
        refused(dge, code, call)
        assert snapshot(g) == before, code
    cut = built()
    cut.keep_top_k(min(2, least)); cut.build_alias(True)
    before = snapshot(cut)
    assert cut.num_edges == V * min(2, least) < len(src)
    for call in (lambda: cut.add_edges([0], [1], [1.0]), lambda: cut.reserve_vertices(V + 1)):
        refused(dge, 5, call)
        assert snapshot(cut) == before


def op_sequences():
    """24 seeded sequences of at most 8 operations on at most 40 vertices and 200 edges, as (name, arguments) lists, and the sources and build order of the final
    build.  Four cores by construction, six sequences each: set_out_degree before and after set_sources; set_source_weight_sum, then set_sources (the fixed sum
    goes); add_edges after build_alias; keep_top_k after set_sources.  The rest is drawn.  The arguments are made legal on a host model of the store (vertex
    count, least degree, pruned or not): no edges or new vertices after a prune, k within the least degree."""
    seqs = []
    for i in range(24):
        rng = np.random.default_rng(1000 + i)
        V0 = int(rng.integers(6, 25))
        deg = np.zeros(40, np.int64)
        st = dict(V=0, E=0, pruned=False, sources=[])
        ops = []

        def weights(n):
            return rng.integers(1, 1000, n) * 10.0 ** rng.integers(-3, 3, n)

        def add_edges(n, cover=False):
            n = min(n, 200 - st["E"])
            s = np.concatenate([np.tile(np.arange(V0), 2), rng.integers(0, V0, n - 2 * V0)]) if cover else rng.integers(0, max(st["V"], 2), n)
            d = rng.integers(0, max(st["V"], V0) + (0 if cover or st["V"] >= 40 else 1), n)
            s, d = rng.permutation(s).astype(np.int32), d.astype(np.int32)
            np.add.at(deg, s, 1)
            st["V"] = max(st["V"], int(max(s.max(), d.max())) + 1); st["E"] += n
            ops.append(("add_edges", (s, d, weights(n))))

        def set_sources(empty_ok=True):
            n = int(rng.integers(0 if empty_ok else 1, min(st["V"], 9) + 1))
            st["sources"] = rng.integers(0, st["V"], n).astype(np.int32)               # repeats allowed, as addSourceVertex allows them
            ops.append(("set_sources", (st["sources"], bool(rng.integers(0, 2)))))

        def op(name, core=False):
            least = int(deg[:st["V"]].min())
            if name == "add_edges" and not st["pruned"] and st["E"] < 190:
                add_edges(int(rng.integers(1, 9)))
            elif name == "reserve_vertices" and not st["pruned"] and st["V"] < 40:
                st["V"] = int(rng.integers(st["V"], 41)); ops.append((name, (st["V"],)))
            elif name == "set_sources":
                set_sources(empty_ok=not core)
            elif name == "set_out_degree":
                ops.append((name, (weights(st["V"]),)))
            elif name == "set_source_weight_sum":
                ops.append((name, (float(weights(1)[0]),)))
            elif name == "build_alias":
                ops.append((name, (bool(rng.integers(0, 2)),)))
            elif name == "keep_top_k" and least >= 1:
                k = int(rng.integers(1, least + 1))
                deg[:st["V"]] = k; st["pruned"] = True; st["E"] = st["V"] * k
                ops.append((name, (k,)))
            else:
                ops.append(("get_csr", ()))
        add_edges(int(rng.integers(3 * V0, 5 * V0)), cover=True)           # every vertex has two out-edges and more: a prune is possible and cuts
        for name in (["set_out_degree", "set_sources", "set_out_degree"], ["set_sources", "set_source_weight_sum", "set_sources"],
                     ["set_sources", "build_alias", "add_edges"], ["set_sources", "keep_top_k"])[i % 4]:
            op(name, core=True)
        names = ["add_edges", "reserve_vertices", "set_sources", "set_out_degree", "set_source_weight_sum", "build_alias", "keep_top_k", "get_csr"]
        while len(ops) < 8:
            op(names[int(rng.integers(0, len(names)))])
        set_sources(empty_ok=False)                                        # sources set after the last edge, as the reference asks (J/LayeredGraph.java:177)
        seqs.append((ops, ops.pop()[1], bool(i & 1)))
    return seqs


def apply_op(g, name, args, sources, is_oracle):
    """keep_top_k on a graph with sources: the library refreshes the sources' weights and sums them as DoubleStream.sum() with no fixed sum (csrc/dge_internal.h:
    dge_graph_adopt_pruned), which is keep_top_k followed by set_sources(the same, stream_sum) — the reference never prunes after addSourceVertex, so the oracle is
    given that second call in words."""
    if name == "get_csr":
        g.get_csr(tables=False)
        return
    getattr(g, name)(*args)
    if name == "keep_top_k" and is_oracle and len(sources):
        g.set_sources(sources, True)


def weight_sum(g):
    """get_source_alias()["weight_sum"]; the device hands its tables out only once they are built, the sum at any time (cap 0, no arrays)."""
    if not hasattr(g, "device"):
        return g.get_source_alias()["weight_sum"]
    import ctypes as C
    from embedding_amd._native import check, lib
    k, ws = C.c_int32(0), C.c_double(0)
    check(lib.dge_graph_get_source_alias(g._h, None, None, None, 0, C.byref(k), C.byref(ws)))
    return ws.value


def read_state(g):
    counts = np.int64([g.num_vertices, g.num_edges])              # read first: the CSR may not be built yet
    c = g.get_csr(tables=False)
    return [(np.asarray(a).shape, np.ascontiguousarray(a).tobytes()) for a in
            (counts, c["row_ptr"], c["nbr"], c["weight"], c["out_degree"], np.float64([weight_sum(g)]))]


@pytest.mark.parametrize("i", range(24))
def test_operation_sequences_against_the_oracle(dge, oracle, i):
    ops, final_sources, exact = op_sequences()[i]
    assert len(ops) <= 8
    og, dg = oracle.Graph(), dge.DeviceGraph(0)
    sources = []
    for step, (name, args) in enumerate(ops):
        for g in (og, dg):
            apply_op(g, name, args, sources, g is og)
        if name == "set_sources":
            sources = args[0]
        assert read_state(og) == read_state(dg), (step, name)
        assert og.num_vertices <= 40 and og.num_edges <= 200
    for g in (og, dg):
        g.set_sources(*final_sources); g.build_alias(exact)
    a, b = og.get_csr(), dg.get_csr()
    for k in a:
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), k
    a, b = og.get_source_alias(), dg.get_source_alias()
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    for mode in (0, 1):
        assert np.array_equal(og.sample_walks(64, 5, seed=3, rng_mode=mode), dg.sample_walks(64, 5, seed=3, rng_mode=mode)), mode


def test_a_flow_table_ends_where_a_host_ends(dge):
    """from_flows against a second graph fed the same slot edges by add_edges, reserve_vertices and set_sources: 5 regions, ids not in order, 8 slices.  (The .od
    reader and the spatial graph have this comparison in test_gpu_od_read.py: check, and test_gpu_spatial.py: check_against_old_path.)"""
    ids = [50, 10, 40, 20, 30]
    ring = [(0.0, 0.0), (0.0, 1.0), (1.0, 1.0), (1.0, 0.0), (0.0, 0.0)]
    xy = [(x + 2.0 * r, y) for r in range(5) for x, y in ring]
    rg = dge.Regions.from_arrays(ids, np.arange(6), np.arange(6) * 5, xy)
    rng = np.random.default_rng(8)
    f = dge.Flows(rg)
    f.add_entries(rng.integers(0, 24, 60), rng.integers(0, 4, 60), rng.integers(1, 5, 60), rng.integers(1, 9, 60))     # region 0 never a source, region 4 never a destination
    T = 8
    g, _, info = dge.DeviceGraph.from_flows(f, T, dge.Flows.EVEN, names=False)
    slot, sid, did, w = f.slot_edges(T, dge.Flows.EVEN)
    regions = np.unique(np.concatenate([sid, did]))
    R = len(regions)
    assert R == 5 and info["edges"] == len(slot) > 20 and np.array_equal(g.regions(), regions)
    src = slot * R + np.searchsorted(regions, sid); nxt = (slot + 1) % T
    dst = nxt * R + np.searchsorted(regions, did)
    h = dge.DeviceGraph(0)
    h.add_edges(src, dst, w.astype(np.float64)); h.reserve_vertices(T * R); h.set_sources(np.unique(np.concatenate([src[slot == 0], dst[nxt == 0]])))
    g.build_alias(True); h.build_alias(True)
    assert snapshot(g, L=T + 1) == snapshot(h, L=T + 1)


def test_counted_host_waits_of_the_graph_entries(dge):
    """dge_host_sync_count around one call, on layered_graph(R=60, T=5, deg=9, seed=0): 1550 edges, so build_alias(False) takes its hub-list path, and no vertex
    with 1024 edges, so there is no hub.  The figures are those of the build of commit 8cce4c7, the last one before the handle's groups, measured on an MI355X:
    upper bounds, but for sample_walks_into, which the trainer's zero-wait episode counts on."""
    src, dst, w, sources = layered_graph(R=60, T=5, deg=9, seed=0)
    assert len(src) >= 1024 and np.bincount(src).max() < 1024

    def waits(call):
        c0 = dge.host_sync_count(); call()
        return dge.host_sync_count() - c0
    g = dge.DeviceGraph(0); g.add_edges(src, dst, w)
    assert waits(lambda: g.set_sources(sources)) <= 2              # 8cce4c7: 2 (the CSR is built in the call)
    assert waits(lambda: g.set_sources(sources)) <= 1              # 8cce4c7: 1
    assert waits(lambda: g.build_alias(True)) <= 2                 # 8cce4c7: 2
    assert waits(lambda: g.build_alias(False)) <= 4                # 8cce4c7: 4
    corpus = dge.WalkCorpus.from_host(np.zeros((256, 5), np.int32), 0)
    assert waits(lambda: g.sample_walks_into(corpus, 0, 256, 7, 0)) == 1        # 8cce4c7: 1
    assert waits(lambda: g.keep_top_k(1)) <= 3                     # 8cce4c7: 3 (least degree, compaction, the sources' refresh)


def test_walk_handles_made_and_dropped_on_every_path(dge, oracle, tmp_path):
    """Every creator of a walk corpus with no row and with one row, and the .seq reader refused after the device has worked (a NUL byte in the last line of the
    last piece): the handle comes back null, the message names the entry, and the next good call on the device gives what the text says."""
    import ctypes as C
    W = dge.WalkCorpus
    # from_host
    for rows in (np.zeros((0, 4), np.int32), np.array([[3, 1, 2, -1]], np.int32)):
        c = W.from_host(rows, 0)
        assert c.shape == rows.shape and np.array_equal(c.to_host(), rows)
        c.close()
    # sample_walks_device
    src, dst, w, sources = layered_graph(R=20, T=4, deg=3, seed=5)
    og, dg = build_both(oracle, dge, src, dst, w, sources)
    for n in (0, 1):
        c = dg.sample_walks_device(n, 6, seed=9)
        assert c.shape == (n, 6) and np.array_equal(c.to_host(), og.sample_walks(1, 6, seed=9, rng_mode=1)[:n])
        c.close()
    # from_seq
    c, names, info = W.from_seq(b"")
    assert c.shape[0] == 0 and c.to_host().size == 0 and len(names) == 0 and info["rows"] == 0
    c.close()
    c, names, info = W.from_seq(b"a b c\n")
    assert c.to_host().tolist() == [[0, 1, 2]] and names.as_bytes() == [b"a", b"b", b"c"]
    c.close()
    ok, bad, good = (str(tmp_path / name) for name in ("ok.seq", "bad.seq", "good.seq"))
    open(ok, "wb").write(b"a b c\nb a\n")
    open(bad, "wb").write(b"c d\nd \0e\n")
    open(good, "wb").write(b"c d\n")
    names = dge.Names(["a"])
    text = b"a b\nb \0c\n"
    for entry, call in (("dge_walks_from_seq_text", lambda out: dge.lib.dge_walks_from_seq_text(0, text, len(text), names._h, 1, C.byref(out), None)),
                        ("dge_walks_from_seq_files", lambda out: dge.lib.dge_walks_from_seq_files(0, (C.c_char_p * 2)(ok.encode(), bad.encode()), 2, names._h, 1, C.byref(out), None))):
        out = C.c_void_p(0xdead)
        assert call(out) == 7 and not out.value
        msg = dge.lib.dge_last_error().decode()
        assert entry in msg and "NUL" in msg, msg
    assert names.as_bytes() == [b"a"]                                # a refused text adds no names
    c, names, info = W.from_seq([ok, good], names=names)
    from embedding_amd import io
    want, want_names = io.read_seq([ok, good])                       # the host reader: "a", the name held before, is also the first it meets
    assert np.array_equal(c.to_host(), want) and list(names) == want_names == ["a", "b", "c", "d"] and info["rows"] == len(want) == 3
    c.close()
