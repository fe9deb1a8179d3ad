"""GPU: dge_line_coo / dge_line_flows (csrc/line.hip) against the rule of include/dge.h as tests/line_ref.py reads it: X, Y and touched as bits and the counters
of info, for both orders, at the row widths where a lane takes another column (dim 1, 15, 16, 17, 20, 33, 64, 65, 128, 256), K 0, 1, 5, 32 and batches of 1, 7
and 256 samples with a short last batch; a larger run equals the host loop of tests/native/line_rule_harness.cpp; two calls and a shuffled input give the same
bits; leaving the bound is an error that names the batch; errors name the right entry and leave the outputs untouched, in the order of their kinds, a repeat across
a workgroup boundary of the check and dropped entries that are none included; the flow table's slots as graphs; and the three-block graph is learnt: every cosine neighbour of every vertex lies in its block.

The "mixed" graph has 40 vertices: vertex 38 has in-edges and no out-edge (never a negative, touched), vertex 39 no edge at all (untouched, its row stays at its
initial value).  The "hub" graph points every edge at vertex 3, so one row takes every target add of a batch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import line_ref as ref  # noqa: E402
import trip_ref  # noqa: E402
from line_harness import harness_line, load_harness  # noqa: E402

pytestmark = pytest.mark.gpu

DIMS = [1, 15, 16, 17, 20, 33, 64, 65, 128, 256]
KS = [0, 1, 5, 32]
BATCHES = {1: 301, 7: 1000, 256: 1999}                     # batch -> samples, never a multiple of the batch


def mixed_graph():
    s, d, w = ref.random_graph(40, 300, 3)
    keep = (s < 38) & (d < 38)
    s, d, w = s[keep], d[keep], w[keep]
    extra = np.array([0, 5, 9], np.int32)                    # 38 is pointed at
    return np.concatenate([s, extra]), np.concatenate([d, np.full(3, 38, np.int32)]), np.concatenate([w, [2.0, 7.0, 1.0]]), 40


def hub_graph():
    s = np.array([i for i in range(40) if i != 3], np.int32)
    return s, np.full(39, 3, np.int32), (1.0 + (np.arange(39) * 7) % 13).astype(np.float64), 40


def loop_graph():
    return np.array([0], np.int32), np.array([0], np.int32), np.array([5.0]), 1


GRAPHS = {"mixed": mixed_graph, "hub": hub_graph, "loop": loop_graph}


def _cases():
    out = []
    for i, dim in enumerate(DIMS):                           # every width, both orders; K and the batch rotate
        for order in (1, 2):
            out.append(("mixed", dim, order, KS[(i + order) % 4], [1, 7, 256][(i + order) % 3]))
    for K in KS:                                             # every K with every batch, both orders, at the reference's width
        for batch in BATCHES:
            for order in (1, 2):
                if ("mixed", 20, order, K, batch) not in out:
                    out.append(("mixed", 20, order, K, batch))
    for order in (1, 2):
        out += [("hub", 20, order, 5, 256), ("hub", 128, order, 5, 256), ("loop", 20, order, 5, 7), ("loop", 1, order, 0, 1)]
    return out


CASES = _cases()
_refs = {}


def config(case):
    graph, dim, order, K, batch = case
    return dict(dim=dim, order=order, negative=K, samples=BATCHES[batch], batch=batch, rho0=0.025, seed=12345)


def reference(case):
    """computed once per case, shared, never changed"""
    if case not in _refs:
        s, d, w, n = GRAPHS[case[0]]()
        _refs[case] = (s, d, w, n, ref.line(s, d, w, n, **config(case)))
    return _refs[case]


def same(got, want):
    X, Y, touched, info = got
    assert ref.same_bits(X, want["X"]), "X differs in %d of %d values" % ((X.view(np.uint64) != want["X"].view(np.uint64)).sum(), X.size)
    assert ref.same_bits(Y, want["Y"]), "Y differs in %d of %d values" % ((Y.view(np.uint64) != want["Y"].view(np.uint64)).sum(), Y.size)
    assert np.array_equal(touched, want["touched"])
    for f in ("vertices", "entries", "zeros", "batches", "samples", "total_weight", "neg_total", "max_abs"):
        assert info[f] == want[f], (f, info[f], want[f])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-dim%d-order%d-K%d-batch%d" % c)
def test_tables_equal_the_rule_as_bits(dge, case):
    import embedding_amd.evaluate as ev
    s, d, w, n, want = reference(case)
    got = ev.line_gpu(s, d, w, n, **config(case))
    same(got, want)
    assert got[3]["kernel_ms"] > 0
    graph, dim, order, K, batch = case
    if order == 1:
        assert not got[1].any()                              # order 1 leaves Y all zero
    else:
        assert got[1].any()
    if graph == "mixed":
        X, _, touched, _ = got
        assert touched[38] and not touched[39] and touched[:38].all()
        assert ref.same_bits(X[39], ref.init_table(n, dim, 12345)[39].astype(np.float64) * ref.UNFIX)          # an isolated vertex keeps its initial row
        dr = want["G"].draws(12345, 0, BATCHES[batch], K)
        assert not (dr[:, 2:] == 38).any() and not (dr[:, 2:] == 39).any()                                       # no out-edge: never a negative
        if K == 32:
            assert (dr[:, 2:] == dr[:, :1]).any()                                                                # a negative equal to u is trained like any other
    if graph == "hub":
        assert (want["G"].ed == 3).all()


@pytest.mark.parametrize("dim", [20, 128])
@pytest.mark.parametrize("order", [1, 2])
def test_a_larger_run_equals_the_host_loop(dge, tmp_path, dim, order):
    import embedding_amd.evaluate as ev
    H = load_harness(str(tmp_path / "libline_rule_harness.so"))
    s, d, w = ref.random_graph(2000, 28100, 21, hub=11)
    assert 2.95e4 < len(w) < 3.05e4
    kw = dict(dim=dim, order=order, negative=5, samples=200000, batch=4096, rho0=0.025, seed=1)
    same(ev.line_gpu(s, d, w, 2000, **kw), harness_line(H, s, d, w, 2000, **kw))


def test_two_calls_a_shuffled_input_zeros_and_a_supplied_init(dge):
    import embedding_amd.evaluate as ev
    case = ("mixed", 20, 2, 5, 256)
    s, d, w, n, want = reference(case)
    kw = config(case)
    a = ev.line_gpu(s, d, w, n, **kw)
    b = ev.line_gpu(s, d, w, n, **kw)
    assert ref.same_bits(a[0], b[0]) and ref.same_bits(a[1], b[1])
    o = np.random.default_rng(1).permutation(len(w))
    same(ev.line_gpu(s[o], d[o], w[o], n, **kw), want)
    # zeros are dropped and counted, wherever they stand — on a pair another entry holds too
    s2 = np.concatenate([s[:5], s, [39, 38]]).astype(np.int32); d2 = np.concatenate([d[:5], d, [39, 0]]).astype(np.int32); w2 = np.concatenate([np.zeros(5), w, [0.0, -0.0]])
    same(ev.line_gpu(s2, d2, w2, n, **kw), dict(want, zeros=7))
    # the generated initial table fed back; then both tables, which is not the same run
    x0 = ref.init_table(n, 20, 12345).astype(np.float64) * ref.UNFIX
    same(ev.line_gpu(s, d, w, n, init=x0, **dict(kw, seed=12345)), want)
    y0 = np.random.default_rng(2).uniform(-0.01, 0.01, (n, 20))
    same(ev.line_gpu(s, d, w, n, init=(x0, y0), **kw), ref.line(s, d, w, n, init=(x0, y0), **kw))
    other = ev.line_gpu(s, d, w, n, **dict(kw, seed=99))
    assert not ref.same_bits(other[0], want["X"])


@pytest.mark.parametrize("order", [1, 2])
def test_leaving_the_bound_is_an_error_that_names_the_batch(dge, order):
    """init_X near 255.9 with rho0 = 1: the tables leave (-256, 256) after a batch the reference names; an error return, the outputs untouched"""
    from embedding_amd._native import LineCfg, LineInfo
    s, d, w, n = mixed_graph()
    x0 = np.full((n, 4), 255.9)
    y0 = np.full((n, 4), 255.9) if order == 2 else None      # order 2 from Y = 0 stays inside the bound for these 50 samples: the context table starts high too
    kw = dict(dim=4, order=order, negative=2, samples=50, batch=1, rho0=1.0, seed=3)
    with pytest.raises(ref.BoundLeft) as left:
        ref.line(s, d, w, n, init=x0 if y0 is None else (x0, y0), **kw)
    at = left.value.batch
    print("order %d: the reference leaves the bound after batch %d" % (order, at))
    assert 1 <= at < 50                                      # not the first batch: the word is folded over many launches
    X = np.full((n, 4), 9.0); Y = np.full((n, 4), 7.0); touched = np.full(n, 5, np.uint8); info = LineInfo(); info.vertices = -5
    cfg = LineCfg(4, order, 2, 1, 50, 1.0, 3)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    si = np.ascontiguousarray(s, np.int32); di = np.ascontiguousarray(d, np.int32)
    rc = dge.lib.dge_line_coo(0, p(si), p(di), p(w), len(w), n, C.byref(cfg), p(x0), None if y0 is None else p(y0), p(X), p(Y), p(touched), C.byref(info))
    msg = (dge.lib.dge_last_error() or b"").decode()
    assert rc == 1 and "dge_line_coo" in msg and ("batch %d " % at) in msg, (rc, msg)
    assert (X == 9.0).all() and (Y == 7.0).all() and (touched == 5).all() and info.vertices == -5
    cfg.rho0 = 0.025                                         # the same call inside the bound
    x1 = np.full((n, 4), 0.1)
    rc = dge.lib.dge_line_coo(0, p(si), p(di), p(w), len(w), n, C.byref(cfg), p(x1), None, p(X), p(Y), p(touched), C.byref(info))
    assert rc == 0 and info.vertices == n and (X != 9.0).all()


def test_errors_name_the_entry_and_leave_the_outputs_untouched(dge):
    from embedding_amd._native import LineCfg, LineInfo
    lib = dge.lib
    s, d, w, n = mixed_graph()
    n_e = len(w)
    X = np.full((n, 8), 9.0); Y = np.full((n, 8), 7.0); touched = np.full(n, 5, np.uint8); info = LineInfo(); info.vertices = -5
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731

    def call(s=s, d=d, w=w, dim=8):
        cfg = LineCfg(dim, 2, 5, 64, 500, 0.025, 1)
        s = np.ascontiguousarray(s, np.int32); d = np.ascontiguousarray(d, np.int32); w = np.ascontiguousarray(w, np.float64)
        rc = lib.dge_line_coo(0, p(s), p(d), p(w), len(w), n, C.byref(cfg), None, None, p(X), p(Y), p(touched), C.byref(info))
        return rc, (lib.dge_last_error() or b"").decode()

    def poke(values):
        v = w.copy()
        for at, x in values.items():
            v[at] = x
        return v

    dup = np.concatenate([s, s[[30, 10, 30]]]), np.concatenate([d, d[[30, 10, 30]]]), np.concatenate([w, [1.0, 2.0, 3.0]])
    first = np.concatenate([s[[10]], s]), np.concatenate([d[[10]], d]), np.concatenate([[4.0], w])      # the copy in front: the original, at 11, is the second occurrence
    for what, kw, words in (("negative", dict(w=poke({17: -1.0, 40: -1.0})), ("entry 17 ", "integer")),
                            ("NaN", dict(w=poke({23: np.nan, 90: np.inf, 4: 0.0})), ("entry 23 ", "integer")),
                            ("a fraction", dict(w=poke({60: 1.5, 61: np.nan})), ("entry 60 ", "integer")),
                            ("2^31", dict(w=poke({33: 2.0 ** 31, 70: 2.0 ** 40})), ("entry 33 ", "2^31")),
                            ("duplicate", dict(s=dup[0], d=dup[1], w=dup[2]), ("entry %d " % n_e, "repeats")),
                            ("duplicate in front", dict(s=first[0], d=first[1], w=first[2]), ("entry 11 ", "repeats")),
                            ("outside", dict(d=np.where(np.arange(n_e) == 8, 40, d)), ("entry 8 ", "outside")),
                            ("negative vertex", dict(s=np.where(np.arange(n_e) == 2, -1, s)), ("entry 2 ", "outside")),
                            ("dim 257", dict(dim=257), ("dim = 257",)),
                            ("all zero", dict(w=np.zeros(n_e)), ("zero",))):
        rc, msg = call(**kw)
        assert rc == 1 and "dge_line_coo" in msg, (what, rc, msg)
        for word in words:
            assert word in msg, (what, msg)
        assert (X == 9.0).all() and (Y == 7.0).all() and (touched == 5).all() and info.vertices == -5, what
    assert call(w=poke({33: 2.0 ** 31 - 1}))[0] == 0 and info.total_weight == int(w.sum() - w[33]) + 2 ** 31 - 1      # the greatest weight
    assert call()[0] == 0 and (X[:39] != 9.0).all() and info.vertices == n and info.entries == n_e and (touched <= 1).all()


def _error_call(dge):
    """dge_line_coo on 40 vertices with sentinel-filled outputs: call(s, d, w) -> the message; asserts the error return and the untouched outputs"""
    from embedding_amd._native import LineCfg, LineInfo
    X = np.full((40, 8), 9.0); Y = np.full((40, 8), 7.0); touched = np.full(40, 5, np.uint8); info = LineInfo(); info.vertices = -5
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731

    def call(s, d, w):
        cfg = LineCfg(8, 2, 5, 64, 500, 0.025, 1)
        s = np.ascontiguousarray(s, np.int32); d = np.ascontiguousarray(d, np.int32); w = np.ascontiguousarray(w, np.float64)
        rc = dge.lib.dge_line_coo(0, p(s), p(d), p(w), len(w), 40, C.byref(cfg), None, None, p(X), p(Y), p(touched), C.byref(info))
        msg = (dge.lib.dge_last_error() or b"").decode()
        assert rc == 1 and "dge_line_coo" in msg, (rc, msg)
        assert (X == 9.0).all() and (Y == 7.0).all() and (touched == 5).all() and info.vertices == -5, msg
        return msg
    return call


def test_faults_of_every_kind_at_once_are_reported_in_the_order_of_the_kinds(dge):
    """one input holds a weight of 2^31 (entry 20), a fraction (30), a repeat (40 repeats 3) and a vertex outside (60): the kinds are looked for in the order
    outside, not an integer, too great, repeat, whatever their indices — the least index over all kinds, 20, comes third"""
    call = _error_call(dge)
    s, d, w, n = mixed_graph()
    assert n == 40 and len(w) > 61
    s = s.copy(); d = d.copy(); w = w.copy()
    good_d60 = d[60]
    s[40], d[40] = s[3], d[3]
    w[20] = 2.0 ** 31; w[30] = 1.5; d[60] = 40
    msg = call(s, d, w)
    assert "entry 60 " in msg and "outside" in msg, msg
    d[60] = good_d60
    msg = call(s, d, w)
    assert "entry 30 " in msg and "integer" in msg, msg
    w[30] = 2.0
    msg = call(s, d, w)
    assert "entry 20 " in msg and "2^31" in msg, msg
    w[20] = 2.0
    msg = call(s, d, w)
    assert "entry 40 " in msg and "repeats" in msg, msg


def distinct_edges(count, seed):
    """count edges among 40 vertices on distinct (source, destination) pairs, in no order, integer weights"""
    rng = np.random.default_rng(seed)
    k = rng.permutation(40 * 40)[:count]
    return (k // 40).astype(np.int32), (k % 40).astype(np.int32), rng.integers(1, 51, count).astype(np.float64)


def test_a_repeat_whose_two_entries_sort_into_different_workgroups_of_the_check(dge):
    """258 kept entries; the last repeats the pair of the entry that sorts to position 255 of the others, so the two sit at sorted positions 255 and 256"""
    call = _error_call(dge)
    s, d, w = distinct_edges(258, 11)
    at = int(np.argsort(s[:257].astype(np.int64) * 40 + d[:257])[255])
    s[257], d[257] = s[at], d[at]
    msg = call(s, d, w)
    assert "entry 257 " in msg and "repeats" in msg, msg
    front = lambda a: np.concatenate([a[[257]], a[:257]])      # noqa: E731    the copy in front: the original, shifted by one, is the second occurrence
    msg = call(front(s), front(d), front(w))
    assert ("entry %d " % (at + 1)) in msg and "repeats" in msg, msg


def test_dropped_entries_are_no_repeats(dge):
    """three zeros on one pair that a kept entry holds and two -0.0 on another, spread through the input: counted, and the tables are those without them"""
    import embedding_amd.evaluate as ev
    s, d, w = distinct_edges(258, 11)
    kw = dict(dim=8, order=2, negative=5, samples=500, batch=64, rho0=0.025, seed=5)
    X, Y, touched, info = ev.line_gpu(s, d, w, 40, **kw)
    assert info["entries"] == 258 and info["zeros"] == 0
    s2, d2, w2 = s.tolist(), d.tolist(), w.tolist()
    for at, edge, zero in ((258, 7, 0.0), (200, 100, -0.0), (129, 7, 0.0), (40, 100, -0.0), (0, 7, 0.0)):      # descending places: each insert leaves the earlier ones where they are
        s2.insert(at, int(s[edge])); d2.insert(at, int(d[edge])); w2.insert(at, zero)
    X2, Y2, touched2, info2 = ev.line_gpu(np.array(s2, np.int32), np.array(d2, np.int32), np.array(w2), 40, **kw)
    assert info2["zeros"] == 5 and info2["entries"] == 258
    assert ref.same_bits(X2, X) and ref.same_bits(Y2, Y) and np.array_equal(touched2, touched)


def flows_fixture(dge):
    mesh, _ = trip_ref.quad_mesh(6, 77)                     # 36 regions, shuffled, ids not contiguous
    rg = dge.Regions.from_arrays(*mesh.arrays())
    rng = np.random.default_rng(3)
    hot = rng.uniform([-87.88, 41.62], [-87.42, 42.08], (60, 2))
    s = hot[rng.integers(0, 60, 4000)]; e = hot[rng.integers(0, 60, 4000)]
    hour = rng.integers(0, 24, 4000).astype(np.int32)
    f = dge.Flows(rg); f.add_trips(s, e, hour)
    assert f.info()["mapped"] > 2000
    return rg, f


@pytest.mark.parametrize("T,slot", [(4, 2), (1, 0)])
def test_flows_slots_as_graphs(dge, T, slot):
    import embedding_amd.evaluate as ev
    rg, f = flows_fixture(dge)
    R = rg.info()["regions"]
    index_of = {int(i): k for k, i in enumerate(rg.ids)}
    sl, src, dst, w = f.slot_edges(T, f.EVEN)
    here = sl == slot
    assert here.sum() > 100
    rows = np.array([index_of[int(i)] for i in src[here]], np.int32); cols = np.array([index_of[int(i)] for i in dst[here]], np.int32); vals = w[here].astype(np.float64)
    for order in (1, 2):
        kw = dict(dim=20, order=order, negative=5, samples=1500, batch=256, rho0=0.025, seed=7)
        X, Y, touched, ids, info = f.line(slot, T=T, **kw)
        want = ev.line_gpu(rows, cols, vals, R, **kw)
        assert ref.same_bits(X, want[0]) and ref.same_bits(Y, want[1]) and np.array_equal(touched, want[2])
        assert np.array_equal(ids, rg.ids) and np.array_equal(info["region_index"], np.arange(R))
        assert {k: info[k] for k in info if k not in ("kernel_ms", "region_index")} == {k: want[3][k] for k in want[3] if k != "kernel_ms"}
        same((X, Y, touched, info), ref.line(rows, cols, vals, R, **kw))
        # a mask: the call on the compacted sub-graph
        select = np.random.default_rng(T).random(R) < 0.6
        compact = np.cumsum(select) - 1
        keep = select[rows] & select[cols]
        Xm, Ym, tm, idm, infm = f.line(slot, T=T, select=select, **kw)
        wantm = ev.line_gpu(compact[rows[keep]], compact[cols[keep]], vals[keep], int(select.sum()), **kw)
        assert Xm.shape == (select.sum(), 20) and ref.same_bits(Xm, wantm[0]) and ref.same_bits(Ym, wantm[1]) and np.array_equal(tm, wantm[2])
        assert np.array_equal(idm, rg.ids[select]) and np.array_equal(infm["region_index"], np.nonzero(select)[0]) and infm["entries"] == keep.sum()
    with pytest.raises(dge.DgeError, match="no region is selected"):
        f.line(slot, T=T, select=np.zeros(R, bool))
    with pytest.raises(dge.DgeError, match="slot = %d" % T):
        f.line(T, T=T)


@pytest.mark.parametrize("order", [1, 2])
def test_the_three_block_graph_is_learnt(dge, order):
    """every one of the 5 cosine neighbours (dge_knn_cosine_vectors) of every one of the 36 vertices lies in the vertex's block; no vertex is left out"""
    import embedding_amd.evaluate as ev
    s, d, w, n = ref.three_blocks()
    X, Y, touched, info = ev.line_gpu(s, d, w, n, dim=16, order=order, negative=5, samples=20000, batch=256, rho0=0.025, seed=1)
    assert n == 36 and touched.all() and info["max_abs"] < 256
    vec = dge.Vectors.from_line(X, touched)
    assert vec.present().all()
    idx, _, _ = vec.knn(5)
    block = np.arange(n) // 12
    assert idx.shape == (36, 5) and (idx >= 0).all()
    wrong = [(v, idx[v].tolist()) for v in range(n) if not (block[idx[v]] == block[v]).all()]
    assert not wrong, wrong
    feats = ev.line_features(X, touched)
    assert feats.dtype == np.float32 and feats.shape == (36, 16) and np.array_equal(feats, X.astype(np.float32))
