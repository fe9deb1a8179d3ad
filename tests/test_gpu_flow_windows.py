"""GPU: the flow table by hour window (include/dge.h: dge_flows_add_entries, dge_flows_window_edges, dge_graph_add_flow_windows, dge_flows_triplets;
csrc/flow_windows.hip) against tests/flow_ref.py — window sums in plain loops, the triplet search as the reference's loop with its ten conditions.  Every
comparison is exact equality.  The references are computed once and shared."""
import ctypes as C
import os
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_ref  # noqa: E402
import trip_ref  # noqa: E402

pytestmark = pytest.mark.gpu
MESH, _ = trip_ref.quad_mesh(13, 20251019)                    # 169 quads, shuffled, ids not contiguous
R = len(MESH.ids)
CENTRES = np.array([np.mean(region[0][:-1], 0) for region in MESH.rings])
RULES = {"default": flow_ref.DEFAULT_RULE,
         "ratio1": dict(A=(7, 3), B=(17, 8), C=(17, 6), D=(6, 7), E=(7, 7), min_a=0, min_b=0, ratio=1),         # B runs past midnight into hour 0
         "ratio3": dict(A=(23, 11), B=(17, 7), C=(16, 7), D=(7, 6), E=(7, 7), min_a=0, min_b=0, ratio=3),       # A runs from 23 to 9; no pair of the generators holds 3 : 1 in C
         "wrap2": dict(A=(7, 3), B=(17, 8), C=(17, 6), D=(7, 6), E=(6, 8), min_a=0, min_b=0, ratio=2)}          # the minima gone: the counts at 30 and 70 pass, the ninth decides
_cache = {}


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def regions(dge):
    return dge.Regions.from_arrays(*MESH.arrays())


def table_of(flows):
    h, s, e, c = flows.to_host()
    return list(zip(zip(h.tolist(), s.tolist(), e.tolist()), c.tolist()))


def state_of(flows):
    return [a.tobytes() for a in flows.to_host()], {k: v for k, v in flows.info().items() if k != "kernel_ms"}


def split_entries(c, seed):
    """the table as shuffled entries with repeats: every count cut into one to three parts"""
    rng = np.random.default_rng(seed)
    rows = []
    for key, w in c.items():
        parts = int(min(w, rng.integers(1, 4)))
        cuts = sorted(rng.choice(np.arange(1, w), parts - 1, replace=False).tolist()) if parts > 1 else []
        rows += [key + (b - a,) for a, b in zip([0] + cuts, cuts + [w])]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    return [np.array([r[q] for r in rows], t) for q, t in enumerate((np.int32, np.int32, np.int32, np.int64))]


def flows_from(dge, c, calls=1, seed=0):
    """a table built from c by `calls` calls of add_entries: calls = 1 in the dict's order without repeats, more: shuffled, with repeats"""
    f = dge.Flows(regions(dge))
    if calls == 1:
        f.add_entries(*flow_ref.arrays(c))
    else:
        h, s, e, w = split_entries(c, seed)
        for part in np.array_split(np.arange(len(h)), calls):
            f.add_entries(h[part], s[part], e[part], w[part])
    return f


def random_table(n, seed, among=20):
    """n draws of (hour, s, e) over `among` regions: most pairs are silent in some hours and not in others"""
    rng = np.random.default_rng(seed)
    some = rng.choice(R, among, replace=False)
    c = Counter()
    for h, s, e, w in zip(rng.integers(0, 24, n).tolist(), some[rng.integers(0, among, n)].tolist(), some[rng.integers(0, among, n)].tolist(), rng.integers(1, 60, n).tolist()):
        c[(h, s, e)] += w
    return dict(c)


# ------------------------------------------------------------------------------------------ 1. add_entries
def test_add_entries_in_any_order_with_repeats_over_any_number_of_calls(dge):
    c = random_table(3000, 1, among=R)
    want = sorted(c.items())
    first = None
    for calls in (1, 2, 7):
        f = flows_from(dge, c, calls, seed=calls)
        assert table_of(f) == want, calls
        info = f.info()
        total = sum(c.values())
        assert (info["trips"], info["mapped"], info["entries"]) == (total, total, len(c)) and info["kernel_ms"] > 0
        assert all(info[k] == 0 for k in ("bad", "no_start", "no_end", "located", "on_boundary", "multi", "outside", "exact"))
        first = first or state_of(f)
        assert state_of(f) == first
    f.add_entries(*[a[:0] for a in flow_ref.arrays(c)])
    assert state_of(f) == first


def test_add_entries_gives_the_table_of_the_trips(dge):
    rng = np.random.default_rng(2)
    s, e, h = rng.integers(0, R, 2000), rng.integers(0, 40, 2000), rng.integers(0, 24, 2000).astype(np.int32)
    by_trips = dge.Flows(regions(dge)); by_trips.add_trips(CENTRES[s], CENTRES[e], h)
    c = Counter(zip(h.tolist(), s.tolist(), e.tolist()))
    assert max(c.values()) > 1 and by_trips.info()["mapped"] == 2000 and table_of(by_trips) == sorted(c.items())      # every centre lies in its own quad
    by_entries = flows_from(dge, c, 3, seed=3)
    assert [a.tobytes() for a in by_entries.to_host()] == [a.tobytes() for a in by_trips.to_host()]
    a, b = by_entries.info(), by_trips.info()
    assert all(a[k] == b[k] for k in ("trips", "mapped", "bad", "no_start", "no_end", "entries")) and a["located"] == 0 and b["located"] == 4000
    # entries on top of trips, and trips on top of entries
    by_trips.add_entries(*flow_ref.arrays(c)); by_entries.add_trips(CENTRES[s], CENTRES[e], h)
    assert table_of(by_trips) == table_of(by_entries) == sorted((k, 2 * w) for k, w in c.items()) and by_trips.info()["trips"] == by_entries.info()["trips"] == 4000


def test_add_entries_refuses_bad_entries_and_leaves_the_table(dge):
    c = random_table(200, 4)
    f = flows_from(dge, c)
    before = state_of(f)
    h, s, e, w = [a[:6].copy() for a in flow_ref.arrays(c)]
    for column, value, at, word in ((h, 24, 4, "hour"), (h, -1, 2, "hour"), (s, R, 3, "indices"), (e, -1, 5, "indices"), (s, -7, 0, "indices"), (w, 0, 1, "count"), (w, -5, 4, "count")):
        keep = column.copy()
        column[at] = value; column[5] = value if at < 5 else column[5]                  # a second offender behind it: the least position is named
        with pytest.raises(dge.DgeError) as ei:
            f.add_entries(h, s, e, w)
        assert ei.value.code == 1 and "entry %d " % at in str(ei.value) and word in str(ei.value), str(ei.value)
        column[:] = keep
        assert state_of(f) == before
    w[2] = 2 ** 40 + 1
    with pytest.raises(dge.DgeError) as ei:
        f.add_entries(h, s, e, w)
    assert ei.value.code == 2 and state_of(f) == before
    w[2] = 2 ** 40 - c[(int(h[2]), int(s[2]), int(e[2]))]                               # the key's total is 2^40 exactly: fine; one more is not
    f.add_entries(h[2:3], s[2:3], e[2:3], w[2:3])
    full = state_of(f)
    assert dict(table_of(f))[(int(h[2]), int(s[2]), int(e[2]))] == 2 ** 40
    with pytest.raises(dge.DgeError) as ei:
        f.add_entries(h[:4], s[:4], e[:4], np.ones(4, np.int64))
    assert ei.value.code == 2 and "2^40" in str(ei.value) and state_of(f) == full


# ------------------------------------------------------------------------------------------ 2. window_edges
def shared_table(dge):
    if "table" not in _cache:
        c = random_table(3000, 5)
        _cache["table"] = (c, flows_from(dge, c, 2, seed=6))
    return _cache["table"]


def edges_of(got):
    return list(zip(*[a.tolist() for a in got]))


def test_window_edges_are_the_references(dge):
    c, f = shared_table(dge)
    rng = np.random.default_rng(7)
    singles = [(int(h), 1) for h in rng.permutation(24)]
    forty = singles[:10] + [(0, 0), (0, 24), (22, 5), (22, 5), (23, 24), (5, 0)] + [(int(a), int(b)) for a, b in zip(rng.integers(0, 24, 24), rng.integers(0, 25, 24))]
    assert len(forty) == 40
    for windows in ([(0, 0)], [(0, 24)], [(22, 5)], [(13, 1)], singles, forty):
        got = f.window_edges(windows)
        assert got[0].dtype == np.int32 and all(a.dtype == np.int64 for a in got[1:])
        want = flow_ref.window_edges(c, MESH.ids, windows)
        assert edges_of(got) == want, windows
        assert (len(want) > 0) == any(n > 0 for _, n in windows)
    two = edges_of(f.window_edges([(22, 5), (22, 5)]))
    assert [x[1:] for x in two if x[0] == 0] == [x[1:] for x in two if x[0] == 1] and len(two) > 100          # a repeated window repeats its edges
    assert edges_of(f.window_edges(dge.Flows.windows_from_intervals([20, 2, 9, 9, 20]))) == flow_ref.window_edges(c, MESH.ids, [(20, 6), (2, 7), (9, 0), (9, 11)])
    empty = dge.Flows(regions(dge))
    assert edges_of(empty.window_edges(forty)) == []


def test_window_edges_against_the_slots(dge):
    c, f = shared_table(dge)
    for T in (1, 2, 3, 4, 6, 8, 12, 24):
        w = 24 // T
        assert edges_of(f.window_edges([(k * w, w) for k in range(T)])) == edges_of(f.slot_edges(T, dge.Flows.EVEN)), T
    day = edges_of(f.window_edges(dge.Flows.windows_cross_time(24)))
    assert day == edges_of(f.slot_edges(24, dge.Flows.EVEN)) == edges_of(f.slot_edges(24, dge.Flows.AS_TRACTS))
    # the cross-time graph of T = 8 against AS_TRACTS: every AS_TRACTS edge is there with its weight, and edges AS_TRACTS does not have
    cross = edges_of(f.window_edges(dge.Flows.windows_cross_time(8)))
    want = flow_ref.window_edges(c, MESH.ids, [(h, 3) for h in range(8)])
    as_tracts = edges_of(f.slot_edges(8, dge.Flows.AS_TRACTS))
    assert set(want) > set(as_tracts) and len(want) > len(as_tracts) + 50
    assert cross == want


def test_window_edges_cap_and_size_query(dge):
    c, f = shared_table(dge)
    n = C.c_int64(0)
    win = (dge.HourWindow * 2)(dge.HourWindow(22, 5), dge.HourWindow(3, 0))
    want = flow_ref.window_edges(c, MESH.ids, [(22, 5), (3, 0)])
    b32 = np.zeros(len(want), np.int32); a, b, w = (np.zeros(len(want), np.int64) for _ in range(3))
    assert dge.lib.dge_flows_window_edges(f._h, win, 2, None, None, None, None, 0, C.byref(n)) == 4 and n.value == len(want)
    assert dge.lib.dge_flows_window_edges(f._h, win, 2, p(b32), p(a), p(b), p(w), len(want) - 1, C.byref(n)) == 4 and n.value == len(want) and not a.any()
    assert dge.lib.dge_flows_window_edges(f._h, win, 2, p(b32), p(a), p(b), p(w), len(want), C.byref(n)) == 0 and edges_of((b32, a, b, w)) == want
    assert dge.lib.dge_flows_window_edges(f._h, (dge.HourWindow * 1)(dge.HourWindow(3, 0)), 1, None, None, None, None, 0, C.byref(n)) == 0 and n.value == 0


# ------------------------------------------------------------------------------------------ 3. the graph
def store_of(g):
    c = g.get_csr(tables=True)
    s = g.get_source_alias()
    return [c["row_ptr"], c["nbr"], c["weight"], c["out_degree"], c["prob"], c["alias"], s["prob"], s["alias"], s["src"], np.float64(s["weight_sum"])]


@pytest.mark.parametrize("windows", [[(h, 3) for h in range(8)], [(20, 6), (2, 7), (9, 0), (9, 11)], [(0, 24)]], ids=["cross_time_8", "intervals", "static"])
def test_the_graph_is_the_one_the_window_edges_texts_give(dge, windows):
    c, f = shared_table(dge)
    K = len(windows)
    a, a_names, a_info = dge.DeviceGraph.from_flow_windows(f, windows)
    b, b_names, b_info = dge.DeviceGraph.from_od(trip_ref.od_texts(edges_of(f.window_edges(windows)), K))
    assert a.num_vertices == b.num_vertices > 0 and a.num_edges == b.num_edges > 0
    a.build_alias(True); b.build_alias(True)
    for x, y in zip(store_of(a), store_of(b)):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes() and np.asarray(x).shape == np.asarray(y).shape
    assert a.sample_walks(512, min(K + 2, 12), seed=11).tobytes() == b.sample_walks(512, min(K + 2, 12), seed=11).tobytes()
    assert np.array_equal(a.regions(), b.regions()) and list(a_names) == list(b_names) and len(a_names) == K * len(a.regions())
    assert (a_info["bytes"], a_info["lines"], a_info["dropped"], a_info["host_values"]) == (0, 0, 0, 0) and a_info["flows"] == a_info["edges"] == b_info["edges"]
    assert {k: a_info[k] for k in ("regions", "sources", "slices")} == {k: b_info[k] for k in ("regions", "sources", "slices")} and a_info["slices"] == K


def test_a_used_graph_is_refused_and_an_empty_table_gives_an_empty_graph(dge):
    c, f = shared_table(dge)
    win = (dge.HourWindow * 8)(*[dge.HourWindow(h, 3) for h in range(8)])
    used = dge.DeviceGraph(0); used.add_edges([0], [1], [1.0])
    held = dge.Names(["a"])
    for graph, names, code, word in ((used, None, 5, "fresh"), (dge.DeviceGraph(0), held, 1, "names must be empty")):
        rc = dge.lib.dge_graph_add_flow_windows(graph._h, f._h, win, 8, names._h if names else None, None)
        assert rc == code and word in dge.lib.dge_last_error().decode()
    assert used.num_edges == 1 and used.num_vertices == 2 and len(used.regions()) == 0 and held.as_bytes() == [b"a"]
    for flows, windows in ((dge.Flows(regions(dge)), [(h, 3) for h in range(8)]), (f, [(4, 0)] * 8)):          # an empty table, and eight empty windows
        g, names, info = dge.DeviceGraph.from_flow_windows(flows, windows)
        e, e_names, _ = dge.DeviceGraph.from_od([b""] * 8)
        assert g.num_vertices == e.num_vertices == 0 and g.num_edges == e.num_edges == 0 and len(names) == len(e_names) == 0 and len(g.regions()) == 0 and info["edges"] == 0


# ------------------------------------------------------------------------------------------ 4. triplets
def reference(kind, seed, rule):
    """the table, and the reference's triplets as ids, ascending, with its counters: once per (generator, seed, rule)"""
    if (kind, seed) not in _cache:
        _cache[(kind, seed)] = flow_ref.critical(seed) if kind == "critical" else flow_ref.tripartite(seed) + (None,)
    c, n, must = _cache[(kind, seed)]
    if (kind, seed, rule) not in _cache:
        got, info = flow_ref.triplets(c, n, RULES[rule])
        _cache[(kind, seed, rule)] = (sorted(tuple(MESH.ids[t] for t in tr) for tr in got), info)
    return (c, must) + _cache[(kind, seed, rule)]


def check_triplets(dge, f, rule, want, info):
    got, got_info = f.triplets(None if rule == "default" else RULES[rule], return_info=True)
    assert got.dtype == np.int64 and got.shape == (len(want), 3)
    assert [tuple(r) for r in got.tolist()] == want
    assert {k: got_info[k] for k in info} == info and got_info["kernel_ms"] > 0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_triplets_on_the_edge_of_every_condition(dge, seed):
    c, must, want, info = reference("critical", seed, "default")
    assert want == sorted(tuple(MESH.ids[t] for t in tr) for tr in must) and len(want) == 22 and info["candidates"] >= 24
    check_triplets(dge, flows_from(dge, c), "default", want, info)


@pytest.mark.parametrize("seed", [1, 2])
def test_triplets_where_the_lists_cross_a_wave(dge, seed):
    c, _, want, info = reference("tripartite", seed, "default")
    assert len(want) >= 100 and info["candidates"] >= len(want) + 100 and info["pairs_31"] > 2 * 64
    check_triplets(dge, flows_from(dge, c), "default", want, info)


@pytest.mark.parametrize("kind,seed", [("critical", 1), ("tripartite", 1)])
@pytest.mark.parametrize("rule", ["ratio1", "ratio3", "wrap2"])
def test_triplets_under_another_rule(dge, kind, seed, rule):
    c, _, want, info = reference(kind, seed, rule)
    assert want != reference(kind, seed, "default")[2] and info["pairs_12"] > 0 and info["pairs_23"] > 0 and info["pairs_31"] > 0
    if rule == "wrap2":
        assert info["candidates"] > info["triplets"] > 22
    check_triplets(dge, flows_from(dge, c), rule, want, info)


@pytest.mark.parametrize("kind,seed", [("critical", 2), ("tripartite", 2)])
def test_triplets_do_not_depend_on_how_the_table_was_built(dge, kind, seed):
    c, _, want, info = reference(kind, seed, "default")
    for calls in (2, 5):
        f = flows_from(dge, c, calls, seed=10 + calls)
        assert table_of(f) == sorted(c.items())
        check_triplets(dge, f, "default", want, info)


# ------------------------------------------------------------------------------------------ 5. the edges of the interface
def test_triplets_on_trivial_tables(dge):
    zero = dict(pairs_12=0, pairs_23=0, pairs_31=0, candidates=0, triplets=0)
    ring = lambda x: [(x, 0.0), (x + 1.0, 0.0), (x + 1.0, 1.0), (x, 1.0), (x, 0.0)]  # noqa: E731
    two = dge.Flows(dge.Regions.from_arrays(*trip_ref.Regions([5, 6], [[ring(0.0)], [ring(2.0)]]).arrays()))
    two.add_entries([8, 8, 18, 18], [0, 1, 1, 0], [1, 0, 0, 1], [40, 10, 50, 20])
    only_self = dge.Flows(regions(dge))
    only_self.add_entries(np.repeat([8, 19, 20], R), np.tile(np.arange(R), 3), np.tile(np.arange(R), 3), np.full(3 * R, 500))
    for f in (two, dge.Flows(regions(dge)), only_self):
        got, info = f.triplets(return_info=True)
        assert got.shape == (0, 3) and got.dtype == np.int64 and {k: info[k] for k in zero} == zero
    # (t1, t2) pairs pass and no (t2, t3) does: pairs without a triangle
    c, _, _, _ = reference("critical", 1, "default")
    morning = {k: w for k, w in c.items() if k[0] in (8, 18) and k[1] != k[2]}
    want, want_info = flow_ref.triplets(morning, 144)
    got, info = flows_from(dge, morning).triplets(return_info=True)
    assert want == [] and want_info["pairs_12"] > 20 and want_info["pairs_31"] == 0
    assert got.shape == (0, 3) and {k: info[k] for k in want_info} == want_info


def test_triplets_cap_and_size_query(dge):
    c, _, want, _ = reference("critical", 1, "default")
    f = flows_from(dge, c)
    n = C.c_int64(0)
    a, b, d = (np.zeros(len(want), np.int64) for _ in range(3))
    info = dge.TripletInfo()
    assert dge.lib.dge_flows_triplets(f._h, None, None, None, None, 0, C.byref(n), C.byref(info)) == 4 and n.value == len(want) == info.triplets
    assert dge.lib.dge_flows_triplets(f._h, None, p(a), p(b), p(d), len(want) - 1, C.byref(n), None) == 4 and n.value == len(want) and not a.any()
    assert dge.lib.dge_flows_triplets(f._h, None, p(a), p(b), p(d), len(want), C.byref(n), None) == 0 and list(zip(a.tolist(), b.tolist(), d.tolist())) == want
