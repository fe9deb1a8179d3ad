"""GPU: trips into regions, regions into flows, flows into the graph (include/dge.h: dge_regions_*, dge_flows_*, dge_graph_add_flows; csrc/trip_map.hip) against
tests/trip_ref.py — exact rational location against every segment of every region, flows by Counter, the slot rules in plain loops — and, for the counter
`exact`, against the host build of csrc/pip_exact.h (tests/native/pip_exact_harness.cpp).  Every comparison is exact equality.  Every locate case runs with
grid = 1, 7, 64 and 0 (the library's rule): the regions and every counter must be the same."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trip_ref  # noqa: E402
from test_pip_exact_host import load_harness  # noqa: E402

pytestmark = pytest.mark.gpu
GRIDS = (1, 7, 64, 0)
COUNTERS = ("points", "located", "on_boundary", "multi", "outside", "exact")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return load_harness(tmp_path_factory.mktemp("pip_exact_harness"))


def host_locate(H, ref, xy):
    seg, first = ref.segments()
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    region = np.zeros(len(xy), np.int32); c = np.zeros(5, np.int64)
    H.harness_pip_locate(seg.ctypes.data_as(C.c_void_p), first.ctypes.data_as(C.c_void_p), len(first) - 1, xy.ctypes.data_as(C.c_void_p), len(xy), region.ctypes.data_as(C.c_void_p),
                         c.ctypes.data_as(C.c_void_p))
    return region, dict(zip(("located", "on_boundary", "multi", "outside", "exact"), c.tolist()))


def check_locate(dge, H, ref, xy, want=None):
    """every grid, host and device entries, against trip_ref (or `want`, computed once) and the host harness's counters -> regions, info"""
    import torch
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    if want is None:
        want = ref.locate(xy)
    host_region, host_counters = host_locate(H, ref, xy)
    assert np.array_equal(host_region, want[0])
    first = None
    for grid in GRIDS:
        rg = dge.Regions.from_arrays(*ref.arrays(), grid=grid)
        assert rg.info()["grid"] == (grid or rg.info()["grid"]) and rg.info()["regions"] == len(ref.ids)
        got, info = rg.locate(xy, return_info=True)
        assert got.dtype == np.int32 and np.array_equal(got, want[0]), (grid, np.nonzero(got != want[0])[0][:5])
        for k, v in want[1].items():
            assert info[k] == v, (grid, k, info[k], v)
        for k, v in host_counters.items():
            assert info[k] == v, (grid, k, info[k], v)             # `exact` and `outside` among them
        assert info["points"] == len(xy) and info["kernel_ms"] >= 0
        dev, dinfo = rg.locate(torch.from_numpy(xy).cuda(), return_info=True)
        assert np.array_equal(dev.cpu().numpy(), got) and {k: dinfo[k] for k in COUNTERS} == {k: info[k] for k in COUNTERS}
        if first is None:
            first = {k: info[k] for k in COUNTERS}
        assert {k: info[k] for k in COUNTERS} == first
    return want[0], first


def ulp(v, k):
    return (np.array(v, np.float64).view(np.int64) + k).view(np.float64)


# ------------------------------------------------------------------------------------------ the quad mesh, shared
MESH, MESH_V = trip_ref.quad_mesh(12, 20251018)


def mesh_points(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-87.95, -87.35, n), rng.uniform(41.55, 42.15, n)], 1)


_shared = {}


def mesh_reference():
    """4 000 random points, every vertex, the exactly representable midpoints of shared edges and the points 1 ulp to either side: located once by trip_ref."""
    if not _shared:
        v = MESH_V
        a = np.concatenate([v[:-1, :].reshape(-1, 2), v[:, :-1].reshape(-1, 2)]); b = np.concatenate([v[1:, :].reshape(-1, 2), v[:, 1:].reshape(-1, 2)])
        mid = a + (b - a) / 2
        from fractions import Fraction
        keep = np.array([all(2 * Fraction(m) == Fraction(p) + Fraction(q) for m, p, q in zip(*row)) for row in zip(mid.tolist(), a.tolist(), b.tolist())])      # the exact midpoint
        mid = mid[keep]
        assert len(mid) > 20
        near = [np.stack([ulp(mid[:, 0], dx), ulp(mid[:, 1], dy)], 1) for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1))]
        xy = np.concatenate([mesh_points(4000, 1), v.reshape(-1, 2), mid] + near)
        _shared["xy"] = xy
        _shared["want"] = MESH.locate(xy)
        _shared["n_mid"] = len(mid)
    return _shared


def test_the_jittered_quad_mesh(dge, harness):
    s = mesh_reference()
    region, info = check_locate(dge, harness, MESH, s["xy"], s["want"])
    assert info["multi"] == 0 and info["on_boundary"] >= 13 * 13 + s["n_mid"] and info["located"] > 2000 and info["outside"] > 0 and info["exact"] > 0
    assert (region[4000:4000 + 169] == -1).all()


def ring(points):
    return [tuple(map(float, p)) for p in points] + [tuple(map(float, points[0]))]


def test_holes_islands_parts_and_a_comb(dge, harness):
    comb = [(0, -10)]
    for k in range(9):
        comb += [(2 * k, -6), (2 * k + 0.5, -1), (2 * k + 1, -6)]
    comb += [(18, -6), (18, -10)]
    regions = trip_ref.Regions([40, 7, 1000, 3], [
        [ring([(0, 0), (10, 0), (10, 10), (0, 10)]), ring([(3, 3), (7, 3), (7, 7), (3, 7)])],          # a square with a hole
        [ring([(4, 4), (6, 4), (6, 6), (4, 6)])],                                                      # an island inside the hole
        [ring([(20, 0), (22, 0), (22, 2), (20, 2)]), ring([(24, 5), (26, 5), (25, 8)])],               # two disjoint parts
        [ring(comb)]])
    verts = np.array([v for region in regions.rings for r in region for v in r])
    xs = np.unique(np.concatenate([verts[:, 0], verts[:, 0] + 0.25, [-1.0, 30.0]]))
    on_lines = np.array([(x, y) for y in np.unique(verts[:, 1]) for x in xs])                          # on the ray-through-vertex line of every vertex
    rng = np.random.default_rng(2)
    xy = np.concatenate([on_lines, verts, np.stack([rng.uniform(-2, 28, 1500), rng.uniform(-11, 11, 1500)], 1)])
    region, info = check_locate(dge, harness, regions, xy)
    assert set(region.tolist()) == {-1, 0, 1, 2, 3} and info["on_boundary"] > len(verts) // 2


def test_the_ulp_lattice_as_a_triangle(dge, harness):
    tri = trip_ref.Regions([9], [[ring([(-12, -12), (24, 24), (-12, 24)])]])
    i, j = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    xy = np.stack([0.5 + i.reshape(-1) * 2.0 ** -53, 0.5 + j.reshape(-1) * 2.0 ** -53], 1)
    region, info = check_locate(dge, harness, tri, xy)
    assert np.array_equal(region, np.where(j.reshape(-1) > i.reshape(-1), 0, -1))
    assert (info["located"], info["on_boundary"], info["outside"]) == (2016, 64, 0) and info["exact"] >= 4096


def test_a_ring_longer_than_a_tile(dge, harness):
    tile = dge.Regions.from_arrays(*trip_ref.Regions([1], [[ring([(0, 0), (1, 0), (0, 1)])]]).arrays()).info()["tile_segments"]
    m = 2 * tile + 3
    t = np.arange(m) * (2 * np.pi / m)
    circle = ring(np.stack([3 * np.cos(t), 3 * np.sin(t)], 1).tolist())
    regions = trip_ref.Regions([5, 6], [[circle], [ring([(3.5, -1), (5.5, -1), (5.5, 1), (3.5, 1)])]])
    assert len(circle) - 1 == m
    rng = np.random.default_rng(3)
    r = 3 + rng.uniform(-0.01, 0.01, 300)
    a = rng.uniform(0, 2 * np.pi, 300)
    xy = np.concatenate([np.stack([r * np.cos(a), r * np.sin(a)], 1), np.array(circle)[::97], np.stack([rng.uniform(-4, 6, 300), rng.uniform(-4, 4, 300)], 1)])
    region, info = check_locate(dge, harness, regions, xy)
    assert info["located"] > 100 and set(region.tolist()) == {-1, 0, 1}


def test_overlapping_regions(dge, harness):
    regions = trip_ref.Regions([2, 1], [[ring([(0, 0), (4, 0), (4, 4), (0, 4)])], [ring([(2, 2), (6, 2), (6, 6), (2, 6)])]])
    g = np.arange(-1, 15) * 0.5
    xy = np.array([(x, y) for x in g for y in g])
    region, info = check_locate(dge, harness, regions, xy)
    assert info["multi"] == 9 and region[(xy == (3.0, 3.0)).all(1)].tolist() == [0] and region[(xy == (5.0, 5.0)).all(1)].tolist() == [1]


def test_out_of_range_points_and_trivial_sizes(dge, harness):
    two = trip_ref.Regions([1, 2], [[ring([(0, 0), (4, 0), (4, 4), (0, 4)])], [ring([(6, 6), (8, 6), (8, 8), (6, 8)])]])
    nan, inf = float("nan"), float("inf")
    xy = np.array([(-1, 1), (9, 1), (1, -1), (1, 9), (0, 0), (8, 8), (0, 8), (8, 0), (4, 8), (0, 3), (8, 7), (nan, 1), (1, nan), (inf, 1), (1, -inf), (2.0 ** -451, 1), (1, 2.0 ** 501),
                   (1, 1), (7, 7), (5, 5), (0.0, 1), (-0.0, 1), (2.0 ** -450, 1)])
    region, info = check_locate(dge, harness, two, xy)
    assert region.tolist() == [-1] * 17 + [0, 1, -1, -1, -1, 0] and info["outside"] == 14
    empty = np.zeros((0, 2))
    assert check_locate(dge, harness, two, empty)[1]["points"] == 0
    none = trip_ref.Regions([], [])
    region, info = check_locate(dge, harness, none, xy)
    assert (region == -1).all() and info["outside"] == len(xy)
    one = trip_ref.Regions([77], [[ring([(0, 0), (1, 0), (0, 1)])]])
    region, info = check_locate(dge, harness, one, [(0.25, 0.25), (0.5, 0.5), (1, 1)])
    assert region.tolist() == [0, -1, -1] and dge.Regions.from_arrays(*one.arrays(), grid=1).info()["max_cell_candidates"] == 1


# ------------------------------------------------------------------------------------------ flows
def trips(n, seed):
    rng = np.random.default_rng(seed)
    return mesh_points(n, seed), mesh_points(n, seed + 100), rng.integers(0, 24, n).astype(np.int32)


def table_of(flows):
    h, s, e, c = flows.to_host()
    return list(zip(zip(h.tolist(), s.tolist(), e.tolist()), c.tolist()))


def reference_flows(H, s, e, h):
    c, n = trip_ref.flows(host_locate(H, MESH, s)[0], host_locate(H, MESH, e)[0], h, s, e)      # (the harness's regions are checked against trip_ref above)
    return c, n


def test_twenty_thousand_trips(dge, harness):
    import torch
    rg = dge.Regions.from_arrays(*MESH.arrays())
    s, e, h = trips(20_000, 5)
    h[:3] = (-1, 24, -2 ** 31); s[3] = (float("nan"), 41.8); e[4] = (2.0 ** 501, 41.8)
    want, n = reference_flows(harness, s, e, h)
    assert n["bad"] == 5 and n["no_start"] > 0 and n["no_end"] > 0 and n["mapped"] > 5000
    one = dge.Flows(rg); one.add_trips(s, e, h)
    assert table_of(one) == sorted(want.items())
    info = one.info()
    assert {k: info[k] for k in n} == n and info["entries"] == len(want)
    assert info["mapped"] + info["bad"] + info["no_start"] + info["no_end"] == info["trips"] and sum(want.values()) == info["mapped"]
    three = dge.Flows(rg)
    for a, b in ((0, 7000), (7000, 7001), (7001, 20_000)):
        three.add_trips(s[a:b], e[a:b], h[a:b])
    three.add_trips(s[:0], e[:0], h[:0])
    dev = dge.Flows(rg); dev.add_trips(torch.from_numpy(s).cuda(), torch.from_numpy(e).cuda(), torch.from_numpy(h).cuda())
    for other in (three, dev):
        assert [a.tobytes() for a in other.to_host()] == [a.tobytes() for a in one.to_host()]
        assert {k: v for k, v in other.info().items() if k != "kernel_ms"} == {k: v for k, v in info.items() if k != "kernel_ms"}


def test_one_key_twenty_thousand_times_and_all_keys_distinct(dge, harness):
    rg = dge.Regions.from_arrays(*MESH.arrays())
    s, e, h = trips(400, 6)
    region_s, region_e = host_locate(harness, MESH, s)[0], host_locate(harness, MESH, e)[0]
    k = int(np.nonzero((region_s >= 0) & (region_e >= 0))[0][0])
    same = dge.Flows(rg)
    same.add_trips(np.tile(s[k], (12_000, 1)), np.tile(e[k], (12_000, 1)), np.full(12_000, 9, np.int32))
    same.add_trips(np.tile(s[k], (8_000, 1)), np.tile(e[k], (8_000, 1)), np.full(8_000, 9, np.int32))
    assert table_of(same) == [((9, int(region_s[k]), int(region_e[k])), 20_000)]
    ok = np.nonzero((region_s >= 0) & (region_e >= 0))[0]
    _, firsts = np.unique(region_s[ok].astype(np.int64) * 1000 + region_e[ok], return_index=True)
    pick = ok[firsts]
    distinct = dge.Flows(rg)
    distinct.add_trips(s[pick], e[pick], np.zeros(len(pick), np.int32))
    t = table_of(distinct)
    assert len(t) == len(pick) > 100 and all(c == 1 for _, c in t) and [key for key, _ in t] == sorted((0, int(a), int(b)) for a, b in zip(region_s[pick], region_e[pick]))


def slot_trips():
    """few (s, e) pairs over many hours, with hours left empty: some (k, s, e) is empty while (k + 1, s, e) is not."""
    s, e, _ = trips(40, 8)
    rng = np.random.default_rng(9)
    idx = rng.integers(0, 40, 3000)
    hour = rng.choice([0, 1, 3, 4, 7, 8, 9, 13, 16, 21, 23], 3000).astype(np.int32)
    return s[idx], e[idx], hour


def test_slots(dge, harness):
    rg = dge.Regions.from_arrays(*MESH.arrays())
    s, e, h = slot_trips()
    want, _ = reference_flows(harness, s, e, h)
    assert any((k, a, b) not in want and (k + 1, a, b) in want for k in range(23) for (_, a, b) in want)
    f = dge.Flows(rg); f.add_trips(s, e, h)
    assert table_of(f) == sorted(want.items())
    for mode, T in [(m, T) for m in (trip_ref.EVEN, trip_ref.AS_TRACTS) for T in (1, 8, 24)] + [(trip_ref.AS_TRACTS, 5)]:
        ref = trip_ref.slot_edges(want, MESH.ids, T, mode)
        got = f.slot_edges(T, mode)
        assert got[0].dtype == np.int32 and got[3].dtype == np.int64
        assert list(zip(*[a.tolist() for a in got])) == ref, (mode, T)
        assert f.to_od_bytes(T, mode) == trip_ref.od_texts(ref, T)
    assert trip_ref.slot_edges(want, MESH.ids, 24, trip_ref.EVEN) == trip_ref.slot_edges(want, MESH.ids, 24, trip_ref.AS_TRACTS)
    assert trip_ref.slot_edges(want, MESH.ids, 8, trip_ref.EVEN) != trip_ref.slot_edges(want, MESH.ids, 8, trip_ref.AS_TRACTS)
    for mode, T in ((trip_ref.EVEN, 5), (trip_ref.EVEN, 0), (trip_ref.AS_TRACTS, 25), (trip_ref.AS_TRACTS, 0), (2, 1)):
        with pytest.raises(dge.DgeError) as ei:
            f.slot_edges(T, mode)
        assert ei.value.code == 1
    n = C.c_int64(0)
    buf = np.zeros(1, np.int64); b32 = np.zeros(1, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert dge.lib.dge_flows_slot_edges(f._h, 8, 0, p(b32), p(buf), p(buf), p(buf), 1, C.byref(n)) == 4 and n.value == len(trip_ref.slot_edges(want, MESH.ids, 8, 0))
    assert dge.lib.dge_flows_to_host(f._h, p(b32), p(b32), p(b32), p(buf), 1, C.byref(n)) == 4 and n.value == len(want)


# ------------------------------------------------------------------------------------------ the graph
def store_of(g):
    c = g.get_csr(tables=True)
    s = g.get_source_alias()
    return [c["row_ptr"], c["nbr"], c["weight"], c["out_degree"], c["prob"], c["alias"], s["prob"], s["alias"], s["src"], np.float64(s["weight_sum"])]


@pytest.mark.parametrize("T,mode", [(8, trip_ref.AS_TRACTS), (1, trip_ref.EVEN)])
def test_the_graph_is_the_one_the_od_texts_give(dge, T, mode):
    rg = dge.Regions.from_arrays(*MESH.arrays())
    f = dge.Flows(rg); f.add_trips(*slot_trips())
    a, a_names, a_info = dge.DeviceGraph.from_flows(f, T, mode)
    b, b_names, b_info = dge.DeviceGraph.from_od(f.to_od_bytes(T, mode))
    assert a.num_vertices == b.num_vertices > 0 and a.num_edges == b.num_edges > 0
    a.build_alias(True); b.build_alias(True)
    for x, y in zip(store_of(a), store_of(b)):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes() and np.asarray(x).shape == np.asarray(y).shape
    assert a.sample_walks(512, min(T + 2, 12), seed=11).tobytes() == b.sample_walks(512, min(T + 2, 12), seed=11).tobytes()
    assert np.array_equal(a.regions(), b.regions()) and list(a_names) == list(b_names) and len(a_names) == T * len(a.regions())
    assert (a_info["bytes"], a_info["lines"], a_info["dropped"], a_info["host_values"]) == (0, 0, 0, 0) and a_info["flows"] == a_info["edges"] == b_info["edges"]
    assert {k: a_info[k] for k in ("regions", "sources", "slices")} == {k: b_info[k] for k in ("regions", "sources", "slices")}


def test_a_used_graph_is_refused_and_an_empty_table_gives_an_empty_graph(dge):
    rg = dge.Regions.from_arrays(*MESH.arrays())
    f = dge.Flows(rg); f.add_trips(*slot_trips())
    used = dge.DeviceGraph(0); used.add_edges([0], [1], [1.0])
    held = dge.Names(["a"])
    for graph, names, code, word in ((used, None, 5, "fresh"), (dge.DeviceGraph(0), held, 1, "names must be empty")):
        rc = dge.lib.dge_graph_add_flows(graph._h, f._h, 8, 1, names._h if names else None, None)
        assert rc == code and word in dge.lib.dge_last_error().decode()
    assert used.num_edges == 1 and used.num_vertices == 2 and len(used.regions()) == 0 and held.as_bytes() == [b"a"]
    g, names, info = dge.DeviceGraph.from_flows(dge.Flows(rg), 8, trip_ref.AS_TRACTS)
    e, e_names, _ = dge.DeviceGraph.from_od([b""] * 8)
    assert g.num_vertices == e.num_vertices == 0 and g.num_edges == e.num_edges == 0 and len(names) == len(e_names) == 0 and len(g.regions()) == 0 and info["edges"] == 0
