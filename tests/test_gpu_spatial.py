"""GPU: the spatial graph built on the device (csrc/spatial.hip; include/dge.h: dge_regions_centroids, dge_graph_add_spatial, dge_graph_add_spatial_points) against
the rule's pure-Python reading (tests/spatial_ref.py) and against the path it replaces: dge_graph_add_edges of all R^2 reference weights, dge_graph_keep_top_k,
dge_graph_set_sources(stream_sum=True).  Every comparison is exact equality of bits."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import spatial_ref as ref  # noqa: E402
DYADIC, ROUNDED, reverse_all, square = ref.DYADIC, ref.ROUNDED, ref.reverse_all, ref.square

pytestmark = pytest.mark.gpu
TILE = 2048          # SP_TILE of csrc/spatial.hip: the centroids of one LDS tile; the columns of a row are scanned 64 at a time


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def E_np(x):
    """spatial_ref.E over an array: the same rounded operations in the same order as numpy ufuncs (none fuses); checked against the scalar below"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        k = np.where(x < -ref.THREE_HALF_LN2, np.trunc(ref.INV_LN2 * x - 0.5), np.where(x < -ref.HALF_LN2, -1.0, 0.0))
        k = np.where(np.isfinite(k), k, 0.0)
        far = x <= -ref.THREE_HALF_LN2
        hi = np.where(far, x - k * ref.LN2_HI, np.where(k == -1.0, x + ref.LN2_HI, x))
        lo = np.where(far, k * ref.LN2_LO, np.where(k == -1.0, -ref.LN2_LO, 0.0))
        r = hi - lo
        t = r * r
        c = r - t * (ref.P1 + t * (ref.P2 + t * (ref.P3 + t * (ref.P4 + t * ref.P5))))
        y0 = 1.0 - ((r * c) / (c - 2.0) - r)
        y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi)
        ki = k.astype(np.int64)
        scaled = np.where(ki >= -1021, y * np.ldexp(1.0, np.maximum(ki, -1021)), (y * np.ldexp(1.0, np.clip(ki + 1000, -1000, 0))) * ref.TWOM1000)
        out = np.where(k == 0.0, y0, scaled)
        out = np.where(x >= -ref.TINY, 1.0 + x, out)
        return np.where(x < ref.UNDER, 0.0, out)


def weight_matrix(xy, scale):
    xy = np.asarray(xy, np.float64)
    with np.errstate(all="ignore"):
        dx = xy[:, None, 0] - xy[None, :, 0]
        dy = xy[:, None, 1] - xy[None, :, 1]
        d = np.sqrt(dx * dx + dy * dy)
        return E_np((-d) * scale)


def test_the_array_form_of_the_reference_is_the_reference():
    rng = np.random.default_rng(3)
    xs = np.concatenate([-750.0 * rng.random(4000), -np.exp(rng.uniform(math.log(1e-12), math.log(750.0), 2000)), [0.0, -0.0, -745.13, -745.14, -708.4, -709.9, -1e300, -np.inf,
                         -ref.HALF_LN2, -ref.THREE_HALF_LN2, -ref.TINY]])
    assert np.array_equal(bits(E_np(xs)), bits([ref.E(float(x)) for x in xs]))
    xy = rng.random((9, 2)) * 0.4 + np.array([-87.9, 41.6])
    xy[4] = (1e200, 0.0); xy[5] = (-1e200, 3.0)
    assert np.array_equal(bits(weight_matrix(xy, 100.0)), bits(ref.weight_matrix([tuple(p) for p in xy.tolist()], 100.0)))


def old_path(dge, W, k):
    """what a host did before: all R^2 weights through add_edges, then the prune, then the sources"""
    R = len(W)
    g = dge.DeviceGraph()
    src = np.repeat(np.arange(R, dtype=np.int32), R); dst = np.tile(np.arange(R, dtype=np.int32), R)
    g.add_edges(src, dst, np.ascontiguousarray(W, np.float64).ravel())
    g.keep_top_k(k)
    g.set_sources(np.arange(R, dtype=np.int32), stream_sum=True)
    return g


def state(g, walks=64):
    g.build_alias(exact=True)
    csr = g.get_csr()
    sa = g.get_source_alias()
    out = {name: (bits(v) if v.dtype == np.float64 else v) for name, v in csr.items()}
    out.update(src_prob=bits(sa["prob"]), src_alias=sa["alias"], src=sa["src"], weight_sum=bits([sa["weight_sum"]]))
    out["walks"] = g.sample_walks(walks, 8, 20261018)
    out["V"], out["E"] = g.num_vertices, g.num_edges
    return out


def same(a, b):
    assert a.keys() == b.keys()
    for name in a:
        assert np.array_equal(a[name], b[name]), name


def check_against_old_path(dge, ids, xy, k, scale=100.0, also_ref=False):
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    R = len(xy)
    g, names, info = dge.DeviceGraph.from_spatial((ids, xy), k=k, scale=scale)
    assert info["regions"] == R and info["edges"] == R * k and 0 < info["weights"] <= R * R and info["kernel_ms"] >= 0
    assert names.as_bytes() == [b"%d" % i for i in ids]
    W = weight_matrix(xy, scale)
    new = state(g)
    same(new, state(old_path(dge, W, k)))
    assert new["V"] == R and new["E"] == R * k and np.array_equal(new["row_ptr"], np.arange(R + 1) * k) and np.array_equal(new["src"], np.arange(R))
    csr_w = new["weight"].view(np.float64)
    assert info["zero_weights"] == int((csr_w == 0.0).sum())
    with pytest.raises(dge.DgeError) as e:                    # the pruned state: no edges after keepNearestKVertices
        g.add_edges([0], [0], [1.0])
    assert e.value.code == 5
    if also_ref:                                              # the rule itself, in plain Python
        want = ref.spatial_graph([tuple(p) for p in xy.tolist()], k, scale)
        assert new["nbr"].reshape(R, k).tolist() == want["nbr"] and np.array_equal(new["weight"], bits(np.array(want["weight"]).ravel()))
        assert np.array_equal(new["out_degree"], bits(want["out_degree"])) and new["weight_sum"][0] == bits([want["source_sum"]])[0]
    return new, info


def points(R, seed=1):
    rng = np.random.default_rng(seed + R)
    return rng.permutation(np.arange(1000, 1000 + 3 * R))[:R].astype(np.int64), rng.random((R, 2)) * np.array([0.4, 0.4]) + np.array([-87.9, 41.6])


# 63 / 64 / 65: the 64 columns a wave scans at a time; 2047 / 2048 / 2049: the LDS tile of 2048 centroids; the odd sizes leave a workgroup's four rows part empty
# k > R is DGE_ERR_TOPK and is left out here: test_k_beyond_R_is_the_references_exception
@pytest.mark.parametrize("R,k", [(R, k) for R in (1, 10, 11, 63, 64, 65, 257, 1025, TILE - 1, TILE, TILE + 1) for k in (1, 10, 32) if k <= R])
def test_the_graph_is_the_old_paths_graph(dge, R, k):
    ids, xy = points(R)
    check_against_old_path(dge, ids, xy, k, also_ref=R <= 65)


def test_k_beyond_R_is_the_references_exception(dge):
    ids, xy = points(10)
    with pytest.raises(dge.DgeError) as e:
        dge.DeviceGraph.from_spatial((ids, xy), k=11)
    assert e.value.code == 3 and "keepNearestKVertices(11)" in str(e.value)
    g, names, info = dge.DeviceGraph.from_spatial((ids[:0], xy[:0]), k=10)          # R = 0: an empty graph, not an error
    assert g.num_vertices == 0 and g.num_edges == 0 and len(names) == 0 and info["regions"] == 0 and info["edges"] == 0


def test_a_unit_lattice_where_four_neighbours_sit_at_each_distance(dge):
    ids = np.arange(13 * 11, dtype=np.int64) + 5
    xy = np.array([(x, y) for y in range(11) for x in range(13)], np.float64)
    for k, scale in ((10, 1.0), (32, 0.5)):
        new, _ = check_against_old_path(dge, ids, xy, k, scale=scale, also_ref=True)
        w = new["weight"].view(np.float64).reshape(len(ids), k)
        assert (w[:, 0] == 1.0).all() and (w[:, 1:5] == w[:, 1:2]).sum() > 3 * len(ids)       # ties are the common case: most rows hold four equal weights behind the self loop


def test_duplicate_centroids_tie_with_the_self_loop_and_the_lower_index_wins(dge):
    rng = np.random.default_rng(9)
    base = rng.random((40, 2)) * 0.3 + np.array([-87.8, 41.7])
    xy = np.concatenate([base, base, base])[rng.permutation(120)]
    ids = np.arange(120, dtype=np.int64) * 7
    new, _ = check_against_old_path(dge, ids, xy, 10, also_ref=True)
    nbr = new["nbr"].reshape(120, 10); w = new["weight"].view(np.float64).reshape(120, 10)
    assert (w[:, :3] == 1.0).all() and (w[:, 3] < 1.0).all()
    assert (np.diff(nbr[:, :3], axis=1) > 0).all() and (nbr[:, 0] != np.arange(120)).sum() >= 60      # the self loop is not always first


def find_two_distances_with_one_weight(scale):
    """d1 < d2, as the rule computes them from the points (0, 0), (a, 0), (b, 0), with E(-d1 * scale) == E(-d2 * scale) < 1: searched for, not assumed"""
    for a in (1.0e-4, 3.0e-5, 2.5e-4):
        b = a
        for _ in range(400):
            b = math.nextafter(b, math.inf)
            d1, d2 = ref.distance((0.0, 0.0), (a, 0.0)), ref.distance((0.0, 0.0), (b, 0.0))
            if d1 < d2 and ref.E((-d1) * scale) == ref.E((-d2) * scale) < 1.0:
                return a, b
    raise AssertionError("no such pair")


def test_the_order_is_by_weight_not_by_distance(dge):
    """Two candidates with d1 < d2 and equal w, the farther one at the lower index: (w descending, j ascending) keeps the farther one first.  An implementation
    that ranks by distance puts the nearer one first and fails."""
    a, b = find_two_distances_with_one_weight(100.0)
    xy = np.array([(b, 0.0), (a, 0.0), (0.0, 0.0), (0.5, 0.5), (0.7, 0.1), (-0.4, 0.3)])          # row 2: j = 0 is farther than j = 1, the weights are equal
    ids = np.array([11, 12, 13, 14, 15, 16], np.int64)
    for k in (2, 3):
        new, _ = check_against_old_path(dge, ids, xy, k, also_ref=True)
        row = new["nbr"].reshape(6, k)[2].tolist()
        assert row == [2, 0, 1][:k]                                                                 # by distance it would be [2, 1, 0]
    W = weight_matrix(xy, 100.0)
    assert W[2, 0] == W[2, 1] < 1.0 and ref.distance((0.0, 0.0), (b, 0.0)) > ref.distance((0.0, 0.0), (a, 0.0))


def test_kept_weights_that_underflow_to_zero_are_counted(dge):
    xy = np.array([(10.0 * i, 10.0 * (i % 3)) for i in range(12)])                                 # d >= 10, scale 100: E(-1000) = 0
    ids = np.arange(12, dtype=np.int64) + 100
    new, info = check_against_old_path(dge, ids, xy, 3, also_ref=True)
    assert info["zero_weights"] == 12 * 2
    assert new["nbr"].reshape(12, 3)[5].tolist() == [5, 0, 1] and new["nbr"].reshape(12, 3)[0].tolist() == [0, 1, 2]      # zeros tie: the lower index wins
    xy[:, 0] *= 0.07                                                                                # a mix: subnormal and tiny weights beside the zeros
    check_against_old_path(dge, ids, xy, 5, also_ref=True)


def test_coordinates_large_enough_that_the_squared_distance_overflows(dge):
    xy = np.array([(1e200, 0.0), (-1e200, 0.0), (0.0, 1e200), (0.0, 0.0), (1e-3, 0.0), (1e200, 1e-3), (1.7e308, 1.7e308), (-1.7e308, -1.7e308)])
    ids = np.arange(8, dtype=np.int64)
    new, info = check_against_old_path(dge, ids, xy, 3, also_ref=True)
    assert info["zero_weights"] > 0 and np.isinf(np.float64(1e200) * np.float64(1e200))
    assert new["nbr"].reshape(8, 3)[0].tolist() == [0, 5, 1] and new["nbr"].reshape(8, 3)[6].tolist() == [6, 0, 1]


# ------------------------------------------------------------------------------------------ centroids, rings to graph
def arrays(regions):
    """[rings of region 0, rings of region 1, ..] -> ring_first, vert_first, xy"""
    ring_first, vert_first, xy = [0], [0], []
    for rings in regions:
        for ring in rings:
            xy += ring
            vert_first.append(len(xy))
        ring_first.append(len(vert_first) - 1)
    return np.array(ring_first, np.int64), np.array(vert_first, np.int64), np.array(xy, np.float64).reshape(-1, 2)


def big_ring(n, cx, cy, r):
    pts = [(cx + r * math.cos(-2 * math.pi * i / n), cy + r * math.sin(-2 * math.pi * i / n)) for i in range(n)]
    return pts + [pts[0]]


def fixtures():
    regions = [r for r in DYADIC.values()] + [reverse_all(r) for r in DYADIC.values()] + [r for r in ROUNDED.values()] + [reverse_all(r) for r in ROUNDED.values()]
    regions.append([[(3.0, 1.0), (4.0, 3.0), (5.0, 1.0), (3.0, 1.0)]])                       # one ring of 4 vertices: a triangle
    regions.append([big_ring(3001, -87.7, 41.9, 0.02)])                                      # a ring of a few thousand vertices
    return regions


def test_centroids_are_the_references(dge):
    regions = fixtures()
    ids = np.arange(len(regions), dtype=np.int64) * 3 + 17
    rg = dge.Regions.from_arrays(ids, *arrays(regions))
    got = rg.centroids()
    want = np.array([ref.centroid(r) for r in regions])
    assert got.shape == (len(regions), 2) and np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(rg.centroids()), bits(want))                                   # kept with the handle
    n = len(DYADIC)
    assert np.array_equal(bits(got[:n]), bits(got[n:2 * n]))                                  # all rings reversed: the same bits where the sums are exact
    one = dge.Regions.from_arrays([5], *arrays([DYADIC["square with a hole"]]))               # R = 1
    assert np.array_equal(bits(one.centroids()), bits([ref.centroid(DYADIC["square with a hole"])]))
    assert dge.Regions.from_arrays([], *arrays([])).centroids().shape == (0, 2)


def test_a_ring_without_area_is_an_argument_error_naming_the_region(dge):
    flat = [[(0.0, 0.0), (1.0, 1.0), (2.0, 2.0), (0.0, 0.0)]]
    rg = dge.Regions.from_arrays([40, 41, 42], *arrays([DYADIC["unit square"], flat, [square(5.0, 5.0, 1.0)]]))
    for call in (rg.centroids, lambda: dge.DeviceGraph.from_spatial(rg, k=1)):
        with pytest.raises(dge.DgeError) as e:
            call()
        assert e.value.code == 1 and "region 1" in str(e.value) and "id 41" in str(e.value)


def tract_mesh(n):
    """n x n tract-sized squares, some with a hole: rings as a shapefile holds them"""
    regions = []
    for j in range(n):
        for i in range(n):
            x0, y0 = -87.9 + 0.011 * i, 41.6 + 0.013 * j
            rings = [square(x0, y0, 0.01)]
            if (i + j) % 3 == 0:
                rings.append(square(x0 + 0.002, y0 + 0.003, 0.004, cw=False))
            regions.append(rings)
    return regions


def test_rings_and_their_centroids_give_the_same_graph(dge):
    regions = tract_mesh(9)
    ids = (np.arange(81, dtype=np.int64) * 13) % 1009 + 17031000000
    rg = dge.Regions.from_arrays(ids, *arrays(regions))
    a, names_a, info_a = dge.DeviceGraph.from_spatial(rg)                                     # k = 10, scale = 100: the reference's
    b, names_b, info_b = dge.DeviceGraph.from_spatial((ids, rg.centroids()))
    assert info_a["edges"] == 810 and {k: v for k, v in info_a.items() if k != "kernel_ms"} == {k: v for k, v in info_b.items() if k != "kernel_ms"}
    assert names_a.as_bytes() == names_b.as_bytes() == [b"%d" % i for i in ids]
    sa = state(a)
    same(sa, state(b))
    same(sa, state(old_path(dge, weight_matrix(np.array([ref.centroid(r) for r in regions]), 100.0), 10)))


def test_rings_to_walk_text_and_back(dge, tmp_path):
    regions = tract_mesh(6)
    ids = np.arange(36, dtype=np.int64) + 17031010100
    rg = dge.Regions.from_arrays(ids, *arrays(regions))
    g, names, _ = dge.DeviceGraph.from_spatial(rg, k=10)
    g.build_alias(exact=True)
    corpus = g.sample_walks_device(500, 8, 7)
    walks = corpus.to_host()
    path = str(tmp_path / "spatial.seq")
    corpus.write_seq(path, names=names, position_prefix=True)
    first = open(path).readline().split()
    assert first == ["%d-%d" % (j, ids[v]) for j, v in enumerate(walks[0])]
    layered = dge.Names(["%d-%d" % (j, i) for j in range(8) for i in ids])                    # token "j-id" is vertex j*R + index of the cross-time id space
    back, _, info = dge.WalkCorpus.from_seq(path, names=layered, intern=False)
    assert info["unknown"] == 0 and np.array_equal(back.to_host(), walks + 36 * np.arange(8, dtype=np.int32)[None, :])


def test_errors_leave_the_graph_usable_and_the_names_empty(dge):
    import ctypes as C
    lib = dge.lib
    ids, xy = points(20)
    g = dge.DeviceGraph()
    names = dge.Names()

    def call(ids, xy, k=3, scale=100.0):
        ids = np.ascontiguousarray(ids, np.int64); xy = np.ascontiguousarray(xy, np.float64)
        return lib.dge_graph_add_spatial_points(g._h, ids.ctypes.data_as(C.c_void_p), xy.ctypes.data_as(C.c_void_p), len(ids), k, scale, names._h, None)

    bad = xy.copy(); bad[7, 1] = np.nan
    dup = ids.copy(); dup[3] = dup[0]
    assert call(ids, xy, k=21) == 3 and call(ids, xy, k=0) == 1 and call(ids, xy, scale=-1.0) == 1 and call(ids, bad) == 1 and call(dup, xy) == 1
    flat = dge.Regions.from_arrays([1, 2], *arrays([DYADIC["unit square"], [[(0.0, 0.0), (1.0, 1.0), (2.0, 2.0), (0.0, 0.0)]]]))
    assert lib.dge_graph_add_spatial(g._h, flat._h, 1, 100.0, names._h, None) == 1
    assert len(names) == 0 and g.num_vertices == 0 and g.num_edges == 0
    assert call(ids, xy) == 0 and len(names) == 20 and g.num_edges == 60                        # the same handles still work
    assert call(ids, xy) == 1 and "names must be empty" in lib.dge_last_error().decode()
    assert lib.dge_graph_add_spatial_points(g._h, ids.ctypes.data_as(C.c_void_p), xy.ctypes.data_as(C.c_void_p), 20, 3, 100.0, None, None) == 5      # not fresh
    same(state(g), state(old_path(dge, weight_matrix(xy, 100.0), 3)))


def test_cpp_host_constructs_the_same_graph_from_points_as_from_the_matrix(tmp_path, dge):
    import subprocess
    exe = str(tmp_path / "host_spatial_test")
    libdir = os.path.join(ROOT, "embedding_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "host_spatial_test.cpp"), "-o", exe,
                           "-L" + libdir, "-l:libdge.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "HOST SPATIAL OK" in out.stdout, out.stdout + out.stderr
    a = out.stdout.split("== matrix overload\n")[1].split("== points overload\n")
    assert a[0] == a[1].split("HOST SPATIAL OK")[0] and a[0].count("\n") == 12 + 1                # the same edgesOut, outDegree, sourceWeightSum, line for line
