"""GPU: dge_nmf_coo / dge_nmf_flows (csrc/nmf.hip) against the rule of include/dge.h as tests/nmf_ref.py reads it: W and H as bits and the counters of info,
for both updates, at the sizes where a segment sum or a blocked sum changes its shape; a larger matrix equals the host loop of
tests/native/nmf_rule_harness.cpp; two calls and a shuffled input give the same bits; errors name the right entry and leave the outputs untouched, in the order
of their kinds, a repeat across a workgroup boundary of the check and dropped entries that are none included; the flow table's slots as matrices; the features end
to end.

The 64 x 48 case holds rows and columns of exactly 0, 1, 15, 16, 17, 31, 32 and 33 entries.  A row or column of 700 entries — the hub — does not fit into a
64 x 48 matrix; it is the 40 x 720 and 720 x 40 cases."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nmf_ref as ref  # noqa: E402
import trip_ref  # noqa: E402
from nmf_harness import harness_nmf, load_harness  # noqa: E402

pytestmark = pytest.mark.gpu

UPDATES = [("divergence", ref.DIVERGENCE), ("euclidean", ref.EUCLIDEAN)]
BOUNDARIES = [0, 1, 15, 16, 17, 31, 32, 33]


def degrees_matrix(row_deg, col_deg, seed):
    """entries of a 0/1 pattern with exactly these row and column counts (the rows in descending count take the columns with the most left), integer values"""
    assert sum(row_deg) == sum(col_deg)
    left = list(col_deg)
    rows, cols = [], []
    for i in sorted(range(len(row_deg)), key=lambda i: -row_deg[i]):
        take = sorted(range(len(left)), key=lambda j: (-left[j], j))[:row_deg[i]]
        assert all(left[j] > 0 for j in take)
        for j in take:
            left[j] -= 1
            rows.append(i); cols.append(j)
    assert not any(left)
    rng = np.random.default_rng(seed)
    o = rng.permutation(len(rows))
    return np.array(rows, np.int32)[o], np.array(cols, np.int32)[o], rng.integers(1, 51, len(rows)).astype(np.float64)


def boundary_case():
    row_deg = BOUNDARIES + [5] * 56                        # 64 rows
    col_deg = BOUNDARIES + [7] * 40                        # 48 columns
    r, c, v = degrees_matrix(row_deg, col_deg, 4)
    assert np.bincount(r, minlength=64).tolist() == row_deg and np.bincount(c, minlength=48).tolist() == col_deg
    return r, c, v


def hub_case(transpose):
    """40 x 720: row 3 holds exactly 700 entries, the others a few"""
    rng = np.random.default_rng(6)
    cells = {3 * 720 + j for j in rng.permutation(720)[:700].tolist()} | {int(i) * 720 + int(j) for i, j in zip(rng.integers(4, 40, 300), rng.integers(0, 720, 300))}
    cells = rng.permutation(np.array(sorted(cells), np.int64))
    r, c = (cells // 720).astype(np.int32), (cells % 720).astype(np.int32)
    assert np.bincount(r)[3] == 700
    v = rng.integers(1, 51, len(cells)).astype(np.float64)
    return (c, r, v) if transpose else (r, c, v)


def vector_case(n, m):
    rng = np.random.default_rng(n + 2 * m)
    k = np.sort(rng.permutation(n * m)[:33])
    return (k // m).astype(np.int32), (k % m).astype(np.int32), rng.integers(1, 51, len(k)).astype(np.float64)


CASES = {
    "1x1": (lambda: (np.array([0], np.int32), np.array([0], np.int32), np.array([3.0])), (1, 1), 1, 2),
    "1x40": (lambda: vector_case(1, 40), (1, 40), 3, 2),
    "40x1": (lambda: vector_case(40, 1), (40, 1), 3, 2),
    "33x33": (lambda: ref.random_sparse(33, 33, 0.3, 2), (33, 33), 32, 2),
    "64x48 boundaries": (boundary_case, (64, 48), 10, 2),
    "40x720 hub row": (lambda: hub_case(False), (40, 720), 10, 1),
    "720x40 hub column": (lambda: hub_case(True), (720, 40), 10, 1),
    "257x513": (lambda: ref.random_sparse(257, 513, 0.03, 3), (257, 513), 10, 2),
    "300x300": (lambda: ref.random_sparse(300, 300, 0.05, 5, hub=(7, 250)), (300, 300), 10, 3),
}
_refs = {}


def reference(name, update):
    """computed once per case and update, shared, never changed"""
    if (name, update) not in _refs:
        make, shape, rank, iters = CASES[name]
        r, c, v = make()
        _refs[(name, update)] = (r, c, v, ref.nmf(r, c, v, shape, rank=rank, max_iter=iters, update=update, seed=12345, exact=name == "1x1"))
    return _refs[(name, update)]


def same(got, want):
    W, H, info = got
    assert ref.same_bits(W, want["W"]), "W differs in %d of %d values" % ((W.view(np.uint64) != want["W"].view(np.uint64)).sum(), W.size)
    assert ref.same_bits(H, want["H"]), "H differs in %d of %d values" % ((H.view(np.uint64) != want["H"].view(np.uint64)).sum(), H.size)
    for f in ("rows", "cols", "entries", "zeros", "iterations", "vmax"):
        assert info[f] == want[f], (f, info[f], want[f])


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("uname,update", UPDATES)
def test_factors_equal_the_rule_as_bits(dge, name, uname, update):
    import embedding_amd.evaluate as ev
    _, shape, rank, iters = CASES[name]
    r, c, v, want = reference(name, update)
    got = ev.nmf_gpu(r, c, v, shape, rank=rank, max_iter=iters, update=uname, seed=12345)
    same(got, want)
    assert got[2]["kernel_ms"] > 0
    # the objective: outside the exact rule, within the derived bound of the reference evaluated on the returned factors
    obj, A = ref.objective(want["E"], got[0], got[1], update)
    print("%s %s: objective %.17g, reference %.17g, bound %.3g" % (name, uname, got[2]["objective"], obj, ref.objective_bound(want["E"], rank, A)))
    assert abs(got[2]["objective"] - obj) <= ref.objective_bound(want["E"], rank, A)
    if name == "64x48 boundaries":                           # an empty row and an empty column end at EPS exactly
        assert (got[0][0] == ref.EPS).all() and (got[1][:, 0] == ref.EPS).all() and (got[0][1:] > ref.EPS).any()


@pytest.mark.parametrize("uname,update", UPDATES)
def test_a_larger_matrix_equals_the_host_loop(dge, tmp_path, uname, update):
    import embedding_amd.evaluate as ev
    H = load_harness(str(tmp_path / "libnmf_rule_harness.so"))
    r, c, v = ref.random_sparse(2000, 2000, 0.0253, 21, hub=(11, 1500))
    assert 0.98e5 < len(v) < 1.1e5
    want = harness_nmf(H, r, c, v, (2000, 2000), rank=10, max_iter=30, update=update, seed=1)
    same(ev.nmf_gpu(r, c, v, (2000, 2000), rank=10, max_iter=30, update=uname, seed=1), want)


@pytest.mark.parametrize("uname,update", UPDATES)
def test_values_that_put_the_factors_on_the_floor(dge, uname, update):
    import embedding_amd.evaluate as ev
    r, c, v = ref.random_sparse(20, 30, 0.2, 8)
    v = v * 1e-300
    want = ref.nmf(r, c, v, (20, 30), rank=4, max_iter=2, update=update, seed=3, exact=True)
    W0, H0 = ref.init_factors(20, 30, 4, 3, want["vmax"])
    assert (W0 == ref.EPS).all() and (H0 == ref.EPS).all() and want["vmax"] == v.max()
    same(ev.nmf_gpu(r, c, v, (20, 30), rank=4, max_iter=2, update=uname, seed=3), want)


def test_two_calls_a_shuffled_input_zeros_and_a_supplied_init(dge):
    import embedding_amd.evaluate as ev
    r, c, v, want = reference("257x513", ref.DIVERGENCE)
    kw = dict(rank=10, max_iter=2, update="divergence", seed=12345)
    a = ev.nmf_gpu(r, c, v, (257, 513), **kw)
    b = ev.nmf_gpu(r, c, v, (257, 513), **kw)
    assert ref.same_bits(a[0], b[0]) and ref.same_bits(a[1], b[1]) and a[2]["objective"] == b[2]["objective"]
    o = np.random.default_rng(1).permutation(len(v))
    same(ev.nmf_gpu(r[o], c[o], v[o], (257, 513), **kw), want)
    # zeros are dropped and counted, wherever they stand — on a cell another entry holds too
    r2 = np.concatenate([r[:5], r, [0, 256]]).astype(np.int32); c2 = np.concatenate([c[:5], c, [0, 512]]).astype(np.int32); v2 = np.concatenate([np.zeros(5), v, [0.0, -0.0]])
    got = ev.nmf_gpu(r2, c2, v2, (257, 513), **kw)
    same(got, dict(want, zeros=7))
    # the generated initial factors fed back
    same(ev.nmf_gpu(r, c, v, (257, 513), init=ref.init_factors(257, 513, 10, 12345, want["vmax"]), **dict(kw, seed=99)), want)
    other = ev.nmf_gpu(r, c, v, (257, 513), **dict(kw, seed=99))
    assert not ref.same_bits(other[0], want["W"])


def test_errors_name_the_entry_and_leave_the_outputs_untouched(dge):
    from embedding_amd._native import NmfCfg, NmfInfo
    lib = dge.lib
    r, c, v = ref.random_sparse(50, 40, 0.2, 9)
    n_e = len(v)
    W = np.full((50, 33), 9.0); H = np.full((33, 40), 7.0); info = NmfInfo(); info.rows = -5
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731

    def call(r=r, c=c, v=v, rank=4):
        cfg = NmfCfg(rank, 2, 0, 0, 1)
        r = np.ascontiguousarray(r, np.int32); c = np.ascontiguousarray(c, np.int32); v = np.ascontiguousarray(v, np.float64)
        rc = lib.dge_nmf_coo(0, p(r), p(c), p(v), len(v), 50, 40, C.byref(cfg), None, None, p(W), p(H), C.byref(info))
        return rc, (lib.dge_last_error() or b"").decode()

    def poke(values):
        w = v.copy()
        for at, x in values.items():
            w[at] = x
        return w

    dup_r = np.concatenate([r, r[[30, 10, 30]]]); dup_c = np.concatenate([c, c[[30, 10, 30]]]); dup_v = np.concatenate([v, [1.0, 2.0, 3.0]])
    first = np.concatenate([r[[10]], r]), np.concatenate([c[[10]], c]), np.concatenate([[4.0], v])      # the copy in front: the original, at 11, is the second occurrence
    for what, kw, words in (("negative", dict(v=poke({17: -1.0, 40: -1.0})), ("entry 17 ", "negative")),
                            ("NaN", dict(v=poke({23: np.nan, 90: np.nan, 4: -1.0})), ("entry 23 ", "not finite")),
                            ("infinite after a negative", dict(v=poke({5: -2.0, 60: np.inf})), ("entry 60 ", "not finite")),
                            ("duplicate", dict(r=dup_r, c=dup_c, v=dup_v), ("entry %d " % n_e, "repeats")),
                            ("duplicate in front", dict(r=first[0], c=first[1], v=first[2]), ("entry 11 ", "repeats")),
                            ("outside", dict(c=np.where(np.arange(n_e) == 8, 40, c)), ("entry 8 ", "outside")),
                            ("rank 33", dict(rank=33), ("rank = 33",)),
                            ("all zero", dict(v=np.zeros(n_e)), ("zero",))):
        rc, msg = call(**kw)
        assert rc == 1 and "dge_nmf_coo" in msg, (what, rc, msg)
        for w in words:
            assert w in msg, (what, msg)
        assert (W == 9.0).all() and (H == 7.0).all() and info.rows == -5, what
    assert call()[0] == 0 and (W.ravel()[:200] != 9.0).all() and info.rows == 50 and info.entries == n_e


def _error_call(dge):
    """dge_nmf_coo on a 50 x 40 matrix with sentinel-filled outputs: call(r, c, v) -> the message; asserts the error return and the untouched outputs"""
    from embedding_amd._native import NmfCfg, NmfInfo
    W = np.full((50, 4), 9.0); H = np.full((4, 40), 7.0); info = NmfInfo(); info.rows = -5
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731

    def call(r, c, v):
        cfg = NmfCfg(4, 2, 0, 0, 1)
        r = np.ascontiguousarray(r, np.int32); c = np.ascontiguousarray(c, np.int32); v = np.ascontiguousarray(v, np.float64)
        rc = dge.lib.dge_nmf_coo(0, p(r), p(c), p(v), len(v), 50, 40, C.byref(cfg), None, None, p(W), p(H), C.byref(info))
        msg = (dge.lib.dge_last_error() or b"").decode()
        assert rc == 1 and "dge_nmf_coo" in msg, (rc, msg)
        assert (W == 9.0).all() and (H == 7.0).all() and info.rows == -5, msg
        return msg
    return call


def test_faults_of_every_kind_at_once_are_reported_in_the_order_of_the_kinds(dge):
    """one input holds a negative value (entry 20), a NaN (30), a repeat (40 repeats 3) and a column outside (60): the kinds are looked for in the order outside,
    not finite, negative, repeat, whatever their indices — the least index over all kinds, 20, comes third"""
    call = _error_call(dge)
    r, c, v = ref.random_sparse(50, 40, 0.2, 9)
    assert len(v) > 61
    r = r.copy(); c = c.copy(); v = v.copy()
    good_c60 = c[60]
    r[40], c[40] = r[3], c[3]
    v[20] = -1.0; v[30] = np.nan; c[60] = 40
    msg = call(r, c, v)
    assert "entry 60 " in msg and "outside" in msg, msg
    c[60] = good_c60
    msg = call(r, c, v)
    assert "entry 30 " in msg and "not finite" in msg, msg
    v[30] = 2.0
    msg = call(r, c, v)
    assert "entry 20 " in msg and "negative" in msg, msg
    v[20] = 2.0
    msg = call(r, c, v)
    assert "entry 40 " in msg and "repeats" in msg, msg


def distinct_cells(count, seed):
    """count entries of a 50 x 40 matrix on distinct cells, in no order, integer values"""
    rng = np.random.default_rng(seed)
    k = rng.permutation(50 * 40)[:count]
    return (k // 40).astype(np.int32), (k % 40).astype(np.int32), rng.integers(1, 51, count).astype(np.float64)


def test_a_repeat_whose_two_entries_sort_into_different_workgroups_of_the_check(dge):
    """258 kept entries; the last repeats the cell of the entry that sorts to position 255 of the others, so the pair sits at sorted positions 255 and 256"""
    call = _error_call(dge)
    r, c, v = distinct_cells(258, 11)
    at = int(np.argsort(r[:257].astype(np.int64) * 40 + c[:257])[255])
    r[257], c[257] = r[at], c[at]
    msg = call(r, c, v)
    assert "entry 257 " in msg and "repeats" in msg, msg
    front = lambda a: np.concatenate([a[[257]], a[:257]])      # noqa: E731    the copy in front: the original, shifted by one, is the second occurrence
    msg = call(front(r), front(c), front(v))
    assert ("entry %d " % (at + 1)) in msg and "repeats" in msg, msg


def test_dropped_entries_are_no_repeats(dge):
    """three zeros on one cell that a kept entry holds and two -0.0 on another, spread through the input: counted, and the factors are those without them"""
    import embedding_amd.evaluate as ev
    r, c, v = distinct_cells(258, 11)
    kw = dict(rank=4, max_iter=2, update="divergence", seed=5)
    W, H, info = ev.nmf_gpu(r, c, v, (50, 40), **kw)
    assert info["entries"] == 258 and info["zeros"] == 0
    r2, c2, v2 = r.tolist(), c.tolist(), v.tolist()
    for at, cell, zero in ((258, 7, 0.0), (200, 100, -0.0), (129, 7, 0.0), (40, 100, -0.0), (0, 7, 0.0)):      # descending places: each insert leaves the earlier ones where they are
        r2.insert(at, int(r[cell])); c2.insert(at, int(c[cell])); v2.insert(at, zero)
    W2, H2, info2 = ev.nmf_gpu(np.array(r2, np.int32), np.array(c2, np.int32), np.array(v2), (50, 40), **kw)
    assert info2["zeros"] == 5 and info2["entries"] == 258
    assert ref.same_bits(W2, W) and ref.same_bits(H2, H)


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
def test_flows_slots_as_matrices(dge, T, slot):
    import embedding_amd.evaluate as ev
    rg, f = flows_fixture(dge)
    R = rg.info()["regions"]
    index_of = {int(i): k for k, i in enumerate(rg.ids)}
    sl, src, dst, w = f.slot_edges(T, f.EVEN)
    here = sl == slot
    assert here.sum() > 100
    rows = np.array([index_of[int(i)] for i in src[here]], np.int32); cols = np.array([index_of[int(i)] for i in dst[here]], np.int32); vals = w[here].astype(np.float64)
    for uname in ("divergence", "euclidean"):
        kw = dict(rank=5, max_iter=3, update=uname, seed=7)
        W, H, ids, info = f.nmf(slot, T=T, **kw)
        want = ev.nmf_gpu(rows, cols, vals, (R, R), **kw)
        assert ref.same_bits(W, want[0]) and ref.same_bits(H, want[1]) and np.array_equal(ids, rg.ids) and np.array_equal(info["region_index"], np.arange(R))
        assert {k: info[k] for k in ("rows", "cols", "entries", "zeros", "vmax", "objective")} == {k: want[2][k] for k in ("rows", "cols", "entries", "zeros", "vmax", "objective")}
        ref_res = ref.nmf(rows, cols, vals, (R, R), rank=5, max_iter=3, update=dict(UPDATES)[uname], seed=7)
        assert ref.same_bits(W, ref_res["W"]) and ref.same_bits(H, ref_res["H"])
        # a mask: the call on the compacted sub-matrix
        select = np.random.default_rng(T).random(R) < 0.6
        compact = np.cumsum(select) - 1
        keep = select[rows] & select[cols]
        Wm, Hm, idm, infm = f.nmf(slot, T=T, select=select, **kw)
        wantm = ev.nmf_gpu(compact[rows[keep]], compact[cols[keep]], vals[keep], (int(select.sum()), int(select.sum())), **kw)
        assert Wm.shape == (select.sum(), 5) and ref.same_bits(Wm, wantm[0]) and ref.same_bits(Hm, wantm[1])
        assert np.array_equal(idm, rg.ids[select]) and np.array_equal(infm["region_index"], np.nonzero(select)[0]) and infm["entries"] == keep.sum()
    with pytest.raises(dge.DgeError, match="no region is selected"):
        f.nmf(slot, T=T, select=np.zeros(R, bool))
    with pytest.raises(dge.DgeError, match="slot = %d" % T):
        f.nmf(T, T=T)
    lonely = np.zeros(R, bool); lonely[int(np.argmin(np.bincount(np.concatenate([rows, cols]), minlength=R)))] = True
    if not ((rows == np.nonzero(lonely)[0][0]) & (cols == np.nonzero(lonely)[0][0])).any():
        with pytest.raises(dge.DgeError, match="no entry"):
            f.nmf(slot, T=T, select=lonely)


def test_features_to_ndcg_end_to_end(dge):
    import embedding_amd.evaluate as ev
    r, c, v, want = reference("300x300", ref.DIVERGENCE)
    W, H, _ = ev.nmf_gpu(r, c, v, (300, 300), rank=10, max_iter=3, update="divergence", seed=12345)
    gnd = dge.Vectors.from_host(np.random.default_rng(4).standard_normal((300, 6)).astype(np.float32))
    feats = ev.nmf_features(W, H)
    assert feats.shape == (300, 20)
    got = dge.Vectors.from_host(feats).ndcg_against(gnd, 10)[0]
    expect = dge.Vectors.from_host(ev.nmf_features(want["W"], want["H"])).ndcg_against(gnd, 10)[0]
    assert got == expect and np.isfinite(got) and got <= 1.0
