"""GPU: dge_tree_fit* / dge_tree_predict_vectors / dge_tree_cv* (csrc/tree.hip) against the rule of include/dge.h as tests/tree_ref.py reads it.  Every
comparison is EQUALITY: the five arrays of a tree (thresholds as bits) and the per-fold counts.  The shapes are the smallest at which the kernels can go wrong:
one row, one wave, one block and their neighbours, more than one block, lattice values where the tie rule decides most nodes and float32 normals where it
rarely does, segments of one and two rows next to long ones, every limit biting, and the trees of a cross-validation together and one after another."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tree_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

ARRAYS = ("feature", "left", "count", "pos")


def same_tree(got, want):
    for a in ARRAYS:
        assert got[a].dtype == want[a].dtype and np.array_equal(got[a], want[a]), (a, got[a][:12], want[a][:12])
    assert np.array_equal(np.asarray(got["threshold"], np.float64).view(np.uint64), np.asarray(want["threshold"], np.float64).view(np.uint64))


def fit(dge, X, y, present=None, select=None, **limits):
    v = dge.Vectors.from_host(X, present=present)
    tree, info = v.tree_fit(y, select=select, **limits)
    return tree, info, v


def check(dge, X, y, present=None, select=None, **limits):
    want = ref.tree_fit(X, y, present=present, select=select, **limits)
    tree, info, v = fit(dge, X, y, present=present, select=select, **limits)
    same_tree(tree, want)
    assert info["n_nodes"] == want["n_nodes"] and info["depth"] == want["depth"] and info["rows"] == want["rows"] and info["trees"] == 1 and info["batches"] == 1
    assert info["kernel_ms"] > 0.0
    # the tree sends its own training rows where training sent them
    votes = v.tree_predict(tree)
    assert np.array_equal(votes, ref.tree_predict(want, X, present=present))
    return tree, info, want


@functools.lru_cache(maxsize=None)
def data(kind, n, dim, seed=0):
    rng = np.random.default_rng(1000 * n + 10 * dim + seed)
    if kind == "lattice":
        X = rng.integers(0, 4, (n, dim)).astype(np.float32)
        y = rng.integers(0, 2, n).astype(np.uint8)
    else:
        X = rng.standard_normal((n, dim)).astype(np.float32)
        y = ((X[:, 0] + 0.5 * X[:, dim - 1] + rng.standard_normal(n)) > 0).astype(np.uint8)
    X.setflags(write=False); y.setflags(write=False)
    return X, y


SIZES = [1, 2, 3, 63, 64, 65, 255, 257, 1025]
DIMS = [1, 3, 20]


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("n", SIZES)
def test_lattice_values_where_the_tie_rule_decides(dge, n, dim):
    X, y = data("lattice", n, dim)
    check(dge, X, y)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("n", SIZES)
def test_float32_normals(dge, n, dim):
    X, y = data("normal", n, dim)
    check(dge, X, y)


def test_more_rows_than_any_chunk_with_a_depth_limit(dge):
    X, y = data("normal", 4099, 4)
    _, info, want = check(dge, X, y, max_depth=6)
    assert info["depth"] == 6 and info["levels"] == 6


def test_all_labels_equal_and_a_single_row_of_the_other_class(dge):
    X, _ = data("normal", 130, 3)
    for lab in (0, 1):
        tree, _, _ = check(dge, X, np.full(130, lab, np.uint8))
        assert len(tree["feature"]) == 1 and tree["count"][0] == 130 and tree["pos"][0] == 130 * lab
        y = np.full(130, lab, np.uint8); y[77] = 1 - lab
        tree, _, _ = check(dge, X, y)
        assert len(tree["feature"]) >= 3


def test_constant_columns(dge):
    rng = np.random.default_rng(3)
    y = rng.integers(0, 2, 100).astype(np.uint8)
    X = np.tile(np.array([[1.5, -2.0, 0.0, 7.0]], np.float32), (100, 1))
    tree, _, _ = check(dge, X, y)                                # no candidate anywhere: the root is an impure leaf
    assert len(tree["feature"]) == 1
    X2 = X.copy(); X2[:, 3] = rng.integers(0, 5, 100)
    tree, _, _ = check(dge, X2, y)                               # the one column that varies is the last
    assert set(tree["feature"].tolist()) == {-1, 3}


def test_identical_rows_with_opposite_labels(dge):
    X = np.array([[1, 5], [1, 5]], np.float32)
    tree, _, v = fit(dge, X, [0, 1])
    same_tree(tree, ref.tree_fit(X, [0, 1]))
    assert len(tree["feature"]) == 1 and tree["count"][0] == 2 and tree["pos"][0] == 1 and v.tree_predict(tree).tolist() == [0, 0]      # the tie votes 0
    X3 = np.array([[1, 5], [1, 5], [2, 5], [1, 5]], np.float32)
    tree, _, _ = check(dge, X3, [0, 1, 1, 1])                    # 2 of 3 in the impure leaf: it votes 1
    assert tree["feature"].tolist() == [0, -1, -1]


def test_a_column_of_signed_zeros(dge):
    rng = np.random.default_rng(4)
    X = np.zeros((90, 3), np.float32)
    X[:, 0] = np.where(rng.random(90) < 0.5, np.float32(-0.0), np.float32(0.0))
    X[:, 1] = np.where(rng.random(90) < 0.5, np.float32(-0.0), np.float32(1e-45))
    X[:, 2] = np.where(rng.random(90) < 0.5, np.float32(0.0), np.float32(-1e-45))
    y = (np.signbit(X[:, 0]) ^ (rng.random(90) < 0.2)).astype(np.uint8)      # the sign of a zero says the label — and must not be seen
    tree, _, _ = check(dge, X, y)
    assert 0 not in tree["feature"].tolist()
    tree, _, _ = check(dge, X[:, :1], y)
    assert len(tree["feature"]) == 1


def test_a_chain(dge):
    """values 0 .. 199 in one column, labels alternating: every split peels rows off, the tree is deep, segments of one and two rows sit next to long ones"""
    X = np.arange(200, dtype=np.float32).reshape(200, 1)
    y = (np.arange(200) % 2).astype(np.uint8)
    tree, info, _ = check(dge, X, y)
    assert len(tree["feature"]) == 399 and info["depth"] >= 8
    X2 = np.concatenate([X, np.zeros((200, 1), np.float32), X[::-1]], axis=1)
    check(dge, X2, y)


@pytest.mark.parametrize("limits", [dict(max_depth=1), dict(max_depth=3), dict(min_samples_split=20), dict(min_samples_split=258), dict(min_samples_leaf=7),
                                    dict(min_samples_leaf=128), dict(min_samples_leaf=129), dict(max_depth=4, min_samples_split=9, min_samples_leaf=4)])
def test_the_limits_bite(dge, limits):
    X, y = data("lattice", 257, 3)
    tree, info, _ = check(dge, X, y, **limits)
    free = ref.tree_fit(X, y)
    assert len(tree["feature"]) < free["n_nodes"]
    if "max_depth" in limits:
        assert 1 <= info["depth"] <= limits["max_depth"]
    if "min_samples_leaf" in limits:
        assert tree["count"][tree["feature"] < 0].min() >= limits["min_samples_leaf"] or len(tree["feature"]) == 1
    Xn, yn = data("normal", 257, 3)
    check(dge, Xn, yn, **limits)


def test_absent_rows_and_a_select_mask(dge):
    rng = np.random.default_rng(5)
    X, y = (a.copy() for a in data("normal", 300, 5))
    present = rng.random(300) < 0.8
    select = rng.random(300) < 0.7
    X[~present] = np.nan                                          # never read
    X[present & ~select] = np.inf
    y[~(present & select)] = 9
    tree, info, _ = check(dge, X, y, present=present, select=select)
    take = present & select
    assert info["rows"] == take.sum()
    compact, _, _ = fit(dge, X[take], y[take])
    same_tree(tree, compact)
    only_present, _, _ = check(dge, np.where(np.isinf(X), np.float32(1.0), X), np.where(present, np.minimum(y, 1), 9).astype(np.uint8), present=present)
    assert only_present["count"][0] == present.sum()


def test_a_value_that_is_not_finite(dge):
    X, y = (a.copy() for a in data("normal", 100, 4))
    for bad in (np.nan, np.inf, -np.inf):
        Xb = X.copy(); Xb[40, 3] = bad; Xb[41, 0] = bad; Xb[40, 1] = bad
        with pytest.raises(dge.DgeError) as ei:
            fit(dge, Xb, y)
        assert ei.value.code == 1 and "row 40, column 1" in str(ei.value) and "not finite" in str(ei.value)
        select = np.ones(100, bool); select[[40, 41]] = False
        with pytest.raises(dge.DgeError) as ei:
            fit(dge, Xb, y, select=np.where(np.arange(100) == 40, False, True))
        assert "row 41, column 0" in str(ei.value)
        tree, _, _ = fit(dge, Xb, y, select=select)               # the same values in rows that are not used
        same_tree(tree, ref.tree_fit(X, y, select=select))
    with pytest.raises(dge.DgeError) as ei:
        fit(dge, X, np.where(np.arange(100) == 7, 2, y))
    assert ei.value.code == 1 and "row 7" in str(ei.value)


def test_the_order_of_the_rows_does_not_matter_and_two_calls_agree(dge):
    for kind, n, dim in (("lattice", 257, 3), ("normal", 255, 20), ("lattice", 65, 20)):
        X, y = data(kind, n, dim)
        a, _, _ = fit(dge, X, y)
        b, _, _ = fit(dge, X, y)
        same_tree(a, b)
        for seed in (1, 2):
            perm = np.random.default_rng(seed).permutation(n)
            c, _, _ = fit(dge, X[perm], y[perm])
            same_tree(a, c)
    X, y = data("lattice", 257, 3)
    import embedding_amd.evaluate as ev
    t, info = ev.tree_fit_gpu(X, y)                               # the host-rows entry
    same_tree(t, fit(dge, X, y)[0])


def test_a_capacity_that_is_too_small_is_reported_with_the_size(dge):
    import ctypes as C
    from embedding_amd._native import TreeCfg, TreeInfo
    X, y = data("lattice", 65, 3)
    want = ref.tree_fit(X, y)
    m = want["n_nodes"]
    assert m > 3
    for cap in (m - 1, m):
        feature = np.full(m, -9, np.int32); threshold = np.zeros(m); left = np.zeros(m, np.int32); count = np.zeros(m, np.int64); pos = np.zeros(m, np.int64)
        info = TreeInfo(); cfg = TreeCfg(0, 2, 1, 0)
        p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        rc = dge.lib.dge_tree_fit(0, p(np.ascontiguousarray(X)), 65, 3, p(np.ascontiguousarray(y)), None, C.byref(cfg), cap, p(feature), p(threshold), p(left), p(count), p(pos),
                                  C.byref(info))
        assert info.n_nodes == m
        if cap < m:
            assert rc == 4 and (feature == -9).all()
        else:
            assert rc == 0 and np.array_equal(feature, want["feature"])


# ---------------------------------------------------------------------------------------------- cross-validation
def folds_of(n, F, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, F, n).astype(np.int32)


@functools.lru_cache(maxsize=None)
def cv_want(kind, n, dim, F):
    X, y = data(kind, n, dim)
    return ref.tree_cv(X, y, folds_of(n, F, n + F), F)


def same_cv(got, want):
    for a in ("correct", "tested", "n_nodes", "depth"):
        assert np.array_equal(got[a], want[a]), (a, got[a], want[a])
    assert np.array_equal(got["scores"].view(np.uint64), want["scores"].view(np.uint64))
    assert np.float64(got["mean"]).view(np.uint64) == np.float64(want["mean"]).view(np.uint64)


@pytest.mark.parametrize("n", [65, 257])
@pytest.mark.parametrize("F", [2, 3, 10])
def test_cross_validation(dge, F, n):
    for kind in ("lattice", "normal"):
        X, y = data(kind, n, 3)
        fold = folds_of(n, F, n + F)
        want = cv_want(kind, n, 3, F)
        v = dge.Vectors.from_host(X)
        got = v.tree_cv(y, fold, F)
        same_cv(got, want)
        assert got["info"]["trees"] == F and got["info"]["batches"] == 1 and got["info"]["rows"] == n and got["info"]["n_nodes"] == want["n_nodes"].sum()
        # ... equal to F separate fits and predictions on the device
        for t in range(F):
            tree, info = v.tree_fit(y, select=fold != t)
            votes = v.tree_predict(tree)
            assert int((votes[fold == t] == y[fold == t]).sum()) == got["correct"][t] and len(tree["feature"]) == got["n_nodes"][t] and info["depth"] == got["depth"][t]
        # ... and the trees one after another, and in batches the last of which is smaller, give the same counts
        for batch in (1, 3):
            with dge.tuning(tree_batch=batch):
                seq = v.tree_cv(y, fold, F)
            same_cv(seq, want)
            assert seq["info"]["batches"] == -(-F // batch)


def test_cross_validation_edge_folds(dge):
    import embedding_amd.evaluate as ev
    X, y = data("normal", 65, 3)
    fold = folds_of(65, 3, 9)
    # a fold nobody is in: its tree trains on every row and tests none: 0 of 0, NaN, left out of the mean
    f4 = np.where(fold == 2, 3, fold).astype(np.int32)
    got = dge.Vectors.from_host(X).tree_cv(y, f4, 4)
    want = ref.tree_cv(X, y, f4, 4)
    same_cv(got, want)
    assert got["tested"][2] == 0 and got["correct"][2] == 0 and np.isnan(got["scores"][2]) and not np.isnan(got["mean"])
    # a fold everybody is in: no training rows
    with pytest.raises(dge.DgeError) as ei:
        dge.Vectors.from_host(X).tree_cv(y, np.full(65, 1, np.int32), 3)
    assert ei.value.code == 1 and "fold 1 has no training rows" in str(ei.value)
    # rows with fold -1 are out, whatever they hold; absent rows likewise
    Xb = X.copy(); yb = y.copy()
    out = np.arange(65) % 5 == 0
    fo = np.where(out, -1, fold).astype(np.int32)
    Xb[out] = np.nan; yb[out] = 7
    got = ev.tree_cv_gpu(Xb, yb, 3, fold=fo)
    same_cv(got, ref.tree_cv(X[~out], y[~out], fold[~out], 3))
    assert got["info"]["rows"] == (~out).sum()
    got2 = dge.Vectors.from_host(Xb, present=~out).tree_cv(yb, fold, 3)
    same_cv(got2, got)
    with pytest.raises(dge.DgeError) as ei:
        ev.tree_cv_gpu(Xb, y, 3, fold=fold)
    assert "not finite" in str(ei.value) and "row 0, column 0" in str(ei.value)


# ---------------------------------------------------------------------------------------------- prediction
def test_prediction_at_between_and_outside(dge):
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2.0))
    X = np.array([[0.0, one], [1.0, one], [3.0, up], [4.0, up]], np.float32)
    y = [0, 1, 1, 0]
    tree, _, _ = check(dge, X, y)
    m = tree["threshold"][tree["feature"] >= 0]
    probe = [[-1e30, 0], [0.0, 0], [0.5, 0], [np.nextafter(np.float32(0.5), one), 0], [1.0, 0], [2.0, 0], [np.nextafter(np.float32(2.0), np.float32(3.0)), 0], [3.5, 0], [3.4e38, 0]]
    for thr in m:                                                 # every threshold, its float32 neighbours on both sides
        t32 = np.float32(thr)
        probe += [[t32, t32], [np.nextafter(t32, np.float32(np.inf)), t32], [np.nextafter(t32, np.float32(-np.inf)), t32]]
    P = np.array(probe, np.float32)
    want = ref.tree_fit(X, y)
    got = dge.Vectors.from_host(P).tree_predict(tree)
    assert np.array_equal(got, ref.tree_predict(want, P))
    # a and b one float32 step apart: m lies between them and is no float32; a goes left, b goes right
    Xs = np.array([[one], [one], [up], [up]], np.float32)
    tree, _, _ = check(dge, Xs, [0, 0, 1, 1])
    assert float(one) < tree["threshold"][0] < float(up) and tree["threshold"][0] == (float(one) + float(up)) * 0.5
    assert dge.Vectors.from_host(Xs).tree_predict(tree).tolist() == [0, 0, 1, 1]
    pres = np.array([True, False, True, False])
    assert dge.Vectors.from_host(Xs, present=pres).tree_predict(tree).tolist() == [0, 255, 1, 255]


def test_a_malformed_tree_is_refused(dge):
    X, y = data("lattice", 65, 3)
    v = dge.Vectors.from_host(X)
    tree, _ = v.tree_fit(y)
    m = len(tree["feature"])
    inner = int(np.flatnonzero(tree["feature"] >= 0)[-1])

    def broken(**kw):
        t = {k: a.copy() for k, a in tree.items()}
        for k, (i, val) in kw.items():
            t[k][i] = val
        return t

    for what, t in (("child past the end", broken(left=(inner, m - 1))), ("child far past the end", broken(left=(inner, 2**31 - 2))), ("child is the node", broken(left=(inner, inner))),
                    ("child before the node", broken(left=(inner, 0))), ("negative child", broken(left=(0, -1))), ("column past the rows", broken(feature=(0, 3))),
                    ("column far past the rows", broken(feature=(0, 2**31 - 1))), ("negative column", broken(feature=(0, -2)))):
        with pytest.raises(dge.DgeError) as ei:
            v.tree_predict(t)
        assert ei.value.code == 1 and "node" in str(ei.value), what
    with pytest.raises(dge.DgeError):
        v.tree_predict({k: a[:0] for k, a in tree.items()})
    assert np.array_equal(v.tree_predict(tree), ref.tree_predict(ref.tree_fit(X, y), X))          # the tree itself is still fine


# ---------------------------------------------------------------------------------------------- the reference's shape, end to end
def test_end_to_end_in_the_references_shape(dge):
    """77 regions x 8 columns, labels by median_labels of generated POI counts, folds by stratified_folds, cv = 10: the mean accuracy is the reference reading's
    mean as a binary64"""
    import embedding_amd.evaluate as ev
    rng = np.random.default_rng(77)
    X = rng.standard_normal((77, 8)).astype(np.float32)
    counts = np.maximum(0, np.rint(3 + 2 * X[:, 0] + X[:, 5] + rng.standard_normal(77))).astype(np.int64)
    y, keep = ev.median_labels(counts)
    assert keep and 0 < y.sum() < 77
    got = ev.tree_cv_gpu(X, y, n_folds=10)
    fold = ev.stratified_folds(y, 10)
    assert np.array_equal(fold, ref.stratified_folds(y, 10))
    want = ref.tree_cv(X, y, fold, 10)
    same_cv(got, want)
    assert got["mean"] == want["scores"].mean() and got["tested"].sum() == 77 and 0.5 < got["mean"] <= 1.0
