"""The shared intake of k-means, the tree, ridge and the SVM on the device (csrc/used_rows.h, the scan of csrc/dge_device.h) through the public entries: the
least used row — for the SVM and the tree, row and column — that holds a value that is not finite is what every estimator reports, in the table's own row
numbers; rows that are absent or left out may hold anything; a refusal has code 1 and writes nothing; the scan reaches the elements behind its grid; k-means'
scale comes from the greatest |x| wherever it sits."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_ref as kref  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS, DIM = 300, 5
ABSENT = [2, 50, 90, 130, 170, 210, 250]                              # 7 rows
LEFT_OUT = [5, 20, 40, 60, 80, 100, 120, 140, 160, 180, 200]          # 11 more, by select or by fold -1
D, C_ROW, B, A = 2, 5, 9, 33                                          # absent < left out < used < used
SCAN_ELEMS = 4096 * 256                                               # the scan's grid: what lies behind is reached in its stride loop only


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def small_table():
    rng = np.random.default_rng(11)
    X = rng.standard_normal((ROWS, DIM)).astype(np.float32)
    y = (X[:, 0] + 0.5 * X[:, 1] > 0).astype(np.uint8)
    t = (X @ np.arange(1, DIM + 1) + 40.0 + rng.standard_normal(ROWS)).astype(np.float64)
    present = np.ones(ROWS, bool); present[ABSENT] = False
    select = np.ones(ROWS, np.uint8); select[LEFT_OUT] = 0
    fold = (np.arange(ROWS) % 3).astype(np.int32); fold[LEFT_OUT] = -1
    return X, y, t, present, select, fold


def calls(dge, X, y, t, present, select, fold):
    """name -> (what the refusal has to say, a call of the entry on sentinel outputs -> (code, message, the outputs))"""
    from embedding_amd._native import KmeansCfg, KmeansInfo, RidgeInfo, SvmCfg, SvmInfo, TreeCfg, TreeInfo
    lib = dge.lib
    v = dge.Vectors.from_host(X, present=present)
    Y = np.ascontiguousarray(np.stack([y, 1 - y]))
    svm = SvmCfg(1.0, 1.0 / DIM, 1e-3, 1000000, 0, 0)

    def done(rc, outs, info):
        return rc, (lib.dge_last_error() or b"").decode(), outs + [np.array([info.rows])]

    def kmeans():
        labels = np.full(ROWS, -7, np.int32); centres = np.full((3, DIM), -7, np.float32); info = KmeansInfo(); info.rows = -7
        cfg = KmeansCfg(3, 2, 20, 0, 1)
        return done(lib.dge_kmeans_vectors(v._h, _p(select), C.byref(cfg), None, _p(labels), _p(centres), C.byref(info)), [labels, centres], info)

    def ridge():
        mae = np.full(1, -7.0); mre = np.full(1, -7.0); beta = np.full(DIM + 1, -7.0); pred = np.full(ROWS, -7.0); lam = np.ones(1); info = RidgeInfo(); info.rows = -7
        return done(lib.dge_ridge_loo_vectors(v._h, _p(t), 1, _p(select), _p(lam), 1, _p(mae), _p(mre), _p(beta), _p(pred), C.byref(info)), [mae, mre, beta, pred], info)

    def svm_fit():
        coef = np.full((2, ROWS), -7.0); bias = np.full(2, -7.0); it = np.full(2, -7, np.int64); conv = np.full(2, -7, np.int32); info = SvmInfo(); info.rows = -7
        return done(lib.dge_svm_fit_vectors(v._h, _p(Y), 2, _p(select), C.byref(svm), _p(coef), _p(bias), _p(it), _p(conv), C.byref(info)), [coef, bias, it, conv], info)

    def svm_cv():
        correct = np.full((2, 3), -7, np.int64); tested = np.full(3, -7, np.int64); dec = np.full((2, ROWS), -7.0); info = SvmInfo(); info.rows = -7
        return done(lib.dge_svm_cv_vectors(v._h, _p(Y), 2, _p(fold), 3, C.byref(svm), _p(correct), _p(tested), None, None, None, _p(dec), C.byref(info)), [correct, tested, dec], info)

    def tree_fit():
        cap = 2 * ROWS
        arrays = [np.full(cap, -7, np.int32), np.full(cap, -7.0), np.full(cap, -7, np.int32), np.full(cap, -7, np.int64), np.full(cap, -7, np.int64)]
        info = TreeInfo(); info.rows = -7; cfg = TreeCfg(0, 2, 1, 0)
        return done(lib.dge_tree_fit_vectors(v._h, _p(y), _p(select), C.byref(cfg), cap, *[_p(a) for a in arrays], C.byref(info)), arrays, info)

    row, cell = "row %d holds" % B, "row %d, column 1 holds" % B
    return dict(kmeans=(row, kmeans), ridge=(row, ridge), svm_fit=(cell, svm_fit), svm_cv=(cell, svm_cv), tree_fit=(cell, tree_fit))


def test_every_estimator_reports_the_least_used_row_and_writes_nothing(dge):
    X, y, t, present, select, fold = small_table()
    X[A, 3] = np.nan
    X[B, 4] = np.inf; X[B, 1] = np.inf
    X[C_ROW, 0] = np.nan
    X[D, 2] = -np.inf
    for name, (words, call) in calls(dge, X, y, t, present, select, fold).items():
        rc, msg, outs = call()
        assert rc == 1 and words in msg and "not finite" in msg, (name, rc, msg)
        for o in outs:
            assert (o == -7).all(), (name, o)


def test_rows_that_are_not_used_may_hold_anything(dge):
    X, y, t, present, select, fold = small_table()
    X[C_ROW, 0] = np.nan
    X[D, 2] = -np.inf
    used = present & (select != 0)
    for name, (_, call) in calls(dge, X, y, t, present, select, fold).items():
        rc, msg, outs = call()
        assert rc == 0, (name, rc, msg)
        assert outs[-1][0] == used.sum(), name                         # info.rows: the used rows
    rc, msg, (labels, centres, _) = calls(dge, X, y, t, present, select, fold)["kmeans"][1]()
    assert (labels[~used] == -1).all() and (labels[used] >= 0).all() and np.isfinite(centres).all()


def big(rows, dim, last):
    assert rows * dim > SCAN_ELEMS and (rows - 1) * dim < SCAN_ELEMS + 4096 * 256      # behind the grid, and within its second trip
    X = np.ones((rows, dim), np.float32)
    X[rows - 1, dim - 1] = last
    return X


def test_the_scan_reaches_the_last_element_kmeans(dge):
    rows, dim = 33000, 32
    with pytest.raises(dge.DgeError) as ei:
        dge.Vectors.from_host(big(rows, dim, np.nan)).kmeans(1, n_init=1, max_iter=1)
    assert ei.value.code == 1 and "row %d holds a value that is not finite" % (rows - 1) in str(ei.value)
    # the greatest |x| in the last element decides the scale
    labels, centres, info = dge.Vectors.from_host(big(rows, dim, 1000.0)).kmeans(1, n_init=1, max_iter=1)
    assert info["scale_bits"] == kref.scale_bits(1000.0, rows) and info["scale_bits"] != kref.scale_bits(1.0, rows)
    assert info["rows"] == rows and (labels == 0).all()


def test_the_scan_reaches_the_last_element_ridge(dge):
    rows, dim = 33000, 32
    with pytest.raises(dge.DgeError) as ei:
        dge.Vectors.from_host(big(rows, dim, np.nan)).ridge_loo(np.arange(rows, dtype=np.float64), [1.0], want_beta=False, want_pred=False)
    assert ei.value.code == 1 and "row %d holds a feature or a target that is not finite" % (rows - 1) in str(ei.value)


def test_the_scan_reaches_the_last_element_svm(dge):
    rows, dim = 40000, 32                                             # refused before the kernel matrix of 40 000 rows is asked for
    y = (np.arange(rows) % 2).astype(np.uint8)
    with pytest.raises(dge.DgeError) as ei:
        dge.Vectors.from_host(big(rows, dim, np.nan)).svm_fit(y)
    assert ei.value.code == 1 and "row %d, column %d holds a value that is not finite" % (rows - 1, dim - 1) in str(ei.value)
