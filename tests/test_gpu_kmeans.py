"""GPU: dge_kmeans_vectors / dge_kmeans (csrc/kmeans.hip) against the rule of include/dge.h as tests/kmeans_ref.py reads it: labels, centres (as bits),
inertia (as bits), iterations, best_restart, total_iterations, scale_bits and empty are EQUAL, at tile, block and limit sizes and on edge inputs; two calls give
the same bits; a larger table equals the host loop of tests/native/kmeans_rule_harness.cpp; errors leave the outputs untouched; the accuracy end to end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kmeans_ref as ref  # noqa: E402
from kmeans_harness import harness_kmeans, load_harness, same_result  # noqa: E402

pytestmark = pytest.mark.gpu


def run(dge, X, k, present=None, select=None, **kw):
    v = dge.Vectors.from_host(X, present=present)
    labels, centres, info = v.kmeans(k, select=select, **kw)
    return dict(info, labels=labels, centres=centres)


def check(dge, X, k, present=None, select=None, **kw):
    want = ref.kmeans_rows(X, k, present=present, select=select, **kw)
    got = run(dge, X, k, present=present, select=select, **kw)
    same_result(got, want)
    assert got["kernel_ms"] > 0.0
    return got


SHAPES = [(1, 3, 1), (255, 20, 4), (256, 20, 4), (257, 20, 4), (513, 20, 4), (300, 1, 3), (300, 255, 64), (300, 256, 64), (37, 6, 37), (64, 5, 64), (129, 9, 5), (150, 7, 20), (200, 12, 33)]


@pytest.mark.parametrize("n,dim,k", SHAPES)
def test_equal_to_the_reference(dge, n, dim, k):
    X, _ = ref.blobs(n, dim, min(k, 8), seed=12345 + n + dim, spread=1.5)
    got = check(dge, X, k, seed=12345, n_init=3)
    assert got["rows"] == n and 0 <= got["best_restart"] < 3


def test_duplicates(dge):
    """Two distinct points, k = 4: the seeding total becomes 0 (the fall-back picks row 0), ties go to the least centre, two centres stay empty where they are."""
    rng = np.random.default_rng(1)
    X = np.where(rng.random((300, 1)) < 0.5, np.float32(1.0), np.float32(-3.0)) * np.ones((1, 4), np.float32)
    got = check(dge, X, 4, seed=7, n_init=3)
    assert got["empty"] == 2 and got["inertia"] == 0.0


def test_absent_rows_and_a_select_mask(dge):
    rng = np.random.default_rng(2)
    X, _ = ref.blobs(400, 10, 4)
    present = rng.random(400) < 0.8
    select = rng.random(400) < 0.7
    X[~present] = 0.0
    got = check(dge, X, 4, present=present, select=select, seed=3, n_init=3)
    take = present & select
    assert (got["labels"][~take] == -1).all() and (got["labels"][take] >= 0).all() and got["rows"] == take.sum()
    compact = run(dge, X[take], 4, seed=3, n_init=3)
    assert np.array_equal(compact["labels"], got["labels"][take]) and np.array_equal(compact["centres"].view(np.uint32), got["centres"].view(np.uint32))
    assert compact["inertia"] == got["inertia"]
    only_present = check(dge, X, 4, present=present, seed=3, n_init=2)
    assert only_present["rows"] == present.sum()
    # the host-buffer entry: every row present, the mask alone selects
    import embedding_amd.evaluate as ev
    labels, centres, info = ev.kmeans_gpu(X, 4, seed=3, n_init=3, select=take)
    same_result(dict(info, labels=labels, centres=centres), got)


def test_extreme_values(dge):
    rng = np.random.default_rng(3)
    huge = (rng.uniform(-1, 1, (130, 6)) * 3.2e38).astype(np.float32); huge[0, 0] = 3.0e38
    assert check(dge, huge, 3, n_init=3)["scale_bits"] < 0
    zeros = check(dge, np.zeros((70, 3), np.float32), 2, n_init=3)
    assert zeros["scale_bits"] == 62 - 7 and zeros["empty"] == 1 and zeros["inertia"] == 0.0
    mixed = (rng.standard_normal((260, 8)) * 2.0 ** rng.integers(-20, 21, (260, 8))).astype(np.float32)
    mixed[:, 0] *= np.float32(2.0 ** 20)
    check(dge, mixed, 5, n_init=3)
    tiny = (rng.standard_normal((90, 4)) * 1e-42).astype(np.float32)                                     # denormal rows
    check(dge, tiny, 3, n_init=2)


def test_supplied_initial_centres(dge):
    X, _ = ref.blobs(513, 20, 4)
    got = check(dge, X, 3, init=X[[5, 100, 200]].copy(), n_init=7)
    assert got["best_restart"] == 0 and got["total_iterations"] == got["iterations"]


def test_max_iter_1(dge):
    X, _ = ref.blobs(257, 20, 4)
    got = check(dge, X, 5, n_init=2, max_iter=1)
    assert got["iterations"] == 1 and got["total_iterations"] == 2


def test_two_calls_give_the_same_bits(dge):
    X, _ = ref.blobs(5000, 33, 9, spread=4.0)
    v = dge.Vectors.from_host(X)
    a = v.kmeans(9, seed=5, n_init=3)
    b = v.kmeans(9, seed=5, n_init=3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert {k: x for k, x in a[2].items() if k != "kernel_ms"} == {k: x for k, x in b[2].items() if k != "kernel_ms"}
    c = v.kmeans(9, seed=6, n_init=3)
    assert c[2]["inertia"] > 0.0 and a[2]["total_iterations"] >= 3


def test_a_larger_table_equals_the_host_loop(dge, tmp_path):
    H = load_harness(str(tmp_path / "libkmeans_rule_harness.so"))
    X, _ = ref.blobs(20011, 128, 16, spread=6.0)
    want = harness_kmeans(H, X, 16, seed=12345, n_init=2, max_iter=8)
    got = run(dge, X, 16, seed=12345, n_init=2, max_iter=8)
    same_result(got, want)


def test_from_vec_then_kmeans(dge, tmp_path):
    """The golden file is the head of a longer one: its first line still says 77 rows, so that line is put right first (as tests/test_gpu_vec_read.py does).
    A name known beforehand that the file lacks makes row 0 absent."""
    data = open(os.path.join(ROOT, "tests", "golden", "taxi_all_head.vec"), "rb").read()
    path = str(tmp_path / "taxi_all_head3.vec")
    open(path, "wb").write(b"3 8 \n" + data[data.index(b"\n") + 1:])
    v, names, info = dge.Vectors.from_vec(path, header=True, names=dge.Names(["not-in-the-file"]))
    rows, present = v.to_host(), v.present()
    assert rows.shape == (4, 8) and present.tolist() == [False, True, True, True]
    for k in (1, 2, 3):
        labels, centres, inf = v.kmeans(k, seed=1, n_init=3)
        same_result(dict(inf, labels=labels, centres=centres), ref.kmeans_rows(rows, k, present=present, seed=1, n_init=3))
        assert labels[0] == -1 and inf["rows"] == 3


def test_errors_leave_the_outputs_untouched(dge):
    from embedding_amd._native import KmeansCfg, KmeansInfo, DgeError
    lib = dge.lib
    X, _ = ref.blobs(100, 6, 3)
    X[41, 2] = np.nan; X[17, 5] = np.inf
    select = np.ones(100, np.uint8); select[[17, 41]] = 0
    v = dge.Vectors.from_host(X)

    def call(k, sel, n_init=2, max_iter=10):
        labels = np.full(100, -7, np.int32); centres = np.full((max(k, 1), 6), 9.0, np.float32); info = KmeansInfo(); info.rows = -5
        cfg = KmeansCfg(k, n_init, max_iter, 0, 1)
        rc = lib.dge_kmeans_vectors(v._h, None if sel is None else sel.ctypes.data_as(C.c_void_p), C.byref(cfg), None, labels.ctypes.data_as(C.c_void_p),
                                    centres.ctypes.data_as(C.c_void_p), C.byref(info))
        return rc, (lib.dge_last_error() or b"").decode(), labels, centres, info

    rc, msg, labels, centres, info = call(3, None)
    assert rc == 1 and "row 17" in msg and "not finite" in msg and (labels == -7).all() and (centres == 9.0).all() and info.rows == -5
    only41 = select.copy(); only41[17] = 0; only41[41] = 1
    rc, msg, labels, centres, info = call(3, only41)
    assert rc == 1 and "row 41" in msg and (labels == -7).all() and info.rows == -5
    rc, msg, labels, centres, info = call(3, select)                                                    # the NaN sits in rows that are not selected: passes
    assert rc == 0 and info.rows == 98 and (labels[[17, 41]] == -1).all() and np.isfinite(centres).all()
    few = np.zeros(100, np.uint8); few[:2] = 1
    rc, msg, labels, centres, info = call(3, few)
    assert rc == 1 and "k = 3" in msg and "2 selected rows" in msg and (labels == -7).all() and (centres == 9.0).all()
    rc, msg, labels, centres, info = call(65, select)
    assert rc == 1 and "k = 65" in msg and (labels == -7).all() and info.rows == -5
    with pytest.raises(ValueError, match="init must be"):
        v.kmeans(3, select=select, init=np.zeros((3, 5), np.float32))
    with pytest.raises(DgeError, match="k = 101"):
        dge.Vectors.from_host(X[:50]).kmeans(101)


def test_accuracy_end_to_end(dge):
    import embedding_amd.evaluate as ev
    rng = np.random.default_rng(4)
    X, truth = ref.blobs(600, 12, 4, spread=2.5)
    present = rng.random(600) < 0.85
    gnd = np.where(rng.random(600) < 0.9, truth, -1).astype(np.int32)
    v = dge.Vectors.from_host(X, present=present)
    acc, labels, info = ev.clustering_accuracy_vectors(v, gnd, 4, seed=12345, n_init=3)
    want_labels = ref.kmeans_rows(X, 4, present=present, seed=12345, n_init=3)["labels"]
    want, cnt, m = ref.clustering_accuracy(want_labels, gnd, 4)
    assert np.array_equal(labels, want_labels) and np.array_equal(info["cnt"], cnt) and np.array_equal(info["map"], m)
    assert np.float64(acc).view(np.uint64) == np.float64(want).view(np.uint64) and 0.25 < acc <= (present & (gnd >= 0)).sum() / (gnd >= 0).sum()      # absent rows with a ground label count below
