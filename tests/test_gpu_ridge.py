"""GPU: dge_ridge_loo_vectors / dge_ridge_loo / dge_ridge_predict_vectors (csrc/ridge.hip) against the rule of include/dge.h: mae, mre, beta, the left-out
predictions (all as bits) and the info counts are EQUAL to tests/ridge_ref.py at small shapes and, from dim 63 on, to the host loop of
tests/native/ridge_rule_harness.cpp, which tests/test_ridge_host.py ties to the reference — at the edges of the blocks, where P crosses a wave's width and at
its limit, with absent and deselected rows, for one and several targets and penalties, for every chunk size; the refusals are status returns that name their
column or row and leave the outputs untouched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ridge_ref as ref  # noqa: E402
from ridge_harness import harness_ridge, load_harness, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return load_harness(os.path.join(str(tmp_path_factory.mktemp("ridge_rule_harness")), "libridge_rule_harness.so"))


def table(n, dim, T, seed):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n, dim)) * 10.0 ** rng.integers(-1, 2, dim)).astype(np.float32)
    Y = rng.standard_normal((n, T)) * 50.0 + 20.0
    return X, Y


def used_rows(n, present, select):
    use = np.ones(n, bool)
    if present is not None:
        use &= np.asarray(present) != 0
    if select is not None:
        use &= np.asarray(select) != 0
    return np.flatnonzero(use)


def same_as(got, want, idx, n_rows, chunk=64):
    """got: what Vectors.ridge_loo gives; want: the rule on the used rows idx"""
    for f in ("mae", "mre", "beta"):
        assert same_bits(got[f], want[f]), (f, got[f].ravel()[:4], want[f].ravel()[:4])
    pred = got["loo_pred"]
    assert pred.shape == want["loo_pred"].shape[:2] + (n_rows,)
    assert same_bits(pred[:, :, idx], want["loo_pred"])
    rest = np.setdiff1d(np.arange(n_rows), idx)
    assert np.isnan(pred[:, :, rest]).all()
    info = got["info"]
    blocks = (len(idx) + 255) // 256
    assert info["rows"] == len(idx) and info["blocks"] == blocks and info["chunks"] == (blocks + chunk - 1) // chunk
    assert same_bits(info["min_pivot"], want["d"].min()) and same_bits(info["max_leverage"], want["h"].max())
    assert info["kernel_ms"] > 0.0


def check(dge, harness, X, Y, lambdas, present=None, select=None, by_ref=None):
    idx = used_rows(len(X), present, select)
    Yu = np.asarray(Y, np.float64).reshape(len(X), -1)[idx]
    by_ref = X.shape[1] < 63 and len(idx) * X.shape[1] <= 2000 if by_ref is None else by_ref
    want = ref.ridge_loo(X[idx], Yu, lambdas) if by_ref else harness_ridge(harness, X[idx], Yu, lambdas)
    assert "refused" not in want, want
    v = dge.Vectors.from_host(X, present=present)
    got = v.ridge_loo(Y, lambdas, select=select)
    same_as(got, want, idx, len(X))
    return got, want, v


@pytest.mark.parametrize("n", [2, 255, 256, 257, 513])
def test_block_edges_against_the_reference(dge, harness, n):
    X, Y = table(n, 3, 2, 100 + n)
    check(dge, harness, X, Y, [0.5, 4.0] if n == 2 else [0.0, 0.5], by_ref=True)


@pytest.mark.parametrize("dim", [1, 63, 64, 65, 256])
def test_where_P_crosses_a_wave_and_at_its_limit(dge, harness, dim):
    n = 300
    X, Y = table(n, dim, 2, 200 + dim)
    check(dge, harness, X, Y, [0.25, 2.0] if dim == 256 else [0.0, 0.25])


def test_absent_and_deselected_rows_are_never_read(dge, harness):
    n = 400
    X, Y = table(n, 5, 2, 7)
    rng = np.random.default_rng(8)
    present = (rng.random(n) < 0.8).astype(np.uint8)
    select = (rng.random(n) < 0.7).astype(np.uint8)
    present[0] = 0; select[1] = 0; present[n - 1] = 0
    unused = np.setdiff1d(np.arange(n), used_rows(n, present, select))
    X[unused] = np.nan                                            # what an unused row holds decides nothing
    Y[unused] = np.inf
    got, _, _ = check(dge, harness, X, Y, [0.0, 1.0], present=present, select=select)
    assert got["info"]["rows"] == n - len(unused) and got["info"]["blocks"] == 1


@pytest.mark.parametrize("T,lambdas", [(1, [0.5]), (5, [0.0, 0.125, 1.0, 64.0]), (1, [0.0, 0.5, 2.0, 8.0]), (5, [3.0])])
def test_targets_and_penalties(dge, harness, T, lambdas):
    X, Y = table(90, 4, T, 31 + T)
    got, _, _ = check(dge, harness, X, Y, lambdas)
    assert got["mae"].shape == (len(lambdas), T)
    y1 = Y[:, 0] if T == 1 else Y
    v = dge.Vectors.from_host(X)
    again = v.ridge_loo(y1, lambdas, want_beta=False, want_pred=False)      # a one-dimensional y is one target; the optional outputs decide nothing
    assert again["beta"] is None and again["loo_pred"] is None and same_bits(again["mae"], got["mae"]) and same_bits(again["mre"], got["mre"])


def test_every_chunk_size_gives_the_same_bits(dge, harness):
    """n = 700 is three blocks: the knob at 1 and 2 takes the moments in three and two chunks, the default in one"""
    X, Y = table(700, 9, 2, 41)
    want = harness_ridge(harness, X, Y, [0.0, 0.5])
    v = dge.Vectors.from_host(X)
    for chunk, chunks in ((1, 3), (2, 2), (None, 1)):
        if chunk is None:
            got = v.ridge_loo(Y, [0.0, 0.5])
        else:
            with dge.tuning(ridge_chunk=chunk):
                got = v.ridge_loo(Y, [0.0, 0.5])
        same_as(got, want, np.arange(700), 700, chunk=chunk or 64)
        assert got["info"]["chunks"] == chunks and got["info"]["blocks"] == 3


def test_host_rows_equal_the_resident_form(dge, harness):
    import embedding_amd.evaluate as ev
    X, Y = table(300, 17, 3, 51)
    select = (np.arange(300) % 7 != 0).astype(np.uint8)
    a = ev.ridge_loo_gpu(X, Y, [0.0, 2.0], select=select)
    b = dge.Vectors.from_host(X).ridge_loo(Y, [0.0, 2.0], select=select)
    for f in ("mae", "mre", "beta", "loo_pred"):
        assert same_bits(a[f], b[f]), f
    assert {k: v for k, v in a["info"].items() if k != "kernel_ms"} == {k: v for k, v in b["info"].items() if k != "kernel_ms"}
    same_as(a, harness_ridge(harness, X[select != 0], Y[select != 0], [0.0, 2.0]), np.flatnonzero(select), 300)


def test_predict_is_the_chain_of_the_rule(dge, harness):
    """a fit on one mask applied to all rows: every present row gets the p chain of its model, an absent row NaN"""
    for n, dim in ((300, 5), (257, 70)):
        X, Y = table(n, dim, 2, 61 + dim)
        present = np.ones(n, np.uint8); present[[3, n - 1]] = 0
        select = (np.arange(n) % 2 == 0).astype(np.uint8)
        v = dge.Vectors.from_host(X, present=present)
        fit = v.ridge_loo(Y, [0.5, 2.0], select=select)
        out = v.ridge_predict(fit["beta"])
        assert out.shape == (2, 2, n) and np.isnan(out[:, :, [3, n - 1]]).all()
        for l in range(2):
            for t in range(2):
                b = np.ascontiguousarray(fit["beta"][l, t])
                for i in range(n):
                    if present[i]:
                        want = harness.harness_ridge_predict(X[i].ctypes.data, b.ctypes.data, dim)
                        assert same_bits(out[l, t, i], want), (l, t, i)
                if dim == 5:
                    for i in (0, 1, 2, 255, 256, n - 2):
                        assert same_bits(out[l, t, i], ref.predict(ref.design(X[i:i + 1])[0], b))
        # on a used row the left-out prediction is not the fit's own: y - e against p
        assert not same_bits(out[0, 0, 0], fit["loo_pred"][0, 0, 0])
        one = v.ridge_predict(fit["beta"][1, 0])
        assert one.shape == (n,) and same_bits(one, out[1, 0])


def test_the_refusals_name_their_column_and_row(dge, harness):
    rng = np.random.default_rng(5)
    X = rng.integers(-8, 9, (12, 4)).astype(np.float32)
    y = rng.integers(-20, 21, 12).astype(np.float64)
    X[:, 3] = X[:, 2]                                             # z's column 4 repeats column 3: its pivot is exactly 0 under lambda = 0
    assert harness_ridge(harness, X, y, [0.5, 0.0]).get("refused") == ("pivot", 1, 4)
    v = dge.Vectors.from_host(X)
    with pytest.raises(dge.DgeError) as ei:
        v.ridge_loo(y, [0.5, 0.0])
    assert ei.value.code == 1 and "column 4" in str(ei.value) and "lambda[1]" in str(ei.value), str(ei.value)
    assert np.isfinite(v.ridge_loo(y, [0.5, 2.0])["mae"]).all()

    # used row 3 is the only one with a second feature: leverage 1 under lambda = 0; with row 0 absent it is row 4 of all rows
    X = np.array([[9, 9], [1, 0], [2, 0], [4, 0], [3, 5], [7, 0], [8, 0]], np.float32)
    y = np.array([0.0, 1.0, 2.0, 0.0, 4.0, 5.0, 3.0])
    present = np.array([0, 1, 1, 1, 1, 1, 1], np.uint8)
    assert harness_ridge(harness, X[1:], y[1:], [1.0, 0.0]).get("refused") == ("leverage", 1, 3)
    v = dge.Vectors.from_host(X, present=present)
    from embedding_amd._native import RidgeInfo
    lam = np.array([1.0, 0.0]); mae = np.full((2, 1), -7.0); mre = np.full((2, 1), -7.0); beta = np.full((2, 1, 3), -7.0); pred = np.full((2, 1, 7), -7.0)
    info = RidgeInfo(); info.rows = -5
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    rc = dge.lib.dge_ridge_loo_vectors(v._h, p(y), 1, None, p(lam), 2, p(mae), p(mre), p(beta), p(pred), C.byref(info))
    msg = dge.lib.dge_last_error().decode()
    assert rc == 1 and "row 4 " in msg and "lambda[1]" in msg and "leverage" in msg, (rc, msg)
    assert (mae == -7).all() and (mre == -7).all() and (beta == -7).all() and (pred == -7).all() and info.rows == -5
    assert np.isfinite(v.ridge_loo(y, [1.0])["mae"]).all()

    # a value that is not finite in a used row: the least such row, features and targets alike
    X, Y = table(300, 3, 2, 71)
    X[280, 1] = np.inf; Y[270, 1] = np.nan
    v = dge.Vectors.from_host(X)
    with pytest.raises(dge.DgeError) as ei:
        v.ridge_loo(Y, [1.0])
    assert ei.value.code == 1 and "row 270 " in str(ei.value) and "not finite" in str(ei.value)
    Y[270, 1] = 0.0
    with pytest.raises(dge.DgeError) as ei:
        v.ridge_loo(Y, [1.0])
    assert ei.value.code == 1 and "row 280 " in str(ei.value)
    sel = np.ones(300, np.uint8); sel[280] = 0
    assert np.isfinite(v.ridge_loo(Y, [1.0], select=sel)["mae"]).all()
    with pytest.raises(dge.DgeError) as ei:
        v.ridge_loo(Y, [1.0], select=np.eye(1, 300, 5, dtype=np.uint8)[0])
    assert ei.value.code == 1 and "at least 2" in str(ei.value)
