"""CPU: the test of the KNN / nDCG tests (tests/knn_ref.py).  The exactness the device tests claim on lattice inputs must not rest on the device run:
a float32 model of the kernel's arithmetic, accumulating forward and backward, equals the float64 reference bit for bit on every lattice case; the
reference order is a plain sort by (distance, index); the float legs' model stays inside tol(D); the nDCG cases meet the 1e-9 condition."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knn_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def cases():
    return ref.lattice_cases()


def test_lattice_rows_are_lattice_rows(cases):
    for name, f in cases.items():
        g = ref.zeroed(f).astype(np.float64)
        cnt = (g != 0).sum(axis=1)
        assert set(cnt.tolist()) <= {0} | set(ref.COUNTS), name
        mag = np.abs(g).max(axis=1)
        assert ((g == 0) | (np.abs(g) == mag[:, None])).all(), name                      # one magnitude per row ...
        live = mag > 0
        assert (np.frexp(mag[live])[0] == 0.5).all(), name                                # ... and it is a power of two
    assert len({f.shape for f in cases.values()}) >= len(ref.SHAPES) + 3


def test_float32_model_equals_the_float64_reference_bit_for_bit(cases):
    ties = {}
    for name, f in cases.items():
        d = ref.distances(f)
        d32 = d.astype(np.float32)
        assert np.array_equal(d32.astype(np.float64), d), name                             # the reference itself is a float32 number
        for reverse in (False, True):
            m = ref.model_f32(f, reverse)
            off = ~np.eye(len(f), dtype=bool)                                               # (a list never holds its own row)
            assert np.array_equal(m[off].view(np.uint32), d32[off].view(np.uint32)), (name, reverse)
        if len(f) > 11:
            key = d.copy(); np.fill_diagonal(key, np.inf); key.sort(axis=1)
            ties[name] = float((key[:, 9] == key[:, 10]).mean())
    # the inputs are about ties: in most cases most rows have one exactly at the k = 10 boundary
    assert sorted(ties.values())[len(ties) // 4] > 0.5, ties


def test_reference_order_is_a_sort_by_distance_then_index():
    f = ref.shape_case(65, 33)
    d = ref.distances(f)
    for k in (1, 10, 64, 70):
        idx, dist = ref.reference_lists(f, k)
        for r in range(len(f)):
            want = sorted((d[r, j], j) for j in range(len(f)) if j != r)[:k]
            assert idx[r, :len(want)].tolist() == [j for _, j in want]
            assert dist[r, :len(want)].tolist() == [np.float32(x) for x, _ in want]
            assert (idx[r, len(want):] == -1).all() and (dist[r, len(want):] == 3.0).all()


def test_planted_structure_is_what_the_device_test_says():
    f = ref.planted_case()
    idx, dist = ref.reference_lists(f, 64)
    for r in ref.GROUP:                                 # the 64 smallest other indices of the group, at distance 0
        assert idx[r].tolist() == [j for j in ref.GROUP if j != r][:64] and (dist[r] == 0).all()
    for r in ref.ZERO_ROWS:                             # a zero row: everything at distance 2, in index order
        assert idx[r].tolist() == [j for j in range(65) if j != r][:64] and (dist[r] == 2).all()
    idx, dist = ref.reference_lists(ref.sparse_case(), 64)
    for r in ref.SPARSE_LIVE:
        m = int((dist[r] < 2).sum())
        assert m < len(ref.SPARSE_LIVE) and (dist[r, m:] == 2).all() and (np.diff(idx[r, m:]) > 0).all()


def test_row_orders_displace_list_tails():
    """In the descending order most rows near the probe meet closer and closer columns: their lists are rewritten many times."""
    f = ref.order_case()
    perms = ref.order_permutations(f)
    d0 = ref.distances(f)[0]
    assert (np.diff(d0[perms["descending"]]) <= 0).all() and (np.diff(d0[perms["ascending"]]) >= 0).all()
    assert (d0 < 0.5).sum() > 200 and len(np.unique(d0)) > 20


@pytest.mark.parametrize("D", ref.FLOAT_DIMS)
def test_float_model_stays_inside_the_derived_bound(D):
    for kind in ref.FLOAT_KINDS:
        f = ref.float_case(kind, D)
        d = ref.distances(f)
        off = ~np.eye(len(f), dtype=bool)
        err = max(np.abs(ref.model_f32(f, rev).astype(np.float64) - d)[off].max() for rev in (False, True))
        assert err <= ref.tol(D), (kind, err / ref.tol(D))
        if kind == "cluster":                           # the bound still discriminates: one dropped product term on these rows is an error of about 1 / D
            assert d[off].max() < 1e-4 and 1.0 / D > 100 * ref.tol(D)


def test_ndcg_cases_meet_the_condition():
    flat = {}
    for dim, gnd_dim in ref.NDCG_DIMS:
        f, g = ref.ndcg_case(dim, gnd_dim)
        for k in ref.KS:
            value, bound, flat[dim, gnd_dim, k] = ref.ndcg_reference(f, g, k)
            assert bound < 1e-9 and np.isfinite(value), (dim, gnd_dim, k, bound)
    assert all(flat[33, 100, k] >= 3 for k in ref.KS)  # the planted regions with ideal DCG 0, at every k


def test_ndcg_reading_agrees_with_the_oracle_where_the_oracle_is_defined():
    from oracle import quality as qo
    seen = 0
    for dim, gnd_dim in ref.NDCG_DIMS:                  # lattice rows: the float32 ground distances the reading takes are the oracle's float64 ones
        f, g = ref.ndcg_case(dim, gnd_dim)
        f, g = ref.zeroed(f)[:120], ref.zeroed(g)[:120]
        value, _, flat = ref.ndcg_reference(f, g, 10)
        if flat == 0:
            seen += 1
            assert abs(value - qo.ndcg_against(f, g, range(120), k=10)) < 1e-12
    assert seen >= 2
