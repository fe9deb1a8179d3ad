"""GPU: dge_knn_cosine / dge_ndcg_at_k and their resident-row entries (csrc/knn.hip) against the float64 reading of tests/knn_ref.py.

On LATTICE inputs (rows of c in {1, 4, 16, 64, 256} entries +-2^e: every float32 partial sum is exact in any order; tests/test_knn_ref.py shows that
on the CPU) the lists are EQUAL to the reference's: indices in a stable sort by (distance, index) with the row itself removed, distances as bits,
-1 / 3.0 past n-1 — at every padded-width class and its borders, odd widths, workgroup and tile edges, k = 1, 10, 64, planted zero rows, a group of
70 identical rows, lists that run into the distance-2 block, three row orders of one matrix, magnitudes 2^+-60, all-subnormal rows, non-finite rows
(zero vectors by the rule of include/dge.h), absent resident rows.  These inputs are nearly all ties: the (distance, index) order of the insertion
under the row locks is what they test.

On FLOAT inputs (a tight cluster, all-positive rows, near-duplicates at relative 2^-20) every distance is within tol(D) = (D + 10) 2^-24 of the float64
one — derived in tests/knn_ref.py, not measured — and the lists are right up to 2 tol around the k-th distance, with nothing excused.

nDCG on lattice inputs is within the rounding bound of knn_ref.ndcg_reference (below 1e-9 for every case, by tests/test_knn_ref.py), regions with an
ideal DCG of exactly 0 contributing 0."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knn_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_exact(got, want, what=""):
    (idx, dist), (ridx, rdist) = got, want
    bad = np.nonzero((idx != ridx).any(axis=1) | (bits(dist) != bits(rdist)).any(axis=1))[0]
    assert bad.size == 0, "%s: %d rows differ, first row %d:\n idx  %s\n want %s\n dist %s\n want %s" % (
        what, bad.size, bad[0], idx[bad[0]].tolist(), ridx[bad[0]].tolist(), dist[bad[0]].tolist(), rdist[bad[0]].tolist())


def check_exact(f, k, what=""):
    from embedding_amd import evaluate as ev
    idx, dist, _ = ev.knn_cosine_gpu(f, k)
    assert_exact((idx, dist), ref.reference_lists(f, k), "%s k=%d" % (what, k))
    return idx, dist


@pytest.mark.parametrize("k", ref.KS)
@pytest.mark.parametrize("n,D", ref.SHAPES)
def test_lattice_shapes_exact(dge, n, D, k):
    idx, dist = check_exact(ref.shape_case(n, D), k, "%dx%d" % (n, D))
    assert (idx[:, n - 1:] == -1).all() and (dist[:, n - 1:] == 3.0).all()           # (the tail, where k > n - 1)


def test_planted_zero_rows_identical_group_and_short_lists(dge):
    f = ref.planted_case()
    for k in (10, 64):
        idx, dist = check_exact(f, k, "planted")
        for r in ref.GROUP:                              # said again without the reference: the k smallest other indices of the group, at distance 0
            assert idx[r].tolist() == [j for j in ref.GROUP if j != r][:k] and (dist[r] == 0).all()
        for r in ref.ZERO_ROWS:
            assert idx[r].tolist() == [j for j in range(k + 1) if j != r][:k] and (dist[r] == 2).all()
    idx, dist = check_exact(ref.sparse_case(), 64, "sparse")
    for r in ref.SPARSE_LIVE:                            # fewer than k live others: on through the distance-2 block in index order
        m = int((dist[r] < 2).sum())
        assert m < len(ref.SPARSE_LIVE) and (np.diff(idx[r, m:]) > 0).all()


def test_three_row_orders_same_neighbours(dge):
    f = ref.order_case()
    k = 64
    d = ref.distances(f)
    key = d.copy(); np.fill_diagonal(key, np.inf)
    kth = np.sort(key, axis=1)[:, k - 1]
    back = {}
    for name, perm in ref.order_permutations(f).items():
        idx, dist = check_exact(f[perm], k, "order " + name)
        inv = np.argsort(perm)
        back[name] = (perm[idx][inv], dist[inv])         # lists of the original rows, in original indices
    first = back["descending"]
    for name, (idx, dist) in back.items():
        assert np.array_equal(bits(dist), bits(first[1])), name
        for r in range(0, len(f), 7):                    # the same neighbours wherever the k-th place is no tie; inside the tie the smaller index of THAT order wins
            inside = key[r] < kth[r]
            assert set(idx[r][d[r, idx[r]] < kth[r]].tolist()) == set(np.nonzero(inside)[0].tolist()), (name, r)


@pytest.mark.parametrize("case", ["huge", "subnormal", "nonfinite"])
def test_magnitudes_and_non_finite_rows(dge, case):
    """2^+-60 in one matrix; rows of subnormal entries only (norm below 2^-128) are ordinary vectors; a row with a NaN or an infinity is a zero vector."""
    f = getattr(ref, case + "_case")()
    for k in (10, 64):
        idx, dist = check_exact(f, k, case)
        if case == "nonfinite":
            from embedding_amd import evaluate as ev
            idx0, dist0, _ = ev.knn_cosine_gpu(ref.zeroed(f), k)
            assert np.array_equal(idx, idx0) and np.array_equal(bits(dist), bits(dist0))
            assert (dist[[3, 70, 130, 131]] == 2).all()


def test_absent_resident_rows_are_zero_vectors(dge):
    from embedding_amd import evaluate as ev
    f, present = ref.absent_case()
    f0 = f.copy(); f0[~present] = 0.0
    part = dge.Vectors.from_host(f, present)
    for k in (1, 10, 64):
        got = part.knn(k)[:2]
        assert_exact(got, ref.reference_lists(f0, k), "absent k=%d" % k)
        idx0, dist0, _ = ev.knn_cosine_gpu(f0, k)
        assert np.array_equal(got[0], idx0) and np.array_equal(bits(got[1]), bits(dist0))


worst = {}


@pytest.mark.parametrize("D", ref.FLOAT_DIMS)
@pytest.mark.parametrize("kind", ref.FLOAT_KINDS)
def test_float_rows_within_the_derived_bound(dge, kind, D):
    """|dist - float64| <= tol(D) = (D + 10) 2^-24 everywhere (derivation: tests/knn_ref.py); every returned neighbour within 2 tol of the k-th
    reference distance, every clearly closer one present, lists ascending, no row in its own list."""
    from embedding_amd import evaluate as ev
    f = ref.float_case(kind, D)
    for k in (10, 64):
        idx, dist, _ = ev.knn_cosine_gpu(f, k)
        worst[kind, D, k] = ref.check_float_lists(f, k, idx, dist)
    print("largest |dist - ref| / tol(D) so far: %.4f" % max(worst.values()))


@pytest.mark.parametrize("k", ref.KS)
@pytest.mark.parametrize("dim,gnd_dim", ref.NDCG_DIMS)
def test_ndcg_lattice_within_the_rounding_bound(dge, dim, gnd_dim, k):
    """Both entries; the bound (knn_ref.ndcg_reference) is a few 1e-14 here.  (33, 100) holds regions whose ideal DCG is exactly 0 (ratio 0 by rule),
    (64, 64) zero and non-finite rows on both sides."""
    from embedding_amd import evaluate as ev
    f, g = ref.ndcg_case(dim, gnd_dim)
    want, bound, flat = ref.ndcg_reference(f, g, k)
    assert bound < 1e-9 and (flat > 0) == ((dim, gnd_dim) == (33, 100))
    dev, _ = ev.ndcg_against_gpu(f, g, k)
    print("ndcg (%d, %d) k=%d: device - reference = %.3g, bound %.3g, %d regions with ideal DCG 0" % (dim, gnd_dim, k, dev - want, bound, flat))
    assert abs(dev - want) <= bound, (dev, want, bound)
    res, _ = dge.Vectors.from_host(f).ndcg_against(dge.Vectors.from_host(g), k)
    assert np.float64(res).view(np.uint64) == np.float64(dev).view(np.uint64)


def test_ndcg_float_rows(dge):
    """Gaussian rows, (dim, gnd_dim) = (100, 256): the lane loop of k_ndcg makes four trips; the project's 1e-5 against the host pipeline."""
    from embedding_amd import evaluate as ev
    from oracle import quality as qo
    rng = np.random.default_rng(5)
    g = rng.normal(size=(300, 256)).astype(np.float32)
    f = (g[:, :100] + 0.3 * rng.normal(size=(300, 100))).astype(np.float32)
    for k in (1, 10, 64):
        host = qo.ndcg_against(f, g, range(300), k=k)
        dev, _ = ev.ndcg_against_gpu(f, g, k)
        assert abs(dev - host) < 1e-5, (k, dev, host)
