"""CPU: the per-element pieces of the decision-tree rule (embedding_amd/csrc/tree_rule.h, built for the host by tests/native/tree_rule_harness.cpp) against
exact arithmetic — the comparator against fractions.Fraction on random and extreme counts, the threshold and a <= m < b on neighbouring and far-apart float32
values, the value key, the leaf test and the vote — and the two host rules of the Python view, stratified_folds and median_labels, against tests/tree_ref.py and
the reference's own np.median reading."""
import ctypes as C
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tree_ref as ref  # noqa: E402

SRC = os.path.join(ROOT, "tests", "native", "tree_rule_harness.cpp")
NMAX = 1 << 20


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tree") / "libtree_rule_harness.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-Wall", "-ffp-contract=off", "-o", so, SRC])
    h = C.CDLL(so)
    h.harness_tree_key.argtypes = [C.c_float]; h.harness_tree_key.restype = C.c_uint32
    h.harness_tree_unkey.argtypes = [C.c_uint32]; h.harness_tree_unkey.restype = C.c_float
    h.harness_tree_score.argtypes = [C.c_int64] * 4 + [C.POINTER(C.c_uint64)] * 2
    h.harness_tree_score_cmp.argtypes = [C.c_uint64] * 4
    h.harness_tree_better.argtypes = [C.c_int64] * 4 + [C.c_int32, C.c_uint32, C.c_int64, C.c_int64, C.c_int32, C.c_uint32]
    h.harness_tree_better_raw.argtypes = [C.c_uint64, C.c_uint64, C.c_int32, C.c_uint32] * 2
    h.harness_tree_threshold.argtypes = [C.c_float, C.c_float]; h.harness_tree_threshold.restype = C.c_double
    h.harness_tree_goes_left.argtypes = [C.c_float, C.c_double]
    h.harness_tree_is_leaf.argtypes = [C.c_int64, C.c_int64] + [C.c_int32] * 4
    h.harness_tree_valid_cut.argtypes = [C.c_int64, C.c_int64, C.c_int32]
    h.harness_tree_vote.argtypes = [C.c_int64, C.c_int64]
    return h


def score(n, p, nL, pL):
    nR, pR = n - nL, p - pL
    return Fraction(pL * pL + (nL - pL) ** 2, nL) + Fraction(pR * pR + (nR - pR) ** 2, nR)


def cuts(rng, n, p, k):
    """k cuts (nL, pL) a node of n rows, p of label 1, can have: extreme and random"""
    out = []
    for nL in [1, n - 1, n // 2, max(1, n // 3)] + [int(v) for v in rng.integers(1, n, k)]:
        lo, hi = max(0, p - (n - nL)), min(p, nL)
        for pL in {lo, hi, (lo + hi) // 2, int(rng.integers(lo, hi + 1))}:
            out.append((nL, pL))
    return out


def test_the_score_is_the_rational_of_the_rule(H):
    rng = np.random.default_rng(1)
    for n in (2, 3, 7, 1000, NMAX - 1, NMAX):
        for p in sorted({0, 1, n - 1, n, n // 2, int(rng.integers(0, n + 1))}):
            for nL, pL in cuts(rng, n, p, 6):
                N = C.c_uint64(0); D = C.c_uint64(0)
                H.harness_tree_score(n, p, nL, pL, C.byref(N), C.byref(D))
                assert D.value == nL * (n - nL) and Fraction(N.value, D.value) == score(n, p, nL, pL)
                assert N.value <= 1 << 58 and D.value <= 1 << 38


def test_the_comparator_against_fractions(H):
    """tr_better on random and extreme counts: the greater score, then the lesser feature, then the lesser a — and never both ways"""
    rng = np.random.default_rng(2)
    seen_equal = 0
    for n in (2, 3, 4, 10, 64, 4099, NMAX - 1, NMAX):
        for p in sorted({0, 1, n - 1, n, n // 2, int(rng.integers(0, n + 1))}):
            cs = cuts(rng, n, p, 5)
            for i in range(len(cs)):
                for j in range(len(cs)):
                    (nL1, pL1), (nL2, pL2) = cs[i], cs[j]
                    f1, f2 = int(rng.integers(0, 3)), int(rng.integers(0, 3))
                    a1, a2 = int(rng.integers(1, 4)), int(rng.integers(1, 4))
                    s1, s2 = score(n, p, nL1, pL1), score(n, p, nL2, pL2)
                    want = s1 > s2 if s1 != s2 else (f1 < f2 if f1 != f2 else a1 < a2)
                    seen_equal += s1 == s2
                    assert H.harness_tree_better(n, p, nL1, pL1, f1, a1, nL2, pL2, f2, a2) == int(want), (n, p, cs[i], cs[j], f1, a1, f2, a2)
                    assert not (H.harness_tree_better(n, p, nL1, pL1, f1, a1, nL2, pL2, f2, a2) and H.harness_tree_better(n, p, nL2, pL2, f2, a2, nL1, pL1, f1, a1))
    assert seen_equal > 100
    # equal scores of different cuts: the mirror cut of a balanced node scores the same; (column, a) decides
    assert score(8, 4, 2, 2) == score(8, 4, 6, 2)
    assert H.harness_tree_better(8, 4, 2, 2, 0, 9, 8 - 2, 2, 1, 3) == 1 and H.harness_tree_better(8, 4, 6, 2, 1, 3, 2, 2, 0, 9) == 0      # the lesser column
    assert H.harness_tree_better(8, 4, 2, 2, 1, 3, 6, 2, 1, 9) == 1 and H.harness_tree_better(8, 4, 6, 2, 1, 9, 2, 2, 1, 3) == 0          # then the lesser a
    # cross products that need all 96 bits, one apart
    big_n, big_d = 1 << 58, 1 << 38
    assert H.harness_tree_score_cmp(big_n, big_d, big_n - 1, big_d) == 1 and H.harness_tree_score_cmp(big_n - 1, big_d, big_n, big_d) == -1
    assert H.harness_tree_score_cmp(big_n, big_d, big_n, big_d) == 0 and H.harness_tree_score_cmp(big_n, big_d - 1, big_n, big_d) == 1
    for _ in range(2000):
        N1, N2 = (int(v) for v in rng.integers(1, (1 << 58) + 1, 2)); D1, D2 = (int(v) for v in rng.integers(1, (1 << 38) + 1, 2))
        want = (Fraction(N1, D1) > Fraction(N2, D2)) - (Fraction(N1, D1) < Fraction(N2, D2))
        assert H.harness_tree_score_cmp(N1, D1, N2, D2) == want
    # no candidate (D = 0) loses against any candidate and wins against none
    assert H.harness_tree_better_raw(0, 0, 0, 1, 5, 3, 7, 1) == 0 and H.harness_tree_better_raw(5, 3, 7, 1, 0, 0, 0, 1) == 1 and H.harness_tree_better_raw(0, 0, 0, 1, 0, 0, 1, 1) == 0


def f32(x):
    return np.float32(x)


def pairs():
    out = [(f32(-1e30), f32(-1e-30)), (f32(1e-30), f32(1e30)), (f32(-1e30), f32(1e30)), (f32(-0.0), f32(1e-45)), (f32(-1e-45), f32(0.0)), (f32(-1e-45), f32(-0.0)),
           (f32(1e-45), f32(3e-45)), (f32(-3e-45), f32(-1e-45)), (f32(1.1754942e-38), f32(1.17549435e-38)), (f32(-3.4028235e38), f32(3.4028235e38)),
           (f32(3.4028233e38), f32(3.4028235e38)), (f32(0.0), f32(3.4028235e38)), (f32(-3.4028235e38), f32(-0.0)), (f32(1.0), f32(1e30)), (f32(1e-45), f32(1.0))]
    for x in [0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, 1.1754944e-38, 3.0e38, -3.0e38, 16777216.0, 0.1, -0.3, 1e-30, 1e30]:
        x = f32(x)
        up = np.nextafter(x, f32(np.inf)); dn = np.nextafter(x, f32(-np.inf))
        if np.isfinite(up) and up != x:
            out.append((x, up))
        if np.isfinite(dn) and dn != x:
            out.append((dn, x))
    return [(a, b) for a, b in out if a < b]


def test_the_threshold_lies_between_its_values(H):
    for a, b in pairs():
        m = H.harness_tree_threshold(a, b)
        assert m == (float(a) + float(b)) * 0.5                                     # the two binary64 operations of the rule
        assert float(a) <= m < float(b), (a, b, m)
        assert H.harness_tree_goes_left(a, m) == 1 and H.harness_tree_goes_left(b, m) == 0
        if Fraction(float(a)) + Fraction(float(b)) == Fraction(float(a) + float(b)):  # an exact sum: m is the exact midpoint
            assert Fraction(m) == (Fraction(float(a)) + Fraction(float(b))) / 2
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32)
    v = np.unique(bits.view(np.float32)[np.isfinite(bits.view(np.float32))])
    for a, b in zip(v[:-1].tolist(), v[1:].tolist()):
        if a < b:
            m = H.harness_tree_threshold(a, b)
            assert a <= m < b and m == (a + b) * 0.5


def test_the_key_orders_as_the_values_do(H):
    rng = np.random.default_rng(4)
    bits = rng.integers(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32)
    v = bits.view(np.float32)
    v = np.concatenate([v[np.isfinite(v)], np.array([0.0, -0.0, 1e-45, -1e-45, 3.4028235e38, -3.4028235e38, 1.0, -1.0], np.float32)])
    keys = [H.harness_tree_key(x) for x in v.tolist()]
    assert H.harness_tree_key(-0.0) == H.harness_tree_key(0.0) and 0 not in keys
    for i in range(len(v) - 1):
        a, b = float(v[i]), float(v[i + 1])
        assert (a < b) == (keys[i] < keys[i + 1]) and (a == b) == (keys[i] == keys[i + 1])
    for x, k in zip(v.tolist(), keys):
        assert H.harness_tree_unkey(k) == x                                          # as numbers: -0.0 comes back as +0.0


def test_leaf_test_cut_test_and_vote(H):
    for n in range(0, 9):
        for p in range(0, n + 1):
            assert H.harness_tree_vote(n, p) == (1 if 2 * p > n else 0)
            for d, md, ms in ((0, 0, 2), (3, 3, 2), (2, 3, 2), (5, 0, 4), (1, 1, 5), (7, 3, 2)):
                want = p == 0 or p == n or n < ms or (md > 0 and d >= md)
                assert H.harness_tree_is_leaf(n, p, d, md, ms, 1) == int(want)
    assert H.harness_tree_vote(NMAX, NMAX // 2) == 0 and H.harness_tree_vote(NMAX, NMAX // 2 + 1) == 1
    for n, nL, ml, want in ((10, 1, 1, 1), (10, 1, 2, 0), (10, 2, 2, 1), (10, 8, 2, 1), (10, 9, 2, 0), (4, 2, 2, 1), (3, 1, 2, 0)):
        assert H.harness_tree_valid_cut(n, nL, ml) == want


def test_stratified_folds(dge):
    import embedding_amd.evaluate as ev
    rng = np.random.default_rng(5)
    for n, F in ((1, 1), (7, 2), (10, 10), (77, 10), (100, 3), (65, 64)):
        y = rng.integers(0, 2, n)
        for select in (None, rng.random(n) < 0.7):
            got = ev.stratified_folds(y, F, select)
            assert got.dtype == np.int32 and np.array_equal(got, ref.stratified_folds(y, F, select))
            use = np.ones(n, bool) if select is None else select
            assert (got[~use] == -1).all() and (got[use] >= 0).all() and (got < F).all()
            for cls in (0, 1):                                                       # every class is dealt round: fold sizes differ by one at most
                sizes = np.bincount(got[use & (y == cls)], minlength=F)
                assert sizes.max() - sizes.min() <= 1
    assert ev.stratified_folds([1, 1, 0, 1, 0, 1], 2).tolist() == [0, 1, 0, 0, 1, 1]
    with pytest.raises(ValueError):
        ev.stratified_folds([0, 1], 0)


def test_median_labels_is_the_references_reading(dge):
    """generatePOIlabel_helper computes np.median in binary64 and compares; ours decides in integers: the same labels and flag on odd and even lengths"""
    import embedding_amd.evaluate as ev
    rng = np.random.default_rng(6)
    cases = [[0], [1], [0, 0], [0, 1], [0, 2], [1, 1], [0, 0, 1], [0, 1, 1], [0, 0, 0, 5], [3, 1, 2], [4, 1, 3, 2], [0, 0, 1, 2], [1, 0, 1, 2, 1, 2], [2**53 + 1, 2**53 + 2, 0, 1]]
    for n in (5, 6, 77, 78, 801):
        cases += [rng.integers(0, 4, n).tolist(), rng.integers(0, 1000, n).tolist(), (rng.random(n) < 0.3).astype(int).tolist()]
    for c in cases:
        got, flag = ev.median_labels(np.array(c, np.int64))
        want, wflag = ref.median_labels_numpy(c)
        if max(c) < 2**52:                                                           # where binary64 holds the median exactly, the two readings agree
            assert np.array_equal(got, want) and flag == wflag, c
        s = sorted(c)
        med = Fraction(s[len(s) // 2]) if len(s) % 2 else Fraction(s[len(s) // 2 - 1] + s[len(s) // 2], 2)
        assert got.tolist() == [1 if v >= med else 0 for v in c] and flag == (med >= 1)
    assert ev.median_labels(np.array([0, 0, 5]))[1] is False and ev.median_labels(np.array([0, 1, 5]))[1] is True
    with pytest.raises(ValueError):
        ev.median_labels(np.array([0.5, 1.0]))


def test_the_reference_reading_on_a_tree_worked_by_hand():
    """tests/tree_ref.py on a case small enough to check on paper: one column, values 0 0 1 1 2 2, labels 0 0 1 1 0 0"""
    X = np.array([[0], [0], [1], [1], [2], [2]], np.float32)
    t = ref.tree_fit(X, [0, 0, 1, 1, 0, 0])
    # the cut behind 0 scores (0 + 4)/2 + (4 + 4)/4 = 4, the cut behind 1 scores (4 + 4)/4 + (0 + 4)/2 = 4: equal, the least a (0) wins; the right child (1 1 0 0) splits at 1.5
    assert t["feature"].tolist() == [0, -1, 0, -1, -1] and t["threshold"].tolist() == [0.5, 0.0, 1.5, 0.0, 0.0] and t["left"].tolist() == [1, -1, 3, -1, -1]
    assert t["count"].tolist() == [6, 2, 4, 2, 2] and t["pos"].tolist() == [2, 0, 2, 2, 0] and t["depth"] == 2
    assert ref.tree_predict(t, np.array([[0.5], [0.50001], [1.5], [1.6], [-9], [9]], np.float32)).tolist() == [0, 1, 1, 0, 0, 0]
    two = ref.tree_fit(np.array([[1, 5], [1, 5]], np.float32), [0, 1])              # identical rows, opposite labels: an impure leaf, the tie votes 0
    assert two["n_nodes"] == 1 and ref.tree_predict(two, np.array([[1, 5]], np.float32)).tolist() == [0]
