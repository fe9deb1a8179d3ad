"""CPU: embedding_amd/csrc/pairwise_rule.h built for the host (tests/native/pairwise_rule_harness.cpp, g++ -ffp-contract=off) against the numpy reading of
tests/pairwise_ref.py on the full POI fixture: the 801 x 801 ground distances, the ranks of the ground order and the ideal DCG prefixes at the paper's eight k
are equal bit for bit; so are the ratios of a set of lists.  The kernels of csrc/pairwise.hip call the same header."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pairwise_ref as ref  # noqa: E402


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pairwise") / "libpairwise_rule_harness.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-Wall", "-ffp-contract=off", "-o", so,
                           os.path.join(ROOT, "tests", "native", "pairwise_rule_harness.cpp")])
    return C.CDLL(so)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def host_ground(H, gnd, ks, present=None):
    gnd = np.ascontiguousarray(gnd, np.float32)
    n, g = gnd.shape
    ks = np.ascontiguousarray(ks, np.int32)
    pres = None if present is None else np.ascontiguousarray(present, np.uint8)
    dist = np.empty((n, n)); rank = np.empty((n, n), np.int32); idx = np.empty((n, int(ks[-1])), np.int32); ideal = np.empty((len(ks), n))
    assert H.harness_pw_distances(_p(gnd), _p(pres), n, g, _p(dist)) == 0
    assert H.harness_pw_order(_p(dist), n, _p(ks), len(ks), _p(rank), _p(idx), _p(ideal)) == 0
    return dist, rank, idx, ideal


def test_the_header_equals_the_python_reading_on_the_fixture(harness):
    _, gnd = ref.fixture()
    dist, rank, idx, ideal = host_ground(harness, gnd, ref.PAPER_KS)
    d, live = ref.ground_distances(gnd)
    off = ~np.eye(len(gnd), dtype=bool)
    assert np.array_equal(bits(dist)[off], bits(d)[off])
    assert sorted(np.flatnonzero(~live).tolist()) == list(ref.FIXTURE_ZERO_ROWS) and (dist[list(ref.FIXTURE_ZERO_ROWS)] == 2.0).all()
    assert np.array_equal(bits(dist), bits(dist.T))                                   # symmetric bit for bit
    order, rrank = ref.ground_order(d)
    assert np.array_equal(rank, rrank) and np.array_equal(idx, order[:, :70])
    want = ref.chain(np.take_along_axis(d, order[:, :70], 1), ref.discounts(70), ref.PAPER_KS)
    assert np.array_equal(bits(ideal), bits(want))
    # the fixture's ties are what the issue counted: the tie rule decides the figure
    dd = np.take_along_axis(d, order, 1)
    assert int((dd[:, 1:301] == dd[:, :300]).sum()) == 7618 and int((dd[:, 69] == dd[:, 70]).sum()) == 24


def test_absent_and_non_finite_rows_and_the_ratios(harness):
    rng = np.random.default_rng(2)
    gnd = rng.normal(size=(40, 7)).astype(np.float32)
    gnd[3] = 0; gnd[9, 2] = np.nan; gnd[11, 0] = np.inf; gnd[20] = -2 * gnd[19]
    present = np.ones(40, bool); present[30] = False
    ks = (1, 3, 8)
    dist, rank, idx, ideal = host_ground(harness, gnd, ks, present)
    d, live = ref.ground_distances(gnd, present)
    off = ~np.eye(40, dtype=bool)
    assert np.array_equal(bits(dist)[off], bits(d)[off]) and np.flatnonzero(~live).tolist() == [3, 9, 11, 30]
    lists = np.stack([rng.permutation(np.delete(np.arange(40), r))[:8] for r in range(40)])[None].astype(np.int32)
    want = ref.evaluate(gnd, lists, None, ks, 5, gnd_present=present)
    assert np.array_equal(rank, want["rank"]) and np.array_equal(bits(ideal), bits(want["ideal"]))
    kk = np.array(ks, np.int32)
    for r in range(40):
        out = np.empty(3)
        harness.harness_pw_ratios(_p(np.ascontiguousarray(dist[r, lists[0, r]])), _p(kk), 3, _p(np.ascontiguousarray(ideal[:, r])), _p(out))
        assert np.array_equal(bits(out), bits(want["ratio"][0, :, r])), r
    assert (want["ratio"][0][:, [3, 9, 11, 30]] == 1.0).all()                          # a zero-vector ground row: every relevance -1, ratio 1
