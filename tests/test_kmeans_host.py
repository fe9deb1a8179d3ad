"""CPU: embedding_amd/csrc/kmeans_rule.h and cluster_match.h — what every lane of kmeans.hip runs, and the accuracy on top — built for the host
(tests/native/kmeans_rule_harness.cpp, -ffp-contract=off) and held to the rule of include/dge.h: every piece bit for bit equal to tests/kmeans_ref.py, and a
whole small clustering by a host loop over the same header too; the same harness, built stand-alone with -fsanitize=address,undefined, runs clean.  The
reference's own fast distance (dist_all) is first held to its definition in exact rational arithmetic."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kmeans_ref as ref  # noqa: E402
from kmeans_harness import SRC, _p, harness_kmeans, load_harness, same_result  # noqa: E402

CSRC = os.path.join(ROOT, "embedding_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return load_harness(os.path.join(str(tmp_path_factory.mktemp("kmeans_rule_harness")), "libkmeans_rule_harness.so"))


def chain_inputs():
    """rows and centres whose differences span the binary32 range: blobs, huge, tiny (denormal), mixed magnitudes, exact ties"""
    rng = np.random.default_rng(20261018)
    out = []
    for dim in (1, 2, 7, 20, 33):
        for scale in (1.0, 3e38 / 4, 1e-42, 2.0 ** 40):
            x = (rng.standard_normal((6, dim)) * scale).astype(np.float32)
            c = (rng.standard_normal((3, dim)) * scale).astype(np.float32)
            out.append((x, c))
    mixed = (rng.standard_normal((6, 12)) * 2.0 ** rng.integers(-60, 60, (6, 12))).astype(np.float32)
    out.append((mixed, mixed[:3].copy()))
    out.append((np.array([[3.4028235e38, -3.4028235e38]], np.float32), np.array([[-3.4028235e38, 3.4028235e38], [0, 0]], np.float32)))
    return out


def test_the_fast_distance_of_the_reference_is_its_definition(harness):
    """dist_all (numpy, error-free pieces) against dist (fractions.Fraction), and single fma steps at values chosen to make the last rounding hard:
    acc + t*t a hair from a tie."""
    n = 0
    for x, c in chain_inputs():
        D = ref.dist_all(x, c)
        for i in range(len(x)):
            for a in range(len(c)):
                assert D[i, a].view(np.uint64) == np.float64(ref.dist(x[i], c[a])).view(np.uint64), (x[i], c[a])
                n += 1
    rng = np.random.default_rng(3)
    t = np.concatenate([rng.standard_normal(3000) * 2.0 ** rng.integers(-140, 120, 3000), [0.0, 2.0 ** -149, 1 + 2.0 ** -52, 1 + 2.0 ** -26, 3.0 * 2.0 ** 127]])
    acc = np.concatenate([np.abs(rng.standard_normal(3000)) * 2.0 ** rng.integers(-280, 250, 3000), [0.0, 1.0, 2.0 ** 53, 1.0, 0.0]])
    # ties: acc = 2^53 + 2 and t*t = 1 + 2^-51 + 2^-104 (t = 1 + 2^-52): the sum lies just above a half-way point
    t = np.concatenate([t, [1 + 2.0 ** -52, 1 + 2.0 ** -52, 1.0, 2.0 ** -27 + 1]]); acc = np.concatenate([acc, [2.0 ** 53 + 2, 2.0 ** 54, 2.0 ** 53, 2.0 ** 53]])
    got = ref.fma_sq_add(t, acc)
    for tv, av, g in zip(t.tolist(), acc.tolist(), got):
        want = ref.fma(tv, tv, av)
        assert np.float64(g).view(np.uint64) == np.float64(want).view(np.uint64), (tv, av)
        assert np.float64(harness.harness_fma_sq_add(tv, av)).view(np.uint64) == np.float64(want).view(np.uint64), (tv, av)
    assert n > 300


def test_the_distance_chain(harness):
    for x, c in chain_inputs():
        out = np.empty((len(x), len(c)))
        harness.harness_dist_all(_p(x), len(x), x.shape[1], _p(c), len(c), _p(out))
        assert np.array_equal(out.view(np.uint64), ref.dist_all(x, c).view(np.uint64))
    x = np.array([1.5, -2.0], np.float32)
    assert harness.harness_dist(_p(x), _p(x), 2) == 0.0 and math.copysign(1.0, harness.harness_dist(_p(x), _p(x), 2)) == 1.0     # +0.0


def test_the_quantiser_at_ties_at_negative_s_and_at_zero(harness):
    cases = []
    rng = np.random.default_rng(11)
    for M, n in ((1.0, 1), (1.0, 255), (0.999, 256), (3.0e38, 513), (3.4028235e38, 2 ** 31 - 1), (1e-45, 3), (2.0 ** 40, 1000), (0.0, 5), (0.5, 1), (2.0 ** -126, 2 ** 20)):
        s = ref.scale_bits(np.float32(M), n)
        assert harness.harness_scale_bits(np.float32(M), n) == s, (M, n)
        x = np.concatenate([(rng.uniform(-1, 1, 200) * M).astype(np.float32), np.array([M, -M, 0.0, -0.0, M / 2, M / 3], np.float32)])
        cases.append((x, s))
    assert ref.scale_bits(np.float32(0.0), 5) == 62 - 3 and ref.scale_bits(np.float32(3.0e38), 513) == 62 - 10 - 128 < 0 and ref.scale_bits(np.float32(1.0), 1) == 60
    # ties: with s small the scaled values fall on halves
    cases.append((np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5, 0.25, 0.75], np.float32), 0))
    cases.append((np.array([5.0, 6.0, 7.0, -5.0, 10.0, 12.0, 3.0, 1.0], np.float32), -1))
    cases.append((np.array([5.0, 6.0, 7.0, -6.0, 10.0, 12.0, 3.0, 2.0, 14.0], np.float32), -2))
    cases.append((np.array([3.0e38, -3.0e38, 1e30, 2.0 ** 77 * 3, 2.0 ** 76], np.float32), -77))
    for x, s in cases:
        out = np.empty(len(x), np.int64)
        harness.harness_quantise(_p(x), len(x), s, _p(out))
        assert out.tolist() == [ref.quantise(v, s) for v in x], s
    assert [ref.quantise(v, 0) for v in (0.5, 1.5, 2.5, -0.5, -2.5)] == [0, 2, 2, 0, -2] and [ref.quantise(v, -1) for v in (5.0, 7.0, -5.0, 1.0)] == [2, 4, -2, 0]
    # no overflow: n rows of the largest magnitude stay below 2^62
    for M, n in ((3.4028235e38, 2 ** 31 - 1), (1.0, 2 ** 31 - 1), (0.75, 4)):
        assert n * abs(ref.quantise(np.float32(M), ref.scale_bits(np.float32(M), n))) < 2 ** 62


def test_centre_from_sum_beyond_2_to_the_53(harness):
    rng = np.random.default_rng(12)
    cases = [(2 ** 53 + 1, 1, 40), (2 ** 53 + 3, 1, 40), (-(2 ** 53) - 1, 3, 40), (2 ** 61 + 2 ** 8 + 1, 7, 52), (2 ** 62 - 1, 2 ** 31 - 1, 30), (-(2 ** 62) + 1, 1, -70), (0, 5, 10),
             (1, 3, 200), (-1, 7, 209), (3 * 2 ** 60, 1, -66), (12345678901234567, 1000, 33)]
    for _ in range(400):
        cases.append((int(rng.integers(-2 ** 62 + 1, 2 ** 62 - 1)), int(rng.integers(1, 2 ** 31 - 1)), int(rng.integers(-90, 211))))
    for S, cnt, s in cases:
        want = ref.centre_from_sum(S, cnt, s)
        got = np.float32(harness.harness_centre_from_sum(S, cnt, s))
        assert got.view(np.uint32) == want.view(np.uint32), (S, cnt, s)
    assert float(2 ** 53 + 1) == 2.0 ** 53 and float(2 ** 53 + 3) == 2.0 ** 53 + 4                       # int -> binary64 is to nearest even


def test_the_draw(harness, algos_harness):
    for seed in (0, 1, 12345, 2 ** 64 - 1, 2 ** 63 + 17):
        assert ref.mix64(seed) == algos_harness.harness_mix64(seed)
        for r, k, c, n in ((0, 1, 0, 1), (0, 4, 1, 700), (2, 4, 3, 513), (9, 64, 63, 2 ** 31 - 1), (3, 64, 1, 300)):
            assert harness.harness_first_pick(seed, r, k, n) == ref.first_pick(seed, r, k, n)
            u = ref.draw(seed, r, k, c)
            assert harness.harness_draw(seed, r, k, c) == u and 0.0 <= u < 1.0


def test_the_blocked_walk_at_block_edges(harness):
    rng = np.random.default_rng(13)
    for n in (1, 255, 256, 257, 512, 513, 1000):
        v = rng.random(n) * 10.0 ** rng.integers(-3, 3, n)
        assert np.float64(harness.harness_blocked_sum(_p(v), n)).view(np.uint64) == np.float64(ref.blocked_sum(v)).view(np.uint64)
        bs = ref.block_sums(v)
        total = ref.sum_blocks(bs)
        run, edges = 0.0, []
        for b in bs:                                                                                  # targets at and next to every running block total
            run += b
            edges += [run, math.nextafter(run, 0.0), math.nextafter(run, math.inf)]
        for target in edges + [0.0, total, total * 0.5, float(v[0]), math.nextafter(float(v[0]), 0.0)] + list(rng.random(40) * total):
            assert harness.harness_walk(_p(v), n, target) == ref.walk(v, bs, target), (n, target)
        for u in (0.0, 0.5, 1.0 - 2.0 ** -53):
            assert harness.harness_pick(_p(v), n, u) == ref.pick(v, u)
    ones = np.ones(600)
    assert [ref.walk(ones, ref.block_sums(ones), t) for t in (0.5, 255.5, 256.5, 511.5, 599.5, 600.0)] == [0, 255, 256, 511, 599, -1]
    # no row exceeds the target: the greatest dmin, the least row among equals
    z = np.zeros(300)
    assert ref.pick(z, 0.7) == 0 and harness.harness_pick(_p(z), 300, 0.7) == 0
    tie = np.zeros(300); tie[[70, 280]] = 2.0 ** -1074                                                # u * total rounds to 0 or to total: with u = 0.75, to total
    assert ref.pick(tie, 0.75) == harness.harness_pick(_p(tie), 300, 0.75)


def accuracy_cases():
    rng = np.random.default_rng(14)
    yield np.array([0, 0, 1, 1, 2, 2], np.int32), np.array([1, 1, 0, 0, 2, 2], np.int32), 3                  # tied totals everywhere
    yield np.array([0, 0, 0, 1, 1, 1], np.int32), np.array([0, 1, 2, 0, 1, 2], np.int32), 3                  # tied counts inside a row, an empty cluster
    yield np.array([0, 1, 2, 3], np.int32), np.array([-1, -1, -1, -1], np.int32), 4                          # no ground label: NaN
    yield np.array([-1, -1, 1, 0], np.int32), np.array([0, 1, 1, -1], np.int32), 2                           # labelled regions the embedding lacks count below
    yield np.zeros(0, np.int32), np.zeros(0, np.int32), 1
    for k in (1, 2, 4, 7, 64):
        for n in (10, 200):
            a = rng.integers(-1, k, n).astype(np.int32); g = rng.integers(-1, k, n).astype(np.int32)
            yield a, g, k
            yield a, np.where(rng.random(n) < 0.7, a, g).astype(np.int32), k


def test_the_greedy_map_with_tied_totals_and_tied_counts(harness):
    for a, g, k in accuracy_cases():
        cnt = np.empty((k, k), np.int64); m = np.empty(k, np.int32); acc = C.c_double(-1)
        assert harness.harness_accuracy(_p(a), _p(g), len(a), k, _p(cnt), _p(m), C.byref(acc)) == 0
        want, wcnt, wmap = ref.clustering_accuracy(a, g, k)
        assert np.array_equal(cnt, wcnt) and np.array_equal(m, wmap), (a, g, k)
        assert (math.isnan(want) and math.isnan(acc.value)) or np.float64(acc.value).view(np.uint64) == np.float64(want).view(np.uint64)
    acc, _, m = ref.clustering_accuracy([0, 0, 1, 1, 2, 2], [1, 1, 0, 0, 2, 2], 3)
    assert acc == 1.0 and m.tolist() == [1, 0, 2]
    acc, _, m = ref.clustering_accuracy([0, 0, 0, 1, 1, 1], [0, 1, 2, 0, 1, 2], 3)
    assert m.tolist() == [1, 2, 0] and acc == 2 / 6                       # cluster 2 (no row) is visited first and takes label 2, cluster 1 then label 1, cluster 0 label 0
    assert ref.clustering_accuracy([-1, -1, 1, 0], [0, 1, 1, -1], 2)[0] == 1 / 3
    bad = np.array([0, 5], np.int32)
    assert harness.harness_accuracy(_p(bad), _p(bad), 2, 2, _p(np.empty((2, 2), np.int64)), _p(np.empty(2, np.int32)), C.byref(C.c_double())) == 1


def small_runs():
    rng = np.random.default_rng(15)
    X, _ = ref.blobs(257, 5, 4)
    yield "blobs", X, 4, dict(seed=12345, n_init=3)
    yield "one row", np.array([[2.5, -1.0]], np.float32), 1, dict(n_init=2)
    yield "k = n", rng.standard_normal((9, 3)).astype(np.float32), 9, dict(n_init=2)
    two = np.where(rng.random((300, 1)) < 0.5, np.float32(1.0), np.float32(-3.0)) * np.ones((1, 4), np.float32)
    yield "two distinct points", two, 4, dict(n_init=3, seed=7)
    yield "huge", (rng.standard_normal((130, 6)) * 8e37).astype(np.float32), 3, dict(n_init=2)
    yield "zeros", np.zeros((70, 3), np.float32), 2, dict(n_init=2)
    yield "max_iter 1", X, 5, dict(n_init=2, max_iter=1)
    yield "initial centres", X, 3, dict(init=X[[5, 100, 200]].copy(), n_init=7)


def test_a_whole_clustering_by_the_host_loop(harness):
    for name, X, k, kw in small_runs():
        want = ref.kmeans(X, k, **kw)
        got = harness_kmeans(harness, X, k, **kw)
        same_result(got, want)
        if name == "two distinct points":
            assert want["empty"] == 2 and want["inertia"] == 0.0
        if name == "huge":
            assert want["scale_bits"] < 0
        if name == "zeros":
            assert want["scale_bits"] == 62 - 7 and want["empty"] == 1 and (want["labels"] == 0).all()
        if name == "max_iter 1":
            assert want["iterations"] == 1 and want["total_iterations"] == 2
        if name == "initial centres":
            assert want["best_restart"] == 0 and want["total_iterations"] == want["iterations"]


def test_the_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "kmeans_rule_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    run = subprocess.run([exe, "12", "7"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert " wrong 0" in run.stdout and "rounds 12 " in run.stdout


def test_the_headers_fuse_only_where_they_say_so():
    rule = open(os.path.join(CSRC, "kmeans_rule.h")).read()
    code = "\n".join(l.split("//")[0] for l in rule.splitlines())
    assert code.count("fma(") == 1 and "return fma(t, t, acc);" in code
    hip = open(os.path.join(CSRC, "kmeans.hip")).read()
    hcode = "\n".join(l.split("//")[0] for l in hip.splitlines())
    for word in ("fma(", "atomicAdd(float", "atomicAdd(double", "unsafeAtomicAdd", "__fdividef", "__ddiv"):
        assert word not in hcode, word
    assert '#include "kmeans_rule.h"' in hip and "km_dist_step(" in hcode and "km_quantise(" in hcode and "km_centre_from_sum(" in hcode and "km_walk(" in hcode
    assert "-ffp-contract=off" in open(os.path.join(CSRC, "Makefile")).read()
