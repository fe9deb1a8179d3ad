"""CPU: embedding_amd/csrc/nmf_rule.h — what every lane of nmf.hip runs — built for the host (tests/native/nmf_rule_harness.cpp, -ffp-contract=off) and held to
the rule of include/dge.h: every piece bit for bit equal to tests/nmf_ref.py, and whole factorisations — a one-thread loop over those pieces with std::fma —
equal to the reference as bits.  The stand-alone build of the harness runs clean under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nmf_ref as ref  # noqa: E402
from nmf_harness import FLAGS, SRC, _p, harness_nmf, load_harness  # noqa: E402

CSRC = os.path.join(ROOT, "embedding_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return load_harness(os.path.join(str(tmp_path_factory.mktemp("nmf_rule_harness")), "libnmf_rule_harness.so"))


def bits(x):
    return np.float64(x).view(np.uint64)


def test_the_pieces(harness):
    rng = np.random.default_rng(5)
    for seed, t in ((1, 0), (1, 1), (12345, 10 ** 9), ((1 << 64) - 1, 5), (7, (1 << 64) - 3)):
        assert harness.harness_nmf_u(seed, t) == ref.u(seed, t) and 0.0 <= ref.u(seed, t) < 1.0
    for x in (0.0, ref.EPS, np.nextafter(ref.EPS, 0.0), np.nextafter(ref.EPS, 1.0), 1e-300, 3.5, 5e-324):
        assert bits(harness.harness_nmf_floor(x)) == bits(ref.floor_eps(np.float64(x)))
    for _ in range(200):
        x, num, den = (float(v) for v in rng.random(3) * 10.0 ** rng.integers(-20, 20, 3))
        assert bits(harness.harness_nmf_update(x, num, den)) == bits(ref.floor_eps(np.float64(x) * (np.float64(num) / np.float64(den))))
        a, b, c = (float(v) for v in (rng.random(3) - 0.3) * 10.0 ** rng.integers(-8, 8, 3))
        assert bits(harness.harness_nmf_fma(a, b, c)) == bits(ref.fma(a, b, c))
    assert harness.harness_nmf_update(2.0, 0.0, 3.0) == ref.EPS                   # an empty segment: the floor


@pytest.mark.parametrize("count", [0, 1, 15, 16, 17, 31, 32, 33, 700])
def test_segment_sum_and_blocked_sum(harness, count):
    rng = np.random.default_rng(count)
    a = rng.random(count) * 10.0 ** rng.integers(-6, 6, count); b = rng.random(count) * 50
    p = [0.0] * ref.LANES
    for t in range(count):
        p[t % ref.LANES] = ref.fma(a[t], b[t], p[t % ref.LANES])
    s = ref.LANES // 2
    while s:
        for l in range(s):
            p[l] = p[l] + p[l + s]
        s //= 2
    assert bits(harness.harness_nmf_segment_sum(_p(a), _p(b), count)) == bits(p[0])
    got = ref.segment_sums(np.zeros(count, np.int64), np.arange(count), a[:, None], b, 1)
    assert bits(got[0, 0]) == bits(p[0])
    assert bits(harness.harness_nmf_blocked_sum(_p(a), count)) == bits(ref.blocked_sum(a))
    if count:
        assert bits(ref.blocked_sum_rows(a[:, None])[0]) == bits(ref.blocked_sum(a))


def _same(got, want):
    assert ref.same_bits(got["W"], want["W"]) and ref.same_bits(got["H"], want["H"])
    for f in ("vmax", "entries", "zeros", "rows", "cols", "iterations"):
        assert got[f] == want[f], f


@pytest.mark.parametrize("update", [ref.DIVERGENCE, ref.EUCLIDEAN])
def test_a_small_factorisation_equals_the_reference_on_exact_fma(harness, update):
    r, c, v = ref.random_sparse(60, 45, 0.08, 3, hub=(5, 9))
    v[::17] = 0.0                                                                  # dropped, counted
    kw = dict(rank=3, max_iter=3, update=update, seed=12345)
    want = ref.nmf(r, c, v, (60, 45), exact=True, **kw)
    assert want["zeros"] == len(v[::17])
    _same(harness_nmf(harness, r, c, v, (60, 45), **kw), want)
    _same(ref.nmf(r, c, v, (60, 45), exact=False, **kw), want)                     # the numpy form of the reference, whole
    init = (np.abs(np.random.default_rng(1).standard_normal((60, 3))), np.random.default_rng(2).random((3, 45)))
    init[0][4] = 0.0                                                               # below the floor
    _same(harness_nmf(harness, r, c, v, (60, 45), init=init, **kw), ref.nmf(r, c, v, (60, 45), init=init, exact=True, **kw))


@pytest.mark.parametrize("update", [ref.DIVERGENCE, ref.EUCLIDEAN])
def test_a_large_factorisation_equals_the_numpy_form(harness, update):
    r, c, v = ref.random_sparse(5000, 5000, 0.008, 11, hub=(17, 4000))            # about 2e5 entries
    assert 1.9e5 < len(v) < 2.2e5
    kw = dict(rank=10, max_iter=30, update=update, seed=1)
    _same(harness_nmf(harness, r, c, v, (5000, 5000), **kw), ref.nmf(r, c, v, (5000, 5000), **kw))


def test_tiny_values_sit_on_the_floor(harness):
    r, c, v = ref.random_sparse(20, 30, 0.2, 8)
    v = v * 1e-300
    for update in (ref.DIVERGENCE, ref.EUCLIDEAN):
        want = ref.nmf(r, c, v, (20, 30), rank=4, max_iter=2, update=update, seed=3, exact=True)
        assert want["vmax"] == v.max() and (want["W"] >= ref.EPS).all() and (want["H"] >= ref.EPS).all()
        _same(harness_nmf(harness, r, c, v, (20, 30), rank=4, max_iter=2, update=update, seed=3), want)


def test_the_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "nmf_rule_harness")
    subprocess.check_call(["g++", "-O1", "-g"] + FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DNMF_HARNESS_MAIN", "-o", exe, SRC])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert "nmf_rule_harness ok" in run.stdout


def test_the_sources_fuse_only_where_they_say_so():
    hip = open(os.path.join(CSRC, "nmf.hip")).read()
    hcode = "\n".join(l.split("//")[0] for l in hip.splitlines())
    for word in ("atomicAdd(float", "atomicAdd(double", "unsafeAtomicAdd", "__fdividef", "__ddiv", "__shared__"):
        assert word not in hcode, word
    assert '#include "nmf_rule.h"' in hip
    for piece in ("nmf_p(", "nmf_seg_step(", "nmf_update(", "nmf_init(", "nmf_block_sum(", "nmf_block_dot(", "nmf_sum_blocks("):
        assert piece in hcode, piece
    assert "-ffp-contract=off" in open(os.path.join(CSRC, "Makefile")).read()
