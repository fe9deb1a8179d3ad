"""CPU: embedding_amd/csrc/line_rule.h — what every lane of line.hip runs — built for the host (tests/native/line_rule_harness.cpp, -ffp-contract=off) and held to
the rule of include/dge.h: every piece equal to tests/line_ref.py at its edges, and whole runs — a one-thread loop over those pieces with std::fma — equal to the
reference as bits.  The stand-alone build of the harness runs clean under the address and undefined-behaviour sanitizers.  The host loop alone learns the
three-block graph, which the GPU learning test relies on."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import line_ref as ref  # noqa: E402
import spatial_ref  # noqa: E402
from line_harness import FLAGS, SRC, _p, harness_line, load_harness  # noqa: E402

CSRC = os.path.join(ROOT, "embedding_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return load_harness(os.path.join(str(tmp_path_factory.mktemp("line_rule_harness")), "libline_rule_harness.so"))


def bits(x):
    return np.float64(x).view(np.uint64)


def test_the_sigmoid_table_and_its_look_up(harness):
    T = ref.sig_table()
    for k in range(ref.SIG_N):
        assert bits(harness.harness_line_sig_entry(k)) == bits(T[k])
    assert T[0] == spatial_ref.E(-6.0) / (1.0 + spatial_ref.E(-6.0)) and T[500] == 0.5 and (np.diff(T) > 0).all() and 0 < T[0] < T[-1] < 1
    x = np.arange(ref.SIG_N) * 12.0 / 1000.0 - 6.0
    assert np.abs(T - 1.0 / (1.0 + np.exp(-x))).max() < 2.0 ** -50          # E is within an ulp of exp
    up, down = np.nextafter(6.0, 7.0), np.nextafter(-6.0, -7.0)
    for f, want in ((6.0, T[999]), (up, 1.0), (-6.0, T[0]), (down, 0.0), (np.nextafter(6.0, 0.0), T[999]), (5.99, T[999]), (5.98, T[998]),
                    (0.0, T[500]), (-0.0, T[500]), (np.nextafter(0.0, -1.0), T[500]), (-0.001, T[499]), (1e300, 1.0), (-1e300, 0.0), (np.inf, 1.0), (-np.inf, 0.0)):
        got = harness.harness_line_sig(f)
        assert bits(got) == bits(want) == bits(ref.sig(f)), (f, got, want)
    for f in (5.988, np.nextafter(5.988, 0.0), np.nextafter(5.988, 6.0), -5.988, 0.012, np.nextafter(0.012, 0.0)):      # a step of the table, in Python's own floats
        assert bits(harness.harness_line_sig(f)) == bits(T[min(999, int(((float(f) + 6.0) * 1000.0) / 12.0))])
    # f = 6 lands on k = 1000: the clamp to 999
    assert int(((6.0 + 6.0) * 1000.0) / 12.0) == 1000
    rng = np.random.default_rng(1)
    f = rng.uniform(-6.5, 6.5, 2000)
    assert np.array_equal(np.array([harness.harness_line_sig(x) for x in f]).view(np.uint64), ref.sig(f).view(np.uint64))


def test_rho_of_a_batch(harness):
    for rho0, first, samples in ((0.025, 0, 1000), (0.025, 960, 1000), (0.025, 999, 1000), (1.0, 0, 1), (0.025, (1 << 40) - 65536, 1 << 40), (0.025, 10 ** 7 - 1, 10 ** 7),
                                 (0.3, 99990, 100000), (0.3, 99989, 100000)):
        assert bits(harness.harness_line_rho(rho0, first, samples)) == bits(ref.rho_b(rho0, first, samples))
    # the floor: below rho0 * 0.0001 it is rho0 * 0.0001
    assert ref.rho_b(0.025, 10 ** 7 - 1, 10 ** 7) == 0.025 * 0.0001 and ref.rho_b(0.3, 99989, 100000) > 0.3 * 0.0001
    assert ref.rho_b(0.025, 0, 1000) == 0.025


def test_both_searches_at_their_edges(harness):
    w = np.array([3, 1, 1, 7, 2], np.int64)
    Cs = np.cumsum(w); total = int(Cs[-1])
    for e in range(len(w)):
        for r, want in ((int(Cs[e]) - 1, e), (int(Cs[e]), e + 1 if e + 1 < len(w) else 0)):      # a draw equal to C[e] - 1 is edge e, equal to C[e] the next (W wraps to 0)
            for lift in (0, total, total * 1000003):
                got = harness.harness_line_search(_p(Cs), len(Cs), r + lift, total)
                assert got == want == ref.search(Cs, r + lift, total), (e, r, lift, got)
    big = (1 << 64) - 1
    assert harness.harness_line_search(_p(Cs), len(Cs), big, total) == ref.search(Cs, big, total)
    # a nw of 0: the vertex is never the least v with NC[v] > r
    nw = np.array([0, 5, 0, 0, 2, 0], np.int64)
    NC = np.cumsum(nw); N = int(NC[-1])
    hit = {harness.harness_line_search(_p(NC), len(NC), r, N) for r in range(3 * N)}
    assert hit == {1, 4} and all(harness.harness_line_search(_p(NC), len(NC), r, N) == ref.search(NC, r, N) for r in range(3 * N))
    one = np.array([9], np.int64)
    assert harness.harness_line_search(_p(one), 1, 12345, 9) == 0
    for d in (0, 1, 2, 16, 81, 10 ** 6, (1 << 31) - 1, (1 << 40) - 1):
        assert harness.harness_line_neg_weight(d) == ref.neg_weight(d), d
    assert ref.neg_weight(0) == 0 and ref.neg_weight(1) == 1024 and ref.neg_weight(16) == 8 * 1024 and ref.neg_weight(81) == 27 * 1024


def test_init_cells_draws_and_quantised_terms(harness):
    for seed in (0, 1, 12345, (1 << 64) - 1):
        s2 = ref.seed2(seed)
        assert harness.harness_line_seed2(seed) == s2
        for t, dim in ((0, 1), (1, 20), (10 ** 9, 256), ((1 << 64) - 3, 16)):
            assert harness.harness_line_u(s2, t) == ref.u(s2, t)
            assert harness.harness_line_init_cell(s2, t, dim) == ref.init_cell(s2, t, dim)
            assert abs(ref.init_cell(s2, t, dim)) <= (1 << 31) // dim
        for s, d in ((0, 0), (5, 3), (1 << 40, 32)):
            assert harness.harness_line_draw(seed, s, d) == ref.mix64((seed + 64 * s + d) & ref.MASK)
    tab = ref.init_table(7, 20, 12345)
    s2 = ref.seed2(12345)
    assert all(int(tab[v, j]) == ref.init_cell(s2, v * 20 + j, 20) for v in range(7) for j in range(20))
    # ties in rint go to even
    for x, want in ((0.5 * 2.0 ** -32, 0), (1.5 * 2.0 ** -32, 2), (2.5 * 2.0 ** -32, 2), (-0.5 * 2.0 ** -32, 0), (-1.5 * 2.0 ** -32, -2), (-2.5 * 2.0 ** -32, -2), (255.9, int(np.rint(255.9 * 2.0 ** 32))),
                    (1.0, 1 << 32), (-1.0, -(1 << 32))):
        assert harness.harness_line_quant(x) == want == ref.quant(x), x
    assert harness.harness_line_term(0.5, 3.0 * 2.0 ** -32) == 2 and harness.harness_line_term(0.5, 5.0 * 2.0 ** -32) == 2 and harness.harness_line_term(-0.5, 3.0 * 2.0 ** -32) == -2
    rng = np.random.default_rng(2)
    g = rng.uniform(-1, 1, 500) * 10.0 ** rng.integers(-6, 0, 500); x = rng.uniform(-2, 2, 500)
    assert [harness.harness_line_term(float(a), float(b)) for a, b in zip(g, x)] == ref.term(g, x).tolist()
    for P in (0, 1, -1, (1 << 40) - 1, -(1 << 40) + 1, 123456789012):
        assert harness.harness_line_value(P) == float(P) * ref.UNFIX and ref.quant(harness.harness_line_value(P)) == P         # exact both ways


@pytest.mark.parametrize("dim", [1, 15, 16, 17, 20, 33, 64, 65, 128, 256])
def test_the_dot_is_the_segment_sum(harness, dim):
    rng = np.random.default_rng(dim)
    a = rng.uniform(-1, 1, dim) * 10.0 ** rng.integers(-6, 3, dim); b = rng.uniform(-1, 1, dim)
    p = [0.0] * ref.LANES
    for j in range(dim):
        p[j % ref.LANES] = ref.fma(a[j], b[j], p[j % ref.LANES])
    s = ref.LANES // 2
    while s:
        for l in range(s):
            p[l] = p[l] + p[l + s]
        s //= 2
    assert bits(harness.harness_line_dot(_p(a), _p(b), dim)) == bits(p[0]) == bits(ref.dot(a, b))


def _same(got, want):
    assert ref.same_bits(got["X"], want["X"]) and ref.same_bits(got["Y"], want["Y"]) and np.array_equal(got["touched"], want["touched"])
    for f in ("vertices", "entries", "zeros", "batches", "samples", "total_weight", "neg_total", "max_abs"):
        assert got[f] == want[f], f


def small_graphs():
    s, d, w = ref.random_graph(40, 300, 3)
    keep = (s < 38) & (d < 38)
    mixed = (np.concatenate([s[keep], [0, 5, 9]]).astype(np.int32), np.concatenate([d[keep], [38, 38, 38]]).astype(np.int32), np.concatenate([w[keep], [2.0, 7.0, 0.0]]), 40)
    hub = (np.array([i for i in range(40) if i != 3], np.int32), np.full(39, 3, np.int32), (1.0 + (np.arange(39) * 7) % 13).astype(np.float64), 40)
    loop = (np.array([0], np.int32), np.array([0], np.int32), np.array([5.0]), 1)
    return dict(mixed=mixed, hub=hub, loop=loop)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("graph,dim,K,batch,samples", [("mixed", 20, 5, 256, 1999), ("mixed", 17, 32, 7, 500), ("mixed", 1, 0, 1, 301), ("mixed", 65, 1, 7, 300), ("hub", 20, 5, 256, 1999),
                                                       ("hub", 128, 5, 256, 700), ("loop", 20, 5, 7, 50), ("loop", 1, 0, 1, 9), ("mixed", 256, 32, 256, 600)])
def test_the_whole_loop_equals_the_reference(harness, graph, dim, K, batch, samples, order):
    s, d, w, n = small_graphs()[graph]
    kw = dict(dim=dim, order=order, negative=K, samples=samples, batch=batch, rho0=0.025, seed=12345)
    want = ref.line(s, d, w, n, **kw)
    _same(harness_line(harness, s, d, w, n, **kw), want)
    if graph == "mixed":
        assert want["zeros"] == 1 and want["touched"][38] and not want["touched"][39]
        assert ref.same_bits(want["X"][39], ref.init_table(n, dim, 12345)[39].astype(np.float64) * ref.UNFIX)
    if order == 1:
        assert not want["Y"].any()


def test_supplied_tables_and_the_bound(harness):
    s, d, w, n = small_graphs()["mixed"]
    kw = dict(dim=8, order=2, negative=3, samples=400, batch=64, rho0=0.05, seed=4)
    x0 = np.random.default_rng(1).uniform(-0.3, 0.3, (n, 8)); y0 = np.random.default_rng(2).uniform(-0.3, 0.3, (n, 8))
    _same(harness_line(harness, s, d, w, n, init=x0, **kw), ref.line(s, d, w, n, init=x0, **kw))
    _same(harness_line(harness, s, d, w, n, init=(x0, y0), **kw), ref.line(s, d, w, n, init=(x0, y0), **kw))
    hot = np.full((n, 4), 255.9)
    for order, init in ((1, hot), (2, (hot, hot))):
        kw = dict(dim=4, order=order, negative=2, samples=50, batch=1, rho0=1.0, seed=3)
        with pytest.raises(ref.BoundLeft) as a:
            ref.line(s, d, w, n, init=init, **kw)
        with pytest.raises(ref.BoundLeft) as b:
            harness_line(harness, s, d, w, n, init=init, **kw)
        assert a.value.batch == b.value.batch >= 1


@pytest.mark.parametrize("order", [1, 2])
def test_the_host_loop_alone_learns_the_three_blocks(harness, order):
    """all 5 cosine neighbours of all 36 vertices lie inside the vertex's block (float64 cosines on the host; the GPU test takes them from dge_knn_cosine_vectors)"""
    s, d, w, n = ref.three_blocks()
    r = harness_line(harness, s, d, w, n, dim=16, order=order, negative=5, samples=20000, batch=256, rho0=0.025, seed=1)
    assert n == 36 and r["touched"].all() and r["max_abs"] < 4
    X = r["X"] / np.linalg.norm(r["X"], axis=1, keepdims=True)
    S = X @ X.T
    np.fill_diagonal(S, -9.0)
    nb = np.argsort(-S, axis=1)[:, :5]
    assert ((nb // 12) == (np.arange(n) // 12)[:, None]).all()


def test_the_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "line_rule_harness")
    subprocess.check_call(["g++", "-O1", "-g"] + FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DLINE_HARNESS_MAIN", "-o", exe, SRC])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert "line_rule_harness ok" in run.stdout


def test_the_sources_fuse_only_where_they_say_so():
    hip = open(os.path.join(CSRC, "line.hip")).read()
    hcode = "\n".join(l.split("//")[0] for l in hip.splitlines())
    for word in ("atomicAdd(float", "atomicAdd(double", "atomicAdd((float", "atomicAdd((double", "unsafeAtomicAdd", "__fdividef", "__ddiv", "hipLaunchCooperativeKernel", "cooperative_groups"):
        assert word not in hcode, word
    assert '#include "line_rule.h"' in hip
    for piece in ("line_value(", "line_search(", "line_draw(", "line_rho(", "line_sig(", "line_sig_entry(", "nmf_seg_step(", "line_term(", "line_init_cell(", "line_neg_weight(", "line_cell_over("):
        assert piece in hcode, piece
    assert "-ffp-contract=off" in open(os.path.join(CSRC, "Makefile")).read()
