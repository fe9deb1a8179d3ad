"""CPU: the numpy reading of the pairwise evaluation's rule (tests/pairwise_ref.py) is sound — equal, bit for bit, to a plain scalar-loop reading of
include/dge.h on 12 ground rows that hold a zero row, a NaN row, proportional rows and duplicate rows — and sensitive: its result on the POI fixture changes if
ties go to the larger region number, if the ideal list is taken over the members only, or if the discounts start at log2(i + 1)."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pairwise_ref as ref  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def scalar_reading(gnd, lists, test, ks, rel_m):
    """steps 2-7 one Python float at a time"""
    n, g = gnd.shape
    x = [[float(v) for v in row] for row in gnd]
    ss = []
    for a in range(n):
        acc = 0.0
        for j in range(g):
            acc = acc + x[a][j] * x[a][j]
        ss.append(acc)
    zero = [not (0.0 < s < math.inf) for s in ss]

    def dist(a, b):
        if zero[a] or zero[b]:
            return 2.0
        acc = 0.0
        for j in range(g):
            acc = acc + x[a][j] * x[b][j]
        return 1.0 - acc / math.sqrt(ss[a] * ss[b])

    kmax = ks[-1]
    disc = [1.0 / math.log2(i + 2) for i in range(kmax)]
    order = [sorted((c for c in range(n) if c != r), key=lambda c: (dist(r, c), c)) for r in range(n)]
    rank = [{c: i for i, c in enumerate(o)} for o in order]

    def chain(r, nbs):
        acc, out = 0.0, []
        for i, c in enumerate(nbs):
            acc = acc + (1.0 - dist(r, c)) * disc[i]
            if i + 1 in ks:
                out.append(acc)
        return out

    n_sets = len(lists)
    ratio = np.zeros((n_sets, len(ks), n)); hits = np.zeros((n_sets, len(ks), n), np.int32)
    ndcg = np.zeros((n_sets, len(ks))); precision = np.zeros((n_sets, len(ks))); tested = []
    for s in range(n_sets):
        rows = [r for r in range(n) if lists[s][r][0] >= 0 and (test is None or test[r])]
        tested.append(len(rows))
        for r in rows:
            nbs = [int(c) for c in lists[s][r]]
            dcg, ideal = chain(r, nbs), chain(r, order[r][:kmax])
            for j, k in enumerate(ks):
                ratio[s, j, r] = dcg[j] / ideal[j] if ideal[j] != 0.0 else 0.0
                hits[s, j, r] = sum(1 for c in nbs[:k] if rank[r][c] < rel_m)
        for j, k in enumerate(ks):
            acc = 0.0
            for r in rows:
                acc = acc + float(ratio[s, j, r])
            ndcg[s, j] = acc / len(rows) if rows else 0.0
            precision[s, j] = int(sum(int(hits[s, j, r]) for r in rows)) / (k * len(rows)) if rows else 0.0
    return dict(ndcg=ndcg, precision=precision, ratio=ratio, hits=hits, tested=tested)


def test_sound_equal_to_a_scalar_loop_reading():
    rng = np.random.default_rng(4)
    gnd = rng.integers(0, 5, (12, 4)).astype(np.float32)
    gnd[2] = 0.0                                     # a zero row
    gnd[5, 1] = np.nan                               # a NaN row: a zero vector by rule
    gnd[7] = 3 * gnd[6]; gnd[8] = 0.5 * gnd[6]       # proportional rows
    gnd[10] = gnd[9]; gnd[11] = gnd[9]               # duplicate rows
    gnd[0] = [0.1, 0.7, 1.3, 2.9]; gnd[1] = [1e-20, 3e19, -2.5, 7.0]           # and entries whose sums round
    ks = (1, 2, 5)
    lists = np.full((2, 12, 5), -1, np.int32)
    for r in range(12):
        lists[0, r] = rng.permutation(np.delete(np.arange(12), r))[:5]
        if r % 3:
            lists[1, r] = rng.permutation(np.delete(np.arange(12), r))[:5]
    test = np.ones(12, np.uint8); test[4] = 0
    for rel_m in (1, 4, 11):
        got = ref.evaluate(gnd, lists, test, ks, rel_m)
        want = scalar_reading(gnd, lists, test, ks, rel_m)
        for key in ("ndcg", "precision", "ratio"):
            assert np.array_equal(bits(got[key]), bits(want[key])), (rel_m, key)
        assert np.array_equal(got["hits"], want["hits"]) and got["tested"].tolist() == want["tested"] == [11, 7]
    assert (got["ratio"][0][:, [2, 5]] == 1.0).all() and (got["ratio"][:, :, 4] == 0.0).all()


def test_sensitive_to_the_tie_rule_the_ideal_lists_coverage_and_the_discounts():
    c = ref.fixture_case(n_sets=2)
    lists, member = ref.estimated_lists(c["features"], c["row_of"], None, 70)
    assert member.sum(axis=1).tolist() == [712, 712]
    base = ref.evaluate(c["gnd"], lists, None, ref.PAPER_KS, 300)
    again = ref.evaluate(c["gnd"], lists, None, ref.PAPER_KS, 300)
    assert np.array_equal(bits(base["ndcg"]), bits(again["ndcg"])) and np.isfinite(base["ndcg"]).all() and (base["ndcg"] > 0).all()
    # equal distances give equal gains, so the tie rule cannot move nDCG: it decides who is among the nearest 300 (24 rows tie exactly at 70 / 71 as well, which
    # changes the ideal LIST, not its DCG) — the hits and the precision are where it shows
    ties = ref.evaluate(c["gnd"], lists, None, ref.PAPER_KS, 300, ties="larger")
    assert np.array_equal(bits(ties["ndcg"]), bits(base["ndcg"])) and not np.array_equal(ties["ideal_idx"], base["ideal_idx"])
    assert not np.array_equal(ties["hits"], base["hits"]) and not np.array_equal(bits(ties["precision"]), bits(base["precision"]))
    for what, kw in (("ideal list over the members only", dict(ideal_over="members")), ("discounts from log2(i + 1)", dict(disc_start=1))):
        other = ref.evaluate(c["gnd"], lists, None, ref.PAPER_KS, 300, **kw)
        assert not np.array_equal(bits(other["ndcg"]), bits(base["ndcg"])), what
    # the fixture needs nothing planted: zero vectors and exact ties are in the data
    ids, gnd = ref.fixture()
    assert gnd.shape == (801, 10) and len(set(ids.tolist())) == 801
    assert np.flatnonzero((gnd == 0).all(axis=1)).tolist() == list(ref.FIXTURE_ZERO_ROWS)
