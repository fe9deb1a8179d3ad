"""The numpy reading of the per-slice pairwise evaluation's rule (include/dge.h: dge_pairwise_eval_vectors), steps 1-7, and the inputs its tests share
(tests/test_pairwise_ref.py, tests/test_pairwise_host.py on the CPU; tests/test_gpu_pairwise.py on the device).  Not a test module.

Every array operation below is one rounded binary64 operation per element in the order the rule writes it: numpy fuses nothing, its sqrt and divide are
correctly rounded, and the product of two widened float32 values is exact, so no Fraction is needed.  The estimated lists (step 5) are taken from
tests/knn_ref.py, which is exact on lattice features; everything else takes lists as an INPUT, so the scoring can be checked on any lists.
The means are summed by an explicit sequential loop, not np.sum (pairwise summation would be another rule)."""
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "poi_tract_counts.npy")
PAPER_KS = (5, 10, 20, 30, 40, 50, 60, 70)
FIXTURE_ZERO_ROWS = (361, 409, 472, 511, 557, 561, 562, 597, 655)


def fixture():
    """-> (region ids int64 [801], counts float32 [801 x 10]): miscs/POI_tract.pickle as tests/golden/make_poi_fixture.py stored it"""
    a = np.load(FIXTURE)
    return a[:, 0].astype(np.int64), a[:, 1:].astype(np.float32)


def discounts(kmax, start=2):
    """disc[i] = 1 / log2(i + 2) with the C library's log2 (math.log2, not numpy's); start: the sensitivity test's other offset"""
    with np.errstate(divide="ignore"):
        return np.array([np.float64(1.0) / np.float64(math.log2(i + start)) for i in range(kmax)], np.float64)


def ground_distances(gnd, present=None):
    """step 2 -> (dist float64 [n x n], live bool [n]); the diagonal holds dist(a, a), which nothing reads"""
    x = np.asarray(gnd, np.float32).astype(np.float64)
    n, g = x.shape
    with np.errstate(all="ignore"):
        ss = np.zeros(n)
        for j in range(g):
            ss = ss + x[:, j] * x[:, j]
        live = (ss > 0.0) & (ss < np.inf)
        if present is not None:
            live &= np.asarray(present) != 0
        dot = np.zeros((n, n))
        for j in range(g):
            dot = dot + np.outer(x[:, j], x[:, j])
        d = 1.0 - dot / np.sqrt(np.outer(ss, ss))
    d[~live, :] = 2.0
    d[:, ~live] = 2.0
    return d, live


def ground_order(d, ties="smaller", among=None):
    """step 3 -> (order int32 [n x (n - 1)]: the other regions of every region by (distance, region number); rank int32 [n x n]: rank[r, c], -1 at c = r).
    ties="larger" and among (a bool mask: only these columns can enter a list) exist for the sensitivity tests alone."""
    n = len(d)
    key = d.copy()
    np.fill_diagonal(key, np.inf)
    if among is not None:
        key[:, ~np.asarray(among, bool)] = np.inf
    if ties == "smaller":
        order = np.argsort(key, axis=1, kind="stable")
    else:
        order = (n - 1 - np.argsort(key[:, ::-1], axis=1, kind="stable"))
    order = order[:, :n - 1].astype(np.int32)                    # the diagonal's +inf sorts last (a real distance is finite)
    rank = np.full((n, n), -1, np.int32)
    np.put_along_axis(rank, order, np.arange(n - 1, dtype=np.int32)[None, :].repeat(n, 0), 1)
    return order, rank


def chain(dist_lists, disc, ks):
    """step 6's chain over lists of distances [m x kmax] -> [n_k x m]: acc = acc + (1 - d_i) * disc[i], cut after i = k - 1"""
    acc = np.zeros(len(dist_lists))
    out = np.zeros((len(ks), len(dist_lists)))
    with np.errstate(all="ignore"):
        for i in range(dist_lists.shape[1]):
            acc = acc + (1.0 - dist_lists[:, i]) * disc[i]
            for j, k in enumerate(ks):
                if i == k - 1:
                    out[j] = acc
    return out


def estimated_lists(features, row_of, present, kmax):
    """steps 1 and 5 on the host: -> (lists int32 [n_sets x n x kmax], -1 rows for non-members; member bool [n_sets x n]).  Exact where tests/knn_ref.py is:
    on lattice features."""
    import knn_ref
    f = np.asarray(features, np.float32)
    row_of = np.asarray(row_of, np.int64)
    n_sets, n = row_of.shape
    pres = np.ones(len(f), bool) if present is None else np.asarray(present) != 0
    member = (row_of >= 0) & pres[np.clip(row_of, 0, None)]
    lists = np.full((n_sets, n, kmax), -1, np.int32)
    for s in range(n_sets):
        regions = np.flatnonzero(member[s])
        if len(regions) < kmax + 1:
            raise ValueError("set %d has %d members" % (s, len(regions)))
        idx, _ = knn_ref.reference_lists(f[row_of[s, regions]], kmax)
        lists[s, regions] = regions[idx]
    return lists, member


def evaluate(gnd, lists, test=None, ks=PAPER_KS, rel_m=0, gnd_present=None, ties="smaller", ideal_over="all", disc_start=2):
    """steps 2-4, 6, 7 on given lists [n_sets x n x kmax] (a row of -1: no member) -> dict(ndcg, precision [n_sets x n_k], members, tested [n_sets], coverage,
    ratio float64, hits int32 [n_sets x n_k x n], ideal [n_k x n], ideal_idx [n x kmax]).  ideal_over="members": the sensitivity test's other reading (the
    ideal list of a set taken over its members only; `ideal` is then the last set's)."""
    lists = np.asarray(lists, np.int32)
    n_sets, n, kmax = lists.shape
    ks = [int(k) for k in ks]
    assert kmax == ks[-1] and all(a < b for a, b in zip(ks, ks[1:]))
    d, _ = ground_distances(gnd, gnd_present)
    disc = discounts(kmax, disc_start)
    order, rank = ground_order(d, ties)
    ideal = chain(np.take_along_axis(d, order[:, :kmax], 1), disc, ks)
    member = lists[:, :, 0] >= 0
    tested_mask = member if test is None else member & (np.asarray(test) != 0)[None, :]
    ratio = np.zeros((n_sets, len(ks), n)); hits = np.zeros((n_sets, len(ks), n), np.int32)
    ndcg = np.zeros((n_sets, len(ks))); precision = np.zeros((n_sets, len(ks)))
    for s in range(n_sets):
        if ideal_over == "members":
            o, _ = ground_order(d, ties, among=member[s])
            ideal = chain(np.take_along_axis(d, o[:, :kmax], 1), disc, ks)
        rows = np.flatnonzero(tested_mask[s])
        nb = lists[s, rows]
        dcg = chain(d[rows[:, None], nb], disc, ks)
        with np.errstate(all="ignore"):
            ratio[s][:, rows] = np.where(ideal[:, rows] != 0.0, dcg / ideal[:, rows], 0.0)
        if rel_m:
            hit = rank[rows[:, None], nb] < rel_m
            for j, k in enumerate(ks):
                hits[s, j, rows] = hit[:, :k].sum(axis=1)
        for j, k in enumerate(ks):
            acc = 0.0
            for r in rows:                                        # the rule's plain ascending sum
                acc = acc + float(ratio[s, j, r])
            ndcg[s, j] = acc / len(rows) if len(rows) else 0.0
            precision[s, j] = int(hits[s, j, rows].sum()) / (k * len(rows)) if len(rows) else 0.0
    return dict(ndcg=ndcg, precision=precision if rel_m else None, members=member.sum(axis=1).astype(np.int64), tested=tested_mask.sum(axis=1).astype(np.int64),
                coverage=member.sum(axis=1) / float(n), ratio=ratio, hits=hits, ideal=ideal, ideal_idx=order[:, :kmax], dist=d, rank=rank)


def ground_lists(gnd, m, gnd_present=None):
    """what dge_pairwise_ground_vectors returns: -> (idx int32 [n x m], dist float64 [n x m])"""
    d, _ = ground_distances(gnd, gnd_present)
    order, _ = ground_order(d)
    return order[:, :m], np.take_along_axis(d, order[:, :m], 1)


# ---- the inputs of the device tests
def small_case(n=130, g=10, D=20, kmax=70, seed=11):
    """n regions of small integer counts with planted zero rows and proportional rows; lattice features (tests/knn_ref.py) so that the estimated lists are exact;
    three sets: all regions, about 70 % of them, exactly kmax + 1 members; test = the members of both of the first two (:324).
    -> dict(gnd, features [V x D], present [V], row_of [3 x n], test [n])"""
    import knn_ref
    rng = np.random.default_rng(seed)
    gnd = rng.integers(0, 6, (n, g)).astype(np.float32)
    gnd[[3, 64, 129]] = 0.0                                       # zero vectors: one in each 64-row strip
    gnd[7] = 2 * gnd[5]; gnd[70] = 3 * gnd[5]; gnd[128] = gnd[5]  # proportional rows and a duplicate: distances that tie, on both sides of 0
    gnd[20] = gnd[21]
    sets = [np.arange(n), np.sort(rng.choice(n, int(0.7 * n), replace=False)), np.sort(rng.choice(n, kmax + 1, replace=False))]
    V = sum(len(s) for s in sets) + 5
    features = knn_ref.lattice(V, D, seed=seed + 1)
    rows = rng.permutation(V)
    row_of = np.full((3, n), -1, np.int64)
    at = 0
    for s, regions in enumerate(sets):
        row_of[s, regions] = rows[at:at + len(regions)]
        at += len(regions)
    present = np.ones(V, bool)
    test = ((row_of[0] >= 0) & (row_of[1] >= 0)).astype(np.uint8)
    return dict(gnd=gnd, features=features, present=present, row_of=row_of, test=test)


def fixture_case(n_sets=8, D=20, seed=5):
    """the fixture at full size: set s drops every region whose number is = s (mod 9); the sets' rows are shuffled into one table of V = n_sets x 801 rows"""
    import knn_ref
    _, gnd = fixture()
    n = len(gnd)
    rng = np.random.default_rng(seed)
    V = n_sets * n
    features = knn_ref.lattice(V, D, seed=seed + 1)
    rows = rng.permutation(V)
    row_of = np.full((n_sets, n), -1, np.int64)
    for s in range(n_sets):
        keep = np.arange(n) % 9 != s
        row_of[s, keep] = rows[s * n:(s + 1) * n][keep]
    return dict(gnd=gnd, features=features, row_of=row_of)
