"""GPU: dge_pairwise_eval_vectors / dge_pairwise_ground_vectors (csrc/pairwise.hip) against the numpy reading of the rule, tests/pairwise_ref.py.
EXACT equality everywhere — binary64 values compared as bits, nothing excused.

  - n = 130 regions (two 64-row strips and a ragged third; three column tiles with a tail), g = 10 small integer counts with planted zero, proportional and
    duplicate rows, D = 20 lattice features (tests/knn_ref.py: the estimated lists are exact), three sets (all regions, about 70 %, exactly kmax + 1
    members), test = the members of both of the first two, ks = (1, 5, 20, 70), rel_m in {1, 30, n - 1}: every output array equals the reference, and the
    lists equal dge_knn_cosine on the stacked members mapped back (its first 64 columns: the public entry stops at k = 64; columns 64 .. 69 are pinned by
    tests/knn_ref.py, which is exact on lattice features, through the comparison of the whole lists with the reference's).
  - float features: the scoring is checked on the lists the device returned, whatever they are.
  - the POI fixture at full size, 801 regions, 8 sets shuffled into one table, the paper's eight k, rel_m = 300; the sets one at a time give the same bits.
  - dge_pairwise_ground_vectors, m in {1, 70, 128}, on the fixture.
  - the refusals that need the device."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pairwise_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_equal(got, want, rel_m, what):
    for key in ("ndcg", "ratio", "ideal"):
        assert same_bits(got[key], want[key]), (what, key, np.argwhere(got[key] != want[key])[:5].tolist())
    if rel_m:
        assert same_bits(got["precision"], want["precision"]), (what, "precision")
    else:
        assert got["precision"] is None
    assert np.array_equal(got["hits"], want["hits"]), (what, "hits", np.argwhere(got["hits"] != want["hits"])[:5].tolist())
    assert np.array_equal(got["members"], want["members"]) and np.array_equal(got["tested"], want["tested"]), (what, "counts")
    assert same_bits(got["coverage"], want["coverage"]), (what, "coverage")


_small = {}


def small():
    """the 130-region case, its resident rows and its reference lists: made once"""
    if not _small:
        import embedding_amd as E
        c = ref.small_case()
        c["lists"], c["member"] = ref.estimated_lists(c["features"], c["row_of"], c["present"], 70)
        c["F"] = E.Vectors.from_host(c["features"]); c["G"] = E.Vectors.from_host(c["gnd"])
        _small.update(c)
    return _small


@pytest.mark.parametrize("rel_m", [0, 1, 30, 129])
def test_small_case_every_output_equals_the_reference(dge, rel_m):
    c = small()
    ks = (1, 5, 20, 70)
    got = c["F"].pairwise_eval(c["G"], c["row_of"], ks=ks, rel_m=rel_m, test=c["test"], want_rows=True, want_lists=True)
    assert np.array_equal(got["lists"], c["lists"])
    want = ref.evaluate(c["gnd"], c["lists"], c["test"], ks, rel_m)
    assert_equal(got, want, rel_m, "small rel_m=%d" % rel_m)
    assert got["members"].tolist() == [130, 91, 71] and (got["tested"] <= got["members"]).all() and got["tested"][0] == 91
    assert got["info"]["regions"] == 130 and got["info"]["members"] == 292
    # the zero-vector ground rows: every relevance -1, ratio exactly 1 wherever they are tested
    for r in (3, 64, 129):
        t = c["test"][r] != 0
        assert (got["ratio"][0, :, r] == (1.0 if t else 0.0)).all()


def test_small_case_lists_are_knn_cosine_on_the_stacked_members(dge):
    from embedding_amd import evaluate as ev
    c = small()
    got = c["F"].pairwise_eval(c["G"], c["row_of"], ks=(1, 5, 20, 70), want_lists=True)["lists"]
    for s in range(3):
        regions = np.flatnonzero(c["member"][s])
        idx, _, _ = ev.knn_cosine_gpu(c["features"][c["row_of"][s, regions]], 64)          # the public entry stops at 64: the first 64 of 70 are its list
        assert np.array_equal(got[s, regions][:, :64], regions[idx])
        assert (got[s, ~c["member"][s]] == -1).all()
    # without a test mask every member is tested
    res = c["F"].pairwise_eval(c["G"], c["row_of"], ks=(70,))
    assert np.array_equal(res["tested"], res["members"])


def test_scoring_is_decoupled_from_the_lists(dge):
    """float features, not on a lattice: whatever lists the strip kernel returns, ratio, hits, ndcg and precision are the reference applied to THOSE lists"""
    c = small()
    rng = np.random.default_rng(3)
    f = rng.normal(size=c["features"].shape).astype(np.float32)
    ks = (1, 5, 20, 70)
    got = dge.evaluate.pairwise_eval(f, c["G"], c["row_of"], ks=ks, rel_m=30, test=c["test"], want_rows=True, want_lists=True)
    assert_equal(got, ref.evaluate(c["gnd"], got["lists"], c["test"], ks, 30), 30, "float features")


def test_fixture_at_full_size_and_set_by_set(dge):
    c = ref.fixture_case()
    lists, _ = ref.estimated_lists(c["features"], c["row_of"], None, 70)
    want = ref.evaluate(c["gnd"], lists, None, ref.PAPER_KS, 300)
    F = dge.Vectors.from_host(c["features"]); G = dge.Vectors.from_host(c["gnd"])
    got = F.pairwise_eval(G, c["row_of"], rel_m=300, want_rows=True, want_lists=True)
    assert np.array_equal(got["ks"], ref.PAPER_KS) and np.array_equal(got["lists"], lists)
    assert_equal(got, want, 300, "fixture")
    assert (got["members"] == 712).all() and got["info"]["threshold_keys"] == 1024
    for s in range(len(c["row_of"])):
        one = F.pairwise_eval(G, c["row_of"][s], rel_m=300, want_rows=True, want_lists=True)
        for key in ("ndcg", "precision", "ratio"):
            assert same_bits(one[key][0], got[key][s]), (s, key)
        assert np.array_equal(one["hits"][0], got["hits"][s]) and np.array_equal(one["lists"][0], got["lists"][s]) and same_bits(one["ideal"], got["ideal"])


@pytest.mark.parametrize("m", [1, 70, 128])
def test_ground_lists_on_the_fixture(dge, m):
    _, gnd = ref.fixture()
    idx, dist = dge.evaluate.pairwise_ground(gnd, m)
    ridx, rdist = ref.ground_lists(gnd, m)
    assert np.array_equal(idx, ridx) and same_bits(dist, rdist)


def test_the_limits_k_128_and_rows_of_256_values(dge):
    """kmax = 128, g = D = 256: the ideal pass runs 16 regions a workgroup and 16-column tiles, the strip kernel takes 132 KB of LDS, the rank pass sorts 256
    slots; float ground rows with a NaN row, an infinite row and a zero row; n = 150 leaves a ragged block and a ragged tile"""
    import knn_ref
    rng = np.random.default_rng(9)
    n = 150
    gnd = rng.normal(size=(n, 256)).astype(np.float32)
    gnd[4] = 0; gnd[17, 200] = np.nan; gnd[140, 3] = -np.inf; gnd[60] = 2 * gnd[61]
    features = knn_ref.lattice(2 * n, 256, seed=10)
    row_of = np.stack([np.arange(n), np.where(np.arange(n) % 7 == 3, -1, np.arange(n) + n)]).astype(np.int64)
    ks = (64, 65, 128)
    lists, _ = ref.estimated_lists(features, row_of, None, 128)
    got = dge.evaluate.pairwise_eval(features, gnd, row_of, ks=ks, rel_m=100, want_rows=True, want_lists=True)
    assert np.array_equal(got["lists"], lists) and got["info"]["threshold_keys"] == 256
    assert_equal(got, ref.evaluate(gnd, lists, None, ks, 100), 100, "limits")


def test_absent_ground_rows_are_zero_vectors(dge):
    c = small()
    present = np.ones(130, bool); present[[5, 100]] = False
    G = dge.Vectors.from_host(c["gnd"], present)
    got = c["F"].pairwise_eval(G, c["row_of"], ks=(1, 5, 20, 70), rel_m=30, test=c["test"], want_rows=True)
    assert_equal(got, ref.evaluate(c["gnd"], c["lists"], c["test"], (1, 5, 20, 70), 30, gnd_present=present), 30, "absent ground rows")


def test_refusals_that_need_the_device(dge):
    c = small()
    ks = (1, 5, 20, 70)
    # a row_of entry that names an absent row makes no member
    present = c["present"].copy(); gone = c["row_of"][0, [10, 11]]; present[gone] = False
    Fp = dge.Vectors.from_host(c["features"], present)
    res = Fp.pairwise_eval(c["G"], c["row_of"][:2], ks=ks)
    assert res["members"].tolist() == [128, 91]
    # ... and a set it leaves with kmax members is refused, by number and count
    gone = c["row_of"][2, np.flatnonzero(c["row_of"][2] >= 0)[0]]
    present = c["present"].copy(); present[gone] = False
    with pytest.raises(dge.DgeError) as ei:
        dge.Vectors.from_host(c["features"], present).pairwise_eval(c["G"], c["row_of"], ks=ks)
    assert ei.value.code == 1 and "set 2 has 70 members" in str(ei.value)
    short = c["row_of"].copy(); short[2, np.flatnonzero(short[2] >= 0)[-1]] = -1
    with pytest.raises(dge.DgeError) as ei:
        c["F"].pairwise_eval(c["G"], short, ks=ks)
    assert ei.value.code == 1 and "set 2 has 70 members" in str(ei.value)
    # a feature row named twice within a set
    twice = c["row_of"].copy(); twice[1, np.flatnonzero(twice[1] < 0)[0]] = twice[1, np.flatnonzero(twice[1] >= 0)[0]]
    with pytest.raises(dge.DgeError) as ei:
        c["F"].pairwise_eval(c["G"], twice, ks=ks)
    assert ei.value.code == 1 and "set 1 names feature row" in str(ei.value) and "twice" in str(ei.value)
