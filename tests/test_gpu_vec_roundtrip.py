"""GPU: the .vec writer and the .vec reader against each other (dge_write_vec -> dge_vectors_from_vec_files), vectors into a model (dge_model_load_vectors) and
the two quality entries on resident rows (dge_knn_cosine_vectors, dge_ndcg_at_k_vectors).  Everything is compared bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
T, R = 4, 64
NV = T * R


@pytest.fixture(scope="module")
def walks(dge):
    rng = np.random.default_rng(0)
    src, dst, w = [], [], []
    for h in range(T):
        for s in range(R):
            for d in rng.integers(0, R, 4):
                src.append(h * R + s); dst.append(((h + 1) % T) * R + int(d)); w.append(float(rng.integers(1, 50)))
    g = dge.DeviceGraph(0); g.add_edges(src, dst, w); g.set_sources(np.arange(R)); g.build_alias(True)
    return g.sample_walks_device(3000, T, 7).to_host()


VNAMES = ["%d-%d" % (v // R, 17000 + v % R) for v in range(NV)]


def model(dge, walks, dim):
    return dge.SgnsModel.fit(walks, dge.make_config(dim, T, NV, workers=1, table_size=10007), 0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    nan_a, nan_b = (a & 0x7FFFFFFF) > 0x7F800000, (b & 0x7FFFFFFF) > 0x7F800000
    return a.shape == b.shape and bool(np.where(nan_a | nan_b, nan_a & nan_b, a == b).all())


@pytest.mark.parametrize("dim", [20, 128])
def test_writer_round_trip(dge, walks, tmp_path, dim):
    m = model(dge, walks, dim)
    syn0, vid = m.vectors()
    assert 100 < len(vid) <= NV and syn0.shape == (len(vid), dim)
    for named in (True, False):
        for header in (False, True):
            path = str(tmp_path / ("m%d_%d_%d.vec" % (dim, named, header)))
            held = VNAMES if named else [str(v) for v in range(NV)]
            names = dge.Names(held)
            m.write_vec(path, names if named else None, header=header)
            vec, got_names, info = dge.Vectors.from_vec(path, header=header, names=names)
            host, present = vec.to_host(), vec.present()
            assert host.shape == (NV, dim) and list(got_names) == held and info["names_added"] == 0 and info["dropped"] == 0
            assert np.array_equal(bits(host[vid]), bits(syn0))                      # nine digits give every float32 back, placed by vocab_ids
            want = np.zeros(NV, bool); want[vid] = True
            assert np.array_equal(present, want) and not bits(host[~want]).any()
            assert info["rows"] == len(vid) and info["missing"] == NV - len(vid) and info["dim"] == dim and info["values"] == len(vid) * dim
            assert info["host_values"] == 0                                          # what the writer's fast path spells, the device decides
            # ... and without prior names the rows come in file order
            vec2, names2, info2 = dge.Vectors.from_vec(path, header=header)
            assert np.array_equal(bits(vec2.to_host()), bits(syn0)) and names2.as_bytes() == [held[v].encode() for v in vid] and vec2.present().all()


def patterns(rng, n, dim):
    """float32 BIT PATTERNS: normals of every exponent, denormals, +-0, +-inf, NaNs."""
    u = rng.integers(0, 2 ** 32, (n, dim), dtype=np.uint64).astype(np.uint32)
    flat = u.reshape(-1)
    k = len(flat)
    flat[0:k:7] = (np.arange(len(flat[0:k:7]), dtype=np.uint32) % 256) << 23 | (flat[0:k:7] & 0x807FFFFF)      # every exponent field in turn
    flat[1:k:31] &= 0x807FFFFF                                                                                  # denormals
    special = np.array([0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x00000001, 0x80000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF,
                        0xFF7FFFFF, 0x3F800001], np.uint32)
    flat[2:2 + 13 * len(special):13] = np.resize(special, len(flat[2:2 + 13 * len(special):13]))
    return u.view(np.float32)


def test_the_whole_float32_range_through_writer_and_reader(dge, walks, tmp_path):
    dim = 20
    rng = np.random.default_rng(12)
    pat = patterns(rng, NV, dim)
    v = dge.Vectors.from_host(pat)
    assert same_bits(v.to_host(), pat) and np.array_equal(bits(v.to_host()), bits(pat)) and v.present().all()
    m = model(dge, walks, dim)
    _, vid = m.vectors()
    assert m.load_vectors(v) == len(vid)
    syn0, _ = m.vectors()
    assert np.array_equal(bits(syn0), bits(pat[vid]))
    path = str(tmp_path / "range.vec")
    names = dge.Names(VNAMES)
    m.write_vec(path, names)
    vec, _, info = dge.Vectors.from_vec(path, names=names)
    host = vec.to_host()
    assert same_bits(host[vid], pat[vid])                                            # NaN by NaN-ness; everything else bit for bit
    finite = np.isfinite(pat[vid])
    assert np.array_equal(bits(host[vid])[finite], bits(pat[vid])[finite])
    text = [t for line in open(path, "rb").read().split(b"\n") for t in line.split()[1:]]
    assert info["values"] == len(text) == len(vid) * dim
    # the writer spells %.9g, inf and nan, and csrc/vec_parse.h decides every one of those itself (tests/test_vec_parse_host.py holds it to that over the
    # whole range, denormals included): nothing is left for the host
    assert info["host_values"] == 0


def test_load_vectors(dge, walks):
    dim = 20
    m = model(dge, walks, dim)
    before, vid = m.vectors()
    before = before.copy()
    rng = np.random.default_rng(5)
    rows = rng.normal(0, 0.1, (NV, dim)).astype(np.float32)
    present = rng.integers(0, 2, NV).astype(bool)
    present[vid[0]] = True; present[vid[1]] = False
    v = dge.Vectors.from_host(rows, present)
    assert np.array_equal(v.present(), present)
    assert m.load_vectors(v) == int(present[vid].sum())
    after, vid2 = m.vectors()
    after = after.copy()
    assert np.array_equal(vid, vid2)
    held = present[vid]
    assert np.array_equal(bits(after[held]), bits(rows[vid][held]))
    assert np.array_equal(bits(after[~held]), bits(before[~held])) and (~held).any()          # rows absent in v are untouched
    short = dge.Vectors.from_host(rows[:50])                                                  # fewer rows than vertices: the rest is absent
    assert m.load_vectors(short) == int((vid < 50).sum())
    with pytest.raises(dge.DgeError) as ei:
        m.load_vectors(dge.Vectors.from_host(rows[:, :dim - 1]))
    assert ei.value.code == 1 and "dim" in str(ei.value)
    # a training launch afterwards runs and moves the loaded rows
    m.load_vectors(v)
    loaded = m.vectors()[0].copy()
    m.train(dge.WalkCorpus.from_host(walks))
    trained = m.vectors()[0]
    assert np.isfinite(trained).all() and (bits(trained[held]) != bits(loaded[held])).any()


def test_quality_entries_on_resident_rows(dge):
    from embedding_amd import evaluate
    rng = np.random.default_rng(8)
    n = 333
    f = rng.normal(0, 1, (n, 20)).astype(np.float32); g = rng.normal(0, 1, (n, 7)).astype(np.float32)
    f[5] = 0                                                                                  # a zero vector: at distance 2 from everything
    text = b"".join(b"r%d " % i + b" ".join(b"%.9g" % float(x) for x in f[i]) + b"\n" for i in range(n))
    vf, names, _ = dge.Vectors.from_vec(text)
    assert np.array_equal(bits(vf.to_host()), bits(f))
    vg = dge.Vectors.from_host(g)
    for k in (1, 10):
        idx, dist, _ = evaluate.knn_cosine_gpu(vf.to_host(), k)
        idx2, dist2, ms = evaluate.knn_cosine_vectors(vf, k)
        assert np.array_equal(idx, idx2) and np.array_equal(bits(dist), bits(dist2)) and ms > 0
        a, _ = evaluate.ndcg_against_gpu(vf.to_host(), vg.to_host(), k)
        b, _ = evaluate.ndcg_vectors(vf, vg, k)
        assert np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64) and 0 < b <= 1
    # absent rows are zero vectors for the KNN, and an argument error for nDCG
    present = np.ones(n, bool); present[17] = False
    part = dge.Vectors.from_host(f, present)
    idx, dist, _ = part.knn(5)
    assert idx.shape == (n, 5)
    f0 = f.copy(); f0[17] = 0
    idx0, dist0, _ = evaluate.knn_cosine_gpu(f0, 5)                                           # (more absent rows, exactly: tests/test_gpu_knn_exact.py)
    assert np.array_equal(idx, idx0) and np.array_equal(bits(dist), bits(dist0)) and (dist[17] == 2).all()
    for a, b in ((part, vg), (vg, part)):
        with pytest.raises(dge.DgeError) as ei:
            a.ndcg_against(b, 5)
        assert ei.value.code == 1 and "absent" in str(ei.value)
    with pytest.raises(dge.DgeError) as ei:
        vf.ndcg_against(dge.Vectors.from_host(g[:100]), 5)
    assert ei.value.code == 1
    # by name: the same rows in another order align through the names
    order = rng.permutation(n)
    shuffled = b"".join(b"r%d " % i + b" ".join(b"%.9g" % float(x) for x in g[i]) + b"\n" for i in order)
    vg2, _, info = dge.Vectors.from_vec(shuffled, names=names, intern=False)
    assert info["missing"] == 0 and np.array_equal(bits(vg2.to_host()), bits(g))
    assert vf.ndcg_against(vg2, 10)[0] == vf.ndcg_against(vg, 10)[0]
