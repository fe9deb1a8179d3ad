"""GPU: the stream-order promise of include/dge.h (conventions): entry points that READ a caller's device buffer first wait for the device, entry points that
WRITE one return after their stream has drained, and a walk corpus that a model's queued launch still uses orders every other handle behind that launch.

Every other GPU test hands the library buffers that were finished long before the call and reads results after a call that had drained its stream: a missing
wait cannot show there.  Here the producer is DELAYED (tests/stream_delay.py): a buffer holds valid contents X, a torch side stream sleeps and then writes Y,
and the library is called at once — the result must be Y's, compared with the same entry on settled buffers.  Every check runs with the delay on each of the
helper's four side streams in turn (two streams can share a hardware queue), and the module fails unless the helper's control shows that the delay delays.
Both X and Y are valid arguments everywhere (ids in range, points inside the mesh, counts >= 0, walks over existing vertices): a missing wait gives a wrong
answer, never an out-of-range access.  The one place where a stale read meets ids beyond the vocabulary — the position prefix — rests on the trainer's own
bound check (k_remap_compact drops ids >= n_vertices).  Nothing queued work may still use is freed: every check ends in torch.cuda.synchronize().

Where the Python wrapper would add a wait or allocate the output itself, the C ABI is called through dge.lib.  Training uses workers=1: bit-exact, repeatable.

Against the library as it stood before the corpus event and the three device waits (one run on an MI355X, delay 5 ms, control stale on 10 of 12 stream pairs)
ten of the eighteen tests failed: count_tokens on its counts, regions_locate_device, flows_add_trips_device, all five readers behind walk_and_train, and both
rewrites behind train (with the position prefix the queued launch trained nothing: it met the prefixed ids).  The other eight passed there too: those entries
already waited."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_delay  # noqa: E402
import trip_ref  # noqa: E402
from helpers import bits, layered_graph  # noqa: E402

from embedding_amd._native import check  # noqa: E402

pytestmark = pytest.mark.gpu

R, T = 40, 4
NV = R * T
N_WALKS, L, DIM = 2000, 8, 32
DEV = "cuda:0"


def vp(t):
    return C.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def D():
    d = stream_delay.Delay(DEV)
    pairs = d.require_effective()          # fails the module when the delay holds nothing back
    print("stream_delay: %.2f ms, control stale on %d of %d ordered pairs: %s" % (d.delay_ms, len(pairs), stream_delay.N_SIDE * (stream_delay.N_SIDE - 1), pairs))
    return d


class World:
    """the graph, two walk sets over its vertices (a: seeds 11, b: seed 12), their counts, and models made from one configuration"""

    def __init__(self, dge):
        import torch
        self.dge, self.torch = dge, torch
        self.edges = layered_graph(R=R, T=T)
        src, dst, w, sources = self.edges
        self.g = dge.DeviceGraph(0); self.g.add_edges(src, dst, w); self.g.set_sources(sources); self.g.build_alias(True)
        self.walks_a = self.g.sample_walks(N_WALKS, L, seed=11)
        self.walks_b = self.g.sample_walks(N_WALKS, L, seed=12)
        self.walks_c = self.g.sample_walks(N_WALKS, L, seed=99)
        assert self.walks_a.min() >= 0 and self.walks_a.max() < NV and self.walks_b.min() >= 0 and self.walks_c.min() >= 0
        assert not np.array_equal(self.walks_a, self.walks_b) and not np.array_equal(self.walks_a, self.walks_c)
        self.counts_a = np.bincount(self.walks_a.ravel(), minlength=NV).astype(np.int64)
        self.counts_b = np.bincount(self.walks_b.ravel(), minlength=NV).astype(np.int64)
        assert not np.array_equal(self.counts_a, self.counts_b)
        self.cfg = dge.make_config(DIM, T, NV, negative=5, workers=1, epochs=1, seed=3, min_count=1, table_size=100_003)
        self.d_counts_a = torch.from_numpy(self.counts_a).to(DEV)
        m = self.model()
        self.pf = m.partition_floats(1)
        self.init = [self.export(m, t) for t in (0, 1)]         # a fresh model's tables: what reset() puts back
        m.close()

    def model(self):
        return self.dge.SgnsModel.create(self.cfg, self.d_counts_a, 0)

    def export(self, m, table):
        buf = self.torch.empty(self.pf, dtype=self.torch.float32, device=DEV)
        m.export_partition(table, 1, 0, buf)
        return buf

    def reset(self, m):
        for t in (0, 1):
            m.import_partition(t, 1, 0, self.init[t])

    def tables(self, m):
        return [self.export(m, t).cpu().numpy() for t in (0, 1)]

    def corpus(self, walks):
        return self.dge.WalkCorpus.from_host(walks, 0)


@pytest.fixture(scope="module")
def W(dge, D):
    import torch
    w = World(dge)
    yield w
    torch.cuda.synchronize()


def same_bits(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------ caller buffers the library READS
def delayed_copy(D, s, pairs):
    """queues, behind the delay on s, dst.copy_(src) for every (dst, src); all tensors exist already"""
    with D.delayed(s):
        for dst, src in pairs:
            dst.copy_(src, non_blocking=True)


def test_count_tokens_waits_for_the_producer_of_its_counts(dge, D, W):
    import torch
    corpus = W.corpus(W.walks_a)
    for s in D.side:
        counts = torch.full((NV,), 7, dtype=torch.int64, device=DEV)
        with D.delayed(s):
            counts.zero_()
        corpus.count_tokens(NV, counts)
        torch.cuda.synchronize()
        assert np.array_equal(counts.cpu().numpy(), W.counts_a), "delay on side stream %d" % D.side.index(s)


def test_model_create_waits_for_the_producer_of_its_counts(dge, D, W):
    import torch
    want = W.model()
    want_vocab, want_counts = want.vectors()[1], want.counts()
    x = torch.from_numpy(W.counts_b).to(DEV)
    for s in D.side:
        counts = x.clone()
        delayed_copy(D, s, [(counts, W.d_counts_a)])
        m = dge.SgnsModel.create(W.cfg, counts, 0)
        torch.cuda.synchronize()
        assert np.array_equal(m.vectors()[1], want_vocab) and np.array_equal(m.counts(), want_counts), "delay on side stream %d" % D.side.index(s)
        m.close()


def test_add_edges_device_waits_for_the_producer_of_the_edges(dge, D, W):
    import torch
    src, dst, w, sources = W.edges
    want = W.g.get_csr(tables=False)
    y = [torch.from_numpy(a).to(DEV) for a in (src, dst, w)]
    x = [torch.from_numpy(np.ascontiguousarray(a[::-1])).to(DEV) for a in (dst, src, w)]      # other edges over the same vertices
    for s in D.side:
        t = [a.clone() for a in x]
        delayed_copy(D, s, list(zip(t, y)))
        g = dge.DeviceGraph(0); g.add_edges_device(*t); g.set_sources(sources)
        torch.cuda.synchronize()
        got = g.get_csr(tables=False)
        for k in ("row_ptr", "nbr", "weight", "out_degree"):
            assert np.array_equal(got[k], want[k]), (k, "delay on side stream %d" % D.side.index(s))
        g.close()


@pytest.fixture(scope="module")
def trained(W):
    """a model trained on walks a, settled"""
    m = W.model()
    c = W.corpus(W.walks_a)
    m.train(c); m.stats()
    yield m
    W.torch.cuda.synchronize()


def pair_ids(seed, n=3000):
    rng = np.random.default_rng(seed)
    return rng.integers(0, NV, n).astype(np.int32), rng.integers(0, NV, n).astype(np.int32)


def test_score_pairs_waits_for_the_producer_of_the_ids(dge, D, W, trained):
    import torch
    y = [torch.from_numpy(a).to(DEV) for a in pair_ids(1)]
    x = [torch.from_numpy(a).to(DEV) for a in pair_ids(2)]
    want = trained.score_pairs(*y).cpu().numpy()
    assert not np.array_equal(bits(want), bits(trained.score_pairs(*x).cpu().numpy())) and np.isfinite(want).mean() > 0.9      # (NaN: an id outside the vocabulary)
    for s in D.side:
        t = [a.clone() for a in x]
        delayed_copy(D, s, list(zip(t, y)))
        got = trained.score_pairs(*t)
        torch.cuda.synchronize()
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), "delay on side stream %d" % D.side.index(s)


# the jittered quad mesh of tests/test_gpu_trip_map.py, a few thousand points inside its bounding box
def mesh_points(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-87.95, -87.35, n), rng.uniform(41.55, 42.15, n)], 1)


@pytest.fixture(scope="module")
def mesh(dge):
    ref, _ = trip_ref.quad_mesh(12, 20251018)
    return dge.Regions.from_arrays(*ref.arrays())


def test_regions_locate_device_waits_for_the_producer_of_the_points(dge, D, W, mesh):
    import torch
    n = 3000
    py, px = mesh_points(n, 5), mesh_points(n, 6)
    want = mesh.locate(py)
    assert (want >= 0).sum() > n // 2 and not np.array_equal(want, mesh.locate(px))
    y, x = torch.from_numpy(py).to(DEV), torch.from_numpy(px).to(DEV)
    for s in D.side:
        t = x.clone(); out = torch.full((n,), -7, dtype=torch.int32, device=DEV)
        delayed_copy(D, s, [(t, y)])
        check(dge.lib.dge_regions_locate_device(mesh._h, vp(t), n, vp(out), None))
        got = D.read_on(D.other(s), out)                       # and the output is complete when the call returns
        torch.cuda.synchronize()
        assert np.array_equal(got, want), "delay on side stream %d" % D.side.index(s)


def test_flows_add_trips_device_waits_for_the_producer_of_the_trips(dge, D, W, mesh):
    import torch
    n = 3000
    rng = np.random.default_rng(8)
    ys, ye, yh = mesh_points(n, 5), mesh_points(n, 6), rng.integers(0, 24, n).astype(np.int32)
    xs, xe, xh = mesh_points(n, 15), mesh_points(n, 16), rng.integers(0, 24, n).astype(np.int32)
    ref = dge.Flows(mesh); ref.add_trips(ys, ye, yh)
    want = ref.to_host()
    assert len(want[0]) > 100
    y = [torch.from_numpy(a).to(DEV) for a in (ys, ye, yh)]
    x = [torch.from_numpy(a).to(DEV) for a in (xs, xe, xh)]
    for s in D.side:
        t = [a.clone() for a in x]
        delayed_copy(D, s, list(zip(t, y)))
        f = dge.Flows(mesh)
        check(dge.lib.dge_flows_add_trips_device(f._h, vp(t[0]), vp(t[1]), vp(t[2]), n))
        torch.cuda.synchronize()
        got = f.to_host()
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), "delay on side stream %d" % D.side.index(s)
        f.close()


def table_patterns(W):
    """two valid table images [pf] that differ everywhere"""
    import torch
    y = (torch.arange(W.pf, dtype=torch.float32, device=DEV) % 251 - 125) / 1024
    x = torch.full((W.pf,), 0.5, dtype=torch.float32, device=DEV)
    return x, y


def test_import_partition_waits_for_the_producer_of_the_buffer(dge, D, W):
    import torch
    x, y = table_patterns(W)
    m = W.model()
    for s in D.side:
        t = x.clone()
        delayed_copy(D, s, [(t, y)])
        m.import_partition(1, 1, 0, t)
        got = W.export(m, 1)
        torch.cuda.synchronize()
        assert torch.equal(got, y), "delay on side stream %d" % D.side.index(s)
    m.close()


def test_import_delta_waits_for_the_producer_of_the_buffer(dge, D, W):
    import torch
    x, y = table_patterns(W)
    m = W.model()
    assert m.sync_size() == 2 * W.pf
    zero = torch.zeros(W.pf, dtype=torch.float32, device=DEV)
    x2, y2 = torch.cat([x, x]), torch.cat([y, -y])
    for s in D.side:
        for tb in (0, 1):
            m.import_partition(tb, 1, 0, zero)
        m.snapshot()
        t = x2.clone()
        delayed_copy(D, s, [(t, y2)])
        m.import_delta(t, 1.0)                                  # tables = 0 + 1.0 * delta, exactly
        got = [W.export(m, tb) for tb in (0, 1)]
        torch.cuda.synchronize()
        assert torch.equal(got[0], y) and torch.equal(got[1], -y), "delay on side stream %d" % D.side.index(s)
    m.close()


def test_import_partition_async_orders_the_model_behind_the_producer_stream(dge, D, W):
    """the event path: producer_stream is the delayed side stream, not the model's own; the host does not wait"""
    import torch
    x, y = table_patterns(W)
    m = W.model()
    for s in D.side:
        t = x.clone()
        delayed_copy(D, s, [(t, y)])
        c0 = dge.host_sync_count()
        m.import_partition_async(1, 1, 0, t, s.cuda_stream)
        waits = dge.host_sync_count() - c0
        got = W.export(m, 1)                                    # (blocking, on the model's stream behind the unpack)
        torch.cuda.synchronize()
        assert waits == 0
        assert torch.equal(got, y), "delay on side stream %d" % D.side.index(s)
    m.close()


# ------------------------------------------------------------------------------------------ caller buffers the library WRITES
# The handle works on a delayed torch stream (set_stream); the output holds a sentinel and is read at once on another non-blocking stream.
def test_outputs_are_complete_when_the_call_returns(dge, D, W, trained):
    import torch
    ctx, tgt = [torch.from_numpy(a).to(DEV) for a in pair_ids(1)]
    n = ctx.numel()
    m = W.model(); m.snapshot()
    c = W.corpus(W.walks_a)
    m.train(c); m.stats()
    want_scores = m.score_pairs(ctx, tgt).cpu().numpy()
    want_rows = W.export(m, 1).cpu().numpy()
    want_delta = torch.empty(m.sync_size(), dtype=torch.float32, device=DEV); m.export_delta(want_delta); want_delta = want_delta.cpu().numpy()
    assert np.abs(want_delta).max() > 0 and np.isfinite(want_scores).mean() > 0.9
    g = dge.DeviceGraph(0); g.add_edges(*W.edges[:3]); g.set_sources(W.edges[3]); g.build_alias(True)
    for s in D.side:
        s2 = D.other(s)
        m.set_stream(s.cuda_stream); g.set_stream(s.cuda_stream)
        scores = torch.full((n,), -3.0, dtype=torch.float32, device=DEV)
        rows = torch.full((W.pf,), -3.0, dtype=torch.float32, device=DEV)
        delta = torch.full((m.sync_size(),), -3.0, dtype=torch.float32, device=DEV)
        counts = torch.zeros(NV, dtype=torch.int64, device=DEV)
        packed = torch.full((W.pf,), -3.0, dtype=torch.float32, device=DEV)
        where = "delay on side stream %d" % D.side.index(s)
        with D.delayed(s):
            pass
        check(dge.lib.dge_model_score_pairs(m._h, vp(ctx), vp(tgt), n, vp(scores)))
        assert np.array_equal(bits(D.read_on(s2, scores)), bits(want_scores)), where
        with D.delayed(s):
            pass
        m.export_partition(1, 1, 0, rows)
        assert np.array_equal(bits(D.read_on(s2, rows)), bits(want_rows)), where
        with D.delayed(s):
            pass
        m.export_delta(delta)
        assert np.array_equal(bits(D.read_on(s2, delta)), bits(want_delta)), where
        with D.delayed(s):
            pass
        c.count_tokens(NV, counts)
        assert np.array_equal(D.read_on(s2, counts), W.counts_a), where
        with D.delayed(s):
            pass
        fresh = g.sample_walks_device(N_WALKS, L, seed=11)
        assert np.array_equal(fresh.to_host(), W.walks_a), where
        # stream-ordered export: a copy queued on the consumer stream sees the packed rows, and the host never waited
        with D.delayed(s):
            pass
        c0 = dge.host_sync_count()
        m.export_partition_async(1, 1, 0, packed, s2.cuda_stream)
        waits = dge.host_sync_count() - c0
        got = D.read_on(s2, packed)
        assert waits == 0 and np.array_equal(bits(got), bits(want_rows)), where
        torch.cuda.synchronize()
        fresh.close()
    m.close(); g.close()
    with torch.cuda.stream(D.side[-1]):                          # the handles are gone, the caller's stream is not
        assert float(torch.ones(8, device=DEV).sum()) == 8.0
    D.side[-1].synchronize()


# ------------------------------------------------------------------------------------------ one corpus, several handles
@pytest.fixture(scope="module")
def settled(W, trained):
    """what every reader gives on the settled corpus of walks a (= what sample_walks_into gives for seed 11, index 0)"""
    c = W.corpus(W.walks_b)
    W.g.sample_walks_into(c, 0, N_WALKS, 11, 0)
    assert np.array_equal(c.to_host(), W.walks_a)
    m2 = W.model(); m2.train(c); m2.stats()
    out = dict(seq=c.to_seq_bytes()[0], trained=W.tables(m2), eval=trained.eval_sgns(c))
    assert not same_bits(out["trained"], [b.cpu().numpy() for b in W.init])
    m2.close()
    return out


def behind_walk_and_train(D, W, m1, s):
    """a corpus of walks b; m1, on the delayed stream s, walks (seed 11) and trains into it: the call returns with both launches queued behind the delay"""
    c = W.corpus(W.walks_b)
    m1.set_stream(s.cuda_stream)
    with D.delayed(s):
        pass
    m1.walk_and_train(W.g, c, 0, N_WALKS, 11, 0)
    return c


@pytest.mark.parametrize("reader", ["to_host", "to_seq_bytes", "count_tokens", "train", "eval_sgns"])
def test_readers_of_a_corpus_see_the_walks_a_queued_walk_and_train_writes(dge, D, W, trained, settled, reader):
    import torch
    m1 = W.model()
    m2 = W.model() if reader == "train" else None
    keep = []
    for s in D.side:
        where = "delay on side stream %d" % D.side.index(s)
        if m2:
            W.reset(m2)
        c = behind_walk_and_train(D, W, m1, s); keep.append(c)
        if reader == "to_host":
            assert np.array_equal(c.to_host(), W.walks_a), where
        elif reader == "to_seq_bytes":
            assert c.to_seq_bytes()[0] == settled["seq"], where
        elif reader == "count_tokens":
            counts = torch.zeros(NV, dtype=torch.int64, device=DEV)
            c.count_tokens(NV, counts)
            assert np.array_equal(counts.cpu().numpy(), W.counts_a), where
        elif reader == "train":
            m2.train(c)
            assert same_bits(W.tables(m2), settled["trained"]), where
        else:
            r = trained.eval_sgns(c)
            assert {k: r[k] for k in ("pairs", "negatives", "skipped", "auc", "loss")} == {k: settled["eval"][k] for k in ("pairs", "negatives", "skipped", "auc", "loss")}, where
        torch.cuda.synchronize()
    m1.close()
    if m2:
        m2.close()


@pytest.mark.parametrize("writer", ["sample_walks_into", "add_position_prefix"])
def test_a_queued_train_reads_its_corpus_before_another_handle_rewrites_it(dge, D, W, settled, writer):
    import torch
    m1 = W.model()
    keep = []
    for s in D.side:
        where = "delay on side stream %d" % D.side.index(s)
        W.reset(m1)
        c = W.corpus(W.walks_a); keep.append(c)
        m1.set_stream(s.cuda_stream)
        with D.delayed(s):
            pass
        m1.train(c)
        if writer == "sample_walks_into":
            W.g.sample_walks_into(c, 0, N_WALKS, 99, 0)
            after = W.walks_c
        else:
            c.add_position_prefix(R)
            after = W.walks_a + R * np.arange(L, dtype=np.int32)[None, :]
        assert same_bits(W.tables(m1), settled["trained"]), where
        assert np.array_equal(c.to_host(), after), where
        torch.cuda.synchronize()
    m1.close()


# ------------------------------------------------------------------------------------------ set_stream itself
def test_handles_on_a_users_stream_give_the_bits_they_give_on_their_own(dge, D, W):
    import torch
    src, dst, w, sources = W.edges
    want_csr = W.g.get_csr()
    c = W.corpus(W.walks_a)
    ref = W.model(); ref.train(c); ref.train(c, epoch=0, words_before=N_WALKS * L // 2)
    want_stats = {k: v for k, v in ref.stats().items() if k in ("pairs", "words", "launches")}
    want_tables = W.tables(ref)
    s, s2 = D.side[0], D.side[1]
    # user stream -> stream 0 -> another user stream, something done on each
    g = dge.DeviceGraph(0); g.set_stream(s.cuda_stream)
    g.add_edges(src, dst, w); g.set_sources(sources); g.build_alias(True)
    got = g.get_csr()
    for k in want_csr:                                            # the alias tables among them, by bits
        assert got[k].dtype == want_csr[k].dtype and got[k].tobytes() == want_csr[k].tobytes(), k
    assert np.array_equal(g.sample_walks(N_WALKS, L, seed=11), W.walks_a)
    g.set_stream(0)
    assert np.array_equal(g.sample_walks(N_WALKS, L, seed=12), W.walks_b)
    g.set_stream(s2.cuda_stream)
    assert np.array_equal(g.sample_walks(N_WALKS, L, seed=99), W.walks_c)
    for plan in ((s.cuda_stream, s.cuda_stream), (0, 0), (s.cuda_stream, 0, s2.cuda_stream)):
        m = W.model()
        m.set_stream(plan[0]); m.train(c)
        for p in plan[1:]:
            m.set_stream(p)
        m.train(c, epoch=0, words_before=N_WALKS * L // 2)
        assert {k: v for k, v in m.stats().items() if k in want_stats} == want_stats, plan
        assert same_bits(W.tables(m), want_tables), plan
        m.close()
    g.close(); ref.close()
    for st in (s, s2):                                           # the handles are closed; the user's streams still work
        with torch.cuda.stream(st):
            x = torch.arange(16, device=DEV).sum()
        st.synchronize()
        assert int(x) == 120
    torch.cuda.synchronize()
