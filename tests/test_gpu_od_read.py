"""GPU: .od flow text read on the device (include/dge.h: dge_graph_add_od_files / _texts, csrc/od_read.hip) against two yardsticks.  The first is a byte-level
second reading written here: data.split(b"\\n"), every line through bytes.split(), int() per id, libc strtod per weight, the rule of the graph in plain
Python.  The second is embedding_amd.io.read_od_slices on well-formed texts of non-empty files.  The device-ingested graph is compared with a DeviceGraph
built through add_edges, reserve_vertices and set_sources from the yardstick's arrays: the CSR (row pointers, neighbours, the weights' and out-degrees'
bits), the source table, after build_alias(exact=True) every prob and alias, and the walks under one seed.  Also: regions(), the names and every counter of
dge_od_info — host_values against the classification of the host build of csrc/od_parse.h.  Every comparison is exact equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_libc = C.CDLL("libc.so.6")
_libc.strtod.restype = C.c_double
_libc.strtod.argtypes = [C.c_char_p, C.c_void_p]


@pytest.fixture(scope="module")
def classify(tmp_path_factory):
    """tokens -> how many of them the routine of csrc/od_parse.h hands to the host (the harness of tests/test_od_parse_host.py)."""
    so = str(tmp_path_factory.mktemp("od_parse_harness") / "libod_parse_harness.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-o", so, os.path.join(ROOT, "tests", "native", "od_parse_harness.cpp")])
    H = C.CDLL(so)
    H.harness_od_parse_f64.argtypes = [C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]

    def run(tokens):
        if not tokens:
            return 0
        off = np.zeros(len(tokens) + 1, np.int64); off[1:] = np.cumsum([len(t) for t in tokens])
        bits = np.zeros(len(tokens), np.uint64); status = np.zeros(len(tokens), np.uint8)
        H.harness_od_parse_f64(b"".join(tokens), off.ctypes.data_as(C.c_void_p), len(tokens), bits.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p))
        assert (status < 2).all()
        return int((status == 1).sum())
    return run


def second_reading(pieces, classify=None):
    """-> what read_od_slices returns, plus the counters of dge_od_info."""
    T = len(pieces)
    hs, ss, ds, ws, weights = [], [], [], [], []
    lines = flows = 0
    for h, data in enumerate(pieces):
        parts = bytes(data).split(b"\n")
        lines += len(parts) - (1 if parts[-1] == b"" else 0)
        for line in parts:
            toks = line.split()
            if not toks:
                continue
            assert len(toks) == 3, line
            flows += 1
            weights.append(toks[2])
            w = _libc.strtod(toks[2], None)
            assert np.isfinite(w)
            if w > 0:
                hs.append(h); ss.append(int(toks[0])); ds.append(int(toks[1])); ws.append(w)
    regions = np.array(sorted(set(ss) | set(ds)), np.int64)
    R = len(regions)
    rank = {int(r): i for i, r in enumerate(regions)}
    src = np.array([h * R + rank[s] for h, s in zip(hs, ss)], np.int32)
    dst = np.array([((h + 1) % T) * R + rank[d] for h, d in zip(hs, ds)], np.int32)
    sources = np.unique(np.concatenate([src[src < R], dst[dst < R]])).astype(np.int32)
    info = dict(bytes=sum(len(p) for p in pieces), lines=lines, flows=flows, edges=len(src), dropped=flows - len(src), regions=R, sources=len(sources), slices=T,
                host_values=classify(weights) if classify else None)
    return dict(src=src, dst=dst, w=np.array(ws, np.float64), sources=sources, regions=regions, R=R, T=T,
                names=["%d-%d" % (h, r) for h in range(T) for r in regions.tolist()], info=info)


def same_arrays(a, b):
    """two lists of the same read-backs: same shapes, same bytes (doubles by their bits)."""
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        x = np.ascontiguousarray(x); y = np.ascontiguousarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, (k, x.shape, y.shape, x.dtype, y.dtype)
        assert x.tobytes() == y.tobytes(), (k, np.nonzero(x.view(np.uint8) != y.view(np.uint8))[0][:5])


def store_of(g, tables):
    c = g.get_csr(tables=tables)
    out = [c["row_ptr"], c["nbr"], c["weight"], c["out_degree"]] + ([c["prob"], c["alias"]] if tables else [])
    if tables:
        s = g.get_source_alias()
        out += [s["prob"], s["alias"], s["src"], np.float64(s["weight_sum"])]
    return out


def host_graph(dge, ref):
    g = dge.DeviceGraph(0)
    g.add_edges(ref["src"], ref["dst"], ref["w"])
    g.reserve_vertices(ref["T"] * ref["R"])
    g.set_sources(ref["sources"])
    return g


def check(dge, got, ref, walks=True):
    """the device-ingested graph `got` = (graph, names, info) against the host-built graph of the yardstick's arrays."""
    g, names, info = got
    h = host_graph(dge, ref)
    assert g.num_vertices == h.num_vertices == ref["T"] * ref["R"] and g.num_edges == h.num_edges == len(ref["src"])
    same_arrays(store_of(g, False), store_of(h, False))
    assert np.array_equal(g.regions(), ref["regions"]) and g.regions().dtype == np.int64
    if names is not None:
        assert list(names) == ref["names"]
    for k, v in ref.get("info", {}).items():
        if v is not None:
            assert info[k] == v, (k, info[k], v)
    assert info["read_ms"] >= 0 and info["kernel_ms"] > 0
    if walks and len(ref["src"]):
        g.build_alias(True); h.build_alias(True)
        same_arrays(store_of(g, True), store_of(h, True))
        L = min(ref["T"] + 2, 12)
        same_arrays([g.sample_walks(512, L, seed=11)], [h.sample_walks(512, L, seed=11)])
    return g


def fails(dge, call, code=7):
    with pytest.raises(dge.DgeError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    return str(ei.value)


# ------------------------------------------------------------------------------------------ texts
IDS = [10100 * (i + 1) * (i + 1) for i in range(36)] + [980100, 2 ** 40 + 3, -17, 0]          # 10100 .. 980100 and beyond: not consecutive, one near 2^40, one negative
ONLY_DROPPED, ONLY_LAST_DST = 555555, 777777


def main_pieces():
    rng = np.random.default_rng(20251018)
    seps = [b" ", b"\t", b"  ", b" \t "]
    pieces = []
    for h, n in enumerate((1100, 0, 900)):
        lines = []
        for i in range(n):
            s, d = (int(x) for x in rng.choice(IDS, 2))
            c = int(rng.integers(0, 12))
            w = [b"0", b"-0", b"-3", b"0.0", b"-1e-3"][c] if c < 5 else b"%d" % rng.integers(1, 400)
            a, b = seps[int(rng.integers(0, 4))], seps[int(rng.integers(0, 4))]
            line = b"%d%s%d%s%s" % (s, a, d, b, w)
            if c == 5:
                line = b"%s\n%s" % (line, line)                                    # a duplicate edge
            if c == 6:
                line += b" \t"                                                     # trailing blanks
            if c == 7:
                line = b"\n  \n" + line                                            # blank lines in front
            lines.append(line)
        if h == 0:
            lines.insert(17, b"%d %d 0" % (ONLY_DROPPED, IDS[0]))                 # a region that occurs only in dropped flows: no region
            lines.insert(40, b"%d %d -2" % (IDS[1], ONLY_DROPPED))
        if h == 2:
            lines.insert(5, b"%d %d 7" % (IDS[2], ONLY_LAST_DST))                 # only a destination of slice T-1: a layer-0 vertex without out-edges
        eol = b"\r\n" if h == 0 else b"\n"
        pieces.append(eol.join(lines) + (eol if h == 0 and lines else b""))       # the last piece ends without '\n'
    assert pieces[1] == b"" and not pieces[2].endswith(b"\n")
    return pieces


MAIN = main_pieces()


def test_three_slices_with_every_quirk(dge, classify):
    ref = second_reading(MAIN, classify)
    assert ref["T"] == 3 and ref["R"] == len(IDS) + 1 and ONLY_DROPPED not in ref["regions"] and ref["info"]["dropped"] > 300 and ref["info"]["flows"] > 2000
    last = int(np.searchsorted(ref["regions"], ONLY_LAST_DST))
    assert last in ref["sources"] and last not in ref["src"]                       # a source of weight 0
    assert len(set(zip(ref["src"].tolist(), ref["dst"].tolist(), ref["w"].tolist()))) < len(ref["src"])      # duplicates are there
    g = check(dge, dge.DeviceGraph.from_od(MAIN), ref)
    s = g.get_source_alias()
    assert s["src"].tolist() == ref["sources"].tolist() and g.get_csr()["out_degree"][last] == 0
    check(dge, dge.DeviceGraph.from_od([bytearray(p) for p in MAIN], names=dge.Names()), ref, walks=False)
    g, names, info = dge.DeviceGraph.from_od(MAIN, names=False)
    assert names is None and info["edges"] == ref["info"]["edges"]


SMALL = b"10100 40400 3\n40400 -17 2.5\r\n\n90900\t10100\t1 \n10100 10100 0\n-17 1099511627779 12\n40400 10100 3\n40400 10100 3"
SECOND = b"40400 10100 1\n90900 -17 2"


def test_leading_blanks_lane_and_chunk_boundaries(dge, classify):
    ref = second_reading([SMALL, SECOND], classify)
    want = None
    pads = list(range(64)) + [8192 - 3, 8192 - 8, 8192 - 20, 8192 + 31, 2 * 8192 - 1]
    for k in pads:
        data = b" " * k + SMALL
        if k == 8192 - 3:
            assert data[8191:8193] == b"10"                                        # a token lies across the chunk boundary
        if k == 8192 - 20:
            assert b"\n" not in data[8190:8194] and data[:8192].split()[-1] == b"40400"       # ... and a line does
        g, names, info = dge.DeviceGraph.from_od([data, SECOND])
        got = store_of(g, False) + [g.regions(), np.array(list(names))]
        if want is None:
            check(dge, (g, names, info), ref)
            want = got
        same_arrays(got, want)
        assert info["bytes"] == len(data) + len(SECOND) and {x: info[x] for x in ("lines", "flows", "edges", "dropped", "regions", "sources")} == \
            {x: ref["info"][x] for x in ("lines", "flows", "edges", "dropped", "regions", "sources")}
    starts = {(k + SMALL.index(b"1099511627779")) % 32 for k in range(64)}
    assert {20, 25, 31} <= starts                                                  # the 13-byte token lay across a 32-byte lane boundary


def write_files(tmp_path, pieces, tag):
    paths = []
    for h, data in enumerate(pieces):
        paths.append(str(tmp_path / ("%s-%d.od" % (tag, h))))
        open(paths[-1], "wb").write(data)
    return paths


def random_pieces(rng, T, ids, n, zero_every=9):
    pieces = []
    for h in range(T):
        s = rng.choice(ids, n); d = rng.choice(ids, n); w = rng.integers(1, 1000, n)
        w[::zero_every] = 0
        pieces.append(b"".join(b"%d %d %d\n" % t for t in zip(s.tolist(), d.tolist(), w.tolist())))
    return pieces


def against_both(dge, classify, tmp_path, pieces, tag):
    from embedding_amd import io
    paths = write_files(tmp_path, pieces, tag)
    ref = second_reading(pieces, classify)
    theirs = io.read_od_slices(paths)
    same_arrays([theirs[k] for k in ("src", "dst", "w", "sources", "regions")], [ref[k] for k in ("src", "dst", "w", "sources", "regions")])
    assert theirs["names"] == ref["names"] and theirs["R"] == ref["R"] and theirs["T"] == ref["T"]
    theirs["info"] = ref["info"]
    check(dge, dge.DeviceGraph.from_od(paths), theirs)
    return paths, ref


def test_one_slice_is_the_static_graph(dge, classify, tmp_path):
    rng = np.random.default_rng(1)
    pieces = random_pieces(rng, 1, np.array(IDS[:30]), 700)
    paths, ref = against_both(dge, classify, tmp_path, pieces, "static")
    assert ref["T"] == 1 and int(ref["dst"].max()) < ref["R"]                      # the edges stay inside the layer
    g, names, info = dge.DeviceGraph.from_od(paths[0])                             # a single path
    assert info["slices"] == 1 and list(names) == ref["names"]


def test_24_slices_of_77_regions(dge, classify, tmp_path):
    rng = np.random.default_rng(2)
    pieces = random_pieces(rng, 24, np.arange(1, 78), 400)
    _, ref = against_both(dge, classify, tmp_path, pieces, "ca")
    assert ref["R"] == 77 and ref["T"] == 24 and len(ref["names"]) == 24 * 77


def test_weight_forms(dge, classify):
    forms = [b"3", b"3.0", b"2.5e1", b"1e-3", b"12345678901234567", b"1234567890123456789012345", b"+7", b"007", b".5", b"5.", b"9007199254740993", b"4.9406564584124654e-324",
             b"1e-400", b"2e-324", b"1.7976931348623157e308", b"0.1", b"1e22", b"1e23", b"1E+2"]
    data = b"".join(b"%d %d %s\n" % (i + 1, i + 2, f) for i, f in enumerate(forms))
    ref = second_reading([data], classify)
    g, names, info = got = dge.DeviceGraph.from_od([data])
    check(dge, got, ref)
    assert info["host_values"] == ref["info"]["host_values"] and info["host_values"] >= 1 and classify([b"1234567890123456789012345"]) == 1
    assert classify([b"3", b"3.0", b"2.5e1", b"1e-3", b"12345678901234567"]) == 0
    assert info["dropped"] == 2                                                    # 1e-400 and 2e-324 underflow to 0
    w = g.get_csr(tables=False)["weight"]
    assert w[4] == 12345678901234567.0 and w[5] == float("1234567890123456789012345") and w[10].view(np.uint64) == np.float64(2.0 ** 53).view(np.uint64)


def test_two_hundred_thousand_lines(dge, classify, tmp_path):
    rng = np.random.default_rng(3)
    ids = np.unique(rng.integers(10 ** 4, 10 ** 7, 5000))
    pieces = random_pieces(rng, 2, ids, 100_000, zero_every=13)
    _, ref = against_both(dge, classify, tmp_path, pieces, "large")
    assert ref["info"]["flows"] == 200_000 and 4900 < ref["R"] <= 5000 and sum(map(len, pieces)) > 50 * 8192


def test_files_and_a_missing_file(dge, classify, tmp_path):
    paths = write_files(tmp_path, MAIN, "main")
    ref = second_reading(MAIN, classify)
    check(dge, dge.DeviceGraph.from_od(paths), ref, walks=False)
    check(dge, dge.DeviceGraph.from_od([os.path.relpath(p) for p in paths]), ref, walks=False)
    missing = str(tmp_path / "missing.od")
    names = dge.Names()
    assert missing in fails(dge, lambda: dge.DeviceGraph.from_od([paths[0], missing, paths[2]], names=names))
    assert str(tmp_path) in fails(dge, lambda: dge.DeviceGraph.from_od([paths[0], str(tmp_path)], names=names))          # a directory is no regular file
    assert len(names) == 0


def test_two_identical_calls_give_identical_bytes(dge):
    runs = []
    for _ in range(3):
        g, names, info = dge.DeviceGraph.from_od(MAIN)
        g.build_alias(True)
        runs.append([a.tobytes() for a in store_of(g, True)] + [g.regions().tobytes(), list(names), {k: v for k, v in info.items() if not k.endswith("_ms")},
                                                               g.sample_walks(256, 5, seed=3).tobytes()])
    assert runs[1] == runs[0] and runs[2] == runs[0]


def test_a_text_above_two_to_the_31_bytes(dge, classify):
    """a few flows, 2^31 blanks, a few flows: the flows behind the 2^31 mark read like the ones in front of it."""
    head = b"10100 40400 3\n40400 90900 0\n90900 10100 2\n"
    tail = b"40400 10100 5\n160000 90900 1234567890123456789012345\n90900 160000 1.5"
    second = b"10100 90900 4\n"
    ref = second_reading([head + tail, second], classify)
    data = head + b" " * 2 ** 31 + tail
    got = g, names, info = dge.DeviceGraph.from_od([data, second])
    n = len(data) + len(second)
    del data
    ref["info"]["bytes"] = n
    assert n > 2 ** 31 and info["edges"] == 6 and info["host_values"] == 1
    check(dge, got, ref)
    print("text of %.2f GB: read %.0f ms, kernels %.0f ms" % (n / 1e9, info["read_ms"], info["kernel_ms"]))


def test_errors(dge, classify):
    names = dge.Names()
    g = dge.DeviceGraph(0)
    lib = dge.lib

    def call(*pieces, graph=g, nm=names):
        ptrs = (C.c_char_p * len(pieces))(*pieces); sizes = (C.c_int64 * len(pieces))(*[len(p) for p in pieces])
        dge._native.check(lib.dge_graph_add_od_texts(graph._h, ptrs, sizes, len(pieces), nm._h if nm is not None else None, None))

    ok = b"1 2 3\n2 1 4\n"
    msg = fails(dge, lambda: call(ok, b"1 2 3\n2 \x001 4\n"))
    assert "NUL" in msg and "offset %d" % (len(ok) + 8) in msg
    msg = fails(dge, lambda: call(ok, b"1 2 3\n\n1 2\n1 2 3 4\n"))                 # lines of 2 and of 4 tokens: the least is named
    assert "piece 1" in msg and "line 3" in msg and "has 2 tokens where 3 are expected" in msg
    msg = fails(dge, lambda: call(b"1 2 3\n1 2 3 4\n5\n", b"1 2\n"))
    assert "piece 0" in msg and "line 2" in msg and "has 4 tokens where 3 are expected" in msg
    assert "has 1 token where 3" in fails(dge, lambda: call(b"5\n"))
    msg = fails(dge, lambda: call(ok, b"1 2 3\n1 7.0 3\nx 2 3\n"))                 # two bad ids: the least offset is named
    assert "offset %d " % (len(ok) + 8) in msg and "piece 1" in msg and "line 2, column 3" in msg and "region id" in msg
    for bad in (b"7.0", b"9223372036854775808", b"-9223372036854775809", b"0x7", b"7a", b"+", b"1e3"):
        assert "offset 2 " in fails(dge, lambda: call(b"1 " + bad + b" 3\n")), bad
        assert "offset 0 " in fails(dge, lambda: call(bad + b" 1 3\n")), bad
    msg = fails(dge, lambda: call(b"1 2 3\n1 2 0x10\n1 2 1e\n"))                   # a bad weight
    assert "offset 10 " in msg and "line 2, column 5" in msg
    for bad in (b"inf", b"-inf", b"nan", b"Infinity", b"1e309", b"1.7976931348623159e308", b"-1e999", b"nan(1)", b".", b"1e", b"1,5",
                b"%d" % (2 ** 1024 - 2 ** 970)):
        assert "offset 4 " in fails(dge, lambda: call(b"1 2 " + bad + b"\n")), bad  # not finite (the last one: the host's strtod says so) or malformed
    # precedence: NUL, ragged line, bad token — wherever they stand
    both = b"x 2 inf\n1 2\n1 \x002 3\n"
    assert "NUL" in fails(dge, lambda: call(both))
    assert "tokens where 3" in fails(dge, lambda: call(both.replace(b"\x00", b"")))
    assert "offset 0 " in fails(dge, lambda: call(both.replace(b"\x00", b"").replace(b"1 2\n", b"1 2 1\n")))
    assert "offset 4 " in fails(dge, lambda: call(b"1 2 inf\n1 y 3\n"))            # a bad weight in front of a bad id
    # the arguments: names not empty, g not fresh, fewer than one slice
    held = dge.Names(["a"])
    assert "names must be empty" in fails(dge, lambda: call(ok, nm=held), code=1) and held.as_bytes() == [b"a"]
    assert fails(dge, lambda: dge._native.check(lib.dge_graph_add_od_texts(g._h, None, None, 0, None, None)), code=1)
    used = dge.DeviceGraph(0); used.add_edges([0], [1], [1.0])
    assert "fresh" in fails(dge, lambda: call(ok, graph=used), code=5)
    reserved = dge.DeviceGraph(0); reserved.reserve_vertices(4)
    assert "fresh" in fails(dge, lambda: call(ok, graph=reserved), code=5)
    assert used.num_edges == 1 and reserved.num_vertices == 4
    # after all the refusals g is still empty and usable, names untouched
    assert len(names) == 0 and g.num_edges == 0 and g.num_vertices == 0 and len(g.regions()) == 0
    call(ok, ok)
    ref = second_reading([ok, ok], classify)
    del ref["info"]
    check(dge, (g, names, dict(read_ms=0, kernel_ms=1)), ref)
    assert "fresh" in fails(dge, lambda: call(ok, nm=None), code=5)               # ... and no longer fresh


def test_empty_texts_and_range(dge):
    g, names, info = dge.DeviceGraph.from_od([b"", b" \n\n"])
    assert g.num_vertices == 0 and g.num_edges == 0 and len(names) == 0 and len(g.regions()) == 0 and info["lines"] == 2 and info["flows"] == 0 and info["slices"] == 2
    g, names, info = dge.DeviceGraph.from_od([b"1 2 0\n3 4 -1\n"])                 # every flow dropped: no region, no vertex
    assert info["dropped"] == 2 and info["regions"] == 0 and g.num_vertices == 0
    # T*R beyond int32: 40 000 slices (all but the first empty) of 53 688 regions
    ids = np.arange(53688, dtype=np.int64)
    first = b"".join(b"%d %d 1\n" % (a, b) for a, b in zip(ids[::2].tolist(), ids[1::2].tolist()))
    msg = fails(dge, lambda: dge.DeviceGraph.from_od([first] + [b""] * 39_999), code=2)
    assert "40000 slices of 53688 regions" in msg


# ------------------------------------------------------------------------------------------ the shared hand-back (csrc/seq_tokens.h: seq_pick, seq_tokens_to_host)
def host_count_pieces(n_host):
    """600 flows over 3 pieces, every second weight one the host finishes (more than 19 significant digits) until n_host are placed; every weight is distinct"""
    lines = [b"%d %d %s\n" % (IDS[i % 30], IDS[(i * 7 + 1) % 30], b"%d.00000000000000000001" % (i + 1) if i % 2 == 0 and i // 2 < n_host else b"%d" % (i + 1)) for i in range(600)]
    return [b"".join(lines[:211]), b"".join(lines[211:389]), b"".join(lines[389:])]


@pytest.mark.parametrize("n_host", [1, 256, 257])
def test_the_hand_back_count_across_a_workgroup(dge, classify, n_host):
    """1, 256 and 257 host weights among weights the device finishes, over 3 pieces: one lane, a full workgroup and one lane of a second one in seq_pick's
    index kernel and in the byte copy; a misplaced weight shows in the store, where every edge's weight is its own."""
    pieces = host_count_pieces(n_host)
    ref = second_reading(pieces, classify)
    g, names, info = got = dge.DeviceGraph.from_od(pieces)
    check(dge, got, ref, walks=False)
    assert info["host_values"] == ref["info"]["host_values"] == n_host


def test_host_weights_around_the_eight_byte_loop(dge, classify):
    """Host weights of 7, 8, 9, 16 and 17 bytes (seq_tok_len reads 8 bytes at a time) — od_parse.h hands back no token of fewer than 4 bytes, so there is none of
    1 byte — one of them the last token of the last piece with no newline behind it.  (A weight is never the first token of a piece: test_gpu_vec_read.py
    and test_gpu_seq_ingest.py put a new name there.)  The 25-digit weight of test_weight_forms is the 25-byte case."""
    forms = [b"1.23e99", b"1.234e99", b"1.2345e99", b"1.23456789012e99", b"1.234567890123e99", b"1e55"]
    assert [len(f) for f in forms] == [7, 8, 9, 16, 17, 4] and classify(forms) == len(forms)
    lines = [b"%d %d %s" % (IDS[i], IDS[i + 1], f) for i, f in enumerate(forms + forms[::-1])]
    pieces = [b"\n".join(lines[:5]) + b"\n", b"\n".join(lines[5:]).replace(b" ", b"\t")]
    assert pieces[1].endswith(b"\t1.23e99")
    ref = second_reading(pieces, classify)
    g, names, info = got = dge.DeviceGraph.from_od(pieces)
    check(dge, got, ref, walks=False)
    assert info["host_values"] == 12
    assert sorted(g.get_csr(tables=False)["weight"].tolist()) == sorted(float(f) for f in forms * 2)


RAGGED = {           # row -> the message of the parent commit's library for ragged_pieces(row)
    0: "libdge error 7: dge_graph_add_od_texts: the line at offset 0 of the text (piece 0), line 1, column 1 has 2 tokens where 3 are expected: src dst w",
    256: "libdge error 7: dge_graph_add_od_texts: the line at offset 4802 of the text (piece 1), line 127, column 1 has 2 tokens where 3 are expected: src dst w",
    299: "libdge error 7: dge_graph_add_od_texts: the line at offset 5634 of the text (piece 1), line 170, column 1 has 2 tokens where 3 are expected: src dst w",
}


def ragged_pieces(row):
    """300 flows over 2 pieces; flow `row` lacks its weight"""
    lines = [b"%d %d %d" % (IDS[i % 30], IDS[(i + 3) % 30], i + 1) if i != row else b"%d %d" % (IDS[i % 30], IDS[(i + 3) % 30]) for i in range(300)]
    return [b"\n".join(lines[:130]) + b"\n", b"\n".join(lines[130:]) + b"\n"]


@pytest.mark.parametrize("row", [0, 256, 299])
def test_a_ragged_row_is_named_as_before(dge, row):
    """k_seq_ragged without a skip mask and seq_row_where: a row one token short at row 0, at row 256 (the first lane of the second workgroup) and at the last
    row.  The message — offset, piece, line, column, counts — is the one the library gave before the kernel and the read-back were shared."""
    assert fails(dge, lambda: dge.DeviceGraph.from_od(ragged_pieces(row))) == RAGGED[row]
