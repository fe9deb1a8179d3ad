"""GPU: .seq text tokenised, interned and packed on the device (include/dge.h: dge_walks_from_seq_text / _files, csrc/seq_ingest.hip) against a second
reading written here in a few lines of Python on bytes: data.split(b"\\n"), every line through bytes.split() with no argument — which splits on exactly
the six whitespace bytes 0x09-0x0D and 0x20 (tests/test_seq_abi.py checks that table) — and a dict for first-appearance ids.  Every comparison is exact
equality of the int32 array and of the names list."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
WS = [bytes([c]) for c in (9, 11, 12, 13, 32)]           # separators inside a line; 10 ends it


def second_reading(pieces, prior=(), intern=True):
    """pieces: the text, or the files' contents in order -> (walks int32 [rows x max_len] padded with -1, names, counts)."""
    if isinstance(pieces, bytes):
        pieces = [pieces]
    names = list(prior)
    ids = {n: i for i, n in enumerate(names)}
    rows, unknown, lines, tokens = [], 0, 0, 0
    for data in pieces:
        parts = data.split(b"\n")
        lines += len(parts) - (1 if parts[-1] == b"" else 0)      # a last line without its newline counts
        for line in parts:
            toks = line.split()
            if not toks:
                continue
            r = []
            for t in toks:
                i = ids.get(t)
                if i is None:
                    if intern:
                        i = len(names); ids[t] = i; names.append(t)
                    else:
                        i = -1; unknown += 1
                r.append(i)
            tokens += len(r)
            rows.append(r)
    L = max((len(r) for r in rows), default=1)
    walks = -np.ones((len(rows), L), np.int32)
    for k, r in enumerate(rows):
        walks[k, :len(r)] = r
    return walks, names, dict(lines=lines, rows=len(rows), tokens=tokens, unknown=unknown, max_len=L, names_added=len(names) - len(prior),
                              bytes=sum(map(len, pieces)))


def check(dge, pieces, got, prior=(), intern=True):
    corpus, names, info = got
    walks, want_names, counts = second_reading(pieces, prior, intern)
    host = corpus.to_host()
    assert host.shape == walks.shape and host.dtype == np.int32, (host.shape, walks.shape)
    assert np.array_equal(host, walks)
    assert names.as_bytes() == want_names
    for k, v in counts.items():
        assert info[k] == v, (k, info[k], v)
    assert info["tokens"] == int((host >= 0).sum()) + info["unknown"]
    assert info["read_ms"] >= 0 and info["kernel_ms"] > 0
    return host


def material(rng, n):
    """n bytes of token material: anything but NUL and the six whitespace bytes; 0x85 and 0xA0 (whitespace to some Unicode readers) well represented."""
    pool = np.array([c for c in range(1, 256) if c not in (9, 10, 11, 12, 13, 32)] + [0x85, 0xA0] * 8, np.uint8)
    return pool[rng.integers(0, len(pool), n)].tobytes()


def generated_texts():
    rng = np.random.default_rng(20240917)
    out = {
        "empty": b"", "one newline": b"\n", "only whitespace": b" \t \r\n\x0b\x0c\n   ", "single token": b"x", "single token, newline": b"x\n",
        "no final newline": b"a b c\nd e", "crlf": b"0-1 1-2 2-3\r\n0-4 1-2\r\n\r\n0-1\r\n", "lone carriage returns": b"a\rb\rc\n\rd\r",
        "leading and trailing blanks": b"   a  b \n\t\tc\t\n d\x0b\x0ce  \n", "blank lines between": b"\n\na b\n\n\n \nc\n\n",
        "one token of 5000 bytes": b"q " + material(rng, 5000) + b" q\n", "5000 bytes alone, no newline": material(rng, 5000),
        "0x85 and 0xA0 are token material": b"a\x85b c\xa0d \x85 \xa0\n\xa0\x85\n", "high bytes": bytes(range(0x80, 0x100)) + b" " + bytes(range(0x80, 0x100)) + b"\n",
        "one name": b"\n".join(b" ".join([b"same"] * int(n)) for n in rng.integers(1, 40, 300)) + b"\n",
        "every token new": b"\n".join(b" ".join(b"t%d" % (100 * i + j) for j in range(int(n))) for i, n in enumerate(rng.integers(1, 30, 400))),
        "prefixes of one another": b"a aa aaa aaaa aaaaaaaa aaaaaaaaa aaaaaaaaaaaaaaaa aaaaaaaaaaaaaaaaa a aaa aaaaaaaa\n" * 3,
        "lines of 1 to 300 tokens": b"\n".join(b" ".join(b"%d-%d" % (j % 8, rng.integers(0, 500)) for j in range(n)) for n in range(1, 301)) + b"\n",
        "a token across a chunk boundary": b"x" * 8185 + b" " + b"boundary-token-0123456789" + b" y\n" + b"z " * 5000,
        "newline on a chunk boundary": b"a" * 8191 + b"\n" + b"b" * 8191 + b"\n" + b"c",
    }
    while len(out) < 40:
        k = len(out)
        vocab = [material(rng, int(rng.integers(1, 24))) for _ in range(int(rng.choice([1, 3, 50, 2000])))]
        lines = []
        for _ in range(int(rng.integers(1, 400))):
            n = int(rng.choice([0, 0, 1, 2, 8, 8, 8, 30, rng.integers(1, 301)]))
            line = WS[int(rng.integers(0, 5))] * int(rng.integers(0, 3))
            for _ in range(n):
                line += vocab[int(rng.integers(0, len(vocab)))] + b"".join(WS[int(i)] for i in rng.integers(0, 5, int(rng.integers(1, 4))))
            lines.append(line)
        sep = b"\r\n" if k % 4 == 0 else b"\n"
        out["generated %d" % k] = sep.join(lines) + (sep if k % 3 else b"")
    return out


TEXTS = generated_texts()


@pytest.mark.parametrize("name", list(TEXTS))
def test_generated_texts(dge, name):
    data = TEXTS[name]
    assert b"\0" not in data
    check(dge, data, dge.WalkCorpus.from_seq(data))
    check(dge, data, dge.WalkCorpus.from_seq(bytearray(data)))


def sampled(dge, n=3000, T=4, R=32, seed=7):
    rng = np.random.default_rng(0)
    src, dst, w = [], [], []
    for h in range(T):
        for s in range(R):
            for d in rng.integers(0, R, 4):
                src.append(h * R + s); dst.append(((h + 1) % T) * R + int(d)); w.append(float(rng.integers(1, 50)))
    g = dge.DeviceGraph(0); g.add_edges(src, dst, w); g.set_sources(np.arange(R)); g.build_alias(True)
    names = ["%d-%d" % (h, 17000 + r) for h in range(T) for r in range(R)]
    return g.sample_walks_device(n, T, seed).to_host(), names


def test_the_projects_own_files(dge, tmp_path):
    """Walks sampled on the device, written with io.write_seq (with and without the spatial graph's position prefix), read back on the device: equal to
    io.read_seq of the same files; with the graph's vertex names seeded, equal to the sampled walks themselves."""
    from embedding_amd import io
    walks, vnames = sampled(dge)
    plain, prefixed = str(tmp_path / "taxi-crosstime.seq"), str(tmp_path / "taxi-spatial.seq")
    io.write_seq(plain, walks, vnames)
    io.write_seq(prefixed, walks, vnames, position_prefix=True)
    for paths in (plain, prefixed, [plain, prefixed], [prefixed, plain]):
        corpus, names, info = dge.WalkCorpus.from_seq(paths)
        want, want_names = io.read_seq(paths)
        assert np.array_equal(corpus.to_host(), want) and list(names) == want_names
        assert info["rows"] == len(want) and info["names_added"] == len(want_names)
    corpus, names, info = dge.WalkCorpus.from_seq(plain, names=dge.Names(vnames))
    assert np.array_equal(corpus.to_host(), walks) and list(names) == vnames and info["names_added"] == 0 and info["unknown"] == 0
    corpus, names, info = dge.WalkCorpus.from_seq(tmp_path / "taxi-crosstime.seq", names=dge.Names(vnames), intern=False)       # a PathLike
    assert np.array_equal(corpus.to_host(), walks) and info["unknown"] == 0


def test_several_files_seeded_names_and_intern_off(dge, tmp_path):
    files = [b"a b\nc d", b"e a\n", b"", b"\n\nf", b"g h i j\r\nb", b"a\n"]         # "d" / "e", "f" / "g", "b" / "a" must not merge
    paths = []
    for k, data in enumerate(files):
        paths.append(str(tmp_path / ("f%d.seq" % k)))
        open(paths[-1], "wb").write(data)
    host = check(dge, files, dge.WalkCorpus.from_seq(paths))
    assert host.shape == (7, 4) and host[1].tolist() == [2, 3, -1, -1] and host[2].tolist() == [4, 0, -1, -1]
    # seeded: the held names keep their ids, new ones continue behind them in first-appearance order
    prior = [b"zz", b"d", b"a", b"unused"]
    names = dge.Names(prior)
    host = check(dge, files, dge.WalkCorpus.from_seq(paths, names=names), prior=prior)
    assert host[0].tolist() == [2, 4, -1, -1] and host[1].tolist() == [5, 1, -1, -1] and len(names) == 4 + 8
    # a second text on the same names: ids go on
    more = b"new1 a new2\nzz new1\n"
    before = names.as_bytes()
    host = check(dge, more, dge.WalkCorpus.from_seq(more, names=names), prior=before)
    assert host.tolist() == [[12, 2, 13], [0, 12, -1]]
    # intern off: unknown tokens are -1 in their place, the names are untouched, the count is exact
    held = dge.Names(prior)
    corpus, _, info = got = dge.WalkCorpus.from_seq(paths, names=held, intern=False)
    host = check(dge, files, got, prior=prior, intern=False)
    assert host[0].tolist() == [2, -1, -1, -1] and host[1].tolist() == [-1, 1, -1, -1] and host[4].tolist() == [-1, -1, -1, -1]
    assert held.as_bytes() == prior and info["names_added"] == 0 and info["unknown"] == 9 and info["tokens"] == 13
    # no files at all: what dge_walks_from_host yields for n_walks = 0
    corpus, names, info = dge.WalkCorpus.from_seq([])
    assert corpus.shape == (0, 1) and len(names) == 0 and info["bytes"] == 0 and info["rows"] == 0 and info["max_len"] == 1
    assert dge.WalkCorpus.from_seq(b"")[0].shape == dge.WalkCorpus.from_host(np.zeros((0, 1), np.int32)).shape


def test_equal_hashes_never_merge_names_and_the_table_grows(dge):
    """dge_selftest_seq_intern with the hash cut to 4 bits and a table started at 16 slots, 10 000 distinct tokens each seen several times: 16 hash values
    for 10 000 strings, so every look-up compares bytes and probes, and the table is redone four times on the way up."""
    rng = np.random.default_rng(5)
    distinct = [b"%d-%d" % (i % 8, 17031000000 + i * 7919) for i in range(10000)]
    order = np.concatenate([rng.permutation(10000), rng.integers(0, 10000, 30000)])
    data = b"".join(distinct[int(i)] + (b"\n" if k % 8 == 7 else b" ") for k, i in enumerate(order))
    walks, names, counts = second_reading(data)
    want = walks[walks >= 0]
    for bits, slots in ((4, 16), (9, 1), (64, 16), (64, 1 << 20)):
        ids = np.full(len(want) + 8, -7, np.int32)
        n_tokens, n_names = C.c_int64(0), C.c_int64(0)
        dge._native.check(dge.lib.dge_selftest_seq_intern(0, data, len(data), bits, slots, ids.ctypes.data_as(C.c_void_p), len(ids), C.byref(n_tokens), C.byref(n_names)))
        assert n_tokens.value == len(want) == 40000 and n_names.value == 10000
        assert np.array_equal(ids[:len(want)], want) and (ids[len(want):] == -7).all(), (bits, slots)
    ids = np.zeros(10, np.int32)
    rc = dge.lib.dge_selftest_seq_intern(0, data, len(data), 4, 16, ids.ctypes.data_as(C.c_void_p), 10, C.byref(n_tokens), C.byref(n_names))
    assert rc == 4 and n_tokens.value == 40000                      # DGE_ERR_CAP, with the count the caller needs


def test_a_text_above_two_to_the_31_bytes(dge):
    """64 MiB of lines (8 tokens of about 30 bytes) repeated 33 times: 2.2e9 bytes, 7.4e7 tokens.  Walks are the block's, tiled; names are the block's."""
    rng = np.random.default_rng(11)
    vocab = [b"%d-tract-%021d" % (i % 8, int(rng.integers(0, 10 ** 18))) for i in range(5000)]
    line_tokens = rng.integers(0, len(vocab), (280000, 8))
    block = b"".join(b" ".join(vocab[int(t)] for t in row) + b"\n" for row in line_tokens)
    assert 2 ** 26 <= len(block) < 70e6
    walks, names, counts = second_reading(block)
    data = block * 33
    assert len(data) > 2 ** 31
    corpus, got_names, info = dge.WalkCorpus.from_seq(data)
    del data
    assert info["bytes"] == 33 * len(block) and info["rows"] == 33 * len(walks) and info["tokens"] == 33 * counts["tokens"] and info["lines"] == 33 * counts["lines"]
    assert got_names.as_bytes() == names and info["names_added"] == len(names) and info["max_len"] == 8
    host = corpus.to_host()
    assert host.shape == (33 * len(walks), 8)
    assert np.array_equal(host, np.tile(walks, (33, 1)))
    print("text of %.2f GB: read %.0f ms, kernels %.0f ms" % (info["bytes"] / 1e9, info["read_ms"], info["kernel_ms"]))


def test_training_on_the_ingested_corpus_is_the_same_training(dge, tmp_path):
    walks, vnames = sampled(dge, n=4000)
    from embedding_amd import io
    path = str(tmp_path / "train.seq")
    io.write_seq(path, walks, vnames)
    data = open(path, "rb").read()
    host_walks, host_names, _ = second_reading(data)
    corpus, names, _ = dge.WalkCorpus.from_seq(path)
    cfg = dge.make_config(32, 4, len(host_names), workers=1, table_size=10007)
    a = dge.SgnsModel.fit(host_walks, cfg, 0)                      # dge_train_sgns on the host-read array
    b = dge.SgnsModel.fit(corpus, cfg, 0)                          # dge_train_sgns_device on the ingested corpus
    (sa, va), (sb, vb) = a.vectors(), b.vectors()
    assert len(va) > 100 and np.array_equal(va, vb) and np.array_equal(sa.view(np.int32), sb.view(np.int32))
    assert np.array_equal(a.syn1neg().view(np.int32), b.syn1neg().view(np.int32))
    assert a.stats()["pairs"] == b.stats()["pairs"] > 0
    pa, pb = str(tmp_path / "a.vec"), str(tmp_path / "b.vec")
    a.write_vec(pa, [n.decode() for n in host_names])
    b.write_vec(pb, names)
    assert open(pa, "rb").read() == open(pb, "rb").read() and os.path.getsize(pa) > 0


def test_two_identical_calls_give_identical_results(dge):
    data = TEXTS["lines of 1 to 300 tokens"] * 40 + TEXTS["every token new"]
    runs = []
    for _ in range(3):
        corpus, names, info = dge.WalkCorpus.from_seq(data)
        runs.append((corpus.to_host(), names.as_bytes(), {k: v for k, v in info.items() if not k.endswith("_ms")}))
    for r in runs[1:]:
        assert np.array_equal(r[0], runs[0][0]) and r[1] == runs[0][1] and r[2] == runs[0][2]
    check(dge, data, dge.WalkCorpus.from_seq(data))


def test_errors(dge, tmp_path):
    from embedding_amd._native import SeqInfo
    lib = dge.lib
    names = dge.Names(["a"])
    data = b"a b c\nd e\0f\n"
    with pytest.raises(dge.DgeError) as ei:
        dge.WalkCorpus.from_seq(data, names=names)
    assert ei.value.code == 7 and "offset 9" in str(ei.value) and "NUL" in str(ei.value)
    assert names.as_bytes() == [b"a"]                               # a refused text adds no names
    ok, bad = str(tmp_path / "ok.seq"), str(tmp_path / "bad.seq")
    open(ok, "wb").write(b"a b c\nd e")
    open(bad, "wb").write(b"x\0")
    with pytest.raises(dge.DgeError) as ei:
        dge.WalkCorpus.from_seq([ok, bad], names=names)
    assert ei.value.code == 7 and "offset 10" in str(ei.value) and bad in str(ei.value)      # the offset counts the text: 9 bytes of ok.seq, then bad.seq's "x"
    missing = str(tmp_path / "missing.seq")
    with pytest.raises(dge.DgeError) as ei:
        dge.WalkCorpus.from_seq([ok, missing], names=names)
    assert ei.value.code == 7 and missing in str(ei.value)
    with pytest.raises(dge.DgeError) as ei:
        dge.WalkCorpus.from_seq(str(tmp_path), names=names)         # a directory is not a file to read
    assert ei.value.code == 7 and str(tmp_path) in str(ei.value)
    # ... and no corpus handle is left in *out
    for call in (lambda out: lib.dge_walks_from_seq_text(0, data, len(data), names._h, 1, C.byref(out), None),
                 lambda out: lib.dge_walks_from_seq_files(0, (C.c_char_p * 1)(missing.encode()), 1, names._h, 1, C.byref(out), None)):
        out = C.c_void_p(0xdead)
        assert call(out) == 7 and not out.value
    assert names.as_bytes() == [b"a"]
    corpus, _, info = dge.WalkCorpus.from_seq(ok, names=names)      # the names object is still good
    assert corpus.to_host().tolist() == [[0, 1, 2], [3, 4, -1]] and info["lines"] == 2


# ------------------------------------------------------------------------------------------ the new names' way to the host (csrc/seq_tokens.h: seq_tokens_to_host)
def test_new_names_across_a_workgroup_and_around_the_eight_byte_loop(dge, tmp_path):
    """257 new names behind 3 prior ones — a full workgroup and one lane more in k_seq_name_tok and in the byte copy — among them names of 1, 7, 8, 9, 16 and 17
    bytes (seq_tok_len, which now gives a name its length, reads 8 bytes at a time), one the first token of the second piece and one the last token of the
    last piece with no newline behind it.  The Names bytes are the second reading's, in first-appearance order."""
    prior = [b"p0", b"never-in-the-text", b"p2"]
    sized = [bytes([97 + k]) * n for k, n in enumerate((1, 7, 8, 9, 16, 17))]
    fresh = sized[:3] + [b"n%d" % ((k * 41) % 251) for k in range(251)] + sized[3:]
    assert len(set(fresh)) == len(fresh) == 257
    toks = [b"p2"] + [t for k, n in enumerate(fresh) for t in ((n, fresh[k // 2]) if k % 3 else (n, b"p0"))]          # every name again later, and prior ones between
    cut = toks.index(sized[3])
    lines = lambda ts: b"\n".join(b" ".join(ts[i:i + 9]) for i in range(0, len(ts), 9))
    pieces = [lines(toks[:cut]) + b"\n", lines(toks[cut:] + [sized[5]])]
    assert pieces[1].startswith(sized[3] + b" ") and pieces[1].endswith(b" " + sized[5])
    paths = [str(tmp_path / ("w%d.seq" % k)) for k in range(2)]
    for p, data in zip(paths, pieces):
        open(p, "wb").write(data)
    corpus, names, info = got = dge.WalkCorpus.from_seq(paths, names=dge.Names(prior))
    check(dge, pieces, got, prior=prior)
    assert info["names_added"] == 257 and names.as_bytes() == prior + fresh
