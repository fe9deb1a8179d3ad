"""GPU: a resident walk corpus written as .seq text by the device (include/dge.h: dge_walks_to_seq_text / dge_walks_write_seq, csrc/seq_write.hip) against a
second writing done here in a few lines of Python on bytes (io.write_seq works on str; it is the yardstick of the sampler test only).  Every comparison is
exact equality of bytes or of int32 arrays."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOKEN_BYTES = np.array([c for c in range(1, 256) if c not in (9, 10, 11, 12, 13, 32)], np.uint8)      # everything a name may hold


def second_writing(walks, names=None, prefix=False):
    lines = []
    for row in walks:
        toks = []
        for j, v in enumerate(row):
            if v < 0:
                continue
            t = names[v] if names is not None else b"%d" % v
            toks.append(b"%d-%s" % (j, t) if prefix else t)
        lines.append(b" ".join(toks) + b"\n")
    return lines


def counts(walks, text):
    return dict(bytes=len(text), lines=len(walks), tokens=int((walks >= 0).sum()), empty_lines=int((walks < 0).all(axis=1).sum()) if walks.shape[0] else 0)


def random_names(rng, n, lo=1, hi=300):
    """n distinct names of lo..hi bytes out of every byte a token may hold, 0x80-0xFF among them; the name's number leads, so no two are equal"""
    out = []
    for k in range(n):
        head = b"%d:" % k
        body = rng.choice(TOKEN_BYTES, int(rng.integers(lo, hi + 1))).tobytes()
        out.append((head + body)[:max(len(head), len(body))])
    return out


def check_both_legs(dge, tmp_path, walks, names, prefix, tag):
    """to_seq_bytes and the file against the second writing; info against the counts"""
    want = b"".join(second_writing(walks, names, prefix))
    corpus = dge.WalkCorpus.from_host(walks)
    dn = dge.Names(names) if names is not None else None
    text, info = corpus.to_seq_bytes(dn, prefix)
    assert text == want, (tag, len(text), len(want))
    path = str(tmp_path / ("%s.seq" % tag))
    finfo = corpus.write_seq(path, dn, prefix)
    assert open(path, "rb").read() == want, tag
    for inf in (info, finfo):
        for k, v in counts(walks, want).items():
            assert inf[k] == v, (tag, k, inf[k], v)
        assert inf["write_ms"] >= 0 and (inf["kernel_ms"] > 0 or len(walks) == 0), (tag, inf)
    return corpus, dn, want


@pytest.fixture(scope="module")
def tile(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("seq_out_plan") / "seq_out_plan_harness")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "native", "seq_out_plan_harness.cpp")])
    return int(subprocess.run([exe, "sizes"], capture_output=True, text=True, check=True).stdout.split()[0])


# ---------------------------------------------------------------------------------------------- 1. what the sampler produces
def test_sampler_output_equals_io_write_seq(dge, tmp_path):
    from embedding_amd import io, synth
    R, T = 50, 6
    G = synth.flow_graph_numpy(R, T, 4, seed=5, dead_end_fraction=0.2)
    g = dge.DeviceGraph(0)
    g.add_edges(G["src"], G["dst"], G["w"]); g.set_sources(G["sources"]); g.build_alias(True)
    corpus = g.sample_walks_device(3000, T, seed=11, rng_mode=1)
    walks = corpus.to_host()
    assert (walks[:, -1] < 0).any() and (walks[:, -1] >= 0).any()                     # dead ends: short walks among whole ones
    names = ["%d-17%04d" % (v // R, v % R) for v in range(R * T)]
    for prefix in (False, True):
        want = str(tmp_path / ("host%d.seq" % prefix)); got = str(tmp_path / ("device%d.seq" % prefix))
        io.write_seq(want, walks, names, prefix)
        info = corpus.write_seq(got, names, prefix)
        data = open(got, "rb").read()
        assert data == open(want, "rb").read()
        assert corpus.to_seq_bytes(dge.Names(names), prefix)[0] == data
        assert info["lines"] == 3000 and info["tokens"] == int((walks >= 0).sum()) and info["empty_lines"] == 0 and info["bytes"] == len(data)


# ---------------------------------------------------------------------------------------------- 2. fuzz
def fuzz_walks(rng, n_rows, max_len, n_ids, id_pool=None):
    """ids >= 0 with entries < 0 in leading, middle and trailing positions, and whole rows of them"""
    ids = rng.integers(0, n_ids, (n_rows, max_len)) if id_pool is None else rng.choice(id_pool, (n_rows, max_len))
    walks = ids.astype(np.int32)
    walks[rng.random((n_rows, max_len)) < 0.15] = -1                                   # anywhere
    for r in range(n_rows):
        kind = rng.integers(0, 6)
        if kind == 0:
            walks[r, :rng.integers(0, max_len + 1)] = -1                               # leading
        elif kind == 1:
            walks[r, rng.integers(0, max_len + 1):] = -1                               # trailing
        elif kind == 2:
            walks[r, :] = -int(rng.integers(1, 4))                                     # a whole row, and not only -1
    return walks


def test_fuzz_against_the_second_writing(dge, tmp_path):
    rng = np.random.default_rng(20240607)
    names = random_names(rng, 40)
    names.append(b"L" + rng.choice(TOKEN_BYTES, 4999).tobytes())                      # one name of 5 000 bytes
    names += [b"x", b"\x80", b"\xff\xfe"]
    decimal_ids = np.array([0, 9, 10, 99, 100, 999_999, 1_000_000, 2_147_483_647], np.int64)
    rows_of = [0, 1, 2, 63, 64, 65, 1000]; lens_of = [1, 2, 8, 11, 24, 101]
    seen = set()
    for case in range(42):
        n_rows = rows_of[case % 7]; max_len = lens_of[case // 7]                  # every pair over the 42 cases
        seen.add((n_rows, max_len))
        decimal = case % 4 == 3
        walks = fuzz_walks(rng, n_rows, max_len, len(names), decimal_ids if decimal else None)
        check_both_legs(dge, tmp_path, walks, None if decimal else names, bool(case & 1) if not decimal else bool(case & 4), "fuzz%d" % case)
    assert len(seen) == 42


# ---------------------------------------------------------------------------------------------- 3. windows and alignment
def test_every_window_equals_its_slice_of_the_full_text(dge, tmp_path):
    rng = np.random.default_rng(3)
    names = [b"n%02d" % k + b"y" * k for k in range(16)]                               # 3 .. 18 bytes: one-token lines of every length mod 16
    walks = -np.ones((60, 3), np.int32)
    walks[:, 0] = np.arange(60) % 16
    walks[::5, 2] = rng.integers(0, 16, 12)
    walks[7] = -1
    lines = second_writing(walks, names)
    assert {len(l) % 16 for l in lines} == set(range(16))
    corpus, dn, full = check_both_legs(dge, tmp_path, walks, names, False, "windows")
    start = np.concatenate([[0], np.cumsum([len(l) for l in lines])])
    for row0 in range(41):
        for n in (1, 3, 17):
            text, info = corpus.to_seq_bytes(dn, False, row0, n)
            assert text == full[start[row0]:start[row0 + n]], (row0, n)
            assert info["lines"] == n and info["bytes"] == len(text)
    path = str(tmp_path / "window.seq")
    corpus.write_seq(path, dn, True, row0=33, n_rows=17)
    assert open(path, "rb").read() == b"".join(second_writing(walks[33:50], names, True))


def test_lines_of_a_tile_minus_one_a_tile_and_a_tile_plus_one(dge, tmp_path, tile):
    """three one-token lines of exactly tile - 1, tile and tile + 1 bytes at the start, in the middle and at the end of a text"""
    rng = np.random.default_rng(4)
    names = [rng.choice(TOKEN_BYTES, n).tobytes() for n in (tile - 2, tile - 1, tile)] + random_names(rng, 12, 1, 40)
    trio = -np.ones((3, 4), np.int32); trio[:, 1] = [0, 1, 2]

    def fill(n):
        w = fuzz_walks(rng, n, 4, 12)
        w[w >= 0] += 3
        return w
    walks = np.concatenate([trio, fill(90), trio, fill(37), trio])
    lines = second_writing(walks, names)
    assert [len(lines[k]) for k in (0, 1, 2)] == [tile - 1, tile, tile + 1] and [len(l) for l in lines[-3:]] == [tile - 1, tile, tile + 1]
    check_both_legs(dge, tmp_path, walks, names, False, "tiles")
    check_both_legs(dge, tmp_path, walks, names, True, "tiles_prefixed")


# ---------------------------------------------------------------------------------------------- 4. append
def test_append_and_truncate(dge, tmp_path):
    rng = np.random.default_rng(5)
    names = random_names(rng, 30, 1, 60)
    walks = fuzz_walks(rng, 500, 8, 30)
    corpus, dn, full = check_both_legs(dge, tmp_path, walks, names, True, "one_call")
    path = str(tmp_path / "two_calls.seq")
    open(path, "wb").write(b"z" * (len(full) + 1000))                                   # a longer file is in the way: append=False truncates it
    k = 123
    a = corpus.write_seq(path, dn, True, 0, k, append=False)
    assert os.path.getsize(path) == a["bytes"] < len(full)
    b = corpus.write_seq(path, dn, True, k, 500 - k, append=True)
    assert open(path, "rb").read() == full and a["bytes"] + b["bytes"] == len(full) and a["lines"] + b["lines"] == 500
    corpus.write_seq(path, dn, True, 0, 0, append=True)                                 # no rows: nothing more
    assert os.path.getsize(path) == len(full)
    corpus.write_seq(path, dn, True, 0, 0, append=False)                                # no rows, no append: an empty file
    assert os.path.getsize(path) == 0
    text, info = corpus.to_seq_bytes(dn, True, 17, 0)
    assert text == b"" and info["bytes"] == 0 and info["lines"] == 0


# ---------------------------------------------------------------------------------------------- 5. round trip through the reader
def left_packed(walks):
    rows = [[v for v in row if v >= 0] for row in walks]
    rows = [r for r in rows if r]
    L = max((len(r) for r in rows), default=1)
    out = -np.ones((len(rows), L), np.int32)
    for k, r in enumerate(rows):
        out[k, :len(r)] = r
    return out


def test_round_trip_through_from_seq(dge, tmp_path):
    rng = np.random.default_rng(6)
    names = random_names(rng, 50, 1, 80)
    walks = fuzz_walks(rng, 700, 11, 50)
    corpus = dge.WalkCorpus.from_host(walks)
    path = str(tmp_path / "round.seq")
    corpus.write_seq(path, names)
    back, back_names, info = dge.WalkCorpus.from_seq(path, names=dge.Names(names), intern=False)
    assert np.array_equal(back.to_host(), left_packed(walks))
    assert info["names_added"] == 0 and info["unknown"] == 0 and back_names.as_bytes() == names
    assert info["lines"] == 700 and info["rows"] == int((walks >= 0).any(axis=1).sum())


# ---------------------------------------------------------------------------------------------- 6. above 2^31 bytes
def test_a_text_above_two_to_the_31_bytes(dge, tmp_path):
    """64 names of 4 096 bytes, 70 000 rows x 8 ids: 2 294 320 000 bytes of few, long tokens.  A line is 8 x 4097 bytes, so the second writing can spell
    any window of the text from the rows it covers."""
    rng = np.random.default_rng(7)
    NAME, ROWS, L = 4096, 70_000, 8
    names = [b"%02d" % k + rng.choice(TOKEN_BYTES, NAME - 2).tobytes() for k in range(64)]
    walks = rng.integers(0, 64, (ROWS, L)).astype(np.int32)
    line = L * (NAME + 1)
    total = ROWS * line
    assert total == 2_294_320_000 > 2 ** 31
    corpus = dge.WalkCorpus.from_host(walks)
    dn = dge.Names(names)
    need = C.c_int64(0)
    dge._native.check(dge.lib.dge_walks_to_seq_text(corpus._h, 0, ROWS, dn._h, 0, None, 0, C.byref(need), None))
    assert need.value == total
    path = str(tmp_path / "big.seq")
    info = corpus.write_seq(path, dn)
    assert info["bytes"] == total == os.path.getsize(path) and info["lines"] == ROWS and info["tokens"] == ROWS * L and info["empty_lines"] == 0

    def window(at, n):
        r0, r1 = at // line, (at + n + line - 1) // line
        text = b"".join(second_writing(walks[r0:r1], names))
        return text[at - r0 * line: at - r0 * line + n]
    MB = 1 << 20
    with open(path, "rb") as f:
        for at in (0, total - MB, 2 ** 31 - MB, 2 ** 31, 2 ** 31 + 12345, 65_000 * line - MB // 2):
            f.seek(at)
            assert f.read(MB) == window(at, MB), at
    back, _, rinfo = dge.WalkCorpus.from_seq(path, names=dn, intern=False)
    assert np.array_equal(back.to_host(), walks) and rinfo["unknown"] == 0 and rinfo["names_added"] == 0 and rinfo["bytes"] == total
    os.remove(path)


# ---------------------------------------------------------------------------------------------- 7. errors
def test_errors_leave_everything_as_it_was(dge, tmp_path):
    from embedding_amd._native import SeqOutInfo
    rng = np.random.default_rng(8)
    names = random_names(rng, 20, 1, 30)
    walks = rng.integers(0, 20, (10, 4)).astype(np.int32)
    bad = walks.copy()
    bad[5, 2] = 20; bad[5, 3] = 21; bad[8, 0] = 23                                      # the least (row, column) is reported
    corpus = dge.WalkCorpus.from_host(bad)
    dn = dge.Names(names)
    present, absent = str(tmp_path / "present.seq"), str(tmp_path / "absent.seq")
    open(present, "wb").write(b"keep me\n")
    for path, append in ((present, False), (present, True), (absent, False), (absent, True)):
        with pytest.raises(dge.DgeError) as ei:
            corpus.write_seq(path, dn, append=append)
        msg = str(ei.value)
        assert ei.value.code == 2 and "row 5" in msg and "column 2" in msg and "id 20" in msg, msg
    assert open(present, "rb").read() == b"keep me\n" and not os.path.exists(absent)
    buf = C.create_string_buffer(b"\xAA" * 4096, 4096); n = C.c_int64(-1)
    assert dge.lib.dge_walks_to_seq_text(corpus._h, 0, 10, dn._h, 0, buf, 4096, C.byref(n), None) == 2 and buf.raw == b"\xAA" * 4096
    assert corpus.to_seq_bytes(dn, row0=0, n_rows=5)[0] == b"".join(second_writing(bad[:5], names))      # the rows in front are fine
    corpus.to_seq_bytes(None)                                                            # ... and every id has a decimal form

    good = dge.WalkCorpus.from_host(walks)
    want = b"".join(second_writing(walks, names))
    buf = C.create_string_buffer(b"\xAA" * (len(want) + 64), len(want) + 64); info = SeqOutInfo()
    rc = dge.lib.dge_walks_to_seq_text(good._h, 0, 10, dn._h, 0, buf, len(want) - 1, C.byref(n), C.byref(info))
    assert rc == 4 and n.value == len(want) and buf.raw == b"\xAA" * (len(want) + 64)    # DGE_ERR_CAP: the size, and not a byte written
    rc = dge.lib.dge_walks_to_seq_text(good._h, 0, 10, dn._h, 0, buf, len(want), C.byref(n), C.byref(info))
    assert rc == 0 and n.value == len(want) and buf.raw == want + b"\xAA" * 64           # an exact fit, and nothing behind it
    missing = str(tmp_path / "no_such_dir" / "x.seq")
    with pytest.raises(dge.DgeError) as ei:
        good.write_seq(missing, dn)
    assert ei.value.code == 7 and missing in str(ei.value)
    for row0, n_rows in ((0, 11), (10, 1), (11, 0), (5, 6)):
        with pytest.raises(dge.DgeError) as ei:
            good.to_seq_bytes(dn, row0=row0, n_rows=n_rows)
        assert ei.value.code == 1
        with pytest.raises(dge.DgeError) as ei:
            good.write_seq(absent, dn, row0=row0, n_rows=n_rows)
        assert ei.value.code == 1
    assert not os.path.exists(absent)


# ---------------------------------------------------------------------------------------------- 8. read-only and repeatable
def test_the_entries_only_read_and_repeat_themselves(dge, tmp_path):
    rng = np.random.default_rng(9)
    names = random_names(rng, 25, 1, 100)
    walks = fuzz_walks(rng, 300, 8, 25)
    corpus = dge.WalkCorpus.from_host(walks)
    dn = dge.Names(names)
    a, _ = corpus.to_seq_bytes(dn, True)
    corpus.write_seq(str(tmp_path / "r.seq"), dn, True)
    b, _ = corpus.to_seq_bytes(dn, True)
    assert a == b == open(str(tmp_path / "r.seq"), "rb").read()
    assert np.array_equal(corpus.to_host(), walks) and dn.as_bytes() == names
