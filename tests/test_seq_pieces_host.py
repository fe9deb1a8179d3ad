"""embedding_amd/csrc/seq_pieces.h on the host: the text readers' files and texts as pieces, the one read step, the joiner of the one buffer (.seq, .vec, .od) and
the slab feeder of the trip reader — against the layout of seq_plan.h and the slab rule at the head of trip_text.hip, both restated below.
tests/native/seq_pieces_harness.cpp, built with g++ and bound through ctypes; no device."""
import ctypes as C
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trip_text_ref as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "seq_pieces_harness.cpp")
OK, ERR_ARG, ERR_IO = 0, 1, 7                # include/dge.h
S = 131072
MAX_LINE = 65535


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("seq_pieces") / "seq_pieces_harness.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-Wall", "-o", so, SRC])
    H = C.CDLL(so)
    H.harness_message.restype = C.c_char_p
    return H


def _items(items, as_files):
    """-> the two arrays of a call; a None item is a null pointer.  Texts: (bytes or None, size) pairs are allowed, for the sizes a text does not have"""
    n = len(items)
    ptr = (C.c_char_p * max(n, 1))()
    size = (C.c_int64 * max(n, 1))()
    for k, x in enumerate(items):
        x, nb = x if isinstance(x, tuple) else (x, 0 if x is None or as_files else len(x))
        ptr[k] = os.fsencode(x) if as_files and x is not None else x
        size[k] = nb
    return ptr, size, n


def add(H, items, as_files):
    ptr, size, n = _items(items, as_files)
    sizes = (C.c_int64 * max(n, 1))()
    held = C.c_int32(0)
    rc = H.harness_add(ptr, size, n, int(as_files), sizes, C.byref(held))
    return rc, H.harness_message().decode(), list(sizes[:held.value])


def join(H, prefix, items, as_files, cap, truncate_to=-1):
    ptr, size, n = _items(items, as_files)
    room = len(prefix) + sum(os.path.getsize(x) if as_files else len(x) for x in items) + n + 8
    out = C.create_string_buffer(room)
    n_out = C.c_int64(0)
    rc = H.harness_join(prefix, C.c_int64(len(prefix)), ptr, size, n, int(as_files), C.c_int64(cap), C.c_int64(truncate_to), out, C.c_int64(room), C.byref(n_out))
    return rc, H.harness_message().decode(), out.raw[:n_out.value]


def feed(H, items, as_files):
    ptr, size, n = _items(items, as_files)
    room = sum(os.path.getsize(x) if as_files else len(x) for x in items) + 8
    cap = room // 1000 + 64
    out = C.create_string_buffer(room)
    slab_n = (C.c_int64 * cap)()
    flags = (C.c_uint8 * (2 * cap))()
    n_slabs = C.c_int64(0)
    rc = H.harness_feed(ptr, size, n, int(as_files), C.c_int64(S), out, C.c_int64(room), slab_n, flags, C.c_int64(cap), C.byref(n_slabs))
    assert rc == OK, H.harness_message()
    slabs, at = [], 0
    for s in range(n_slabs.value):
        slabs.append((out.raw[at:at + slab_n[s]], bool(flags[2 * s]), bool(flags[2 * s + 1])))
        at += slab_n[s]
    return slabs


def open_descriptors():
    return len(os.listdir("/proc/self/fd"))


def write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


# ------------------------------------------------------------------------------------------ pieces
def test_files_become_pieces_or_are_refused_and_every_descriptor_is_closed(harness, tmp_path):
    a, b = write(tmp_path / "a.seq", b"one two\nthree"), write(tmp_path / "b.seq", b"")
    before = open_descriptors()
    assert add(harness, [a, b, a], True) == (OK, "", [13, 0, 13])
    rc, msg, _ = add(harness, [a, str(tmp_path / "missing"), b], True)
    assert rc == ERR_IO and msg == "cannot open %s: %s" % (tmp_path / "missing", os.strerror(2))
    rc, msg, _ = add(harness, [a, b, str(tmp_path)], True)
    assert rc == ERR_IO and msg == "cannot read %s: not a regular file" % tmp_path
    rc, msg, held = add(harness, [a, None, b], True)
    assert rc == ERR_ARG and msg == "who: path 1 is null" and held == []          # refused before anything is opened
    assert add(harness, [], True) == (OK, "", [])
    assert open_descriptors() == before


def test_texts_become_pieces_or_are_refused(harness):
    assert add(harness, [b"abc", b"", None, b"de"], False) == (OK, "", [3, 0, 0, 2])          # a null text of size 0 is an empty piece
    rc, msg, _ = add(harness, [b"abc", (b"de", -1)], False)
    assert rc == ERR_ARG and msg == "who: text 1 is null or of negative size"
    rc, msg, _ = add(harness, [(None, 4), b"de"], False)
    assert rc == ERR_ARG and msg == "who: text 0 is null or of negative size"


def test_a_file_that_shrinks_behind_the_fstat_is_a_read_error(harness, tmp_path):
    a = write(tmp_path / "a.seq", b"x" * 5000)
    before = open_descriptors()
    rc, msg, got = join(harness, b"", [a], True, 4096, truncate_to=1234)
    assert rc == ERR_IO and msg == "cannot read %s: the file ends after 1234 of 5000 bytes" % a
    assert open_descriptors() == before


# ------------------------------------------------------------------------------------------ the joiner
def joined(prefix, pieces):
    """seq_plan.h: the prefix, then every piece with its pad byte — the missing "\\n" behind a piece that does not end in one, else a blank"""
    out = prefix
    for p in pieces:
        out += p + (b"\n" if p and not p.endswith(b"\n") else b" ")
    return out


@pytest.mark.parametrize("cap", [1, 7, 4096])
def test_the_joined_stream_is_the_layout_of_the_plan(harness, tmp_path, cap):
    long_piece = b"".join(b"n%d m%d\n" % (i, i * 7) for i in range(1500))                  # several fills of 4096
    lists = [[b"a b\nc d\n", b"", b"e f", b"\n", b"g", b"", long_piece, long_piece[:-1]], [b""], [], [b"x"], [b"", b""]]
    for prefix in (b"", b"p0\np1\np2\n"):
        for k, pieces in enumerate(lists):
            want = joined(prefix, pieces)
            assert join(harness, prefix, pieces, False, cap) == (OK, "", want)
            paths = [write(tmp_path / ("j%d_%d" % (k, i)), p) for i, p in enumerate(pieces)]
            assert join(harness, prefix, paths, True, cap) == (OK, "", want)


# ------------------------------------------------------------------------------------------ the feeder
def slabs_by_the_rule(pieces):
    """The head of trip_text.hip, restated.  A buffer of S bytes is the tail the last slab left and fresh bytes of the piece.  A piece's last buffer goes out
    whole.  Any other goes out up to its last terminator ("\\n" or "\\r") and the rest is the next tail; when that "\\r" is the buffer's last byte and the piece
    goes on with "\\n", that byte is dropped.  A full buffer without a terminator sends its first 65 536 bytes and a "\\n", and the piece goes on behind the
    line's terminator.  -> [(bytes, first, open_end)]"""
    out = []
    for piece in pieces:
        pos, tail, first = 0, b"", True
        while pos < len(piece) or tail:
            buf = tail + piece[pos:pos + S - len(tail)]
            pos += len(buf) - len(tail)
            tail = b""
            if pos < len(piece):
                t = max(buf.rfind(b"\n"), buf.rfind(b"\r"))
                if t < 0:
                    buf = buf[:MAX_LINE + 1] + b"\n"
                    ends = [e for e in (piece.find(b"\n", pos), piece.find(b"\r", pos)) if e >= 0]
                    pos = min(ends) + 1 if ends else len(piece)
                    if ends and piece[pos - 1:pos + 1] == b"\r\n":
                        pos += 1
                else:
                    buf, tail = buf[:t + 1], buf[t + 1:]
                    if not tail and buf.endswith(b"\r") and piece[pos:pos + 1] == b"\n":
                        pos += 1
            if buf:
                out.append((buf, first, buf[-1:] not in (b"\n", b"\r")))
            first = False
    return out


def feeder_texts():
    """the texts of tests/test_gpu_trip_text.py, at the sizes S = 131072 needs"""
    lines = T.corpus_lines(3, 6000, 11)
    good = T.corpus_lines(3, 300, 31, mutated=0)
    short = b"\n".join(good) + b"\n"
    # a "\r\n" whose bytes are the last of one read and the first of the next
    seam = T.join_lines(lines[:3000], 12)
    cut = seam.rindex(b"\n", 0, S - 200) + 1
    seam = seam[:cut] + b"s" * (S - 1 - cut) + b"\r\n" + seam[cut:]
    assert seam[S - 1:S + 1] == b"\r\n" and len(seam) > 3 * S
    # five pieces: one without a last terminator, an empty one, one that is only a header, one that ends in "\r" in front of one that begins with "\n"
    a, b, c = T.join_lines(lines[:2500], 1, last_terminated=False), T.join_lines(lines[2500:4500], 2)[:-1].rstrip(b"\r\n") + b"\r", b"\n" + T.join_lines(lines[4500:], 3)
    five = [a, b"", b"pickup,dropoff,seconds", b, c]
    # a piece of exactly one buffer that ends in "\r", in front of one that begins with "\n": the "\n" is a line of the next piece, not the "\r"'s other half
    exact = [short[:S - 1][:short[:S - 1].rindex(b"\n") + 1], b"\n" + short]
    exact[0] += b"e" * (S - 1 - len(exact[0])) + b"\r"
    assert len(exact[0]) == S
    # lines no slab holds
    longs = short + b"w" * 200_000 + b"\r\n" + short + b"v" * 400_000 + b"\r" + short + b"u" * 131072
    return dict(seam=[seam], five=five, exact=exact, longs=[longs], header_only=[b"pickup,dropoff,seconds"], empty=[b"", b""])


@pytest.mark.parametrize("as_files", [False, True])
def test_the_slabs_are_the_text_cut_by_the_rule(harness, tmp_path, as_files):
    for name, pieces in feeder_texts().items():
        items = [write(tmp_path / ("%s_%d" % (name, i)), p) for i, p in enumerate(pieces)] if as_files else pieces
        got, want = feed(harness, items, as_files), slabs_by_the_rule(pieces)
        assert len(got) == len(want) and all(g == w for g, w in zip(got, want)), (name, len(got), len(want), [k for k, (g, w) in enumerate(zip(got, want)) if g != w][:3])
        # what the rule guarantees the kernels, from the slabs alone: whole lines of ONE piece, only a piece's last slab open-ended; and the lines are the text's,
        # a line of S bytes or more cut to 65 536 (the over-long one that ends its piece is that piece's last buffer and goes out whole)
        k, lines = -1, []
        for s, (data, first, open_end) in enumerate(got):
            assert 0 < len(data) <= S
            if first:
                k = next(j for j in range(k + 1, len(pieces)) if pieces[j])
                lines.append([])
            ls = T.lines_of(data)
            assert not open_end or s + 1 == len(got) or got[s + 1][1], (name, s)
            lines[-1] += ls
        want_lines = [[l if len(l) < S or i + 1 == len(T.lines_of(p)) else l[:MAX_LINE + 1] for i, l in enumerate(T.lines_of(p))] for p in pieces if p]
        assert lines == want_lines, name
        if name == "seam":
            assert got[0][0].endswith(b"\r") and len(got[0][0]) == S and got[1][0][:1] != b"\n" and sum(len(g[0]) for g in got) == len(pieces[0]) - 1
        if name == "exact":
            assert [len(g[0]) for g in got[:2]] == [S, len(pieces[1])] and got[1][0][:1] == b"\n" and got[1][1]
        if name == "longs":
            assert sorted(len(l) for l in lines[0] if len(l) > 60_000) == [65536, 65536, 131072]


# ------------------------------------------------------------------------------------------ the stand-alone program
def test_the_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "seq_pieces_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-DHARNESS_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    work = tmp_path / "work"
    work.mkdir()
    run = subprocess.run([exe, str(work)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.stdout[-2000:], run.stderr[-2000:])
    assert "wrong 0" in run.stdout
