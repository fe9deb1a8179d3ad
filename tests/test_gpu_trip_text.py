"""GPU: taxi trip text in (include/dge.h: dge_trips_parse_texts, dge_flows_add_trip_texts / _files; csrc/trip_text.hip) against tests/trip_text_ref.py, the
pure-Python reading of the rule.  Every comparison is exact equality: statuses, hours, the doubles as bits, every counter but `slabs` and the two times."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trip_ref  # noqa: E402
import trip_text_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu
SLABS = (131072, 1 << 20, 0)
COUNTERS = ("bytes", "lines", "header_lines", "ok", "bad_fields", "bad_parse", "too_long")
MESH, MESH_V = trip_ref.quad_mesh(12, 20251018)


def check(dge, pieces, fmt, header, slabs=SLABS, want=None):
    """every slab size against the reference (computed once) and against each other -> the reference's records and info"""
    rec, info = want or T.parse_texts(pieces, fmt, header)
    ws, wh, wa, wb = T.arrays(rec)
    first = None
    for slab in slabs:
        got = dge.parse_trips(pieces, fmt, header=header, slab_bytes=slab)
        bad = np.flatnonzero((got["status"] != ws) | (got["hour"] != wh)) if len(got["status"]) == len(ws) else None
        assert bad is not None and len(bad) == 0, (slab, len(got["status"]), len(ws), None if bad is None else bad[:5])
        assert got["start_xy"].tobytes() == wa.tobytes() and got["end_xy"].tobytes() == wb.tobytes(), slab
        for k in COUNTERS:
            assert got["info"][k] == info[k], (slab, k, got["info"][k], info[k])
        counters = {k: v for k, v in got["info"].items() if k not in ("slabs", "read_ms", "kernel_ms")}
        first = first or counters
        assert counters == first and got["info"]["slabs"] >= 1
    return rec, info, first


@pytest.mark.parametrize("fmt", [1, 2, 3])
def test_every_format_against_the_reference(dge, fmt):
    lines = T.corpus_lines(fmt, 20_000, 11)
    text = T.join_lines(lines, 12)
    rec, info, counters = check(dge, [text], fmt, False)
    T.check_not_vacuous(info, len(rec))
    assert counters["host_values"] >= 100 and {r[1] for r in rec if r[0] == 0} >= set(range(24))
    check(dge, [text], fmt, True, want=(rec[1:], dict(info, header_lines=1, **{("ok", "bad_fields", "bad_parse", "too_long")[rec[0][0]]: info[("ok", "bad_fields", "bad_parse", "too_long")[rec[0][0]]] - 1})))
    # five pieces: an empty one, one that is only a header, one that ends without a terminator, one that ends in "\r" in front of one that begins with "\n"
    a, b, c = T.join_lines(lines[:7000], 1, last_terminated=False), T.join_lines(lines[7000:12_000], 2)[:-1].rstrip(b"\r\n") + b"\r", b"\n" + T.join_lines(lines[12_000:], 3)
    pieces = [a, b"", b"pickup,dropoff,seconds", b, c]
    for header in (False, True):
        rec5, info5, _ = check(dge, pieces, fmt, header)
        assert info5["header_lines"] == (4 if header else 0) and info5["lines"] == len(rec5) + info5["header_lines"]
        if not header:
            assert T.lines_of(c)[0] == b"" and rec5[len(T.lines_of(a)) + 1 + len(T.lines_of(b))][0] == 1      # the "\n" behind the "\r" is a line of its own


def test_slab_seams(dge):
    rng = np.random.default_rng(5)
    good = T.corpus_lines(3, 400, 21, mutated=0)
    parts, at = [], 0
    targets = [131072, 16 << 20]
    alphabet = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789,./: ", np.uint8)
    while at < (17 << 20):
        n = int(rng.integers(1, 3001))
        term = (b"\n", b"\r\n", b"\r")[int(rng.integers(0, 3))]
        if targets and at + 3001 + 2 > targets[0] - 4000:          # by construction: a "\r\n" whose bytes are the last of one read and the first of the next
            n, term = targets[0] - 1 - at, b"\r\n"
            targets.pop(0)
            while n > 3000:
                parts.append(b"x" * 1000 + b"\n"); at += 1001; n -= 1001
        line = good[int(rng.integers(0, len(good)))] if rng.random() < 0.3 else alphabet[rng.integers(0, len(alphabet), n)].tobytes()
        line = line[:n] if len(line) >= n else line + b"," * (n - len(line))
        parts.append(line + term); at += n + len(term)
    text = b"".join(parts)
    assert text[131071:131073] == b"\r\n" and text[(16 << 20) - 1:(16 << 20) + 1] == b"\r\n"
    ends = np.flatnonzero(np.isin(np.frombuffer(text, np.uint8), (10, 13)))
    assert len(set((ends % 32).tolist())) == 32 and len(set((ends % 16).tolist())) == 16
    rec, info, _ = check(dge, [text], 3, False)
    assert info["ok"] > 1000 and max(len(l) for l in T.lines_of(text)) <= 3000 and min(len(l) for l in T.lines_of(text)) <= 2


def test_line_lengths(dge):
    good = T.corpus_lines(3, 300, 31, mutated=0)
    f = good[0].split(b",")
    long_ok = b",".join(f[:4] + [f[4] + b"z" * (65535 - len(good[0]))] + f[5:])
    long_bad = b",".join(f[:4] + [f[4] + b"z" * (65536 - len(good[0]))] + f[5:])
    assert len(long_ok) == 65535 and len(long_bad) == 65536 and T.parse_line(long_ok, 3)[0] == 0 and T.parse_line(long_bad, 3)[0] == 3
    short = b"\n".join(good) + b"\n"
    S = 131072

    def pad_to(n):                     # n bytes of whole lines: short ones, then one of p's
        lines = short[:n - 1]
        lines = lines[:lines.rindex(b"\n") + 1] if b"\n" in lines else b""
        return lines + b"p" * (n - len(lines) - 1) + b"\n"

    for a, b in ((long_ok, b"q" * 65535), (long_bad, b"q" * 65536)):
        # slabs of 131072 bytes, each ending with a terminator: a long line at the start of the first, in the middle of the second, at the end of the third;
        # then one that opens the fourth, and one as the last line
        text = a + b"\n" + pad_to(S - len(a) - 1)
        text += pad_to(30_000) + a + b"\r" + pad_to(S - 30_000 - len(a) - 1)
        text += pad_to(S - len(b) - 1) + b + b"\n"
        assert len(text) == 3 * S and all(text[k * S - 1] in b"\r\n" for k in (1, 2, 3))
        text += a + b"\r\n" + short + b
        for tail in (b"", b"\n"):
            rec, info, _ = check(dge, [text + tail], 3, False)
            longs = [r[0] for r, l in zip(rec, T.lines_of(text + tail)) if len(l) >= 65535]
            long_status = 3 if len(a) == 65536 else None
            assert len(longs) == 5 and info["too_long"] == (5 if long_status else 0) and rec[-1][0] == (long_status or 1) and longs == ([3] * 5 if long_status else [0, 0, 1, 0, 1])
    # a line no slab holds: status 3, its bytes counted, the lines behind it untouched
    text = short + b"w" * 200_000 + b"\r\n" + short + b"v" * 400_000 + b"\r" + short + b"u" * 131072
    rec, info, _ = check(dge, [text], 3, False)
    assert info["too_long"] == 3 and info["ok"] == 900 and info["bytes"] == len(text)


def trips_of(rec):
    ok = [r for r in rec if r[0] == 0]
    a = np.array(ok, np.float64).reshape(-1, 6)
    return np.ascontiguousarray(a[:, 2:4]), np.ascontiguousarray(a[:, 4:6]), a[:, 1].astype(np.int32)


def state(flows):
    return [a.tobytes() for a in flows.to_host()], {k: v for k, v in flows.info().items() if k != "kernel_ms"}


def test_flows_from_text_and_files(dge, tmp_path):
    from embedding_amd._native import DGE_ERR_IO, DgeError
    fmt = 2
    lines = T.corpus_lines(fmt, 20_000, 41)
    text = T.join_lines(lines, 42)
    rec, info = T.parse_texts([text], fmt, False)
    T.check_not_vacuous(info, len(rec))
    rg = dge.Regions.from_arrays(*MESH.arrays())
    want = dge.Flows(rg); want.add_trips(*trips_of(rec))
    w = state(want)
    assert w[1]["mapped"] > 5000 and w[1]["trips"] == info["ok"] and w[1]["no_start"] > 0
    one = dge.Flows(rg)
    got = one.add_trip_text(text, fmt, header=False)
    assert state(one) == w and {k: got[k] for k in COUNTERS} == info
    # the same lines in three calls, and cut into different pieces with small slabs
    all_lines = T.lines_of(text)
    three = dge.Flows(rg)
    for a, b in ((0, 6000), (6000, 6001), (6001, len(all_lines))):
        three.add_trip_text(b"\n".join(all_lines[a:b]), fmt, header=False, slab_bytes=131072)
    assert state(three) == w
    pieces = [all_lines[0], b"\r\n".join(all_lines[1:9000]) + b"\r", b"", b"\r\n".join(all_lines[9000:]) + b"\n"]
    cut = dge.Flows(rg)
    cut.add_trip_text(pieces, fmt, header=False, slab_bytes=1 << 20)
    assert state(cut) == w
    # files, with a header line each
    paths = []
    for k, (a, b) in enumerate(((0, 5000), (5000, 5000), (5000, len(all_lines)))):
        paths.append(str(tmp_path / ("trips%d.tsv" % k)))
        open(paths[-1], "wb").write(b"a\tb\tc\r\n" + b"\n".join(all_lines[a:b]))
    files = dge.Flows(rg)
    got = files.add_trip_files(paths, fmt, header=True, slab_bytes=131072)
    assert state(files) == w and got["header_lines"] == 3 and got["ok"] == info["ok"] and got["slabs"] > 10
    # a missing file as the second of three: DGE_ERR_IO with its path, and the table is as it was
    missing = str(tmp_path / "no_such_file.tsv")
    with pytest.raises(DgeError) as err:
        files.add_trip_files([paths[0], missing, paths[2]], fmt, header=True)
    assert err.value.code == DGE_ERR_IO and missing in str(err.value) and state(files) == w
    files.add_trip_files(paths[:1], fmt, header=True)          # and it still works
    assert files.info()["trips"] > w[1]["trips"]


def test_points_one_ulp_from_an_edge_keep_their_side_through_the_text(dge):
    from fractions import Fraction
    v = MESH_V
    a = np.concatenate([v[:-1, :].reshape(-1, 2), v[:, :-1].reshape(-1, 2)]); b = np.concatenate([v[1:, :].reshape(-1, 2), v[:, 1:].reshape(-1, 2)])
    mid = a + (b - a) / 2
    keep = np.array([all(2 * Fraction(m) == Fraction(p) + Fraction(q) for m, p, q in zip(*row)) for row in zip(mid.tolist(), a.tolist(), b.tolist())])
    mid = mid[keep][:40]
    ulp = lambda x, k: (np.array(x, np.float64).view(np.int64) + k).view(np.float64)
    pts = np.concatenate([mid] + [np.stack([ulp(mid[:, 0], dx), ulp(mid[:, 1], dy)], 1) for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1))])
    inside = np.array([-87.65, 41.85])
    region, _ = MESH.locate(pts)
    through32, _ = MESH.locate(pts.astype(np.float32).astype(np.float64))
    assert (region != through32).any() and (region >= 0).sum() >= len(mid) and (region[:len(mid)] == -1).all()      # a parse that is a float32 off changes regions
    lines = [b"\t".join([b"5/14/2013", b"%d:00:00 %s" % (i % 12 or 12, b"PM" if i % 24 >= 12 else b"AM"), b"5/14/2013 7:41", b"c", b"d", b"1.2", b"e", b"f", b"g", b"%.17g" % x, b"%.17g" % y,
                          b"%.17g" % inside[0], b"%.17g" % inside[1], b"h", b"9.75", b"540", b"z"]) for i, (x, y) in enumerate(pts.tolist())]
    text = b"\n".join(lines) + b"\n"
    got = dge.parse_trips(text, 2, header=False)
    assert (got["status"] == 0).all() and got["start_xy"].tobytes() == pts.tobytes() and got["hour"].tolist() == [i % 24 for i in range(len(pts))]
    rg = dge.Regions.from_arrays(*MESH.arrays())
    assert np.array_equal(rg.locate(got["start_xy"]), region)
    end_region = MESH.locate(inside[None])[0]
    want, n = trip_ref.flows(region, np.repeat(end_region, len(pts)), got["hour"], pts, np.repeat(inside[None], len(pts), 0))
    f = dge.Flows(rg); f.add_trip_text(text, 2, header=False)
    h, s, e, c = f.to_host()
    assert list(zip(zip(h.tolist(), s.tolist(), e.tolist()), c.tolist())) == sorted(want.items())
    assert {k: f.info()[k] for k in n} == n


def test_a_text_above_two_gib(dge):
    fmt = 3
    block = T.corpus(fmt, 20_000, 51)
    assert block[-1:] in (b"\n", b"\r")
    if block.endswith(b"\r"):
        block += b"\n"
    reps = (1 << 31) // len(block) + 2
    rec, info = T.parse_texts([block], fmt, False)
    rg = dge.Regions.from_arrays(*MESH.arrays())
    one = dge.Flows(rg); one.add_trip_text(block, fmt, header=False)
    big = dge.Flows(rg)
    text = block * reps
    assert len(text) > 1 << 31
    got = big.add_trip_text(text, fmt, header=False)
    for k in COUNTERS:
        assert got[k] == info[k] * reps, k
    h1, s1, e1, c1 = one.to_host()
    h, s, e, c = big.to_host()
    assert np.array_equal(h, h1) and np.array_equal(s, s1) and np.array_equal(e, e1) and np.array_equal(c, c1 * reps) and c1.sum() > 5000
    assert {k: v for k, v in big.info().items() if k not in ("kernel_ms", "entries")} == {k: v * reps for k, v in one.info().items() if k not in ("kernel_ms", "entries")}
