"""CPU: embedding_amd/csrc/trip_parse.h — what every lane of k_trip_parse (trip_text.hip) runs on its line — built for the host
(tests/native/trip_parse_harness.cpp) and compared record by record with tests/trip_text_ref.py: status, hour and the four doubles as bits, on the hand-written
lines of tests/golden/trip_lines.json and on 1e5 seeded lines of every format.  The same source, built stand-alone with -fsanitize=address,undefined, runs
clean on a corpus file and counts what the reference counts; it is not loaded into Python."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import trip_text_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "trip_parse_harness.cpp")
N_LINES = 100_000


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("trip_parse_harness")), "libtrip_parse_harness.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-Wall", "-o", so, SRC])
    H = C.CDLL(so)
    H.harness_trip_parse.argtypes = [C.c_char_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]

    def parse(lines, fmt):
        off = np.zeros(len(lines) + 1, np.int64)
        off[1:] = np.cumsum([len(l) for l in lines])
        n = len(lines)
        status = np.full(n, 9, np.uint8); hour = np.zeros(n, np.int32); xy = np.zeros((n, 4), np.uint64); host = np.zeros(n, np.int32)
        H.harness_trip_parse(b"".join(lines), off.ctypes.data, n, fmt, status.ctypes.data, hour.ctypes.data, xy.ctypes.data, host.ctypes.data)
        return status, hour, xy, host
    return parse


def same(got, rec):
    status, hour, xy, _ = got
    ws, wh, s, e = T.arrays(rec)
    want_xy = np.concatenate([s, e], 1).view(np.uint64)
    bad = np.flatnonzero((status != ws) | (hour != wh) | (xy != want_xy).any(1))
    return bad


def test_the_golden_lines(harness):
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "trip_lines.json")))
    for fmt in (1, 2, 3):
        rows = g["type%d" % fmt]
        lines = [r[0].encode() for r in rows]
        want = [(r[1][0], r[1][1]) + tuple(float(x) for x in r[1][2:]) for r in rows]
        assert [tuple(T.bits(v) for v in T.parse_line(l, fmt)[2:]) for l in lines] == [tuple(T.bits(v) for v in w[2:]) for w in want]      # the reference itself
        assert [T.parse_line(l, fmt)[:2] for l in lines] == [w[:2] for w in want]
        bad = same(harness(lines, fmt), want)
        assert len(bad) == 0, (fmt, lines[bad[0]])
    # the coordinate of 25 digits is the one the device routine hands to the host
    assert harness([g["type3"][2][0].encode()], 3)[3].tolist() == [1]


@pytest.mark.parametrize("fmt", [1, 2, 3])
def test_a_hundred_thousand_seeded_lines_agree_with_the_reference(harness, fmt):
    lines = T.corpus_lines(fmt, N_LINES, 20251018)
    rec = [T.parse_line(l, fmt) for l in lines]
    st = [r[0] for r in rec]
    info = dict(ok=st.count(0), bad_fields=st.count(1), bad_parse=st.count(2))
    T.check_not_vacuous(info, len(rec))
    got = harness(lines, fmt)
    bad = same(got, rec)
    assert len(bad) == 0, (len(bad), lines[bad[0]], rec[bad[0]], got[0][bad[0]], got[1][bad[0]], got[2][bad[0]])
    assert got[3].sum() >= 100                        # the long coordinates went through strtod, and came out as the reference has them
    hours = {r[1] for r in rec if r[0] == 0}
    assert set(range(24)) <= hours


def test_the_references_coordinates_are_strtods():
    tokens = [b"1.", b".5", b"1e2", b"-0", b"41.8812345678901234567890123", b" 4.19001e1 ", b"9007199254740993", b"1.7976931348623157e308", b"4.9406564584124654e-324", b"2e-324"]
    for fmt in (1, 2, 3):
        for l in T.corpus_lines(fmt, 2000, 3):
            tokens += [t for t in l.replace(b"(", b",").replace(b")", b",").replace(b"\t", b",").split(b",") if b"." in t and b"\x00" not in t]
    assert T.check_coord(tokens) > 10_000
    for t in (b"NaN", b"Infinity", b"0x1p3", b"1.0f", b"1.0d", b"1e999", b"", b" ", b"1 2", b"1e", b".", b"+"):
        assert T.coord(t) is None, t


def test_lines_and_splits_of_the_reference():
    assert T.lines_of(b"a\nb\r\nc\rd") == [b"a", b"b", b"c", b"d"] and T.lines_of(b"a\n") == [b"a"] and T.lines_of(b"\n") == [b""] and T.lines_of(b"") == []
    assert T.lines_of(b"a\r") == [b"a"] and T.lines_of(b"\na") == [b"", b"a"] and T.lines_of(b"a\n\r\n\rb") == [b"a", b"", b"", b"b"]
    assert T.split(b"a,b,,", b",") == [b"a", b"b"] and T.split(b",,,", b",") == [] and T.split(b"", b",") == [b""] and T.split(b",a", b",") == [b"", b"a"]
    assert T.split(b"\ta\t\t\tb\t\t", b"\t", plus=True) == [b"", b"a", b"b"] and T.split(b"1/2 3:4", b"/ :") == [b"1", b"2", b"3", b"4"]
    assert T.split2(b"a b c") == [b"a", b"b c"] and T.split2(b"a ") == [b"a", b""] and T.split2(b"ab") == [b"ab"]
    assert T.parse_byte(b"+5") == 5 and T.parse_byte(b"007") == 7 and T.parse_byte(b"128") is None and T.parse_byte(b"-128") == -128 and T.parse_byte(b"") is None
    assert T.date2(b"5/1", b"12:00:00 AM") == 0 and T.date2(b"5/1", b"12:00:00 PM") == 12 and T.date2(b"5/1", b"-7:00:00 PM") == 5 and T.date2(b"5/1", b"-7:00:00 AM") == -7


def test_the_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "trip_parse_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    for fmt in (1, 2, 3):
        text = T.corpus(fmt, 20_000, 7 + fmt) + b"x" * 65535 + b"\r\n" + b"y" * 65536
        path = str(tmp_path / ("trips%d.txt" % fmt))
        open(path, "wb").write(text)
        for header in (0, 1):
            run = subprocess.run([exe, path, str(fmt), str(header)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
            _, info = T.parse_texts([text], fmt, header)
            assert info["too_long"] == 1
            for k in ("bytes", "lines", "ok", "bad_fields", "bad_parse", "too_long"):
                assert " %s %d " % (k, info[k]) in " " + run.stdout, (k, info, run.stdout)
