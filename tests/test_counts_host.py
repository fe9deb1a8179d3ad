"""CPU: the count-table reader's per-line code (embedding_amd/csrc/table_parse.h) built for the host into a program of its own
(tests/native/table_parse_harness.cpp), plain and once more under -fsanitize=address,undefined: random lines, every kind of offence, the 18- and 19-digit
edges, 2^40 and 2^40 + 1, the three terminators — each result against tests/counts_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import counts_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "table_parse_harness.cpp")
IDS = [100, 200, 4242, 999999, 123456789012345678]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("table_parse_" + request.param)
    exe = str(d / "table_parse_harness")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, SRC])
    with open(str(d / "ids.txt"), "w") as f:
        f.write("\n".join(str(t) for t in reversed(IDS)) + "\n")

    def run(text, n_table_cols, sep=",", skip_lines=0, key_field=0, key=(0, 0), cols=(1, 1), col_offset=0, neg_col_offset=None):
        path = str(d / "text.csv")
        with open(path, "wb") as f:
            f.write(text)
        argv = [exe, "read", path, str(d / "ids.txt"), n_table_cols, ord(sep), skip_lines, key_field, key[0], key[1], cols[0], cols[1], col_offset,
                -1 if neg_col_offset is None else neg_col_offset]
        r = subprocess.run([str(a) for a in argv], capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        return r.stdout.splitlines()
    return run


def expected(text, n_table_cols, **kw):
    """what the harness prints, from the reference reading"""
    try:
        got = CR.read([text], IDS, n_table_cols, **kw)
    except CR.Offence as e:
        return ["offence %d %d %d %d" % (e.kind, e.offset, e.line, e.field)]
    head = "ok %d %d %d %d %d %d" % (got["lines"], got["skipped"], got["empty"], got["rows"], got["foreign"], got["total"])
    t = got["table"]
    return [head] + ["%d %d %d" % (r, c, t[r, c]) for r in range(t.shape[0]) for c in range(t.shape[1]) if t[r, c]]


def both(harness, text, n_table_cols, **kw):
    want = expected(text, n_table_cols, **kw)
    assert harness(text, n_table_cols, **kw) == want, (text[:200], kw)
    return want


def random_text(seed, sep, n_lines=300):
    """good lines in every shape the rule allows: keys in and out of the region set, with and without '-', values of 1 .. 13 digits with leading zeros,
    fields in front of, between and behind the ones that are read, all three terminators, empty lines, no last terminator"""
    rng = np.random.default_rng(seed)
    pool = IDS + [7, 101, 999998]
    out = [b"a header" + sep + b"of three" + sep + b"fields, one with a comma\r\n"]
    for _ in range(n_lines):
        if rng.integers(12) == 0:
            out.append([b"\n", b"\r\n", b"\r"][rng.integers(3)])
            continue
        key = b"%s%s%d" % ([b"xy", b"17"][rng.integers(2)], b"-" if rng.integers(3) == 0 else b"", pool[rng.integers(len(pool))])
        vals = [b"0" * int(rng.integers(3)) + b"%d" % rng.integers(0, 10 ** int(rng.integers(1, 13))) for _ in range(4)]
        junk = [b"", b"x-y", b"1.5", b'"q"'][rng.integers(4)]
        out.append(sep.join([junk, key] + vals[:2] + vals[2:] + [junk, b"tail"]) + [b"\n", b"\r\n", b"\r"][rng.integers(3)])
    return b"".join(out).rstrip(b"\r\n") if seed % 2 else b"".join(out)


def test_random_good_texts(harness):
    for seed, sep in ((1, b","), (2, b" "), (3, b"\t"), (4, b",")):
        text = random_text(seed, sep)
        want = both(harness, text, 8, sep=sep.decode(), skip_lines=1, key_field=1, key=(2, 0), cols=(2, 4), col_offset=0, neg_col_offset=4)
        assert want[0].startswith("ok") and len(want) > 10
        # a slice of the key, other columns, another place in the table
        both(harness, text, 8, sep=sep.decode(), skip_lines=1, key_field=1, key=(2, 5), cols=(3, 2), col_offset=6, neg_col_offset=1)


def test_every_kind_of_offence_and_the_one_reported_first(harness):
    kw = dict(key=(5, 0), cols=(1, 2))
    good = b"17031000100,1,1\n"
    lines = {
        CR.SHORT_LINE: b"17031000100,5", CR.SHORT_KEY: b"1703,5,6", CR.BAD_KEY: b"17031x00100,5,6", CR.KEY_SIGN: b"17031-100,5,6", CR.EMPTY_VALUE: b"17031000100,,6",
        CR.BAD_VALUE_BYTE: b"17031000100,5,-6", CR.LONG_VALUE: b"17031000100,5," + b"0" * 20, CR.BIG_VALUE: b"17031000100,1099511627777,6",
        CR.LONG_LINE: b"17031000100,1,1," + b"9" * 65536,
    }
    for kind, line in lines.items():
        for text in (good + line + b"\n" + good, good * 3 + line, b"\r" + line + b"\r\n"):
            want = both(harness, text, 2, **kw)
            assert want[0].split()[:2] == ["offence", str(kind)], (kind, want)
    # on a foreign line too; of two on one line the one in front, of two at one place the one listed first
    assert both(harness, b"17031000777,5,x\n", 2, **kw)[0].split()[1] == str(CR.BAD_VALUE_BYTE)
    assert both(harness, b"17031000100,1099511627777,x\n", 2, **kw)[0].split()[1] == str(CR.BIG_VALUE)
    assert both(harness, b"17031000100,x,1099511627777\n", 2, **kw)[0].split()[1] == str(CR.BAD_VALUE_BYTE)
    assert both(harness, b"17031,5,6\n", 2, **kw)[0].split()[1] == str(CR.SHORT_KEY)
    assert both(harness, b"17031", 2, **kw)[0].split()[1:3] == [str(CR.SHORT_KEY), "0"]             # a short line too, at its end
    assert both(harness, b"100,5,", 3, key=(0, 0), cols=(1, 3))[0].split()[1:3] == [str(CR.SHORT_LINE), "6"]      # and an empty value at the same place
    assert both(harness, b"17031-,5,6\n", 2, neg_col_offset=0, **kw)[0].split()[1:3] == [str(CR.BAD_KEY), "6"]
    # a key slice far beyond any field is clipped to the field's end (key_hi) or leaves the field short (key_lo): no sum of the two leaves the line
    assert both(harness, b"a,100,5\nb,200,6", 2, key_field=1, key=(0, 2 ** 31 - 1), cols=(2, 1)) == ["ok 2 0 0 2 0 11", "0 0 5", "1 0 6"]
    assert both(harness, b"a,100,5\n", 2, key_field=1, key=(1, 2 ** 31 - 1), cols=(2, 1))[0] == "ok 1 0 0 0 1 0"            # key 00: foreign
    assert both(harness, b"a,100,5\n", 2, key_field=1, key=(2 ** 31 - 1, 0), cols=(2, 1))[0] == "offence %d 2 1 1" % CR.SHORT_KEY
    assert both(harness, b"a,100,5\n", 2, key_field=1, key=(2 ** 31 - 2, 2 ** 31 - 1), cols=(2, 1))[0] == "offence %d 2 1 1" % CR.SHORT_KEY
    # the key behind the values, the values in front
    assert both(harness, b"5,6,ab100\n5,,ab-100\n", 2, key_field=2, key=(2, 0), cols=(0, 2))[0] == "offence %d 12 2 1" % CR.EMPTY_VALUE


def test_digit_edges_and_the_limit(harness):
    kw = dict(key=(0, 0), cols=(1, 2))
    want = both(harness, b"123456789012345678,%d,%s7\n" % (2 ** 40, b"0" * 18), 2, **kw)
    assert want == ["ok 1 0 0 1 0 %d" % (2 ** 40 + 7), "4 0 %d" % 2 ** 40, "4 1 7"]
    assert both(harness, b"1234567890123456789,1,1\n", 2, **kw)[0] == "offence %d 18 1 0" % CR.BAD_KEY              # a 19th digit
    assert both(harness, b"100,%d,1\n" % (2 ** 40 + 1), 2, **kw)[0] == "offence %d 4 1 1" % CR.BIG_VALUE
    assert both(harness, b"100,%s,1\n" % (b"9" * 19), 2, **kw)[0] == "offence %d 4 1 1" % CR.BIG_VALUE            # 19 digits are still a value
    assert both(harness, b"100,%s,1\n" % (b"0" * 19), 2, **kw)[0].startswith("ok")
    assert both(harness, b"100,%s,1\n" % (b"0" * 20), 2, **kw)[0] == "offence %d 23 1 1" % CR.LONG_VALUE
    assert both(harness, b"100,%sx,1\n" % (b"0" * 19), 2, **kw)[0] == "offence %d 23 1 1" % CR.BAD_VALUE_BYTE
    assert both(harness, b"100,%sx,1\n" % (b"0" * 20), 2, **kw)[0] == "offence %d 23 1 1" % CR.LONG_VALUE
    # a line of exactly 65 536 bytes is read; the counters of an empty text and of a text of empty lines
    line = b"100,3,4," + b"z" * (65536 - 8)
    assert both(harness, line + b"\n" + line, 2, **kw) == ["ok 2 0 0 2 0 14", "0 0 6", "0 1 8"]
    assert both(harness, b"", 2, **kw) == ["ok 0 0 0 0 0 0"]
    assert both(harness, b"\n\r\n\r\r", 2, **kw) == ["ok 4 0 4 0 0 0"]
    assert both(harness, b"\n\r\n\r\r", 2, skip_lines=3, **kw) == ["ok 4 3 1 0 0 0"]
