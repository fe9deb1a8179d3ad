"""CPU: the .matrix reader's per-element code and its slab feeder (embedding_amd/csrc/matrix_parse.h, matrix_feed.h) built for the host into a program of its
own (tests/native/matrix_parse_harness.cpp), plain and once more under -fsanitize=address,undefined: the lane summary and the segmented operator on random
bytes, a text of about 6 KB at every slab size, and the values' edge cases — each result against tests/matrix_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import matrix_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "matrix_parse_harness.cpp")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("matrix_parse_" + request.param)
    exe = str(d / "matrix_parse_harness")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, SRC])

    def run(mode, text=None, *args):
        argv = [exe, mode]
        if text is not None:
            path = str(d / "text.matrix")
            with open(path, "wb") as f:
                f.write(text)
            argv.append(path)
        r = subprocess.run(argv + [str(a) for a in args], capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        return r.stdout.splitlines()
    return run


def expected(text, n, sep):
    """what the harness prints for one piece, from the reference"""
    try:
        got = M.read([text], [0], n, sep)
    except M.Offence as e:
        return ["offence %d %d %d %d" % (e.kind, e.offset, e.line, e.column)]
    head = "ok %d %d %d %d %d" % (got["lines"], got["rows"], len(got["entries"]), sum(e[3] >> 20 for e in got["entries"]), sum(e[3] & 0xFFFFF for e in got["entries"]))
    return [head] + ["%d %d %d" % e[1:] for e in got["entries"]]


def test_lane_summary_and_operator_on_random_bytes(harness):
    for seed in (1, 2):
        out = harness("ops", None, seed)
        assert out[-1].split()[0] == "ok" and int(out[-1].split()[1]) == 20000


def matrix_text(n, seed, sep=","):
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        vals = []
        for j in range(n):
            k = rng.integers(6)
            v = 0 if k < 3 else int(rng.integers(1, 10 ** int(rng.integers(1, 13))))
            vals.append(("00" if k == 5 else "") + str(v))
        rows.append(sep.join(vals))
    return rows


def test_a_text_of_six_kilobytes_at_every_slab_size(harness):
    """entries and offence must not depend on where the slabs are cut: a good text (CRLF and LF mixed, an empty line, no last terminator) and the same text with
    each kind of offence in its second half"""
    n = 40
    rows = matrix_text(n, 11)
    good = ("\r\n".join(rows[:20]) + "\n\n" + "\n".join(rows[20:])).encode()
    assert 5000 < len(good) < 8000
    half = len(good) // 2 + good[len(good) // 2:].index(b",")          # a separator in the second half
    texts = {
        "good": good,
        "bad byte": good[:half + 1] + b"x" + good[half + 1:],
        "empty value": good[:half] + b"," + good[half:],
        "long value": good[:half + 1] + b"1" * 33 + good[half + 1:],
        "big value": good[:half + 1] + b"1099511627777," + good[half + 1:],
        "ragged": good[:half] + good[half:].replace(b",", b"\n", 1),
        "many": good + b"\n1",
        "few": b"\n".join(good.split(b"\n")[:-1]),
        "cr": good[:half] + b"\r" + good[half:],
    }
    for name, text in texts.items():
        out = harness("sweep", text, ord(","), n)
        assert out[0] == "sizes %d" % (len(text) - 256 + 1), name
        assert out[1:] == expected(text, n, ","), name
    assert expected(texts["good"], n, ",")[0].startswith("ok") and all(expected(t, n, ",")[0].startswith("offence") for k, t in texts.items() if k != "good")


def test_values_of_one_to_nineteen_digits_and_the_limit(harness):
    for sep in (",", " ", "\t"):
        vals = ["1" + "0" * (d - 1) for d in range(1, 14)] + ["0" * (19 - d) + "9" * d for d in range(1, 13)] + [str(2 ** 40), "0" * 6 + str(2 ** 40), "0" * 19, "0"]
        n = len(vals)
        text = ("\n".join(sep.join(vals[(i + j) % n] for j in range(n)) for i in range(n)) + "\n").encode()
        out = harness("read", text, ord(sep), n, 256)
        assert out == expected(text, n, sep) and out[0].startswith("ok")
        assert out == harness("read", text, ord(sep), n, 1 << 24)
    for big, kind in ((str(2 ** 40 + 1), M.BIG_VALUE), ("9" * 19, M.BIG_VALUE), ("0" * 6 + str(2 ** 40 + 1), M.BIG_VALUE), ("1" * 20, M.LONG_VALUE), ("0" * 20, M.LONG_VALUE)):
        text = ("1,2\n3,%s\n" % big).encode()
        out = harness("read", text, ord(","), 2, 256)
        assert out == expected(text, 2, ",") and out[0].split()[:2] == ["offence", str(kind)], big
    # the counters of an empty piece and of a piece of empty lines
    assert harness("read", b"\n\r\n\n", ord(","), 0, 256) == ["ok 3 0 0 0 0"]
