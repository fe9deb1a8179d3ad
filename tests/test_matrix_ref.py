"""CPU: tests/matrix_ref.py, the second reading of the .matrix reader's rule, against numpy on well-formed texts, and its sensitivity to every offence kind
and to the least-offset rule."""
import io

import numpy as np
import pytest

import matrix_ref as M


def spell(a, sep, rng=None, crlf=False, last_newline=True, empty_at=()):
    """the matrix as text; rng: some values get leading zeros"""
    lines = []
    for i, row in enumerate(a):
        vals = []
        for v in row:
            s = str(int(v))
            if rng is not None and rng.integers(4) == 0:
                s = "0" * int(rng.integers(1, 4)) + s
            vals.append(s)
        if i in empty_at:
            lines.append("")
        lines.append(sep.join(vals))
    end = "\r\n" if crlf else "\n"
    text = end.join(lines) + (end if last_newline else "")
    return text.encode()


@pytest.mark.parametrize("sep", [",", " ", "\t"])
@pytest.mark.parametrize("n", [1, 2, 3, 31, 33])
def test_well_formed_texts_read_as_loadtxt_reads_them(sep, n):
    rng = np.random.default_rng(n * 7 + ord(sep))
    for density, crlf, last in ((0.0, False, True), (0.1, True, True), (1.0, False, False)):
        a = np.where(rng.random((n, n)) < density, rng.integers(1, 2 ** 40, (n, n), endpoint=True), 0).astype(np.int64)
        if density == 1.0:
            a[0, 0] = 2 ** 40
        text = spell(a, sep, rng, crlf, last, empty_at=(0, n // 2))
        got = M.read([text], [5], n, sep)
        dense = np.loadtxt(io.BytesIO(text), delimiter=sep, ndmin=2).astype(np.int64)      # (values up to 2^40 are exact in binary64)
        r, c = np.nonzero(dense)
        assert got["entries"] == [(5, int(i), int(j), int(dense[i, j])) for i, j in zip(r, c)]
        assert got["rows"] == n and got["values"] == n * n and got["zeros"] == n * n - len(r) and got["total"] == int(dense.sum())
        assert got["bytes"] == len(text) and got["lines"] == text.count(b"\n") + (0 if text.endswith(b"\n") else 1)


GOOD = b"1,2,3\n4,5,6\n7,8,9\n"


def offence(text, n=3, sep=","):
    with pytest.raises(M.Offence) as e:
        M.read([text], [0], n, sep)
    return e.value.key()


def test_every_offence_kind_is_seen_at_its_place():
    assert M.read([GOOD], [0], 3, ",")["total"] == 45
    assert offence(b"1,2,3\n4,x,6\n7,8,9\n") == (M.ERR_IO, "bad byte", 0, 8, 2, 1)
    assert offence(b"1,2,3\n4,5,6\r7,8,9\n")[:4] == (M.ERR_IO, "bad byte", 0, 11)                 # a '\r' not before '\n'
    assert offence(b"1,2,3\n4,\x00,6\n7,8,9\n")[:4] == (M.ERR_IO, "bad byte", 0, 8)
    assert offence(b"1,2,3\n4,-5,6\n7,8,9\n")[:4] == (M.ERR_IO, "bad byte", 0, 8)
    assert offence(b",1,2\n4,5,6\n7,8,9\n") == (M.ERR_IO, "empty value", 0, 0, 1, 0)
    assert offence(b"1,,3\n4,5,6\n7,8,9\n") == (M.ERR_IO, "empty value", 0, 2, 1, 1)
    assert offence(b"1,2,\r\n4,5,6\n7,8,9\n") == (M.ERR_IO, "empty value", 0, 4, 1, 2)           # the terminator's first byte
    assert offence(b"1,2,3\n4,5,6\n7,8,") == (M.ERR_IO, "empty value", 0, 16, 3, 2)                # the piece's size
    assert offence(b"1,2,3\n4," + b"1" * 20 + b",6\n7,8,9\n") == (M.ERR_IO, "long value", 0, 27, 2, 1)
    assert offence(b"1,2,3\n4," + b"0" * 25 + b",6\n7,8,9\n")[:4] == (M.ERR_IO, "long value", 0, 27)
    assert offence(b"1,2,3\n4,01099511627777,6\n7,8,9\n") == (M.ERR_RANGE, "value above 2^40", 0, 8, 2, 1)
    assert M.read([b"1,2,3\n4,1099511627776,6\n7,8,9\n"], [0], 3, ",")["total"] == 40 + 2 ** 40
    assert offence(b"1,2,3\n4,5\n7,8,9\n") == (M.ERR_IO, "ragged line", 0, 9, 2, 1)
    assert offence(b"1,2,3\n4,5,6,7\r\n7,8,9\n") == (M.ERR_IO, "ragged line", 0, 13, 2, 3)
    assert offence(b"1,2,3\n4,5,6\n7,8") == (M.ERR_IO, "ragged line", 0, 15, 3, 1)
    assert offence(GOOD + b"\n\n1,2,3\n") == (M.ERR_IO, "too many rows", 0, 20, 6, 0)
    assert offence(b"1,2,3\n\n4,5,6\n") == (M.ERR_IO, "too few rows", 0, 13, 4, 0)
    assert offence(b"") == (M.ERR_IO, "too few rows", 0, 0, 1, 0)
    assert offence(b"1,2,3\n4," + b"9" * 19 + b",6\n7,8,9\n")[:4] == (M.ERR_RANGE, "value above 2^40", 0, 8)


def test_the_least_piece_and_offset_win_and_the_header_order_breaks_a_tie():
    assert offence(b"1,2,3\n4,5\n7,x,9\n")[:4] == (M.ERR_IO, "ragged line", 0, 9)
    assert offence(b"1,x,3\n4,5\n7,8,9\n")[:4] == (M.ERR_IO, "bad byte", 0, 2)
    assert offence(GOOD + b"x,2,3\n")[:4] == (M.ERR_IO, "bad byte", 0, 18)                           # a bad byte and row n + 1 at one place
    assert offence(GOOD + b",2,3\n")[:4] == (M.ERR_IO, "empty value", 0, 18)
    assert offence(b"1,2,3\n4,5,") == (M.ERR_IO, "empty value", 0, 10, 2, 2)                        # empty value, then too few rows, at the size
    assert offence(b"1,2,3\n4,5") == (M.ERR_IO, "ragged line", 0, 9, 2, 1)
    with pytest.raises(M.Offence) as e:
        M.read([GOOD, b"1,2,3\n4,5\n7,8,9\n", b"x"], [0, 1, 2], 3, ",")
    assert e.value.key() == (M.ERR_IO, "ragged line", 1, 9, 2, 1)
    got = M.read([GOOD, GOOD], [3, 3], 3, ",")
    assert got["total"] == 90 and [e[0] for e in got["entries"]] == [3] * 18 and got["pieces"] == 2
