"""CPU: tests/counts_ref.py, the second reading of the count-table reader's rule, is sound — it gives what a scalar loop written from the reference's
getLEHDfeatures_helper (P/embeddingEvaluation_tract.py:512-536) gives on a RAC-shaped text — and sensitive: its answer moves when the key slice, col_lo,
skip_lines or the foreign filter is changed."""
import numpy as np
import pytest

import counts_ref as CR

TRACTS = [10100, 10201, 10202, 20100, 330100, 839100, 839200, 980000]
WANTED = [10201, 20100, 839100, 980000, 555555]                     # one of them is in no line


def helper_loop(text, keys):
    """getLEHDfeatures_helper, line for line: readline() for the header, strip / split, int(ls[0][5:11]), `tid in keys`, ls[8:28] added up per tract"""
    acs = {}
    lines = text.decode().split("\n")[1:]
    for l in lines:
        if not l:
            continue
        ls = l.strip().split(",")
        tid = int(ls[0][5:11])
        if tid in keys:
            vec = np.array([int(e) for e in ls[8:28]], np.int64)
            acs[tid] = vec if tid not in acs else acs[tid] + vec
    return acs


@pytest.fixture(scope="module")
def text():
    return CR.lehd_text(TRACTS, 400, seed=5)


def lehd(text, ids=WANTED, **kw):
    args = dict(sep=",", skip_lines=1, key_field=0, key=(5, 11), cols=(8, 20))
    args.update(kw)
    return CR.read([text], ids, 20, **args)


def test_the_reading_gives_what_the_reference_loop_gives(text):
    got = lehd(text)
    acs = helper_loop(text, WANTED)
    assert sorted(acs) == [10201, 20100, 839100, 980000]
    for i, tid in enumerate(sorted(WANTED)):
        assert (got["table"][i] == acs.get(tid, np.zeros(20, np.int64))).all()
    assert got["lines"] == 401 and got["skipped"] == 1 and got["empty"] == 0 and got["rows"] + got["foreign"] == 400
    assert got["rows"] == sum(1 for l in text.split(b"\n")[1:] if l and int(l[5:11]) in WANTED)
    assert got["values"] == 20 * got["rows"] and got["total"] == int(got["table"].sum()) == sum(e[2] for e in got["entries"])


def test_the_reading_moves_with_every_parameter(text):
    base = lehd(text)["table"]
    assert not (lehd(text, key=(5, 10))["table"] == base).all()           # another slice: other keys, most of them foreign
    assert not (lehd(text, cols=(9, 20))["table"] == base).all()
    everyone = lehd(text, ids=TRACTS)                                      # the foreign filter is the region set
    assert everyone["foreign"] == 0 and lehd(text)["foreign"] > 0 and everyone["total"] > lehd(text)["total"]
    with pytest.raises(CR.Offence) as e:                                    # the header is a line like any other when it is not skipped
        lehd(text, skip_lines=0)
    assert e.value.tuple() == (CR.SHORT_KEY, 0, 0, 1, 0)
    two = lehd(text, skip_lines=2)
    assert two["rows"] + two["foreign"] == 399


def test_terminators_lines_and_offence_places():
    t = b"h\r\n17031000100,5,6\r\r\n17031000200,7,8\n17031-00100,1,2"
    got = CR.read([t], [100, 200], 4, skip_lines=1, key=(5, 0), cols=(1, 2), neg_col_offset=2)
    assert got["table"].tolist() == [[5, 6, 1, 2], [7, 8, 0, 0]] and got["lines"] == 5 and got["empty"] == 1
    with pytest.raises(CR.Offence) as e:
        CR.read([t], [100, 200], 4, skip_lines=1, key=(5, 0), cols=(1, 2))
    assert e.value.tuple() == (CR.KEY_SIGN, 0, t.index(b"-"), 5, 0)
    cases = [(b"17031000100,5", CR.SHORT_LINE, 13, 1), (b"1703,5,6", CR.SHORT_KEY, 0, 0), (b"17031x00100,5,6", CR.BAD_KEY, 5, 0), (b"17031000100,,6", CR.EMPTY_VALUE, 12, 1),
             (b"17031000100,5,6 ", CR.BAD_VALUE_BYTE, 15, 2), (b"17031000100,5," + b"1" * 20, CR.LONG_VALUE, 33, 2), (b"17031000100,1099511627777,6", CR.BIG_VALUE, 12, 1),
             (b"17031" + b"1" * 19 + b",5,6", CR.BAD_KEY, 23, 0), (b"17031000100,5," + b"1" * 19 + b"x", CR.BAD_VALUE_BYTE, 33, 2)]
    for line, kind, offset, field in cases:
        with pytest.raises(CR.Offence) as e:
            CR.read([b"17031000100,1,1\n", b"17031000100,1,1\n" + line], [100], 2, key=(5, 0), cols=(1, 2))
        assert e.value.tuple() == (kind, 1, 16 + offset, 2, field), line
    assert CR.read([b"17031000100,1099511627776," + b"0" * 18 + b"7\n"], [100], 2, key=(5, 0), cols=(1, 2))["table"].tolist() == [[2 ** 40, 7]]
    long_line = b"17031000100,1,1," + b"9" * 65536
    with pytest.raises(CR.Offence) as e:
        CR.read([b"\n" + long_line], [100], 2, key=(5, 0), cols=(1, 2))
    assert e.value.tuple() == (CR.LONG_LINE, 0, 1, 2, 0)
    assert CR.read([long_line[:65536]], [100], 2, key=(5, 0), cols=(1, 2))["rows"] == 1
