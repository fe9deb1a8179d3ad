"""GPU: .matrix adjacency text into the flow table (include/dge.h: dge_flows_add_matrix_texts / _files; csrc/matrix_read.hip) against tests/matrix_ref.py, the
second reading of the rule, and against the existing writer.  Every comparison is exact equality.  Texts and references are made once and shared."""
import re

import numpy as np
import pytest

import matrix_ref as M

pytestmark = pytest.mark.gpu
MIN = 256                                                     # csrc/matrix_feed.h: MAT_SLAB_MIN
COUNTERS = ("bytes", "lines", "rows", "values", "entries", "zeros", "total", "pieces", "n")
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def regions(dge, n, seed=0):
    """n regions whose ids are neither ascending by index nor all positive"""
    def make():
        ids = np.random.default_rng(1000 + seed + n).permutation(np.arange(-(n // 3), n - n // 3)).astype(np.int64) * 7
        return dge.Regions.from_ids(ids), ids
    return cached(("regions", n, seed), make)


def rows_of(ids, select=None):
    """text row / column i -> region index: the selected regions in ascending id"""
    return [int(r) for r in np.argsort(ids, kind="stable") if select is None or select[r]]


def spell(a, sep, zeros_rng=None, end="\n", last=True, empty_at=()):
    lines = []
    for i, row in enumerate(a.tolist()):
        if i in empty_at:
            lines.append("")
        lines.append(sep.join(("0" * int(zeros_rng.integers(0, 3)) if zeros_rng is not None else "") + str(v) for v in row))
    if len(a) in empty_at:
        lines.append("")
    return (end.join(lines) + (end if last else "")).encode()


def matrix(n, density, digits, seed, longest=False):
    """values of 1 .. digits digits, 2^40 at most; longest: of `digits` digits all"""
    rng = np.random.default_rng(seed)
    hi = np.minimum(10 ** rng.integers(digits if longest else 1, digits + 1, (n, n)).astype(np.float64), 2.0 ** 40).astype(np.int64)
    a = np.where(rng.random((n, n)) < density, rng.integers(10 ** (digits - 1) if longest else hi // 10, hi), 0).astype(np.int64)
    if density > 0 and digits >= 13:
        a[rng.integers(n), rng.integers(n)] = 2 ** 40
    return a


def with_entries(dge, rg, entries, idx, onto=None):
    """the table add_entries gives on the reference's entries (on top of the table `onto`)"""
    f = dge.Flows(rg)
    if onto is not None:
        f.add_entries(*onto.to_host())
    if entries:
        h, r, c, v = zip(*entries)
        f.add_entries(np.array(h, np.int32), np.array([idx[i] for i in r], np.int32), np.array([idx[j] for j in c], np.int32), np.array(v, np.int64))
    return f


def state(f):
    info = f.info()
    info.pop("kernel_ms")
    return [a.tolist() for a in f.to_host()], info


def counters(info):
    return {k: info[k] for k in COUNTERS}


def ref_counters(ref):
    out = {k: ref[k] for k in COUNTERS if k != "entries"}
    out["entries"] = len(ref["entries"])
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 31, 32, 33, 130])
def test_grammar_sweep(dge, n):
    rg, ids = regions(dge, n)
    idx = rows_of(ids)
    shapes = [(0.0, 1, "\n", True, ()), (0.05, 13, "\r\n", True, (0,)), (0.5, 6, "\n", False, (n // 2,)), (1.0, 13, "\n", True, (0, n // 2, n))]
    if n == 130:
        shapes = shapes[1:2] + shapes[3:]
    for sep in (",", " ", "\t"):
        for k, (density, digits, end, last, empty_at) in enumerate(shapes if sep == "," or n < 130 else shapes[-1:]):
            a = matrix(n, density, digits, 17 * n + k, longest=n == 130 and density == 1.0)
            text = spell(a, sep, np.random.default_rng(k) if k % 2 else None, end, last, empty_at)
            ref = cached(("ref", n, sep, k), lambda: M.read([text], [7], n, sep))
            assert len(ref["entries"]) == np.count_nonzero(a)
            want = cached(("want", n, sep, k), lambda: state(with_entries(dge, rg, ref["entries"], idx)))
            for slab in (MIN, MIN + 1, 0):
                f = dge.Flows(rg)
                info = f.add_matrix(text, 7, sep=sep, slab_bytes=slab)
                assert state(f) == want, (n, sep, k, slab)
                assert counters(info) == ref_counters(ref), (n, sep, k, slab)
                assert info["slabs"] == 1 if slab == 0 else info["slabs"] >= len(text) // (MIN + 1)
            if n == 130 and density == 1.0:
                tile = info["tile_bytes"]
                assert tile == 8192 and len(text) > 200000
                digit = np.isin(np.frombuffer(text, np.uint8), np.arange(48, 58))
                for edge in (32, tile):                       # a value stands across a lane edge and across a tile edge
                    at = np.arange(edge, len(text), edge)
                    assert np.any(digit[at - 1] & digit[at]), edge
                f = dge.Flows(rg)
                assert f.add_matrix(text, 7, sep=sep, slab_bytes=MIN)["slabs"] > len(text) // MIN          # slab edges between the values of a line


def test_one_long_line(dge):
    """no limit on a line's length, and a line far longer than a slab"""
    rg, ids = cached("long regions", lambda: (dge.Regions.from_ids(np.arange(70000, dtype=np.int64)[::-1].copy()), np.arange(70000, dtype=np.int64)[::-1]))
    one = np.zeros(70000, np.uint8); one[123] = 1
    f = dge.Flows(rg)
    before = state(f)
    text = b"0," * 69999 + b"0\n"
    with pytest.raises(dge.DgeError) as e:
        f.add_matrix(text, 0, select=one)
    assert e.value.code == M.ERR_IO and "ragged line at piece 0, offset %d, line 1, column 69999: 70000 values found, 1 expected" % (len(text) - 1) in str(e.value)
    assert state(f) == before
    n = 300
    sel = np.zeros(70000, np.uint8); sel[np.random.default_rng(5).choice(70000, n, replace=False)] = 1
    idx = rows_of(ids, sel)
    a = matrix(n, 1.0, 13, 99, longest=True)
    assert a.min() >= 10 ** 12
    text = spell(a, ",")
    assert len(text) / n > 4000
    info = f.add_matrix(text, 3, select=sel, slab_bytes=MIN)
    assert info["slabs"] > len(text) // MIN and info["entries"] == n * n and info["total"] == int(a.sum()) and info["rows"] == n
    r, c = np.nonzero(a)
    want = with_entries(dge, rg, [(3, int(i), int(j), int(a[i, j])) for i, j in zip(r, c)], idx)
    assert state(f) == state(want)


def seeded_table(dge):
    """130 regions, all 24 hours, about 2 500 entries"""
    def make():
        rg, ids = regions(dge, 130, seed=9)
        rng = np.random.default_rng(77)
        m = 2600
        keys = {}
        for h, s, e, w in zip(rng.integers(0, 24, m).tolist(), rng.integers(0, 130, m).tolist(), rng.integers(0, 130, m).tolist(),
                              (10 ** rng.uniform(0, 12, m)).astype(np.int64).tolist()):
            keys[(h, s, e)] = w
        keys[next(iter(keys))] = 2 ** 40
        f = dge.Flows(rg)
        k = list(keys)
        f.add_entries(np.array([x[0] for x in k], np.int32), np.array([x[1] for x in k], np.int32), np.array([x[2] for x in k], np.int32), np.array([keys[x] for x in k], np.int64))
        select = np.zeros(130, np.uint8); select[rng.choice(130, 97, replace=False)] = 1
        return rg, ids, f, select
    return cached("seeded", make)


HOURLY = [(h, 1) for h in range(24)]


@pytest.mark.parametrize("sep", [",", " ", "\t"])
def test_round_trip_with_the_writer(dge, sep, tmp_path):
    rg, ids, f, select = seeded_table(dge)
    assert 2400 < f.info()["entries"] < 2700 and not np.all(np.diff(ids) > 0) and ids.min() < 0
    texts = [f.matrix_text(h, windows=HOURLY, sep=sep, select=select) for h in range(24)]
    g = dge.Flows(rg)
    info = g.add_matrix(texts, range(24), sep=sep, select=select, slab_bytes=MIN if sep == " " else 0)
    assert info["pieces"] == 24 and info["n"] == 97 and info["rows"] == 24 * 97 and info["values"] == 24 * 97 * 97
    hour, src, dst, count = f.to_host()
    keep = (select[src] != 0) & (select[dst] != 0)
    assert 1000 < keep.sum() == info["entries"]
    assert [a.tolist() for a in g.to_host()] == [a[keep].tolist() for a in (hour, src, dst, count)]
    assert g.info()["trips"] == g.info()["mapped"] == int(count[keep].sum()) == info["total"]
    assert [g.matrix_text(h, windows=HOURLY, sep=sep, select=select) for h in range(24)] == texts
    if sep == ",":                                            # the same through files
        paths = [str(tmp_path / ("taxi-h%d.matrix" % h)) for h in range(24)]
        f.write_matrix(paths, windows=HOURLY, sep=sep, select=select)
        g2 = dge.Flows(rg)
        assert counters(g2.add_matrix(paths, range(24), sep=sep, select=select)) == counters(info) and state(g2) == state(g)
        with pytest.raises(dge.DgeError) as e:
            g2.add_matrix(paths[:3] + [str(tmp_path / "absent.matrix")], range(4), select=select)
        assert e.value.code == M.ERR_IO and "absent.matrix" in str(e.value) and state(g2) == state(g)


def test_additivity(dge):
    rg, ids, f, select = seeded_table(dge)
    idx = rows_of(ids)
    texts = [spell(matrix(130, 0.05, 9, seed), ",") for seed in (41, 42)]          # nine digits: twice a value, and a value on top of the table's, stay below 2^40
    ref = M.read(texts, [4, 5], 130, ",")
    once = with_entries(dge, rg, ref["entries"], idx)
    g = dge.Flows(rg)
    g.add_matrix(texts, [4, 5])
    assert state(g) == state(once)
    g.add_matrix(texts, [4, 5])
    twice = [a.tolist() for a in g.to_host()]
    assert twice[:3] == state(once)[0][:3] and twice[3] == [2 * c for c in state(once)[0][3]]
    # onto a table that is not empty (in an hour away from its one key of 2^40); two pieces under one hour add
    hour, _, _, count = f.to_host()
    h9 = int(hour[np.argmax(count)] + 1) % 24
    onto = dge.Flows(rg)
    onto.add_entries(*f.to_host())
    onto.add_matrix(texts, [h9, h9])
    assert state(onto) == state(with_entries(dge, rg, [(h9,) + e[1:] for e in ref["entries"]], idx, onto=f))
    both = with_entries(dge, rg, [(h9,) + e[1:] for e in ref["entries"]], idx)
    assert both.info()["entries"] < len(ref["entries"])        # the two pieces share keys
    # a key's total above 2^40 is refused and leaves the table alone
    big = dge.Flows(rg)
    top = b"\n".join(b",".join(b"1099511627776" if (i, j) == (0, 0) else b"0" for j in range(130)) for i in range(130)) + b"\n"
    big.add_matrix(top, 1)
    before = state(big)
    with pytest.raises(dge.DgeError) as e:
        big.add_matrix(top.replace(b"1099511627776", b"1"), 1)
    assert e.value.code == M.ERR_RANGE and "2^40" in str(e.value) and state(big) == before


WHERE = re.compile(r": ([a-z0-9^ ]+) at piece (\d+)(?: \(.*?\))?, offset (\d+), line (\d+), column (\d+)")


def refused(dge, f, pieces, hours, n, sep=",", **kw):
    """the call must be refused as the reference refuses the text, and leave the table as it was"""
    before = state(f)
    with pytest.raises(M.Offence) as want:
        M.read(pieces, hours, n, sep)
    with pytest.raises(dge.DgeError) as e:
        f.add_matrix(pieces, hours, sep=sep, **kw)
    m = WHERE.search(str(e.value))
    assert m, str(e.value)
    assert (e.value.code, m.group(1)) + tuple(int(x) for x in m.groups()[1:]) == want.value.key(), str(e.value)
    assert state(f) == before
    return want.value


def test_offences(dge):
    n = 33
    rg, ids = regions(dge, n)
    f = dge.Flows(rg)
    f.add_entries(np.array([1], np.int32), np.array([2], np.int32), np.array([3], np.int32), np.array([5], np.int64))
    good = spell(matrix(n, 0.6, 9, 4), ",", end="\r\n")
    assert len(good) > 6 * MIN
    at = 3 * MIN + good[3 * MIN:].index(b",")                  # a separator behind the first slabs of the piece
    line_end = good.index(b"\r\n", at)
    plants = {
        "bad byte": good[:at + 1] + b"-" + good[at + 1:],
        "bad byte (nul)": good[:at + 1] + b"\x00" + good[at + 1:],
        "bad byte (cr)": good[:at] + b"\r" + good[at:],
        "empty value": good[:at] + b"," + good[at:],
        "empty value at a terminator": good[:line_end] + b"," + good[line_end:],
        "long value": good[:at + 1] + b"0" * 20 + good[at + 1:],
        "value above 2^40": good[:at + 1] + b"001099511627777," + good[at + 1:],
        "ragged line": good[:at] + b"\n" + good[at + 1:],
        "ragged line (long)": good[:line_end] + b",7" + good[line_end:],
        "too many rows": good + b"\r\n\r\n5",
        "too few rows": good[:good.rindex(b"\r\n", 0, len(good) - 2) + 2],
        "cut short": good[:at],
        "empty value at the end": good[:-2] + b",",
    }
    kinds = set()
    for name, bad in plants.items():
        for slab in (MIN, 0):
            o = refused(dge, f, [good, bad], [0, 1], n, slab_bytes=slab)
            assert o.piece == 1 and (o.offset >= 3 * MIN), name
        kinds.add(o.kind)
    assert kinds == set(range(1, 8))
    # two offences in one text: the lesser offset wins; in two pieces: the lesser piece
    both = plants["bad byte"]
    both = both[:line_end + 40] + b"," + both[line_end + 40:]
    assert refused(dge, f, [good, both], [0, 1], n, slab_bytes=MIN).kind == M.BAD_BYTE
    both = plants["empty value"][:MIN + 7] + b"x" + plants["empty value"][MIN + 8:]
    assert refused(dge, f, [good, both], [0, 1], n, slab_bytes=MIN).offset == MIN + 7
    assert refused(dge, f, [plants["ragged line"], plants["bad byte"]], [0, 1], n).piece == 0
    assert refused(dge, f, [good, b"", good], [0, 1, 2], n).key() == (M.ERR_IO, "too few rows", 1, 0, 1, 0)
    # and nothing is wrong with the good text
    f.add_matrix([good, good], [0, 1], slab_bytes=MIN)
    assert f.info()["entries"] > 1
    # no regions: a piece may hold empty lines and nothing else, and a select array is an argument error
    none = dge.Flows(dge.Regions.from_ids([]))
    info = none.add_matrix(b"\n\r\n", 4)
    assert (info["lines"], info["rows"], info["values"], info["entries"], info["n"]) == (2, 0, 0, 0, 0) and none.info()["entries"] == 0
    import ctypes as C
    from embedding_amd._native import MatrixReadOptions
    text = (C.c_char_p * 1)(b"\n"); size = (C.c_int64 * 1)(1); hour = (C.c_int32 * 1)(0); opt = MatrixReadOptions(ord(","), 0, 0)
    assert dge.lib.dge_flows_add_matrix_texts(none._h, text, size, hour, 1, C.create_string_buffer(1), C.byref(opt), None) == 1
    assert "select" in dge.lib.dge_last_error().decode()
    with pytest.raises(M.Offence):
        M.read([b"1\n"], [0], 0, ",")
    with pytest.raises(dge.DgeError, match="too many rows at piece 0, offset 0, line 1, column 0"):
        none.add_matrix(b"1\n", 4)


def test_nmf_of_the_table_read_from_text(dge):
    rg, ids, f, _ = seeded_table(dge)
    g = dge.Flows(rg)
    g.add_matrix([f.matrix_text(h, windows=HOURLY) for h in range(24)], range(24))
    for slot in (0, 17):
        W1, H1, ids1, _ = f.nmf(slot, T=24, rank=5, max_iter=30)
        W2, H2, ids2, _ = g.nmf(slot, T=24, rank=5, max_iter=30)
        assert np.array_equal(ids1, ids2) and np.array_equal(W1.view(np.int64), W2.view(np.int64)) and np.array_equal(H1.view(np.int64), H2.view(np.int64))
        assert np.abs(W1).sum() > 0


def test_a_text_above_two_to_the_31_bytes(dge):
    """33 000 regions: 2.18 GB of "0," with a few values planted; then a bad byte behind the 2^31 mark"""
    n = 33000
    rg = dge.Regions.from_ids(np.arange(n, dtype=np.int64))
    zero = b"0," * (n - 1) + b"0\n"
    first = b"0,7,1099511627776," + b"0," * (n - 4) + b"12\n"
    mid = b"0," * 100 + b"345," + b"0," * (n - 102) + b"0\n"
    last = b"0," * (n - 1) + b"0099\n"
    text = bytearray(first)
    text += zero * (n // 2 - 1)
    text += mid
    text += zero * (n - n // 2 - 2)
    text += last
    assert len(text) > 2 ** 31 + 2 ** 20
    f = dge.Flows(rg)
    info = f.add_matrix(text, 11)
    assert info["bytes"] == len(text) > 2 ** 31 and info["rows"] == info["lines"] == n and info["values"] == n * n and info["entries"] == 5
    hour, src, dst, count = f.to_host()
    assert hour.tolist() == [11] * 5
    assert list(zip(src.tolist(), dst.tolist(), count.tolist())) == [(0, 1, 7), (0, 2, 2 ** 40), (0, n - 1, 12), (n // 2, 100, 345), (n - 1, n - 1, 99)]
    before = state(f)
    at = 2 ** 31 + 12345
    at += text[at:at + 4].index(b",") + 1                      # a "0" behind the mark
    line, column = 1 + text.count(b"\n", 0, at), text.count(b",", text.rindex(b"\n", 0, at) + 1, at)
    text[at:at + 1] = b"x"
    with pytest.raises(dge.DgeError) as e:
        f.add_matrix(text, 11)
    assert e.value.code == M.ERR_IO and "bad byte at piece 0, offset %d, line %d, column %d" % (at, line, column) in str(e.value)
    assert state(f) == before
