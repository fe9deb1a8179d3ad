"""GPU: count tables (include/dge.h: dge_counts_*; csrc/table_read.hip) against tests/counts_ref.py, the second reading of the reader's rule.  Every comparison
is exact equality — the int64 table, the counters, the whole offence — because nothing is floating point until vectors(), which is compared bit for bit with
numpy.  Texts and references are made once and shared."""
import re

import numpy as np
import pytest

import counts_ref as CR

pytestmark = pytest.mark.gpu
MIN = 131072                                                  # csrc/table_read.hip: TAB_SLAB_MIN
SLABS = (MIN, 200000, 0)
COUNTERS = ("bytes", "lines", "skipped", "empty", "rows", "foreign", "values", "total", "pieces")
LEHD = dict(sep=",", skip_lines=1, key_field=0, key=(5, 11), cols=(8, 20))
WHERE = re.compile(r": ([a-z0-9^ ]+) at piece (\d+)(?: \(.*?\))?, offset (\d+), line (\d+), field (\d+)")
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def regions(dge, ids):
    return cached(("regions", tuple(ids)), lambda: dge.Regions.from_ids(np.array(ids, np.int64)))


def counters(info):
    return {k: info[k] for k in COUNTERS}


def read_both(dge, pieces, ids, n_table_cols, slab_bytes=0, ref=None, **kw):
    """the device's table and counters equal the reference's -> (the Counts, the reference)"""
    ref = ref or CR.read([bytes(p) for p in pieces], ids, n_table_cols, **kw)
    c = dge.Counts(regions(dge, ids), n_table_cols)
    info = c.add_table(pieces, slab_bytes=slab_bytes, return_info=True, **kw)
    assert counters(info) == counters(ref), (slab_bytes, counters(info), counters(ref))
    assert np.array_equal(c.to_host(), ref["table"])
    assert c.info() == dict(regions=len(ids), cols=n_table_cols, nonzero=int((ref["table"] != 0).sum()), total=int(ref["table"].sum()))
    return c, ref, info


def refused(dge, c, pieces, ids, n_table_cols, slab_bytes=0, want=None, **kw):
    """the call is refused as the reference refuses the text, and leaves the table as it was -> the offence"""
    before = c.to_host()
    if want is None:
        with pytest.raises(CR.Offence) as w:
            CR.read(pieces, ids, n_table_cols, **kw)
        want = w.value
    with pytest.raises(dge.DgeError) as e:
        c.add_table(pieces, slab_bytes=slab_bytes, **kw)
    m = WHERE.search(str(e.value))
    assert m, str(e.value)
    assert (m.group(1),) + tuple(int(x) for x in m.groups()[1:]) == (CR.KIND_NAME[want.kind],) + want.tuple()[1:], (slab_bytes, str(e.value), want.tuple())
    assert e.value.code == (2 if want.kind == CR.BIG_VALUE else 7)          # DGE_ERR_RANGE, DGE_ERR_IO
    assert np.array_equal(c.to_host(), before)
    return want


# ------------------------------------------------------------------------------------------ 1: runs across every boundary
RUN_IDS = [100 + 37 * i for i in range(12)]
RUNS = (1, 2, 63, 64, 65, 255, 256, 257, 600)


def run_lines():
    """runs of equal keys in the lengths above, a foreign run behind each and single foreign lines inside the long ones: a third of the lines are foreign"""
    rng = np.random.default_rng(7)
    lines = []
    for k, n in enumerate(RUNS):
        keys = [RUN_IDS[(5 * k) % 12]] * n + [700000 + k] * (n // 2)
        for at in rng.integers(1, n, n // 80):
            keys[at] = 800000 + k                              # a foreign line inside the run
        for key in keys:
            vals = rng.integers(0, 10 ** int(rng.integers(1, 7)), 5)
            lines.append(b"17031%06d%04d,x,%s,tail" % (key, rng.integers(10000), b",".join(b"%d" % v for v in vals)))
    lines[300] = lines[300].replace(b",x,", b",x,1099511627776,", 1).rsplit(b",", 2)[0] + b",tail"        # a cell of 2^40
    return lines


def spell(lines, seed):
    """two header lines, the three terminators mixed, an empty line now and then, no terminator behind the last line"""
    rng = np.random.default_rng(seed)
    out = [b"h1,h2\r\n", b"\n"]
    for i, l in enumerate(lines):
        out.append(l)
        if i + 1 < len(lines):
            out.append((b"\n", b"\r\n", b"\r")[rng.integers(3)])
            if rng.integers(40) == 0:
                out.append((b"\n", b"\r\n")[rng.integers(2)])
    return b"".join(out)


def test_runs_across_wave_and_tile_edges(dge):
    lines = cached("run lines", run_lines)
    assert 1500 < len(lines) < 2400
    kw = dict(sep=",", skip_lines=2, key_field=0, key=(5, 11), cols=(2, 5))
    c, ref, _ = read_both(dge, [spell(lines, 1)], RUN_IDS, 5, **kw)
    assert ref["empty"] > 10 and abs(3 * ref["foreign"] - ref["lines"]) < ref["lines"] // 5 and ref["table"].max() >= 2 ** 40
    shuffled = [lines[i] for i in np.random.default_rng(2).permutation(len(lines))]
    d, ref2, _ = read_both(dge, [spell(shuffled, 3)], RUN_IDS, 5, **kw)
    assert np.array_equal(ref2["table"], ref["table"])          # the same multiset of lines


# ------------------------------------------------------------------------------------------ 2: slab independence
TRACTS = [10100 + 7 * i for i in range(40)]
WANTED = TRACTS[::2] + [999999]


def lehd(seed=11):
    def make():
        text = CR.lehd_text(TRACTS, 2000, seed)
        return text, CR.read([text], WANTED, 20, **LEHD)
    return cached(("lehd", seed), make)


def test_slab_independence_pieces_and_files(dge, tmp_path):
    text, ref = lehd()
    assert 280000 < len(text) < 420000 and text.count(b",") == 42 * 2001
    infos = []
    for slab in SLABS:
        infos.append(read_both(dge, [text], WANTED, 20, slab_bytes=slab, ref=ref, **LEHD)[2])
    assert infos[0]["slabs"] >= 3 and infos[1]["slabs"] == 2 and infos[2]["slabs"] == 1
    # three pieces cut at line ends, each with the header in front: the same rows
    ends = [text.index(b"\n", len(text) * k // 3) + 1 for k in (1, 2)]
    header = text[:text.index(b"\n") + 1]
    pieces = [text[:ends[0]], header + text[ends[0]:ends[1]], header + text[ends[1]:]]
    ref3 = CR.read(pieces, WANTED, 20, **LEHD)
    assert np.array_equal(ref3["table"], ref["table"]) and ref3["pieces"] == 3 and ref3["skipped"] == 3
    for slab in SLABS:
        read_both(dge, pieces, WANTED, 20, slab_bytes=slab, ref=ref3, **LEHD)
    paths = []
    for k, p in enumerate(pieces):
        paths.append(str(tmp_path / ("piece%d.csv" % k)))
        with open(paths[-1], "wb") as f:
            f.write(p)
    read_both(dge, paths, WANTED, 20, slab_bytes=MIN, ref=ref3, **LEHD)
    with pytest.raises(dge.DgeError) as e:
        dge.Counts(regions(dge, WANTED), 20).add_table([paths[0], str(tmp_path / "absent.csv")], **LEHD)
    assert e.value.code == 7 and "absent.csv" in str(e.value)


# ------------------------------------------------------------------------------------------ 3: options
def test_col_offset_puts_rac_and_wac_side_by_side(dge):
    rac, ref_rac = lehd(11)
    wac, ref_wac = lehd(12)
    c = dge.Counts(regions(dge, WANTED), 40)
    c.add_table(rac, **LEHD)
    c.add_table(wac, col_offset=20, **LEHD)
    assert np.array_equal(c.to_host(), np.hstack([ref_rac["table"], ref_wac["table"]]))
    with pytest.raises(dge.DgeError) as e:
        c.add_table(wac, col_offset=21, **LEHD)
    assert e.value.code == 1


def test_blank_separated_tweet_counts(dge):
    rng = np.random.default_rng(5)
    ids = [int(t) for t in rng.permutation(np.arange(1, 60) * 101)]
    text = b"".join(b"%d %s\n" % (t, b" ".join(b"%d" % v for v in rng.integers(0, 900, 24))) for t in ids + ids[:7] + [5, 6])
    c, ref, _ = read_both(dge, [text], ids[:50], 24, sep=" ", key=(0, 0), cols=(1, 24))
    assert ref["foreign"] == 9 + 2 and ref["rows"] == 50 + 7


def planted_flows(dge):
    def make():
        rng = np.random.default_rng(9)
        ids = rng.permutation(np.arange(1, 31) * 13).astype(np.int64)          # neither ascending by index nor contiguous
        rg = dge.Regions.from_ids(ids)
        f = dge.Flows(rg)
        n = 4000
        f.add_entries(rng.integers(0, 24, n).astype(np.int32), rng.integers(0, 30, n).astype(np.int32), rng.integers(0, 30, n).astype(np.int32), rng.integers(1, 10 ** 6, n))
        return ids, rg, f
    return cached("flows", make)


def test_the_time_series_text_comes_back(dge):
    ids, rg, f = planted_flows(dge)
    rank = {int(t): i for i, t in enumerate(sorted(ids.tolist()))}
    for select in (None, np.arange(30) % 3 != 1):
        text = f.time_series_text(select)
        got_ids, fin, fout = f.time_series(select)
        c = dge.Counts(rg, 48)
        info = c.add_table(text, cols=(1, 24), neg_col_offset=24, return_info=True)
        want = np.zeros((30, 48), np.int64)
        want[[rank[int(t)] for t in got_ids]] = np.hstack([fin, fout])
        assert np.array_equal(c.to_host(), want) and want.sum() > 0 and info["rows"] == 2 * len(got_ids) and info["foreign"] == 0
        assert np.array_equal(CR.read([text], ids, 48, cols=(1, 24), neg_col_offset=24)["table"], want)
    o = refused(dge, c, [text], ids, 48, cols=(1, 24))
    assert (o.kind, o.offset) == (CR.KEY_SIGN, text.index(b"-"))


# ------------------------------------------------------------------------------------------ 4: offences
def plant(text, line, make):
    """line `line` (0 = the header) of the text replaced by make(that line)"""
    lines = text.split(b"\n")
    lines[line] = make(lines[line])
    return b"\n".join(lines)


def set_field(k, value):
    return lambda l: b",".join(f if i != k else value for i, f in enumerate(l.split(b",")))


PLANTS = {
    CR.SHORT_LINE: lambda l: b",".join(l.split(b",")[:20]),
    CR.SHORT_KEY: set_field(0, b"17031"),
    CR.BAD_KEY: set_field(0, b"17031 10100"),
    CR.KEY_SIGN: set_field(0, b"17031-10100"),
    CR.EMPTY_VALUE: set_field(9, b""),
    CR.BAD_VALUE_BYTE: set_field(27, b"1.5"),
    CR.LONG_VALUE: set_field(8, b"0" * 20),
    CR.BIG_VALUE: set_field(10, b"1099511627777"),
    CR.LONG_LINE: lambda l: l + b"9" * 70000,
}


def test_offences(dge):
    text, ref = lehd()
    c = dge.Counts(regions(dge, WANTED), 20)
    c.add_table(text, **LEHD)
    assert np.array_equal(c.to_host(), ref["table"])
    late = 2 + text[:2 * MIN + 5000].count(b"\n")               # a line of the third slab
    for kind, make in PLANTS.items():
        for line in (100, late):
            bad = plant(text, line, make)
            with pytest.raises(CR.Offence) as w:
                CR.read([text, bad], WANTED, 20, **LEHD)
            assert w.value.kind == kind and w.value.piece == 1 and w.value.line == line + 1 and (line == 100 or w.value.offset > 2 * MIN)
            for slab in SLABS:
                refused(dge, c, [text, bad], WANTED, 20, slab_bytes=slab, want=w.value, **LEHD)
    # a value of exactly 2^40 is none
    ok = plant(text, 100, set_field(10, b"1099511627776"))
    read_both(dge, [ok], WANTED, 20, slab_bytes=MIN, **LEHD)
    # two kinds in one text, the later one first in the list: the place decides; two pieces: the piece decides
    two = plant(plant(text, late, PLANTS[CR.SHORT_KEY]), 100, PLANTS[CR.BIG_VALUE])
    for slab in SLABS:
        assert refused(dge, c, [two], WANTED, 20, slab_bytes=slab, **LEHD).kind == CR.BIG_VALUE
    assert refused(dge, c, [plant(text, late, PLANTS[CR.LONG_VALUE]), plant(text, 3, PLANTS[CR.SHORT_LINE])], WANTED, 20, slab_bytes=MIN, **LEHD).piece == 0
    # two on one line: the one in front; at one place: the one listed first (a short line ends where its last field is empty)
    assert refused(dge, c, [plant(plant(text, 7, set_field(12, b"x")), 7, set_field(20, b""))], WANTED, 20, **LEHD).kind == CR.BAD_VALUE_BYTE
    assert refused(dge, c, [plant(text, 7, lambda l: b",".join(l.split(b",")[:26]) + b",")], WANTED, 20, **LEHD).kind == CR.SHORT_LINE
    # on a foreign line the offence is reported all the same
    foreign = next(i for i, l in enumerate(text.split(b"\n")) if i > 0 and int(l[5:11]) not in WANTED)
    assert refused(dge, c, [plant(text, foreign, PLANTS[CR.EMPTY_VALUE])], WANTED, 20, **LEHD).line == foreign + 1
    # a line no slab holds: the reader's transport cuts it, the verdict is the same at every slab size; so is it behind a "\r\n" that a slab's end splits
    giant = plant(text, late, lambda l: l + b"9" * 300000)
    with pytest.raises(CR.Offence) as w:
        CR.read([giant], WANTED, 20, **LEHD)
    assert w.value.kind == CR.LONG_LINE
    for slab in SLABS:
        refused(dge, c, [giant], WANTED, 20, slab_bytes=slab, want=w.value, **LEHD)
    # a header no slab holds is a header all the same, not looked at; the line behind the headers is
    tall = b"h" * 140000 + b"\n"
    body = text[text.index(b"\n") + 1:]
    one, two = CR.read([tall + body], WANTED, 20, **LEHD), CR.read([body, tall + tall + body], WANTED, 20, **dict(LEHD, skip_lines=2))
    assert np.array_equal(one["table"], ref["table"]) and two["skipped"] == 4
    with pytest.raises(CR.Offence) as w:
        CR.read([tall + tall + body], WANTED, 20, **LEHD)
    assert w.value.tuple() == (CR.LONG_LINE, 0, 140001, 2, 0)
    for slab in SLABS:
        read_both(dge, [tall + body], WANTED, 20, slab_bytes=slab, ref=one, **LEHD)
        read_both(dge, [body, tall + tall + body], WANTED, 20, slab_bytes=slab, ref=two, **dict(LEHD, skip_lines=2))
        refused(dge, c, [tall + tall + body], WANTED, 20, slab_bytes=slab, want=w.value, **LEHD)
    head = text[:MIN - 400]
    head = head[:head.rindex(b"\n") + 1]
    line = text[len(head):text.index(b"\n", len(head))]
    split = head + line + b"," * (MIN - 1 - len(head) - len(line)) + b"\r\n" + b"7" * 200000 + b"\n"
    assert split[MIN - 1:MIN + 1] == b"\r\n"
    refused(dge, c, [split], WANTED, 20, slab_bytes=MIN, **LEHD)
    refused(dge, c, [split], WANTED, 20, **LEHD)


# ------------------------------------------------------------------------------------------ 5: range
def test_a_cell_above_two_to_the_62_is_refused(dge):
    ids = [100, 200]
    c = dge.Counts(regions(dge, ids), 2)
    half = b"200,0,1099511627776\n" * 2 ** 21
    for _ in range(2):
        info = c.add_table(half, cols=(1, 2), return_info=True)
        assert info["total"] == 2 ** 61 and info["rows"] == 2 ** 21
    want = [[0, 0], [0, 2 ** 62]]
    assert c.to_host().tolist() == want and c.info()["total"] == 2 ** 62
    for call in (lambda: c.add_table(b"100,5,5\n200,0,1\n", cols=(1, 2)), lambda: c.add_entries([1], [1], [1]), lambda: c.add_table(half + half + b"100,1,1\n", cols=(1, 2))):
        with pytest.raises(dge.DgeError) as e:
            call()
        assert e.value.code == 2 and c.to_host().tolist() == want
    c.add_table(b"100,5,5\n200,7,0\n", cols=(1, 2))
    assert c.to_host().tolist() == [[5, 5], [7, 2 ** 62]]
    with pytest.raises(dge.DgeError) as e:
        c.add_entries([0, 1], [0, 2], [1, 1])
    assert e.value.code == 1 and "entry 1" in str(e.value)
    with pytest.raises(dge.DgeError) as e:
        c.add_entries([0], [0], [2 ** 40 + 1])
    assert e.value.code == 1


# ------------------------------------------------------------------------------------------ 6: entries, points, merge
def test_add_entries_gives_the_readers_table(dge):
    text, ref = lehd()
    rng = np.random.default_rng(3)
    e = np.array(ref["entries"], np.int64)[rng.permutation(len(ref["entries"]))]
    c = dge.Counts(regions(dge, WANTED), 20)
    for part in np.array_split(e, 3):
        c.add_entries(part[:, 0], part[:, 1], part[:, 2])
    assert np.array_equal(c.to_host(), ref["table"]) and len(e) > 10000


def test_add_points_is_the_histogram_of_locate(dge):
    import trip_ref
    mesh, _ = trip_ref.quad_mesh(12, 20251018)
    rg = dge.Regions.from_arrays(*mesh.arrays())
    rng = np.random.default_rng(6)
    xy = np.stack([rng.uniform(-87.95, -87.35, 5000), rng.uniform(41.55, 42.15, 5000)], 1)
    hour = rng.integers(0, 24, 5000).astype(np.int32)
    region = rg.locate(xy)
    rank = np.argsort(np.argsort(np.array(mesh.ids)))
    want = np.zeros((len(mesh.ids), 24), np.int64)
    inside = region >= 0
    np.add.at(want, (rank[region[inside]], hour[inside]), 1)
    c = dge.Counts(rg, 24)
    assert c.add_points(xy, hour) == int((~inside).sum()) > 0
    assert np.array_equal(c.to_host(), want) and want.sum() == inside.sum() > 2000
    assert c.add_points(xy[:300], hour[:300]) == int((~inside[:300]).sum())
    np.add.at(want, (rank[region[:300][inside[:300]]], hour[:300][inside[:300]]), 1)
    assert np.array_equal(c.to_host(), want)
    with pytest.raises(dge.DgeError):
        c.add_points(xy[:2], [0, 24])
    assert np.array_equal(c.to_host(), want)


def test_merge_is_add_at(dge):
    text, ref = lehd()
    c = dge.Counts(regions(dge, WANTED), 20)
    c.add_table(text, **LEHD)
    groups = regions(dge, [3, 1, 2, 9])
    group_of = np.arange(len(WANTED), dtype=np.int32) % 3          # three groups get rows, the fourth stays empty
    group_of[5] = -1
    want = np.zeros((4, 20), np.int64)
    np.add.at(want, group_of[group_of >= 0], ref["table"][group_of >= 0])
    m = c.merge(groups, group_of)
    assert np.array_equal(m.to_host(), want) and want[3].sum() == 0 and want[:3].sum(axis=1).min() > 0 and m.info()["regions"] == 4
    assert np.array_equal(c.to_host(), ref["table"])
    bad = group_of.copy()
    bad[2] = 4
    with pytest.raises(dge.DgeError) as e:
        c.merge(groups, bad)
    assert e.value.code == 1


# ------------------------------------------------------------------------------------------ 7: vectors
def test_vectors_are_numpy_bit_for_bit(dge):
    rng = np.random.default_rng(8)
    ids = list(range(10, 47))
    t = rng.integers(0, 10 ** rng.integers(1, 13, (37, 9)))
    t[4] = 0
    t[9, 2:] = 0
    t[11, 3] = 2 ** 40
    t[12] = [2 ** 40] * 9
    c = dge.Counts(regions(dge, ids), 9)
    r, k = np.nonzero(t)
    c.add_entries(r, k, t[r, k])
    assert np.array_equal(c.to_host(), t)
    for lo, n in ((0, 9), (2, 7), (8, 1)):
        part = t[:, lo:lo + n]
        s = part.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            normal = np.where(s[:, None] == 0, 0.0, part.astype(np.float64) / s[:, None].astype(np.float64)).astype(np.float32)
        for normalise, want in ((True, normal), (False, part.astype(np.float32))):
            for present, mask in (("all", np.ones(37, bool)), ("nonzero", s != 0)):
                v = c.vectors(cols=(lo, n), normalise=normalise, present=present)
                assert v.shape == (37, n) and np.array_equal(v.to_host().view(np.uint32), want.view(np.uint32)) and np.array_equal(v.present(), mask)
    assert (~(t[:, 2:].sum(axis=1) != 0)).sum() == 2
    with pytest.raises(dge.DgeError):
        c.vectors(cols=(5, 5))


def test_from_text_to_clustering_accuracy(dge):
    import embedding_amd.evaluate as ev
    text, ref = lehd()
    ids40 = TRACTS[:38] + [999998, 999999]                        # two regions no line names
    ref40 = CR.read([text], ids40, 20, **LEHD)
    c = dge.Counts(regions(dge, ids40), 20)
    c.add_table(text, **LEHD)
    v = c.vectors(normalise=True, present="nonzero")
    s = ref40["table"].sum(axis=1)
    assert (s == 0).sum() == 2 and np.array_equal(v.present(), s != 0)
    rows = np.where(s[:, None] == 0, 0.0, ref40["table"] / np.maximum(s, 1)[:, None].astype(np.float64)).astype(np.float32)
    w = dge.Vectors.from_host(rows, present=s != 0)
    gnd = (np.arange(40) % 4).astype(np.int32)
    got = ev.clustering_accuracy_vectors(v, gnd, 4, seed=1)
    want = ev.clustering_accuracy_vectors(w, gnd, 4, seed=1)
    assert np.array_equal(got[1], want[1]) and got[0] == want[0] and np.array_equal(got[2]["cnt"], want[2]["cnt"]) and (got[1] >= 0).sum() == 38


# ------------------------------------------------------------------------------------------ 8: offsets beyond 32 bits
def test_a_text_above_two_to_the_31_bytes(dge):
    """one block of LEHD-shaped lines repeated until the text passes 2^31 bytes; then an offence behind the mark"""
    kw = dict(sep=",", skip_lines=1, key_field=0, key=(5, 11), cols=(8, 4))
    whole = CR.lehd_text(TRACTS, 6000, 21)
    header, block = whole[:whole.index(b"\n") + 1], whole[whole.index(b"\n") + 1:]
    times = (2 ** 31 + 2 ** 22) // len(block) + 1
    text = bytearray(header)
    text += block * times
    assert len(text) > 2 ** 31 + 2 ** 22
    one = CR.read([block], WANTED, 4, **dict(kw, skip_lines=0))
    c = dge.Counts(regions(dge, WANTED), 4)
    info = c.add_table(text, return_info=True, **kw)
    assert info["bytes"] == len(text) and info["lines"] == 1 + 6000 * times and info["rows"] == one["rows"] * times and info["total"] == one["total"] * times
    assert np.array_equal(c.to_host(), one["table"] * times)
    at = text.index(b"\n", 2 ** 31 + 12345) + 1                 # a line behind the mark
    line = 1 + text.count(b"\n", 0, at)
    for _ in range(9):                                          # its second value: field 9
        at = text.index(b",", at) + 1
    text[at:at + 1] = b"x"
    before = c.to_host()
    with pytest.raises(dge.DgeError) as e:
        c.add_table(text, **kw)
    assert e.value.code == 7 and "bad value byte at piece 0, offset %d, line %d, field 9" % (at, line) in str(e.value)
    assert np.array_equal(c.to_host(), before)
