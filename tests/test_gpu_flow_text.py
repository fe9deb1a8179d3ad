"""GPU: the flow table out as text (include/dge.h: dge_flows_to_text, dge_flows_write_text, dge_flows_time_series and its two text forms;
csrc/flow_text.hip) against tests/flow_text_ref.py — the naive loops of the Java, "%d" formatting — and, for the .od kind over slots, against the host writer
Flows.to_od_bytes.  Every comparison is exact equality of bytes or integers.  Tables, regions and references are made once and shared."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_text_ref as ref  # noqa: E402
import trip_ref  # noqa: E402
from test_flow_text_ref import IDS as TINY_IDS, MASK as TINY_MASK, TABLE as TINY_TABLE  # noqa: E402

pytestmark = pytest.mark.gpu
TILE, SLAB = 4096, 16 << 20                                  # csrc/seq_out_plan.h
BIG = 2 ** 63 - 1
WINDOWS = [(0, 24), (22, 5), (22, 5), (7, 0), (3, 1), (23, 1), (20, 8)]          # overlapping, repeated, empty, one hour, past midnight
SLICE_SETS = [dict(T=1), dict(T=8), dict(T=24), dict(T=1, mode=ref.AS_TRACTS), dict(T=8, mode=ref.AS_TRACTS), dict(T=24, mode=ref.AS_TRACTS), dict(windows=WINDOWS)]
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def mesh(side):
    return cached(("mesh", side), lambda: trip_ref.quad_mesh(side, 20260101 + side)[0])


def regions_of(dge, side, ids):
    """the first len(ids) quads of a side x side mesh under the given ids"""
    ids = [int(i) for i in ids]
    return cached(("regions", side, tuple(ids)), lambda: dge.Regions.from_arrays(*trip_ref.Regions(ids, mesh(side).rings[:len(ids)]).arrays()))


def fuzz_ids(seed):
    rng = np.random.default_rng(100 + seed)
    some = rng.choice(np.arange(-50000, 50000), 40, replace=False).tolist()
    ids = [0, BIG, -BIG, -1] + [i for i in some if i not in (0, -1)][:33]
    return [ids[i] for i in rng.permutation(37)]


def fuzz_table(seed):
    """about 2 600 entries over 37 regions in all hours; counts of 1 to 6 digits, a few of 2^40"""
    rng = np.random.default_rng(seed)
    n = 2700
    c = {}
    for h, s, e, w in zip(rng.integers(0, 24, n).tolist(), rng.integers(0, 37, n).tolist(), rng.integers(0, 37, n).tolist(), (10 ** rng.uniform(0, 6, n)).astype(np.int64).tolist()):
        c[(h, s, e)] = w
    for k in rng.choice(len(c), 12, replace=False).tolist():
        c[list(c)[k]] = 2 ** 40
    return c


def arrays(c, order=None):
    keys = list(c) if order is None else [list(c)[i] for i in order]
    return (np.array([k[0] for k in keys], np.int32), np.array([k[1] for k in keys], np.int32), np.array([k[2] for k in keys], np.int32), np.array([c[k] for k in keys], np.int64))


W14 = [h * 2 ** 40 for h in (10, 24, 11)]                    # 14 digits: the longest weight a table can give — a key holds 2^40 at most, a slice 24 hours of it


def put(c, s, e, w):
    """the pair (s, e) with the all-day sum w: one entry, or — above 2^40 — w / 2^40 hours of 2^40 each"""
    if w <= 2 ** 40:
        c[(0, s, e)] = w
    else:
        assert w % 2 ** 40 == 0 and w >> 40 <= 24
        for h in range(w >> 40):
            c[(h, s, e)] = 2 ** 40


def fuzz(dge, seed):
    def make():
        ids, c = fuzz_ids(seed), fuzz_table(seed)
        f = dge.Flows(regions_of(dge, 7, ids))
        f.add_entries(*arrays(c))
        assert 2400 < len(c) == f.info()["entries"] and ref.table(*f.to_host()) == c
        return ids, c, f
    return cached(("fuzz", seed), make)


def half_mask(seed, R=37):
    return (np.random.default_rng(7 + seed).permutation(R) % 2).astype(np.uint8)


def state_of(f):
    return [a.tobytes() for a in f.to_host()], {k: v for k, v in f.info().items() if k != "kernel_ms"}


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


# ------------------------------------------------------------------------------------------ 1. fuzz
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_every_kind_over_slots_and_windows_equals_the_reference(dge, seed, tmp_path):
    ids, c, f = fuzz(dge, seed)
    before = state_of(f)
    mask = half_mask(seed)
    for q, sl in enumerate(SLICE_SETS):
        sums = ref.slices(c, **sl)
        S = len(sums)
        want_od = [ref.od_text(s, ids) for s in sums]
        want_layered = ref.od_layered(sums, ids)
        want_matrix = [ref.matrix_text(s, ids, b",") for s in sums]
        assert any(want_od) and (q != 6 or (want_od[1] == want_od[2] != b"" and want_od[3] == b""))
        # into files: every slice by one call each kind
        od = [str(tmp_path / ("%d_%d.od" % (q, k))) for k in range(S)]
        mx = [str(tmp_path / ("%d_%d.matrix" % (q, k))) for k in range(S)]
        lay = str(tmp_path / ("%d.layered.od" % q))
        info = f.write_od(od, **sl)
        assert [read(p) for p in od] == want_od
        assert (info["bytes"], info["lines"], info["edges"], info["zeros"], info["slices"]) == (sum(map(len, want_od)), sum(map(len, sums)), sum(map(len, sums)), 0, S)
        assert info["kernel_ms"] > 0 and info["write_ms"] > 0
        info = f.write_od(lay, layered=True, **sl)
        assert read(lay) == want_layered and (info["bytes"], info["lines"], info["slices"]) == (len(want_layered), sum(map(len, sums)), 1)
        info = f.write_matrix(mx, **sl)
        assert [read(p) for p in mx] == want_matrix
        assert (info["bytes"], info["lines"], info["edges"], info["zeros"], info["slices"]) == (sum(map(len, want_matrix)), 37 * S, sum(map(len, sums)), 37 * 37 * S - sum(map(len, sums)), S)
        # into memory: all .od slices, the layered text, two matrices with the other separators and the half mask
        assert f.od_text(**sl) == want_od
        assert f.od_text(layered=True, **sl) == want_layered
        if "windows" not in sl:
            assert f.to_od_bytes(sl["T"], sl.get("mode", ref.EVEN)) == want_od                      # the host writer a user has today
        for k, sep in ((0, " "), (S - 1, "\t")):
            assert f.matrix_text(k, sep=sep, **sl) == ref.matrix_text(sums[k], ids, sep.encode())
            assert f.matrix_text(k, sep=sep, select=mask, **sl) == ref.matrix_text(sums[k], ids, sep.encode(), mask)
    assert state_of(f) == before


# ------------------------------------------------------------------------------------------ 2. select
def test_a_mask_of_half_the_regions_and_a_mask_of_none(dge, tmp_path):
    ids, c, f = fuzz(dge, 1)
    mask, none = half_mask(1), np.zeros(37, np.uint8)
    assert 10 < mask.sum() < 27
    sums = ref.slices(c, windows=WINDOWS)
    paths = [str(tmp_path / ("%d.matrix" % k)) for k in range(len(sums))]
    info = f.write_matrix(paths, windows=WINDOWS, sep=" ", select=mask)
    want = [ref.matrix_text(s, ids, b" ", mask) for s in sums]
    n = int(mask.sum())
    assert [read(p) for p in paths] == want and want[3] == (b"0 " * (n - 1) + b"0\n") * n
    kept = sum(1 for s in sums for (a, b) in s if mask[a] and mask[b])
    assert info["lines"] == n * len(sums) and (info["edges"], info["zeros"]) == (kept, n * n * len(sums) - kept) and 0 < kept < sum(map(len, sums))
    info = f.write_matrix(paths, windows=WINDOWS, select=none)
    assert [read(p) for p in paths] == [b""] * len(sums) and (info["bytes"], info["lines"], info["slices"]) == (0, 0, len(sums))
    assert f.matrix_text(0, T=1, select=none) == b"" and f.time_series_text(none) == b""
    got = f.time_series(none)
    assert [a.shape for a in got] == [(0,), (0, 24), (0, 24)]
    with pytest.raises(ValueError):
        f.matrix_text(0, T=1, select=mask[:5])
    # a table without entries: all zeros, n lines
    empty = dge.Flows(f.regions)
    assert empty.matrix_text(0, T=1, select=mask) == (b"0," * (n - 1) + b"0\n") * n and empty.od_text(T=8) == [b""] * 8 and empty.od_text(windows=WINDOWS, layered=True) == b""


# ------------------------------------------------------------------------------------------ 3. tile edges
def big_ids(R, seed):
    return (1000 + 3 * np.random.default_rng(seed).permutation(R)).tolist()


@pytest.mark.parametrize("n", [2047, 2048, 2049])
def test_matrix_rows_of_a_tile_less_two_a_tile_and_a_tile_plus_two(dge, n):
    """n selected of 2 049 regions: an all-zero row is 2 n bytes.  1-digit and 14-digit entries in columns 0 and n - 1 and in the columns on both sides of every
    tile boundary of the first three rows (where the boundary falls in the all-zero text); two flows touch a region the mask leaves out.  (14 digits, not 15:
    24 * 2^40 is the largest sum a table can hold, and it has 14; the plan header's host test goes to 15.)"""
    R = 2049
    ids = big_ids(R, 5)
    mask = np.ones(R, np.uint8)
    by_id = ref.selected(ids, None)
    for rank in (5, 1000)[:R - n]:
        mask[by_id[rank]] = 0
    rows = ref.selected(ids, mask)                            # region indices of row / column 0 .. n - 1
    assert len(rows) == n and 2 * n in (TILE - 2, TILE, TILE + 2)
    cells = {}
    for i in range(3):
        cols = {0, n - 1}
        for b in range(TILE, 4 * 2 * n, TILE):               # boundaries that fall into row i of the all-zero text
            if b // (2 * n) == i:
                col = (b % (2 * n)) // 2
                cols |= {c for c in (col - 1, col, col + 1) if 0 <= c < n}
        for t, col in enumerate(sorted(cols)):
            cells[(i, col)] = [7, W14[0], 3, W14[1]][(t + i) % 4]
    cells[(n - 1, n - 1)] = 24 * 2 ** 40
    cells[(n - 1, 0)] = 5
    c = {}
    for (i, j), w in cells.items():
        put(c, rows[i], rows[j], w)
    for r in np.flatnonzero(mask == 0).tolist():              # dropped: an end is not selected
        c[(0, r, rows[0])] = 77
        c[(0, rows[1], r)] = 88
    f = dge.Flows(regions_of(dge, 46, ids))
    f.add_entries(*arrays(c))
    zero_row = b"0," * (n - 1) + b"0\n"
    want = []
    for i in range(n):
        mine = {j: w for (r, j), w in cells.items() if r == i}
        want.append(b",".join(b"%d" % mine.get(j, 0) for j in range(n)) + b"\n" if mine else zero_row)
    want = b"".join(want)
    got, info = f._text(f._slices(1, 0, None)[0], 2, 0, mask, ord(","), return_info=True)
    assert len(got) == len(want) and got == want
    assert (info["bytes"], info["lines"], info["edges"], info["zeros"]) == (len(want), n, len(cells), n * n - len(cells))


# ------------------------------------------------------------------------------------------ 4. slab edge
def test_a_matrix_across_the_slab_edge(dge):
    """n = 3 000: 18 MB.  Byte 2^24 of the all-zero text is row 2 796, column 608; three 14-digit entries (the longest a table can give) stand just before it,
    across it and just after it.  (Nothing in front of them has more than one digit: the place of byte 2^24 is that of the all-zero text.)"""
    n = 3000
    r0, c0 = SLAB // (2 * n), (SLAB % (2 * n)) // 2
    assert (r0, c0) == (2796, 608)
    ids = big_ids(n, 6)
    rows = ref.selected(ids, None)
    cells = {(r0, c0 - 10): W14[0], (r0, c0 - 9): W14[1], (r0, c0 - 8): W14[2], (r0, 0): 4, (r0, n - 1): W14[1], (r0 - 1, n - 1): 6, (r0 + 1, 0): W14[0], (0, 0): 1,
             (n - 1, n - 1): W14[1]}
    f = dge.Flows(regions_of(dge, 55, ids))
    c = {}
    for (i, j), w in cells.items():
        put(c, rows[i], rows[j], w)
    f.add_entries(*arrays(c))
    zero_row = b"0," * (n - 1) + b"0\n"
    want = []
    for i in range(n):
        mine = {j: w for (r, j), w in cells.items() if r == i}
        want.append(b",".join(b"%d" % mine.get(j, 0) for j in range(n)) + b"\n" if mine else zero_row)
    want = b"".join(want)
    assert want[SLAB - 1:SLAB + 1].isdigit() and want[SLAB - 20:SLAB + 20].count(b",") == 2 and b"%d," % W14[0] in want[SLAB - 30:SLAB] and b",%d" % W14[2] in want[SLAB:SLAB + 30]
    got = f.matrix_text(0, T=1)
    assert len(got) == len(want) > SLAB and got == want


def test_an_od_text_of_short_lines_across_the_slab_edge(dge):
    """1.4 M edges of 14 bytes each; the reference spells them in one vectorised pass"""
    R, E = 3000, 1_400_000
    ids = (10000 + 7 * np.random.default_rng(8).permutation(R)).astype(np.int64)
    rng = np.random.default_rng(9)
    pair = rng.choice(R * R, E, replace=False)
    s, e, w = (pair // R).astype(np.int32), (pair % R).astype(np.int32), rng.integers(1, 10, E).astype(np.int64)
    f = dge.Flows(regions_of(dge, 55, ids.tolist()))
    f.add_entries(np.full(E, 11, np.int32), s, e, w)
    order = np.lexsort((ids[e], ids[s]))
    lines = np.empty((E, 14), np.uint8)
    for col0, v in ((0, ids[s][order]), (6, ids[e][order])):
        for d in range(5):
            lines[:, col0 + d] = 48 + (v // 10 ** (4 - d)) % 10
    lines[:, 5] = lines[:, 11] = 32
    lines[:, 12] = 48 + w[order]
    lines[:, 13] = 10
    want = lines.tobytes()
    (got,) = f.od_text(T=1)
    assert len(got) == len(want) == 14 * E > SLAB and got == want
    assert f.od_text(T=2)[1] == b"" and f.od_text(T=2)[0] == want
    got = f.od_text(windows=[(11, 1), (10, 3)], layered=True)
    assert len(got) == 2 * 18 * E
    lay = np.frombuffer(got, np.uint8).reshape(2, E, 18)                    # "0-sssss 1-ddddd w\n" E times, then "1-sssss 0-ddddd w\n"
    for k in range(2):
        assert np.array_equal(lay[k][:, 2:7], lines[:, 0:5]) and np.array_equal(lay[k][:, 10:15], lines[:, 6:11]) and np.array_equal(lay[k][:, 15:], lines[:, 11:])
        assert (lay[k][:, 0] == 48 + k).all() and (lay[k][:, 8] == 48 + (k + 1) % 2).all() and (lay[k][:, (1, 9)] == 45).all() and (lay[k][:, 7] == 32).all()


# ------------------------------------------------------------------------------------------ 5. files
def test_files_are_truncated_written_in_slice_order_and_left_when_a_later_one_fails(dge, tmp_path):
    ids, c, f = fuzz(dge, 2)
    want = [ref.od_text(s, ids) for s in ref.slices(c, T=3)]
    paths = [str(tmp_path / ("%d.od" % k)) for k in range(3)]
    with open(paths[1], "wb") as fh:
        fh.write(b"x" * (len(want[1]) + 1000))                # a longer file is there already
    f.write_od(paths, T=3)
    assert [read(p) for p in paths] == want
    # an unwritable path at slice 1: slice 0 is complete, slice 2 is not begun
    for p in paths:
        os.remove(p)
    bad = str(tmp_path / "no" / "such" / "dir.od")
    with pytest.raises(dge.DgeError) as ei:
        f.write_od([paths[0], bad, paths[2]], T=3)
    assert ei.value.code == 7 and bad in str(ei.value) and "dge_flows_write_text" in str(ei.value)
    assert read(paths[0]) == want[0] and not os.path.exists(paths[2])
    ts = str(tmp_path / "series.txt")
    info = f.write_time_series(ts)
    assert read(ts) == ref.time_series_text(c, ids) and (info["lines"], info["bytes"], info["slices"]) == (74, os.path.getsize(ts), 1)
    with pytest.raises(dge.DgeError) as ei:
        f.write_time_series(bad)
    assert ei.value.code == 7 and bad in str(ei.value)


def test_a_buffer_one_byte_short_is_refused_and_left_alone(dge):
    from embedding_amd._native import FlowSlices
    ids, c, f = fuzz(dge, 2)
    want = ref.od_text(ref.slices(c, T=1)[0], ids)
    sl = FlowSlices(1, 0, 0, 0, None)
    buf = C.create_string_buffer(b"\xAA" * len(want), len(want))
    n = C.c_int64(-1)
    assert dge.lib.dge_flows_to_text(f._h, C.byref(sl), 0, 0, None, 0, buf, len(want) - 1, C.byref(n), None) == 4          # DGE_ERR_CAP
    assert n.value == len(want) and buf.raw == b"\xAA" * len(want) and "dge_flows_to_text" in dge.lib.dge_last_error().decode()
    assert dge.lib.dge_flows_to_text(f._h, C.byref(sl), 0, 0, None, 0, buf, len(want), C.byref(n), None) == 0 and buf.raw == want
    want = ref.time_series_text(c, ids)
    buf = C.create_string_buffer(b"\xAA" * len(want), len(want))
    assert dge.lib.dge_flows_time_series_text(f._h, None, buf, len(want) - 1, C.byref(n), None) == 4 and n.value == len(want) and buf.raw == b"\xAA" * len(want)
    m = C.c_int64(-1)
    assert dge.lib.dge_flows_time_series(f._h, None, buf, buf, buf, 36, C.byref(m)) == 4 and m.value == 37 and buf.raw == b"\xAA" * len(want)


# ------------------------------------------------------------------------------------------ 6. round trip
def store_of(g):
    c = g.get_csr(tables=True)
    s = g.get_source_alias()
    return [c["row_ptr"], c["nbr"], c["weight"], c["out_degree"], c["prob"], c["alias"], s["prob"], s["alias"], s["src"], np.float64(s["weight_sum"])]


@pytest.mark.parametrize("how", ["slots", "windows"])
def test_the_od_texts_read_back_give_the_graph_the_table_gives(dge, how):
    ids, c, f = fuzz(dge, 3)
    windows = [(h, 6) for h in (0, 6, 12, 18)]
    if how == "slots":
        a, a_names, _ = dge.DeviceGraph.from_flows(f, 8, ref.AS_TRACTS)
        texts = f.od_text(T=8, mode=ref.AS_TRACTS)
    else:
        a, a_names, _ = dge.DeviceGraph.from_flow_windows(f, windows)
        texts = f.od_text(windows=windows)
    b, b_names, _ = dge.DeviceGraph.from_od(texts)
    assert a.num_vertices == b.num_vertices > 0 and a.num_edges == b.num_edges > 0
    a.build_alias(True); b.build_alias(True)
    for x, y in zip(store_of(a), store_of(b)):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes() and np.asarray(x).shape == np.asarray(y).shape
    assert a_names.as_bytes() == b_names.as_bytes() and np.array_equal(a.regions(), b.regions())
    if how == "windows":                                      # the layered text speaks the .seq vocabulary: its tokens are the vertex names
        tokens = {t for line in f.od_text(windows=windows, layered=True).splitlines() for t in line.split(b" ")[:2]}
        assert tokens == set(a_names.as_bytes()) and len(tokens) == 4 * 37


# ------------------------------------------------------------------------------------------ 7. time series
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_time_series_arrays_and_text(dge, seed):
    ids, c, f = fuzz(dge, seed)
    before = state_of(f)
    for mask in (None, half_mask(seed)):
        want_ids, want_in, want_out = ref.time_series(c, ids, mask)
        got_ids, got_in, got_out = f.time_series(mask)
        assert got_ids.tolist() == want_ids and got_in.tolist() == want_in and got_out.tolist() == want_out
        assert f.time_series_text(mask) == ref.time_series_text(c, ids, mask)
    assert state_of(f) == before


def test_time_series_keeps_the_reference_asymmetry(dge):
    f = dge.Flows(regions_of(dge, 7, TINY_IDS))
    f.add_entries(*arrays(TINY_TABLE))
    got = f.time_series_text(TINY_MASK)
    assert got == ref.time_series_text(TINY_TABLE, TINY_IDS, TINY_MASK)
    for a, b in (("all", "all"), ("selected", "selected"), ("all", "selected")):
        assert got != ref.time_series_text(TINY_TABLE, TINY_IDS, TINY_MASK, in_from=a, out_to=b)
    assert f.time_series_text() == ref.time_series_text(TINY_TABLE, TINY_IDS)
    assert f.od_text(windows=[(0, 1), (1, 1), (23, 1)], layered=True) == b"0--5 1-30 12\n0-30 1-0 3\n1-0 2-0 100\n1-7 2--5 4\n2-30 0-7 5\n"
    assert f.matrix_text(0, T=1, sep=" ", select=TINY_MASK) == b"100 0 0\n0 0 0\n3 5 0\n"


def test_an_id_that_cannot_be_negated_is_a_range_error_for_the_series_text_only(dge, tmp_path):
    ids = [4, -2 ** 63, 9]
    f = dge.Flows(regions_of(dge, 7, ids))
    c = {(5, 0, 1): 3, (5, 1, 2): 2 ** 40, (6, 1, 1): 8}
    f.add_entries(*arrays(c))
    path = str(tmp_path / "series.txt")
    for call in (lambda: f.time_series_text(), lambda: f.write_time_series(path), lambda: f.time_series_text([0, 1, 0])):
        with pytest.raises(dge.DgeError) as ei:
            call()
        assert ei.value.code == 2 and "region 1" in str(ei.value) and "-2^63" in str(ei.value)          # DGE_ERR_RANGE
    assert not os.path.exists(path)
    assert f.time_series_text([1, 0, 1]) == ref.time_series_text(c, ids, [1, 0, 1])
    got_ids, got_in, got_out = f.time_series()
    assert got_ids.tolist() == [-2 ** 63, 4, 9] and got_out[0].sum() == 2 ** 40 + 8 and got_in[0].sum() == 11
    (day,) = ref.slices(c, T=1)
    assert f.od_text(T=1) == [ref.od_text(day, ids)] and b"-9223372036854775808 9 1099511627776\n" in f.od_text(T=1)[0]
    assert f.matrix_text(0, T=1) == ref.matrix_text(day, ids)


# ------------------------------------------------------------------------------------------ 8. read-only, repeatable, whatever built the table
def test_the_texts_do_not_depend_on_how_the_table_was_built(dge):
    rng = np.random.default_rng(12)
    R = 37
    ids = fuzz_ids(4)
    regions = regions_of(dge, 7, ids)
    centres = np.array([np.mean(region[0][:-1], 0) for region in mesh(7).rings[:R]])
    s, e, h = rng.integers(0, R, 3000), rng.integers(0, 12, 3000), rng.integers(0, 24, 3000).astype(np.int32)
    by_trips = dge.Flows(regions)
    for part in np.array_split(np.arange(3000), 3):
        by_trips.add_trips(centres[s[part]], centres[e[part]], h[part])
    c = ref.table(*by_trips.to_host())
    assert sum(c.values()) == 3000 and max(c.values()) > 1
    by_entries = dge.Flows(regions)
    by_entries.add_entries(*arrays(c, rng.permutation(len(c))))

    def texts(f):
        return [f.od_text(T=4), f.od_text(windows=WINDOWS, layered=True), f.matrix_text(2, T=3, sep="\t", select=half_mask(4)), f.time_series_text(half_mask(4))]
    before = state_of(by_trips)
    first = texts(by_trips)
    assert texts(by_trips) == first and texts(by_entries) == first                    # two identical calls; the other way to the same table
    assert state_of(by_trips) == before
    sums = ref.slices(c, T=4)
    assert first[0] == [ref.od_text(x, ids) for x in sums] and first[3] == ref.time_series_text(c, ids, half_mask(4))
