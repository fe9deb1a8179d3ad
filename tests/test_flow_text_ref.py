"""CPU: the second writing of the flow table's texts (tests/flow_text_ref.py) against bytes written out by hand on a table of four regions.  The table is
chosen so that every choice the rule makes shows: the order of lines is the order of ids and not of region indices, absent pairs are "0", the last slice's
lines point at slice 0, an id of 0 and a negative id are negated as decimals, and — with region -5 left out — a flow to an unselected destination (7 -> -5) and
one from an unselected source (-5 -> 30) tell the four readings of the traffic sums apart."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_text_ref as ref  # noqa: E402

IDS = [30, 0, -5, 7]                                     # by region index: ascending id is the index order 2, 1, 3, 0
TABLE = {(0, 0, 1): 3,                                   # hour 0:  30 -> 0
         (0, 2, 0): 12,                                  #          -5 -> 30   from the region the mask leaves out
         (1, 1, 1): 100,                                 # hour 1:  0 -> 0     a self flow
         (1, 3, 2): 4,                                   #          7 -> -5    to the region the mask leaves out
         (23, 0, 3): 5}                                  # hour 23: 30 -> 7
WINDOWS = [(0, 1), (1, 1), (23, 1)]
MASK = [1, 1, 0, 1]                                      # ids 30, 0, 7


def series_line(head, values):
    return b"%d," % head + b",".join(b"%d" % values.get(h, 0) for h in range(24)) + b"\n"


def test_table_from_arrays():
    assert ref.table([0, 1], [0, 3], [1, 2], [3, 4]) == {(0, 0, 1): 3, (1, 3, 2): 4}


def test_od_texts_by_window_and_by_slot():
    sums = ref.slices(TABLE, windows=WINDOWS)
    assert [ref.od_text(s, IDS) for s in sums] == [b"-5 30 12\n30 0 3\n", b"0 0 100\n7 -5 4\n", b"30 7 5\n"]
    assert ref.od_text({}, IDS) == b""
    # T = 1: taxi-all.od
    assert [ref.od_text(s, IDS) for s in ref.slices(TABLE, T=1)] == [b"-5 30 12\n0 0 100\n7 -5 4\n30 0 3\n30 7 5\n"]
    # T = 2, even: hours 0 .. 11 and 12 .. 23
    assert [ref.od_text(s, IDS) for s in ref.slices(TABLE, T=2)] == [b"-5 30 12\n0 0 100\n7 -5 4\n30 0 3\n", b"30 7 5\n"]
    # as the tracts do it, T = 12: slot k sums the hours k, k + 1 over the pairs seen in hour k itself — slot 0 does not see the pairs of hour 1
    texts = [ref.od_text(s, IDS) for s in ref.slices(TABLE, T=12, mode=ref.AS_TRACTS)]
    assert texts[0] == b"-5 30 12\n30 0 3\n" and texts[1] == b"0 0 100\n7 -5 4\n" and texts[2:] == [b""] * 10


def test_layered_text_points_at_the_next_slice_and_the_last_at_slice_zero():
    sums = ref.slices(TABLE, windows=WINDOWS)
    assert ref.od_layered(sums, IDS) == b"0--5 1-30 12\n0-30 1-0 3\n1-0 2-0 100\n1-7 2--5 4\n2-30 0-7 5\n"
    assert ref.od_layered(ref.slices(TABLE, T=1), IDS) == b"0--5 0-30 12\n0-0 0-0 100\n0-7 0--5 4\n0-30 0-0 3\n0-30 0-7 5\n"


def test_matrix_rows_and_columns_in_ascending_id_with_zeros():
    (day,) = ref.slices(TABLE, windows=[(0, 24)])
    assert ref.matrix_text(day, IDS) == b"0,0,0,12\n0,100,0,0\n4,0,0,0\n0,3,5,0\n"                  # rows and columns: -5, 0, 7, 30
    assert ref.matrix_text(day, IDS, b" ", MASK) == b"100 0 0\n0 0 0\n3 5 0\n"                    # 0, 7, 30: 7 -> -5 and -5 -> 30 play no part
    assert ref.matrix_text(day, IDS, b"\t", [0, 0, 1, 0]) == b"0\n"
    assert ref.matrix_text(day, IDS, b",", [0, 0, 0, 0]) == b""
    assert ref.matrix_text({}, IDS) == b"0,0,0,0\n" * 4


def test_time_series_sums_in_over_selected_sources_and_out_over_all_destinations():
    want = (series_line(0, {0: 3, 1: 100}) + series_line(0, {1: 100})                             # id 0 negated is 0
            + series_line(7, {23: 5}) + series_line(-7, {1: 4})                                   # out of 7: the flow to -5 counts
            + series_line(30, {}) + series_line(-30, {0: 3, 23: 5}))                              # into 30: the flow from -5 does not
    assert ref.time_series_text(TABLE, IDS, MASK) == want
    ids, fin, fout = ref.time_series(TABLE, IDS, MASK)
    assert ids == [0, 7, 30] and fin[2] == [0] * 24 and fout[1][1] == 4
    # the three other readings give three other texts
    others = [ref.time_series_text(TABLE, IDS, MASK, in_from=a, out_to=b) for a, b in (("all", "all"), ("selected", "selected"), ("all", "selected"))]
    assert len({want, *others}) == 4
    assert series_line(30, {0: 12}) in others[0] and series_line(-7, {}) in others[1]
    # all regions: a negative id is negated into a positive decimal
    full = ref.time_series_text(TABLE, IDS)
    assert full.startswith(series_line(-5, {1: 4}) + series_line(5, {0: 12})) and series_line(30, {0: 12}) in full and full.count(b"\n") == 8
    assert ref.time_series_text(TABLE, IDS, [0, 0, 0, 0]) == b""
