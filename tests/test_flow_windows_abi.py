"""CPU: the hour-window entries (dge_flows_add_entries, dge_flows_window_edges, dge_graph_add_flow_windows, dge_triplet_rule_default, dge_triplet_rule_check,
dge_flows_triplets) are part of the C ABI — declared, exported, bound, added without moving the version or the build stamp — and refuse bad arguments, bad
windows and bad rules with DGE_ERR_ARG before they look for a device; dge_triplet_rule_check, which needs no device, decides the ten conditions as
tests/flow_ref.py does on the lattice around every condition's edge and on random sums; the generators of flow_ref.py plant what they say; the window helpers
give the lists written out here."""
import ctypes as C
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "embedding_amd", "csrc")
ENTRIES = ("dge_flows_add_entries", "dge_flows_window_edges", "dge_graph_add_flow_windows", "dge_triplet_rule_default", "dge_triplet_rule_check", "dge_flows_triplets")


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def last(dge):
    return (dge.lib.dge_last_error() or b"").decode()


def test_the_entries_are_declared_exported_and_bound(dge):
    h = open(os.path.join(ROOT, "include", "dge.h")).read()
    declared = set(re.findall(r"\b(dge_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", h, flags=re.S)))
    raw = C.CDLL(dge.LIB_PATH)
    from embedding_amd._native import SIGNATURES
    for name in ENTRIES:
        assert name in declared and hasattr(raw, name) and name in SIGNATURES, name
    assert dge.lib.dge_version() == 106            # additions only: no bump
    for cls, name in ((dge.Flows, "add_entries"), (dge.Flows, "window_edges"), (dge.Flows, "triplets"), (dge.DeviceGraph, "from_flow_windows"), (dge.Flows, "windows_cross_time"),
                      (dge.Flows, "windows_from_intervals"), (dge.Flows, "windows_ca_default")):
        assert callable(getattr(cls, name))


def test_struct_layouts(dge):
    from embedding_amd._native import HourWindow, TripletInfo, TripletRule
    h = open(os.path.join(ROOT, "include", "dge.h")).read()
    for cls, size, pattern in ((HourWindow, 8, r"typedef struct dge_hour_window \{(.*?)\} dge_hour_window;\s*/\* 8 bytes \*/"),
                               (TripletRule, 64, r"typedef struct dge_triplet_rule \{(.*?)\} dge_triplet_rule;\s*/\* 64 bytes \*/"),
                               (TripletInfo, 48, r"typedef struct dge_triplet_info \{(.*?)\} dge_triplet_info;\s*/\* 48 bytes \*/")):
        assert C.sizeof(cls) == size
        body = re.sub(r"/\*.*?\*/", "", re.search(pattern, h, flags=re.S).group(1), flags=re.S)
        assert re.findall(r"\b(\w+);", body) == [f[0] for f in cls._fields_], cls
        assert all(getattr(cls, f[0]).offset % min(C.sizeof(f[1]), 8) == 0 for f in cls._fields_)


def test_the_default_rule_is_the_references(dge):
    r = dge.TripletRule()
    assert dge.lib.dge_triplet_rule_default(C.byref(r)) == 0
    got = {k: (getattr(r, k).start, getattr(r, k).hours) for k in "ABCDE"}
    got.update(min_a=r.min_a, min_b=r.min_b, ratio=r.ratio)
    assert got == flow_ref.DEFAULT_RULE and r.reserved == 0
    # the reference's inclusive (lo, hi): getFlowTo(.., 7, 9), (17, 23), (17, 22), (7, 12), (7, 13) (J/Tracts.java:391-400)
    assert [flow_ref.hours(*got[k]) for k in "ABCDE"] == [list(range(lo, hi + 1)) for lo, hi in ((7, 9), (17, 23), (17, 22), (7, 12), (7, 13))]
    assert dge.lib.dge_triplet_rule_default(None) == 1
    q = dge.Flows.triplet_rule(A=(22, 5), ratio=3, min_b=0)
    assert (q.A.start, q.A.hours, q.ratio, q.min_b, q.min_a, q.B.start) == (22, 5, 3, 0, 30, 17)


def test_bad_arguments_windows_and_rules_are_argument_errors_without_a_device(dge):
    lib = dge.lib
    n = C.c_int64(-1)
    keep = C.c_int32(-1)
    buf = np.zeros(16, np.int64); b32 = np.zeros(16, np.int32)
    win = lambda *w: (dge.HourWindow * len(w))(*[dge.HourWindow(a, b) for a, b in w])  # noqa: E731
    ok = win((0, 24), (22, 5), (3, 0))
    calls = {
        "dge_flows_add_entries": lambda: lib.dge_flows_add_entries(None, p(b32), p(b32), p(b32), p(buf), 1),
        "dge_flows_window_edges": lambda: lib.dge_flows_window_edges(None, ok, 3, None, None, None, None, 0, C.byref(n)),
        "dge_graph_add_flow_windows": lambda: lib.dge_graph_add_flow_windows(None, None, ok, 3, None, None),
        "dge_flows_triplets": lambda: lib.dge_flows_triplets(None, None, None, None, None, 0, C.byref(n), None),
        "dge_triplet_rule_check": lambda: lib.dge_triplet_rule_check(None, None, C.byref(keep)),
    }
    for name, call in calls.items():
        assert call() == 1, name
        assert name in last(dge) and "null" in last(dge), last(dge)
    assert lib.dge_flows_window_edges(None, ok, 3, None, None, None, None, -1, C.byref(n)) == 1 and lib.dge_flows_window_edges(None, ok, 3, None, None, None, None, 0, None) == 1
    assert lib.dge_flows_window_edges(None, ok, 3, None, p(buf), p(buf), p(buf), 4, C.byref(n)) == 1                   # cap > 0 needs every output
    assert lib.dge_flows_triplets(None, None, p(buf), None, p(buf), 4, C.byref(n), None) == 1 and lib.dge_flows_triplets(None, None, None, None, None, -1, C.byref(n), None) == 1
    # a bad window is named, whatever else is wrong
    for bad, at in ((win((0, 1), (24, 1)), 1), (win((-1, 1)), 0), (win((0, 25)), 0), (win((0, 1), (5, 2), (23, -1)), 2)):
        for call in (lambda: lib.dge_flows_window_edges(None, bad, len(bad), None, None, None, None, 0, C.byref(n)), lambda: lib.dge_graph_add_flow_windows(None, None, bad, len(bad), None, None)):
            assert call() == 1 and "window %d" % at in last(dge), last(dge)
    for K in (0, -3):
        assert lib.dge_flows_window_edges(None, ok, K, None, None, None, None, 0, C.byref(n)) == 1 and "K" in last(dge)
        assert lib.dge_graph_add_flow_windows(None, None, ok, K, None, None) == 1
    assert lib.dge_flows_window_edges(None, None, 1, None, None, None, None, 0, C.byref(n)) == 1
    # a bad rule is named, by both entries that take one
    sums = np.zeros(13, np.int64)
    for field, value, word in (("A", (24, 1), "window A"), ("B", (0, 25), "window B"), ("C", (-1, 0), "window C"), ("D", (3, -1), "window D"), ("E", (99, 99), "window E"),
                               ("min_a", -1, "min_a"), ("min_a", 2 ** 40 + 1, "min_a"), ("min_b", -5, "min_b"), ("min_b", 2 ** 41, "min_b"), ("ratio", 0, "ratio"), ("ratio", 65537, "ratio")):
        r = dge.Flows.triplet_rule(**{field: value})
        assert lib.dge_flows_triplets(None, C.byref(r), None, None, None, 0, C.byref(n), None) == 1 and word in last(dge), (field, last(dge))
        assert lib.dge_triplet_rule_check(C.byref(r), p(sums), C.byref(keep)) == 1 and word in last(dge)
    for field, value in (("min_a", 2 ** 40), ("min_b", 0), ("ratio", 65536), ("ratio", 1), ("A", (23, 24)), ("E", (0, 0))):      # the bounds themselves are fine
        r = dge.Flows.triplet_rule(**{field: value})
        assert lib.dge_triplet_rule_check(C.byref(r), p(sums), C.byref(keep)) == 0 and keep.value == 0
    sums[5] = -1
    assert lib.dge_triplet_rule_check(None, p(sums), C.byref(keep)) == 1 and "sum 5" in last(dge)
    sums[5] = 24 * 2 ** 40 + 1
    assert lib.dge_triplet_rule_check(None, p(sums), C.byref(keep)) == 1
    assert n.value == -1


# ------------------------------------------------------------------------------------------ the ten conditions
BASE = dict(A12=40, A21=10, C21=50, C12=20, B31=200, E31=5, C13=60, D13=10, B13=60, B23=80, C23=80, D23=30, B32=90)      # passes the default rule with room


def lib_keep(dge, rule, sums):
    keep = C.c_int32(-1)
    a = np.array(sums, np.int64)
    assert dge.lib.dge_triplet_rule_check(C.byref(rule) if rule is not None else None, p(a), C.byref(keep)) == 0
    return bool(keep.value)


CONDITIONS = (("A12", None), ("B31", None), ("B23", None), ("A12", "A21"), ("C13", "D13"), ("C21", "C12"), ("C23", "D23"), ("B31", "E31"), ("B31", "B32"), ("B31", "B13"))


def test_the_ten_conditions_on_the_lattice_around_every_edge(dge):
    """one condition at a time: its two sides at edge - 1, edge, edge + 1 (the edge: where they are equal) for three right sides, every other condition passing
    with room — the other right sides that share its left side are 0, the other left sides are large"""
    assert flow_ref.SUMS == ("A12", "A21", "C21", "C12", "B31", "E31", "C13", "D13", "B13", "B23", "C23", "D23", "B32") and len(BASE) == 13
    decided = 0
    for ratio, min_a, min_b in ((2, 30, 70), (1, 0, 0), (3, 7, 2 ** 40), (65536, 30, 70)):
        rule = dict(flow_ref.DEFAULT_RULE, ratio=ratio, min_a=min_a, min_b=min_b)
        native = dge.Flows.triplet_rule(ratio=ratio, min_a=min_a, min_b=min_b)
        big = dict(BASE, A12=10 ** 6 * ratio + min_a, B31=10 ** 6 * ratio + min_b, B23=10 ** 3 + min_b, C21=10 ** 3 * ratio, C13=10 ** 3 * ratio, C23=10 ** 3 * ratio)
        assert flow_ref.keep(rule, [big[k] for k in flow_ref.SUMS])
        for q, (left, right) in enumerate(CONDITIONS):
            for rv in ((max(min_a, min_b) + 7, max(min_a, min_b) + 8, max(min_a, min_b) + 9) if right else (None,)):
                edge = ratio * rv if right else (min_a if left == "A12" else min_b)
                for lv in (edge - 1, edge, edge + 1):
                    if lv < 0:
                        continue
                    s = dict(big)
                    for q2, (left2, right2) in enumerate(CONDITIONS):
                        if q2 != q and left2 == left and right2:
                            s[right2] = 0
                    s[left] = lv
                    if right:
                        s[right] = rv
                    ok = flow_ref.conditions(rule, s)
                    if all(ok[:q] + ok[q + 1:]):                   # (not so where the left side is 0: 0 > ratio * 0 fails as well)
                        assert ok[q] == (lv > edge) == flow_ref.keep(rule, [s[k] for k in flow_ref.SUMS]), (left, right, lv, edge)
                        decided += 1
                    assert lib_keep(dge, native, [s[k] for k in flow_ref.SUMS]) == all(ok), (ratio, left, right, lv, rv)
    assert decided >= 4 * (3 * 3 + 7 * 9) - 6
    # every condition alone decides: from the passing base, breaking one condition breaks the answer
    assert lib_keep(dge, None, [BASE[k] for k in flow_ref.SUMS]) and flow_ref.keep(flow_ref.DEFAULT_RULE, [BASE[k] for k in flow_ref.SUMS])
    for breaks in (dict(A12=30), dict(B31=70, E31=0, B32=0, B13=0), dict(B23=70), dict(A21=20), dict(D13=30), dict(C12=25), dict(D23=40), dict(E31=100), dict(B32=100), dict(B13=100)):
        s = dict(BASE, **breaks)
        ok = flow_ref.conditions(flow_ref.DEFAULT_RULE, s)
        assert ok.count(False) == 1, (breaks, ok)
        assert not lib_keep(dge, None, [s[k] for k in flow_ref.SUMS])


def test_the_ten_conditions_on_random_sums(dge):
    rng = np.random.default_rng(20251019)
    rules = [(None, flow_ref.DEFAULT_RULE)] + [(dge.Flows.triplet_rule(ratio=r, min_a=a, min_b=b), dict(flow_ref.DEFAULT_RULE, ratio=r, min_a=a, min_b=b)) for r, a, b in ((1, 0, 0), (3, 5, 9))]
    kept = 0
    for i in range(10_000):
        native, rule = rules[i % 3]
        # small values so that equalities and both answers occur; the left sides lifted so that a tenth or so passes
        s = rng.integers(0, 6, 13)
        for q in (0, 2, 4, 6, 9, 10):
            s[q] += rng.integers(0, 90)
        if i % 50 == 0:
            s = rng.integers(0, 24 * 2 ** 40 + 1, 13)
        want = flow_ref.keep(rule, [int(v) for v in s])
        assert lib_keep(dge, native, s) == want, (i, s.tolist())
        kept += want
    assert 500 < kept < 9500
    top = [24 * 2 ** 40] * 13                    # the greatest sums with the greatest ratio: no overflow
    assert lib_keep(dge, dge.Flows.triplet_rule(ratio=65536), top) == flow_ref.keep(dict(flow_ref.DEFAULT_RULE, ratio=65536), top) is False


# ------------------------------------------------------------------------------------------ the reference's own generators and the host helpers
def test_critical_plants_exactly_its_list():
    c, R, must = flow_ref.critical(1)
    assert R == 144 and len(must) == 22 and len(set(sum(must, ()))) == 66
    got, info = flow_ref.triplets(c, R)
    assert sorted(got) == sorted(must)
    assert info["triplets"] == 22 and info["candidates"] >= 22 + 2 and info["pairs_12"] >= 22       # (the two d = 0 triples of the ninth condition are candidates)
    assert all(c[(8, s, s)] == 100 and c[(19, s, s)] == 300 for s in range(R))                      # self flows are there and play no part


def test_window_reference_on_a_hand_made_table():
    c = {(23, 0, 1): 5, (0, 0, 1): 7, (1, 0, 1): 11, (12, 2, 0): 3, (0, 1, 1): 2}
    assert flow_ref.window(c, 23, 2) == {(0, 1): 12, (1, 1): 2} and flow_ref.window(c, 0, 24) == {(0, 1): 23, (2, 0): 3, (1, 1): 2} and flow_ref.window(c, 5, 0) == {}
    assert flow_ref.window(c, 22, 4) == {(0, 1): 23, (1, 1): 2} and flow_ref.window(c, 12, 1) == {(2, 0): 3}
    ids = [30, 10, 20]
    assert flow_ref.window_edges(c, ids, [(23, 2), (12, 1), (23, 2)]) == [(0, 10, 10, 2), (0, 30, 10, 12), (1, 20, 30, 3), (2, 10, 10, 2), (2, 30, 10, 12)]


def test_the_window_helpers(dge):
    F = dge.Flows
    assert F.windows_cross_time(8) == [(0, 3), (1, 3), (2, 3), (3, 3), (4, 3), (5, 3), (6, 3), (7, 3)]          # overlapping, starting at hour h: J/CrossTimeGraph.java:36
    assert F.windows_cross_time(24) == [(h, 1) for h in range(24)] and F.windows_cross_time(1) == [(0, 24)] and F.windows_cross_time(5) == [(h, 4) for h in range(5)]
    assert F.windows_from_intervals([0, 6, 10, 16, 20, 0]) == [(0, 6), (6, 4), (10, 6), (16, 4), (20, 4)]
    assert F.windows_from_intervals([22, 3, 3, 22]) == [(22, 5), (3, 0), (3, 19)]                              # past midnight, empty, and the rest of the day
    assert F.windows_ca_default(24) == [(h, 1) for h in range(24)]
    # numLayer = 8 as written: timeStep = 3, the array is new int[9] with [0] = 0, [3] = 9 % 8 = 1, [6] = 18 % 8 = 2 and zeros elsewhere
    assert F.windows_ca_default(8) == F.windows_from_intervals([0, 0, 0, 1, 0, 0, 2, 0, 0]) == [(0, 0), (0, 0), (0, 1), (1, 23), (0, 0), (0, 2), (2, 22), (0, 0)]
    for bad in (lambda: F.windows_cross_time(0), lambda: F.windows_cross_time(25), lambda: F.windows_from_intervals([3]), lambda: F.windows_from_intervals([0, 24]),
                lambda: F.windows_ca_default(0), lambda: F.windows_ca_default(25)):
        try:
            bad()
        except ValueError:
            continue
        raise AssertionError("a bad argument was taken")


def test_flow_windows_is_built_into_the_library_and_stays_out_of_the_stamp():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = next(l for l in mk.splitlines() if l.startswith("OBJS")).split()
    hdrs = next(l for l in mk.splitlines() if l.startswith("HDRS")).split()
    assert "flow_windows.o" in objs and "flow_rule.h" in hdrs and "trip_flows.h" in hdrs
    hash_lines = "".join(l for l in mk.splitlines() if "HASH" in l)
    for word in ("flow_windows", "flow_rule", "trip_flows"):
        assert word not in hash_lines
    # one comparator: the kernels and the host entry read the predicates of flow_rule.h and restate none
    src = open(os.path.join(CSRC, "flow_windows.hip")).read()
    assert '#include "flow_rule.h"' in src and '#include "trip_flows.h"' in src
    for name in ("fr_pair12(", "fr_pair23(", "fr_pair31(", "fr_triple(", "fr_keep(", "fr_window_has(", "fr_rule_fault("):
        assert name in src, name
    assert "r.ratio *" not in src and "rule.ratio *" not in src and "atomicAdd(float" not in src and "atomicAdd(double" not in src
    rule = open(os.path.join(CSRC, "flow_rule.h")).read()
    assert "__host__ __device__" in rule
    # both readers of the table share its passes
    for f in ("trip_map.hip", "flow_windows.hip"):
        s = open(os.path.join(CSRC, f)).read()
        assert '#include "trip_flows.h"' in s
        for name in ("k_slot_decode(const", "int trip_reduce(", "int trip_join("):
            assert name not in s, (f, name)
