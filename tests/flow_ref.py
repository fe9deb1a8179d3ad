"""The second reading of the hour-window and triplet rules (include/dge.h: hour windows of the flow table), CPU only and without the library: a table is a dict
{(hour, s, e): count} over region indices, a window sum a plain loop over its hours, the triplet search the reference's loop over (t1, t2, t3) with its ten
conditions (J/Tracts.java:380-406).  No numpy in the arithmetic.  Also the two table generators the tests and scripts/flow_windows_rate.py share."""
from collections import Counter

import numpy as np

DEFAULT_RULE = dict(A=(7, 3), B=(17, 7), C=(17, 6), D=(7, 6), E=(7, 7), min_a=30, min_b=70, ratio=2)
SUMS = ("A12", "A21", "C21", "C12", "B31", "E31", "C13", "D13", "B13", "B23", "C23", "D23", "B32")      # the order of dge_triplet_rule_check


def hours(start, n):
    return [(start + j) % 24 for j in range(n)]


def window(c, start, n):
    """-> {(s, e): the sum of c(h, s, e) over the window's hours}, the pairs with a sum > 0"""
    inside = set(hours(start, n))
    out = Counter()
    for (h, s, e), w in c.items():
        if h in inside:
            out[(s, e)] += w
    return {k: w for k, w in out.items() if w > 0}


def window_edges(c, ids, windows):
    """-> the window edges [(k, src id, dst id, w)], ascending"""
    out = []
    for k, (start, n) in enumerate(windows):
        out += [(k, ids[s], ids[e], w) for (s, e), w in window(c, start, n).items()]
    return sorted(out)


def conditions(rule, s):
    """the ten conditions on the thirteen sums (a dict by the names of SUMS), in the reference's order"""
    r = rule["ratio"]
    return [s["A12"] > rule["min_a"], s["B31"] > rule["min_b"], s["B23"] > rule["min_b"], s["A12"] > r * s["A21"], s["C13"] > r * s["D13"], s["C21"] > r * s["C12"],
            s["C23"] > r * s["D23"], s["B31"] > r * s["E31"], s["B31"] > r * s["B32"], s["B31"] > r * s["B13"]]


def keep(rule, sums):
    return all(conditions(rule, dict(zip(SUMS, sums))))


def triplets(c, R, rule=DEFAULT_RULE):
    """-> the kept (t1, t2, t3) as region indices in loop order, and the counters of dge_triplet_info"""
    W = {name: window(c, *rule[name]) for name in "ABCDE"}

    def sums(t1, t2, t3):
        t = {"1": t1, "2": t2, "3": t3}
        return {name: W[name[0]].get((t[name[1]], t[name[2]]), 0) for name in SUMS}

    def pair(which, x, y):
        """do (x, y) pass the conditions of their pair alone?  (the sums of the other pairs are not read by them)"""
        s = sums(*{"12": (x, y, -1), "23": (-1, x, y), "31": (y, -1, x)}[which])
        ok = conditions(rule, s)
        return all(ok[q - 1] for q in {"12": (1, 4, 6), "23": (3, 7), "31": (2, 5, 8, 10)}[which])

    out = []
    info = dict(pairs_12=0, pairs_23=0, pairs_31=0, candidates=0, triplets=0)
    for x in range(R):
        for y in range(R):
            if x != y:
                info["pairs_23"] += pair("23", x, y)
                info["pairs_31"] += pair("31", x, y)
    for t1 in range(R):
        for t2 in range(R):
            if t2 == t1 or not pair("12", t1, t2):
                continue
            info["pairs_12"] += 1
            for t3 in range(R):
                if t3 == t1 or t3 == t2:
                    continue
                ok = conditions(rule, sums(t1, t2, t3))
                if all(ok[:8] + ok[9:]):
                    info["candidates"] += 1
                    if ok[8]:
                        out.append((t1, t2, t3))
    info["triplets"] = len(out)
    return out, info


# ------------------------------------------------------------------------------------------ generators
def _base(t1, t2, t3):
    return {"a12": (8, t1, t2, 40), "a21": (8, t2, t1, 10), "c21": (18, t2, t1, 50), "c12": (18, t1, t2, 20), "b31": (19, t3, t1, 200), "e31": (10, t3, t1, 5),
            "c13": (18, t1, t3, 60), "d13": (9, t1, t3, 10), "b23": (20, t2, t3, 80), "d23": (11, t2, t3, 30), "b32": (21, t3, t2, 90)}


def critical(seed, P=48):
    """R = 144 regions, P disjoint triples planted so that triple p sits on the edge of condition p % 12: with d = (p // 12) % 2 = 0 on equality (it must fail),
    with d = 1 one past it (it must pass; kind 10 fails for both).  -> the table, R, the planted triples that must pass (region indices, in planting order)"""
    R = 144
    rng = np.random.default_rng(seed)
    perm = rng.permutation(R).tolist()
    c = Counter()
    must = []
    for p in range(P):
        t1, t2, t3 = perm[3 * p: 3 * p + 3]
        kind, d = p % 12, (p // 12) % 2
        change = [dict(a12=30 + d, a21=5), dict(b31=70 + d, b32=30, c13=30, d13=5), dict(b23=70 + d, d23=10), dict(a21=20, a12=40 + d), dict(d13=25, c13=50 + d), dict(c21=40 + d),
                  dict(d23=38, b23=76 + d), dict(e31=100, b31=200 + d), dict(b32=100, b31=200 + d), dict(c13=100, b31=200 + d), dict(d23=38, b23=76), dict(e31=0, b31=200 + d)][kind]
        for name, (h, s, e, w) in _base(t1, t2, t3).items():
            w = change.get(name, w)
            if w:
                c[(h, s, e)] += w
        if kind == 10:
            c[(23, t2, t3)] += 50                # hour 23 is in B and not in C
        if kind == 11:
            c[(13, t3, t1)] += 100               # hour 13 is in E
            c[(14, t3, t1)] += 1000              # hour 14 is in no window
        if d == 1 and kind != 10:
            must.append((t1, t2, t3))
    n = 40 * R
    for h, s, e, w in zip(rng.choice([0, 3, 6, 14, 15, 16], n).tolist(), rng.integers(0, R, n).tolist(), rng.integers(0, R, n).tolist(), rng.integers(1, 50, n).tolist()):
        c[(h, s, e)] += w
    for s in range(R):
        c[(8, s, s)] += 100
        c[(19, s, s)] += 300
    return dict(c), R, must


def tripartite(seed, n1=3, n2=9, n3=150):
    """R = n1 + n2 + n3 regions in three groups — residences, offices, night life — drawn from a permutation; dense enough that the lists of a (t1, t2) edge are
    longer than a wave is wide and the ninth condition decides hundreds of cases.  -> the table, R"""
    R = n1 + n2 + n3
    rng = np.random.default_rng(seed)
    perm = rng.permutation(R).tolist()
    g1, g2, g3 = perm[:n1], perm[n1:n1 + n2], perm[n1 + n2:]
    c = Counter()
    for t1 in g1:
        for t2 in g2:
            c[(8, t1, t2)] += int(rng.choice([30, 31, 40]))
            c[(8, t2, t1)] += 10; c[(18, t2, t1)] += 50; c[(18, t1, t2)] += 20
    for t3 in g3:
        for t1 in g1:
            if rng.random() < 0.7:
                c[(19, t3, t1)] += 200; c[(10, t3, t1)] += 5; c[(18, t1, t3)] += 60; c[(9, t1, t3)] += 10
    for t2 in g2:
        for t3 in g3:
            if rng.random() < 0.6:
                c[(20, t2, t3)] += int(rng.choice([70, 71, 80])); c[(11, t2, t3)] += 30
    for t3 in g3:
        for t2 in g2:
            if rng.random() < 0.8:
                c[(21, t3, t2)] += int(rng.choice([90, 100, 101]))
    return dict(c), R


def arrays(c):
    """the table as the four arrays Flows.add_entries takes, in the dict's order"""
    keys = list(c)
    return (np.array([k[0] for k in keys], np.int32), np.array([k[1] for k in keys], np.int32), np.array([k[2] for k in keys], np.int32), np.array([c[k] for k in keys], np.int64))
