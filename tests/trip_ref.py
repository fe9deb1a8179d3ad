"""The second reading of the trip-mapping rule (include/dge.h: trips into regions), CPU only and without the library: location of a point by exact rational
arithmetic over the doubles (fractions.Fraction turns every coordinate into the rational it is; one common power of two then makes them integers, so the
arithmetic stays exact and quick) against EVERY segment of EVERY region with no index, flows by collections.Counter, both slot rules in plain loops, and the
.od texts of the slot edges.  Also the region generators the tests and scripts/trip_map_rate.py share."""
from collections import Counter
from fractions import Fraction

import numpy as np

EVEN, AS_TRACTS = 0, 1


def in_domain(v):
    v = float(v)
    return np.isfinite(v) and (v == 0.0 or 2.0 ** -450 <= abs(v) <= 2.0 ** 500)


class Regions:
    """ids [R]; rings: for every region a list of rings, a ring a list of (x, y) doubles with the last equal to the first."""

    def __init__(self, ids, rings):
        self.ids = [int(i) for i in ids]
        self.rings = [[[(float(x), float(y)) for x, y in ring] for ring in region] for region in rings]
        vals = [abs(Fraction(c)) for region in self.rings for ring in region for v in ring for c in v if c != 0]
        self._shift = max([0] + [f.denominator.bit_length() for f in vals])

    def arrays(self):
        ring_first, vert_first, xy = [0], [0], []
        for region in self.rings:
            for ring in region:
                xy += ring
                vert_first.append(len(xy))
            ring_first.append(len(vert_first) - 1)
        return (np.array(self.ids, np.int64), np.array(ring_first, np.int64), np.array(vert_first, np.int64), np.array(xy, np.float64).reshape(-1, 2))

    def segments(self):
        """-> seg float64 [S, 4], seg_first int64 [R + 1]: what the host harness of pip_exact.h takes."""
        seg, first = [], [0]
        for region in self.rings:
            for ring in region:
                seg += [a + b for a, b in zip(ring[:-1], ring[1:])]
            first.append(len(seg))
        return np.array(seg, np.float64).reshape(-1, 4), np.array(first, np.int64)

    def _int(self, v, shift):
        f = Fraction(v) * (1 << shift)
        assert f.denominator == 1
        return f.numerator

    def location(self, px, py):
        """-> per region 'interior' / 'boundary' / 'exterior' for one point inside the domain."""
        shift = max(self._shift, Fraction(px).denominator.bit_length(), Fraction(py).denominator.bit_length())
        key = ("ints", shift)
        if getattr(self, "_cache_key", None) != key:
            self._ints = [[[(self._int(x, shift), self._int(y, shift)) for x, y in ring] for ring in region] for region in self.rings]
            self._cache_key = key
        X, Y = self._int(px, shift), self._int(py, shift)
        out = []
        for region in self._ints:
            crossings, on = 0, False
            for ring in region:
                for (ax, ay), (bx, by) in zip(ring[:-1], ring[1:]):
                    if min(ax, bx) <= X <= max(ax, bx) and min(ay, by) <= Y <= max(ay, by) and (bx - ax) * (Y - ay) - (by - ay) * (X - ax) == 0:
                        on = True
                    if (ay > Y) != (by > Y):
                        d = (bx - ax) * (Y - ay) - (by - ay) * (X - ax)
                        if (d > 0) == (by > ay) and d != 0:
                            crossings += 1
            out.append("boundary" if on else ("interior" if crossings % 2 else "exterior"))
        return out

    def locate(self, xy):
        """-> region int32 [n], and the counters located / on_boundary / multi of dge_locate_info."""
        region = np.full(len(xy), -1, np.int32)
        located = on_boundary = multi = 0
        for i, (px, py) in enumerate(np.asarray(xy, np.float64).reshape(-1, 2).tolist()):
            if not (in_domain(px) and in_domain(py)):
                continue
            loc = self.location(px, py)
            inside = [r for r, what in enumerate(loc) if what == "interior"]
            if inside:
                region[i] = inside[0]
            located += bool(inside)
            multi += len(inside) > 1
            on_boundary += (not inside) and "boundary" in loc
        return region, dict(located=located, on_boundary=on_boundary, multi=multi)


def flows(start_region, end_region, hour, start_xy, end_xy):
    """-> Counter {(hour, s, e): count} and the counters trips / mapped / bad / no_start / no_end."""
    c = Counter()
    n = dict(trips=len(hour), mapped=0, bad=0, no_start=0, no_end=0)
    for s, e, h, p, q in zip(np.asarray(start_region).tolist(), np.asarray(end_region).tolist(), np.asarray(hour).tolist(), np.asarray(start_xy).tolist(), np.asarray(end_xy).tolist()):
        if not 0 <= h <= 23 or not all(in_domain(v) for v in p + q):
            n["bad"] += 1
        elif s < 0:
            n["no_start"] += 1
        elif e < 0:
            n["no_end"] += 1
        else:
            n["mapped"] += 1
            c[(h, s, e)] += 1
    return c, n


def slot_edges(c, ids, T, mode):
    """-> the slot edges [(slot, src id, dst id, w)], ascending."""
    out = Counter()
    if mode == EVEN:
        assert 24 % T == 0
        for (h, s, e), w in c.items():
            out[(h // (24 // T), ids[s], ids[e])] += w
    else:
        assert 1 <= T <= 24
        step = 24 // T
        pairs = {(s, e) for (_, s, e) in c}
        for k in range(T):
            for s, e in pairs:
                if c.get((k, s, e), 0) > 0:
                    out[(k, ids[s], ids[e])] = sum(c.get((h, s, e), 0) for h in range(k, k + step))
    return [(k, s, e, w) for (k, s, e), w in sorted(out.items())]


def od_texts(edges, T):
    texts = [[] for _ in range(T)]
    for k, s, e, w in edges:
        texts[k].append(b"%d %d %d\n" % (s, e, w))
    return [b"".join(t) for t in texts]


# ------------------------------------------------------------------------------------------ generators
def quad_mesh(n, seed, x0=-87.9, y0=41.6, size=0.5, subdivide=1):
    """n x n quads near Chicago; the shared vertices are jittered once, so the mesh is a perfect tiling.  Every edge is cut into `subdivide` pieces whose inner
    points are shared by the two quads of the edge too.  Region order is shuffled, ids are not contiguous.  -> Regions, the vertices [n + 1, n + 1, 2]"""
    rng = np.random.default_rng(seed)
    h = size / n
    gx, gy = np.meshgrid(np.arange(n + 1) * h + x0, np.arange(n + 1) * h + y0, indexing="ij")
    v = np.stack([gx, gy], -1) + rng.uniform(-0.3 * h, 0.3 * h, (n + 1, n + 1, 2))
    edge = {}

    def path(a, b):
        key = (min(a, b), max(a, b))
        if key not in edge:
            p, q = v[key[0]], v[key[1]]
            t = np.arange(1, subdivide)[:, None] / subdivide
            inner = p + (q - p) * t + (rng.uniform(-0.02 * h, 0.02 * h, (subdivide - 1, 2)) if subdivide > 1 else 0)
            edge[key] = [tuple(p.tolist())] + [tuple(x) for x in np.asarray(inner).reshape(-1, 2).tolist()] + [tuple(q.tolist())]
        pts = edge[key]
        return pts if a == key[0] else pts[::-1]

    rings = []
    for i in range(n):
        for j in range(n):
            corners = [(i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1)]
            ring = []
            for a, b in zip(corners, corners[1:] + corners[:1]):
                ring += path(a, b)[:-1]
            rings.append([ring + ring[:1]])
    order = rng.permutation(n * n)
    ids = (10100 + 7 * rng.permutation(n * n) * 13).tolist()
    return Regions(ids, [rings[k] for k in order]), v
