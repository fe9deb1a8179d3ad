"""A pure-Python reading of the spatial-graph rule of include/dge.h (CENTROID, DISTANCE, WEIGHT, SELECTION, GRAPH).  Python floats are binary64 and Python
has no fused multiply-add, so every line below is the rounded operation the header names, in its order: the tests compare bits.  Not a test module."""
import math

LN2_HI = float.fromhex("0x1.62e42feep-1")
LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
INV_LN2 = float.fromhex("0x1.71547652b82fep+0")
P1 = float.fromhex("0x1.555555555553ep-3")
P2 = -float.fromhex("0x1.6c16c16bebd93p-9")
P3 = float.fromhex("0x1.1566aaf25de2cp-14")
P4 = -float.fromhex("0x1.bbd41c5d26bf1p-20")
P5 = float.fromhex("0x1.6376972bea4d0p-25")
UNDER = -float.fromhex("0x1.74910d52d3051p+9")
HALF_LN2 = float.fromhex("0x1.62e42fefa39efp-2")
THREE_HALF_LN2 = float.fromhex("0x1.0a2b23f3bab73p+0")
TINY = 2.0 ** -28
TWOM1000 = 2.0 ** -1000


def E(x):
    """E(x) for x <= 0: the weight's exponential, one fixed sequence of rounded operations (csrc/spatial_weight.h)."""
    if x < UNDER:
        return 0.0
    if x >= -TINY:
        return 1.0 + x
    hi, lo, k = x, 0.0, 0
    if x < -HALF_LN2:
        if x > -THREE_HALF_LN2:
            hi = x + LN2_HI; lo = -LN2_LO; k = -1
        else:
            k = int(INV_LN2 * x - 0.5)          # truncation towards zero, as a C cast
            t = float(k)
            hi = x - t * LN2_HI
            lo = t * LN2_LO
    r = hi - lo
    t = r * r
    c = r - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))))
    if k == 0:
        return 1.0 - ((r * c) / (c - 2.0) - r)
    y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi)
    if k >= -1021:
        return y * math.ldexp(1.0, k)
    return (y * math.ldexp(1.0, k + 1000)) * TWOM1000


def centroid(rings):
    """rings: the region's rings in order, each a closed list of (x, y).  -> (x, y), or None when the area sum is 0 or the result is not finite."""
    bx, by = rings[0][0]
    cx = cy = A = 0.0
    for ring in rings:
        for (px, py), (qx, qy) in zip(ring[:-1], ring[1:]):
            a2 = (px - bx) * (qy - by) - (qx - bx) * (py - by)
            cx += a2 * (bx + px + qx)
            cy += a2 * (by + py + qy)
            A += a2
    if A == 0.0:
        return None
    x, y = cx / 3.0 / A, cy / 3.0 / A
    if not (math.isfinite(x) and math.isfinite(y)):
        return None
    return x, y


def dist2(ci, cj):
    dx = ci[0] - cj[0]
    dy = ci[1] - cj[1]
    return dx * dx + dy * dy            # may be inf: Python's + - * round to inf without raising


def distance(ci, cj):
    return math.sqrt(dist2(ci, cj))


def weight(ci, cj, scale=100.0):
    return E((-distance(ci, cj)) * scale)


def weight_matrix(xy, scale=100.0):
    """all R^2 weights, row-major lists: what the old path feeds dge_graph_add_edges"""
    return [[weight(a, b, scale) for b in xy] for a in xy]


def stream_sum(xs):
    """DoubleStream.sum() of JDK 8 (dge_java8_stream_sum, csrc/dge_algos.h)"""
    s = comp = simple = 0.0
    for x in xs:
        tmp = x - comp
        velvel = s + tmp
        comp = (velvel - s) - tmp
        s = velvel
        simple += x
    tmp = s + comp
    if tmp != tmp and math.isinf(simple):
        return simple
    return tmp


def select(wrow, k):
    """the first k candidates under (w descending, j ascending): [(j, w)]"""
    order = sorted(range(len(wrow)), key=lambda j: (-wrow[j], j))[:k]
    return [(j, wrow[j]) for j in order]


def spatial_graph(xy, k, scale=100.0, W=None):
    """-> dict(nbr [R][k], weight [R][k], out_degree [R], source_sum)"""
    W = W if W is not None else weight_matrix(xy, scale)
    nbr, wt, od = [], [], []
    for row in W:
        kept = select(row, k)
        nbr.append([j for j, _ in kept]); wt.append([w for _, w in kept])
        od.append(stream_sum(wt[-1]))
    return dict(nbr=nbr, weight=wt, out_degree=od, source_sum=stream_sum(od))


# ------------------------------------------------------------------------------------------ fixtures shared by the CPU and the GPU tests
def square(x0, y0, s, cw=True):
    r = [(x0, y0), (x0, y0 + s), (x0 + s, y0 + s), (x0 + s, y0), (x0, y0)]          # clockwise: a shapefile's shell
    return r if cw else r[::-1]


def reverse_all(rings):
    return [r[::-1] for r in rings]


# dyadic coordinates of a few bits: every product and sum of the chain is exact, whatever the order
DYADIC = {
    "unit square": [square(0.0, 0.0, 1.0)],
    "square away from the origin": [square(-88.0, 41.5, 0.25)],
    "square with a hole": [square(0.0, 0.0, 4.0), square(1.0, 1.0, 1.0, cw=False)],
    "two polygons": [square(0.0, 0.0, 2.0), square(5.0, 1.0, 1.0)],
}
# longitude / latitude as a shapefile holds them: nothing is exact
ROUNDED = {
    "tract-sized square": [square(-87.6298, 41.8781, 0.0123)],
    "tract with a hole": [square(-87.6298, 41.8781, 0.0123), square(-87.6251, 41.8811, 0.0031, cw=False)],
    "two-polygon tract": [square(-87.6298, 41.8781, 0.0123), square(-87.6011, 41.8702, 0.0077)],
    "pentagon": [[(-87.7, 41.9), (-87.69, 41.913), (-87.681, 41.907), (-87.683, 41.894), (-87.695, 41.891), (-87.7, 41.9)]],
}
