"""The second writing of the flow table's texts (include/dge.h: flow table out as text), CPU only and without the library: from the table as Flows.to_host()
gives it plus the region ids, through flow_ref.py's window sums and the slot sums of the slot rule, to the bytes of every kind and to the time series.  Written
as the naive loops the Java shows — all pairs for the matrix (J/Tracts.java:269-301), "%d" formatting, a loop over the focus keys for the traffic into a region
(J/Tracts.java:200-206).  It shares nothing with csrc/flow_text_plan.h."""
import flow_ref

EVEN, AS_TRACTS = 0, 1


def table(hour, src, dst, count):
    """Flows.to_host() -> {(hour, s, e): count} over region indices"""
    return {(int(h), int(s), int(e)): int(w) for h, s, e, w in zip(hour, src, dst, count)}


def slot_sums(c, T, mode):
    """-> for every slot the dict {(s, e): w} of its edges (region indices)"""
    if mode == EVEN:
        assert 24 % T == 0
        return [flow_ref.window(c, k * (24 // T), 24 // T) for k in range(T)]
    assert 1 <= T <= 24
    step = 24 // T
    out = []
    for k in range(T):                                   # "only destinations seen in hour k itself"
        out.append({(s, e): sum(c.get((h, s, e), 0) for h in range(k, k + step)) for (h0, s, e) in c if h0 == k})
    return out


def slices(c, T=None, mode=EVEN, windows=None):
    """the edge sets a dge_flow_slices names: the slots of (T, mode), or the windows [(start, hours), ..]"""
    if windows is not None:
        return [flow_ref.window(c, start, n) for start, n in windows]
    return slot_sums(c, T, mode)


def od_text(sums, ids):
    """one slice: the lines "src dst w", ascending by (src id, dst id)"""
    return b"".join(b"%d %d %d\n" % (s, e, w) for s, e, w in sorted((ids[s], ids[e], w) for (s, e), w in sums.items()))


def od_layered(all_sums, ids):
    """all slices in one text: the lines "k-src (k+1)%S-dst w", ascending by (k, src id, dst id)"""
    S = len(all_sums)
    out = []
    for k, sums in enumerate(all_sums):
        out += [b"%d-%d %d-%d %d\n" % (k, s, (k + 1) % S, e, w) for s, e, w in sorted((ids[s], ids[e], w) for (s, e), w in sums.items())]
    return b"".join(out)


def selected(ids, select):
    """the selected region indices in ascending id"""
    return sorted((r for r in range(len(ids)) if select is None or select[r]), key=lambda r: ids[r])


def matrix_text(sums, ids, sep=b",", select=None):
    """one slice: a line per selected region, a decimal per selected region, 0 for an absent pair"""
    rows = selected(ids, select)
    return b"".join(sep.join(b"%d" % sums.get((s, e), 0) for e in rows) + b"\n" for s in rows)


def time_series(c, ids, select=None, in_from="selected", out_to="all"):
    """-> (ids, in [n][24], out [n][24]) over the selected regions in ascending id.  The rule is in_from = "selected", out_to = "all" (J/Tracts.java:200-206); the
    other three readings exist so that a test can tell them apart."""
    rows = selected(ids, select)
    everyone = list(range(len(ids)))
    sources = rows if in_from == "selected" else everyone
    sinks = rows if out_to == "selected" else everyone
    fin = [[sum(c.get((h, s, r), 0) for s in sources) for h in range(24)] for r in rows]
    fout = [[sum(c.get((h, r, e), 0) for e in sinks) for h in range(24)] for r in rows]
    return [ids[r] for r in rows], fin, fout


def time_series_text(c, ids, select=None, **reading):
    out = []
    for k, fin, fout in zip(*time_series(c, ids, select, **reading)):
        out.append(b"%d" % k + b"".join(b",%d" % v for v in fin) + b"\n" + b"%d" % -k + b"".join(b",%d" % v for v in fout) + b"\n")
    return b"".join(out)
