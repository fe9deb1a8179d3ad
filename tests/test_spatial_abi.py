"""CPU: the spatial-graph entries (dge_regions_centroids, dge_graph_add_spatial, dge_graph_add_spatial_points) are part of the C ABI — declared, exported, bound —
were added without moving the version or the trainer's build stamp, and refuse bad arguments with DGE_ERR_ARG before they look for a device."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "embedding_amd", "csrc")
ENTRIES = ("dge_regions_centroids", "dge_graph_add_spatial", "dge_graph_add_spatial_points")


def test_the_entries_are_declared_exported_and_bound(dge):
    h = open(os.path.join(ROOT, "include", "dge.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    declared = set(re.findall(r"\b(dge_[a-z0-9_]+)\s*\(", h))
    raw = C.CDLL(dge.LIB_PATH)
    from embedding_amd._native import SIGNATURES
    for name in ENTRIES:
        assert name in declared, "%s is not declared in include/dge.h" % name
        assert hasattr(raw, name), "libdge.so does not export %s" % name
        assert name in SIGNATURES
    assert dge.lib.dge_version() == 106            # additions only: no bump
    assert callable(dge.Regions.centroids) and callable(dge.DeviceGraph.from_spatial)
    # the argument lists of the header and of the binding have the same lengths
    for name in ENTRIES:
        args = re.search(r"\b%s\s*\((.*?)\);" % name, h, flags=re.S).group(1)
        assert len(args.split(",")) == len(SIGNATURES[name][1]), name


def test_info_layout(dge):
    from embedding_amd._native import SpatialInfo
    assert C.sizeof(SpatialInfo) == 40
    fields = ["regions", "edges", "weights", "zero_weights", "kernel_ms"]
    assert [f[0] for f in SpatialInfo._fields_] == fields and [getattr(SpatialInfo, f).offset for f in fields] == [0, 8, 16, 24, 32]
    h = open(os.path.join(ROOT, "include", "dge.h")).read()
    body = re.search(r"typedef struct dge_spatial_info \{(.*?)\} dge_spatial_info;\s*/\* 40 bytes \*/", h, flags=re.S).group(1)
    assert re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == fields


def test_bad_arguments_are_argument_errors_without_a_device(dge):
    """A graph and a regions handle cannot exist without a device, so on a machine without one every call below has a NULL handle among its faults.  The value
    checks come first and name what they found; the NULL handle is what the last form of each entry shows.  Never DGE_ERR_DEVICE; names and info untouched."""
    from embedding_amd._native import SpatialInfo
    lib = dge.lib
    full = dge.Names(["a"])
    empty = dge.Names()
    info = SpatialInfo(); info.edges = -5

    def p(a):
        return a.ctypes.data_as(C.c_void_p)

    def points(ids, xy, k=2, scale=100.0, names=None, R=None):
        ids = np.array(ids, np.int64); xy = np.array(xy, np.float64).reshape(-1, 2)
        rc = lib.dge_graph_add_spatial_points(None, p(ids), p(xy), len(ids) if R is None else R, k, scale, names._h if names is not None else None, C.byref(info))
        return rc, (lib.dge_last_error() or b"").decode()

    ids, xy = [7, 8, 9], [(0, 0), (1, 0), (0, 1)]
    nan, inf = float("nan"), float("inf")
    for what, kw, words in (("scale 0", dict(scale=0.0), ("scale",)), ("scale negative", dict(scale=-100.0), ("scale",)), ("scale nan", dict(scale=nan), ("scale",)),
                            ("scale inf", dict(scale=inf), ("scale",)), ("k 0", dict(k=0), ("k = 0", "1 .. 32")), ("k 33", dict(k=33), ("k = 33", "1 .. 32")),
                            ("k negative", dict(k=-1), ("k = -1",)), ("names not empty", dict(names=full), ("names must be empty",)), ("R negative", dict(R=-1), ("negative",)),
                            ("no graph", dict(names=empty), ("null graph",))):
        rc, msg = points(ids, xy, **kw)
        assert rc == 1 and "dge_graph_add_spatial_points" in msg, (what, rc, msg)
        for w in words:
            assert w in msg, (what, msg)
    for what, a, words in (("duplicate ids", ([7, 8, 7], xy), ("id 7", "twice")), ("nan point", (ids, [(0, 0), (1, nan), (0, 1)]), ("point 1", "id 8", "not finite")),
                           ("inf point", (ids, [(0, 0), (1, 0), (-inf, 1)]), ("point 2", "id 9", "not finite"))):
        rc, msg = points(*a)
        assert rc == 1, (what, rc, msg)
        for w in words:
            assert w in msg, (what, msg)
    assert lib.dge_graph_add_spatial_points(None, None, None, 3, 2, 100.0, None, None) == 1 and "null" in lib.dge_last_error().decode()

    def regions(k=2, scale=100.0, names=None):
        rc = lib.dge_graph_add_spatial(None, None, k, scale, names._h if names is not None else None, C.byref(info))
        return rc, (lib.dge_last_error() or b"").decode()

    for kw, word in ((dict(scale=0.0), "scale"), (dict(scale=-1.0), "scale"), (dict(scale=nan), "scale"), (dict(k=0), "k = 0"), (dict(k=33), "k = 33"),
                     (dict(names=full), "names must be empty"), (dict(), "null graph")):
        rc, msg = regions(**kw)
        assert rc == 1 and "dge_graph_add_spatial:" in msg and word in msg, (kw, rc, msg)
    n = C.c_int64(-1)
    buf = np.zeros(4)
    for call in (lambda: lib.dge_regions_centroids(None, p(buf), 2, C.byref(n)), lambda: lib.dge_regions_centroids(None, None, 0, C.byref(n)),
                 lambda: lib.dge_regions_centroids(None, None, -1, None)):
        assert call() == 1
        msg = lib.dge_last_error().decode()
        assert "dge_regions_centroids" in msg and "null" in msg
    assert full.as_bytes() == [b"a"] and len(empty) == 0 and info.edges == -5 and n.value == -1


def test_spatial_is_built_into_the_library_and_stays_out_of_the_stamp():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = next(l for l in mk.splitlines() if l.startswith("OBJS")).split()
    hdrs = next(l for l in mk.splitlines() if l.startswith("HDRS")).split()
    assert "spatial.o" in objs and "spatial_weight.h" in hdrs
    for f in ("spatial.hip", "spatial_weight.h"):
        assert os.path.exists(os.path.join(CSRC, f))
    hash_lines = "".join(l for l in mk.splitlines() if "HASH" in l)
    assert "spatial" not in hash_lines
    assert [l for l in mk.splitlines() if l.startswith("\t") and "spatial" in l] == []      # the generic rule builds it
    assert "-ffp-contract=off" in mk
    src = open(os.path.join(CSRC, "spatial.hip")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert '#include "spatial_weight.h"' in src and "sw_weight(" in code and "sw_centroid(" in code and "sw_dist2(" in code
    # the weight and the centroid are written once, in the header; neither kernel fuses, approximates or adds floating point atomically
    for word in ("fma(", "__fdividef", "__fsqrt", "__dsqrt", "__ddiv", "__expf", "exp(", "rsqrt", "atomicAdd(float", "atomicAdd(double"):
        assert word not in code, word
    assert "__shared__" in code and "dge_graph_adopt_pruned(" in code and "dge_graph_set_sources(" in code
    # keep_top_k's state transition is called, not copied: graph.hip defines it once and ends keep_top_k in it
    graph = open(os.path.join(CSRC, "graph.hip")).read()
    assert graph.count("int dge_graph_adopt_pruned(") == 1 and graph.count("dge_graph_adopt_pruned(") >= 2
