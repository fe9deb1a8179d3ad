"""CPU: the trip-mapping entries (dge_regions_*, dge_flows_*, dge_graph_add_flows) are part of the C ABI — declared, exported, bound — were added without moving
the version or the trainer's build stamp, and refuse bad arguments with DGE_ERR_ARG before they look for a device."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "embedding_amd", "csrc")
ENTRIES = ("dge_regions_create", "dge_regions_info", "dge_regions_locate", "dge_regions_locate_device", "dge_regions_free", "dge_flows_create", "dge_flows_add_trips",
           "dge_flows_add_trips_device", "dge_flows_info", "dge_flows_to_host", "dge_flows_slot_edges", "dge_flows_free", "dge_graph_add_flows")


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
    assert callable(dge.Regions.from_arrays) and callable(dge.Flows.add_trips) and callable(dge.DeviceGraph.from_flows) and callable(dge.Flows.to_od_bytes)
    assert re.search(r"DGE_SLOTS_EVEN = 0, DGE_SLOTS_AS_TRACTS = 1", h) and (dge.Flows.EVEN, dge.Flows.AS_TRACTS) == (0, 1)


def test_info_layouts(dge):
    from embedding_amd._native import FlowsInfo, LocateInfo, RegionsInfo
    h = open(os.path.join(ROOT, "include", "dge.h")).read()
    for cls, name, size, pattern in ((RegionsInfo, "dge_regions_info", 72, r"struct dge_regions_info \{(.*?)\};\s*/\* 72 bytes \*/"),
                                     (LocateInfo, "dge_locate_info", 56, r"typedef struct dge_locate_info \{(.*?)\} dge_locate_info;\s*/\* 56 bytes \*/"),
                                     (FlowsInfo, "dge_flows_info", 96, r"struct dge_flows_info \{(.*?)\};\s*/\* 96 bytes \*/")):
        assert C.sizeof(cls) == size, name
        body = re.sub(r"/\*.*?\*/", "", re.search(pattern, h, flags=re.S).group(1), flags=re.S)
        assert re.findall(r"\b(\w+);", body) == [f[0] for f in cls._fields_], name
        assert all(getattr(cls, f[0]).offset % C.sizeof(f[1]) == 0 for f in cls._fields_)


def test_bad_arguments_are_argument_errors_without_a_device(dge):
    lib = dge.lib
    out = C.c_void_p(0)

    def p(a):
        return a.ctypes.data_as(C.c_void_p)

    def create(ids, ring_first, vert_first, xy, grid=0, out=out):
        ids = np.array(ids, np.int64); ring_first = np.array(ring_first, np.int64); vert_first = np.array(vert_first, np.int64); xy = np.array(xy, np.float64).reshape(-1, 2)
        rc = lib.dge_regions_create(0, p(ids), len(ids), p(ring_first), p(vert_first), p(xy), len(vert_first) - 1, len(xy), grid, C.byref(out) if out is not None else None)
        return rc, (lib.dge_last_error() or b"").decode()

    sq = [(0, 0), (1, 0), (1, 1), (0, 1), (0, 0)]
    sq2 = [(2, 0), (3, 0), (3, 1), (2, 1), (2, 0)]
    for what, args, words in (
            ("unclosed ring", ([5, 6], [0, 1, 2], [0, 5, 10], sq + sq2[:-1] + [(2, 0.5)]), ("region 1", "ring 1", "not closed")),
            ("short ring", ([5, 6], [0, 1, 2], [0, 5, 8], sq + [(2, 0), (3, 0), (2, 0)]), ("region 1", "ring 1", "3 vertices")),
            ("duplicate ids", ([5, 5], [0, 1, 2], [0, 5, 10], sq + sq2), ("5", "twice")),
            ("nan vertex", ([5, 6], [0, 1, 2], [0, 5, 10], sq + [(2, 0), (3, float("nan")), (3, 1), (2, 1), (2, 0)]), ("region 1", "ring 1", "vertex 1", "domain")),
            ("inf vertex", ([5], [0, 1], [0, 5], [(0, 0), (1, 0), (float("inf"), 1), (0, 1), (0, 0)]), ("region 0", "ring 0", "vertex 2", "domain")),
            ("tiny vertex", ([5], [0, 1], [0, 5], [(0, 0), (1, 0), (1, 2.0 ** -451), (0, 1), (0, 0)]), ("vertex 2", "domain")),
            ("huge vertex", ([5], [0, 1], [0, 5], [(0, 0), (1, 0), (1, 2.0 ** 501), (0, 1), (0, 0)]), ("vertex 2", "domain")),
            ("ring_first", ([5], [0, 2], [0, 5], sq), ("ring_first",)),
            ("vert_first", ([5], [0, 1], [0, 4], sq), ("vert_first",))):
        rc, msg = create(*args)
        assert rc == 1, (what, rc, msg)
        for w in words:
            assert w in msg, (what, msg)
    assert create([5], [0, 1], [0, 5], sq, grid=-1)[0] == 1 and create([5], [0, 1], [0, 5], sq, out=None)[0] == 1
    assert lib.dge_regions_create(0, None, 1, None, None, None, 0, 0, 0, C.byref(out)) == 1 and lib.dge_regions_create(0, None, -1, None, None, None, 0, 0, 0, C.byref(out)) == 1
    assert out.value is None
    n = C.c_int64(-1)
    buf = np.zeros(4, np.int64)
    calls = {
        "dge_regions_info": lambda: lib.dge_regions_info(None, None),
        "dge_regions_locate": lambda: lib.dge_regions_locate(None, p(buf), 1, p(buf), None),
        "dge_regions_locate_device": lambda: lib.dge_regions_locate_device(None, None, -1, None, None),
        "dge_flows_create": lambda: lib.dge_flows_create(None, C.byref(out)),
        "dge_flows_add_trips": lambda: lib.dge_flows_add_trips(None, p(buf), p(buf), p(buf), 1),
        "dge_flows_add_trips_device": lambda: lib.dge_flows_add_trips_device(None, None, None, None, -1),
        "dge_flows_info": lambda: lib.dge_flows_info(None, None),
        "dge_flows_to_host": lambda: lib.dge_flows_to_host(None, None, None, None, None, 0, C.byref(n)),
        "dge_flows_slot_edges": lambda: lib.dge_flows_slot_edges(None, 1, 0, None, None, None, None, 0, C.byref(n)),
        "dge_graph_add_flows": lambda: lib.dge_graph_add_flows(None, None, 1, 0, None, None),
    }
    for name, call in calls.items():
        assert call() == 1, name
        msg = (lib.dge_last_error() or b"").decode()
        assert name in msg and "null" in msg, msg
    assert n.value == -1
    lib.dge_regions_free(None); lib.dge_flows_free(None)       # freeing nothing is fine


def test_trip_map_is_built_into_the_library_and_stays_out_of_the_stamp():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = next(l for l in mk.splitlines() if l.startswith("OBJS")).split()
    hdrs = next(l for l in mk.splitlines() if l.startswith("HDRS")).split()
    assert "trip_map.o" in objs and "pip_exact.h" in hdrs and "od_commit.h" in hdrs
    for f in ("trip_map.hip", "pip_exact.h", "od_commit.h"):
        assert os.path.exists(os.path.join(CSRC, f))
    hash_lines = "".join(l for l in mk.splitlines() if "HASH" in l)
    for word in ("trip_map", "pip_exact", "od_commit"):
        assert word not in hash_lines
    assert [l for l in mk.splitlines() if l.startswith("\t") and "trip_map" in l] == []      # the generic rule builds it
    # one commit path: both readers include od_commit.h and neither restates its kernels
    for f in ("trip_map.hip", "od_read.hip"):
        src = open(os.path.join(CSRC, f)).read()
        assert '#include "od_commit.h"' in src
        for name in ("k_od_endpoints", "k_od_unique", "k_od_edges", "k_od_sources"):
            assert ") " + name + "(" not in src, (f, name)
    src = open(os.path.join(CSRC, "trip_map.hip")).read()
    assert '#include "pip_exact.h"' in src and "pip_step(" in src and "atomicAdd(float" not in src and "atomicAdd(double" not in src
    pip = open(os.path.join(CSRC, "pip_exact.h")).read()
    assert "fma(" in pip and "__host__ __device__" in pip
