"""CPU: the trip-text entries (dge_trips_parse_texts, dge_flows_add_trip_texts, dge_flows_add_trip_files) are part of the C ABI — declared, exported, bound —
were added without moving the version or the trainer's build stamp, their structs are as large as include/dge.h says, and every bad argument is DGE_ERR_ARG
before a device is looked for."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "embedding_amd", "csrc")
ENTRIES = ("dge_trips_parse_texts", "dge_flows_add_trip_texts", "dge_flows_add_trip_files")


def test_the_entries_are_declared_exported_and_bound(dge):
    h = open(os.path.join(ROOT, "include", "dge.h")).read()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    declared = set(re.findall(r"\b(dge_[a-z0-9_]+)\s*\(", code))
    raw = C.CDLL(dge.LIB_PATH)
    from embedding_amd._native import SIGNATURES
    for name in ENTRIES:
        assert name in declared and hasattr(raw, name) and name in SIGNATURES, name
    assert dge.lib.dge_version() == 106            # additions only: no bump
    assert callable(dge.parse_trips) and callable(dge.Flows.add_trip_text) and callable(dge.Flows.add_trip_files)
    assert re.search(r"DGE_TRIPS_TYPE1 = 1, DGE_TRIPS_TYPE2 = 2, DGE_TRIPS_TYPE3 = 3", code)
    assert "65 535" in h and "DEVIATION" in h      # the rule states its deviations


def test_struct_layouts(dge):
    from embedding_amd._native import TripTextInfo, TripTextOptions
    h = open(os.path.join(ROOT, "include", "dge.h")).read()
    for cls, size, pattern in ((TripTextOptions, 16, r"struct dge_trip_text_options \{(.*?)\};\s*/\* 16 bytes \*/"),
                               (TripTextInfo, 88, r"typedef struct dge_trip_text_info \{(.*?)\} dge_trip_text_info;\s*/\* 88 bytes \*/")):
        assert C.sizeof(cls) == size
        body = re.sub(r"/\*.*?\*/", "", re.search(pattern, h, flags=re.S).group(1), flags=re.S)
        assert re.findall(r"\b(\w+);", body) == [f[0] for f in cls._fields_]
        assert all(getattr(cls, f[0]).offset % C.sizeof(f[1]) == 0 for f in cls._fields_)


def test_bad_arguments_are_argument_errors_without_a_device(dge):
    from embedding_amd._native import TripTextInfo, TripTextOptions
    lib = dge.lib
    text = np.frombuffer(b"a,b\n", np.uint8)
    ptrs = (C.c_void_p * 1)(text.ctypes.data)
    null_ptrs = (C.c_void_p * 1)(None)
    sizes = (C.c_int64 * 1)(text.size)
    neg = (C.c_int64 * 1)(-1)
    paths = (C.c_char_p * 1)(b"/nonexistent/trips.csv")
    n = C.c_int64(-7)
    inf = TripTextInfo()
    good = TripTextOptions(3, 1, 0)
    fake = C.c_void_p(1 << 20)          # never dereferenced: the argument checks come first

    def opt(fmt=3, header=1, slab=0):
        return C.byref(TripTextOptions(fmt, header, slab))

    st = np.zeros(4, np.uint8); hr = np.zeros(4, np.int32); xy = np.zeros(8, np.float64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    parse = lambda texts, sz, k, o, cap=0, out=C.byref(n), arrays=(None, None, None, None): lib.dge_trips_parse_texts(0, texts, sz, k, o, *arrays, cap, out, C.byref(inf))
    cases = {
        "parse: null n_lines": lambda: parse(ptrs, sizes, 1, C.byref(good), out=None),
        "parse: null texts": lambda: parse(None, sizes, 1, C.byref(good)),
        "parse: null sizes": lambda: parse(ptrs, None, 1, C.byref(good)),
        "parse: negative n": lambda: parse(ptrs, sizes, -1, C.byref(good)),
        "parse: negative size": lambda: parse(ptrs, neg, 1, C.byref(good)),
        "parse: null text": lambda: parse(null_ptrs, sizes, 1, C.byref(good)),
        "parse: negative cap": lambda: parse(ptrs, sizes, 1, C.byref(good), cap=-1),
        "parse: null arrays": lambda: parse(ptrs, sizes, 1, C.byref(good), cap=4, arrays=(p(st), None, p(xy), p(xy))),
        "parse: null options": lambda: parse(ptrs, sizes, 1, None),
        "parse: format 0": lambda: parse(ptrs, sizes, 1, opt(fmt=0)),
        "parse: format 4": lambda: parse(ptrs, sizes, 1, opt(fmt=4)),
        "parse: slab 1": lambda: parse(ptrs, sizes, 1, opt(slab=1)),
        "parse: slab 131071": lambda: parse(ptrs, sizes, 1, opt(slab=131071)),
        "parse: slab negative": lambda: parse(ptrs, sizes, 1, opt(slab=-1)),
        "texts: null flows": lambda: lib.dge_flows_add_trip_texts(None, ptrs, sizes, 1, C.byref(good), None),
        "texts: null texts": lambda: lib.dge_flows_add_trip_texts(fake, None, sizes, 1, C.byref(good), None),
        "texts: negative n": lambda: lib.dge_flows_add_trip_texts(fake, ptrs, sizes, -1, C.byref(good), None),
        "texts: null options": lambda: lib.dge_flows_add_trip_texts(fake, ptrs, sizes, 1, None, None),
        "texts: format 9": lambda: lib.dge_flows_add_trip_texts(fake, ptrs, sizes, 1, opt(fmt=9), None),
        "texts: slab 4096": lambda: lib.dge_flows_add_trip_texts(fake, ptrs, sizes, 1, opt(slab=4096), None),
        "files: null flows": lambda: lib.dge_flows_add_trip_files(None, paths, 1, C.byref(good), None),
        "files: null paths": lambda: lib.dge_flows_add_trip_files(fake, None, 1, C.byref(good), None),
        "files: null path": lambda: lib.dge_flows_add_trip_files(fake, null_ptrs, 1, C.byref(good), None),
        "files: negative n": lambda: lib.dge_flows_add_trip_files(fake, paths, -1, C.byref(good), None),
        "files: null options": lambda: lib.dge_flows_add_trip_files(fake, paths, 1, None, None),
        "files: format -1": lambda: lib.dge_flows_add_trip_files(fake, paths, 1, opt(fmt=-1), None),
        "files: slab 131071": lambda: lib.dge_flows_add_trip_files(fake, paths, 1, opt(slab=131071), None),
    }
    for what, call in cases.items():
        assert call() == 1, what
        msg = (lib.dge_last_error() or b"").decode()
        assert "dge_" in msg, (what, msg)
    assert n.value == -7 and inf.lines == 0


def test_trip_text_is_built_into_the_library_and_stays_out_of_the_stamp():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = next(l for l in mk.splitlines() if l.startswith("OBJS")).split()
    hdrs = next(l for l in mk.splitlines() if l.startswith("HDRS")).split()
    assert "trip_text.o" in objs and "trip_parse.h" in hdrs
    hash_lines = "".join(l for l in mk.splitlines() if "HASH" in l)
    assert "trip_text" not in hash_lines and "trip_parse" not in hash_lines
    assert [l for l in mk.splitlines() if l.startswith("\t") and "trip_text" in l] == []      # the generic rule builds it
    src = open(os.path.join(CSRC, "trip_text.hip")).read()
    assert '#include "trip_parse.h"' in src and "trip_parse_line(" in src and "atomicAdd(float" not in src and "atomicAdd(double" not in src
    parse = open(os.path.join(CSRC, "trip_parse.h")).read()
    code = re.sub(r"//.*", "", parse.split("// ---- host only")[0])
    assert "od_parse_f64(" in code and not re.search(r"\b(double|float)\b", code)      # integers only on the device's side
