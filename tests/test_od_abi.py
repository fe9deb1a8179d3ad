"""CPU: the .od reader's entries (dge_graph_add_od_files, dge_graph_add_od_texts, dge_graph_regions) are part of the C ABI — declared, exported, bound — were
added without moving the version or the trainer's build stamp, and refuse null / negative arguments before they look for a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "embedding_amd", "csrc")
ENTRIES = ("dge_graph_add_od_files", "dge_graph_add_od_texts", "dge_graph_regions")


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
    assert callable(dge.DeviceGraph.from_od) and callable(dge.DeviceGraph.regions)


def test_info_layout(dge):
    from embedding_amd._native import OdInfo
    assert C.sizeof(OdInfo) == 88
    fields = ["bytes", "lines", "flows", "edges", "dropped", "regions", "sources", "host_values", "slices", "reserved", "read_ms", "kernel_ms"]
    assert [f[0] for f in OdInfo._fields_] == fields
    assert [getattr(OdInfo, f).offset for f in fields] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 68, 72, 80]
    h = open(os.path.join(ROOT, "include", "dge.h")).read()
    body = re.search(r"typedef struct dge_od_info \{(.*?)\} dge_od_info;", h, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+);", body) == fields


def test_null_and_negative_arguments_are_argument_errors_without_a_device(dge):
    """A graph handle cannot exist without a device, so on a machine without one every call below has g == NULL among its faults; what is checked is that each
    form is DGE_ERR_ARG with the entry's name — never DGE_ERR_DEVICE — and that names and info stay untouched."""
    from embedding_amd._native import OdInfo
    lib = dge.lib
    names = dge.Names(["a"])
    empty = dge.Names()
    info = OdInfo(); info.edges = -5
    n = C.c_int64(-1)
    text = b"1 2 3\n"
    texts = (C.c_char_p * 2)(text, text); sizes = (C.c_int64 * 2)(len(text), len(text)); neg = (C.c_int64 * 2)(len(text), -1)
    null_text = (C.c_char_p * 2)(text, None)
    paths = (C.c_char_p * 2)(b"/nonexistent-0.od", b"/nonexistent-1.od"); null_path = (C.c_char_p * 2)(b"/nonexistent-0.od", None)
    fake = C.c_void_p(0)                                # no graph: the one argument fault a machine without a device can always show
    buf = (C.c_int64 * 4)()
    calls = {
        "dge_graph_add_od_texts": [lambda: lib.dge_graph_add_od_texts(fake, texts, sizes, 2, empty._h, C.byref(info)),
                                   lambda: lib.dge_graph_add_od_texts(None, None, sizes, 2, None, None),
                                   lambda: lib.dge_graph_add_od_texts(None, texts, None, 2, None, None),
                                   lambda: lib.dge_graph_add_od_texts(None, texts, sizes, 0, None, None),
                                   lambda: lib.dge_graph_add_od_texts(None, texts, sizes, -1, None, None),
                                   lambda: lib.dge_graph_add_od_texts(None, texts, neg, 2, names._h, C.byref(info)),
                                   lambda: lib.dge_graph_add_od_texts(None, null_text, sizes, 2, names._h, C.byref(info))],
        "dge_graph_add_od_files": [lambda: lib.dge_graph_add_od_files(fake, paths, 2, empty._h, C.byref(info)),
                                   lambda: lib.dge_graph_add_od_files(None, None, 2, None, None),
                                   lambda: lib.dge_graph_add_od_files(None, paths, 0, None, None),
                                   lambda: lib.dge_graph_add_od_files(None, paths, -3, names._h, C.byref(info)),
                                   lambda: lib.dge_graph_add_od_files(None, null_path, 2, names._h, C.byref(info))],
        "dge_graph_regions": [lambda: lib.dge_graph_regions(None, buf, 4, C.byref(n)),
                              lambda: lib.dge_graph_regions(None, None, 0, C.byref(n))],
    }
    for name, forms in calls.items():
        for k, call in enumerate(forms):
            assert call() == 1, (name, k)              # DGE_ERR_ARG, on a machine with or without a GPU
            msg = (lib.dge_last_error() or b"").decode()
            assert name in msg and "null" in msg, msg
    assert names.as_bytes() == [b"a"] and len(empty) == 0 and info.edges == -5 and n.value == -1


def test_od_read_is_built_into_the_library_and_stays_out_of_the_stamp():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = next(l for l in mk.splitlines() if l.startswith("OBJS")).split()
    hdrs = next(l for l in mk.splitlines() if l.startswith("HDRS")).split()
    assert "od_read.o" in objs and "od_parse.h" in hdrs and os.path.exists(os.path.join(CSRC, "od_read.hip")) and os.path.exists(os.path.join(CSRC, "od_parse.h"))
    hash_lines = "".join(l for l in mk.splitlines() if "HASH" in l)
    for word in ("od_read", "od_parse", "seq_tokens"):
        assert word not in hash_lines
    assert [l for l in mk.splitlines() if l.startswith("\t") and "od_read" in l] == []      # the generic rule builds it
    # the third reader sits on the shared tokeniser and the .vec grammar: it includes both and restates neither
    src = open(os.path.join(CSRC, "od_read.hip")).read()
    assert '#include "seq_tokens.h"' in src and '#include "od_parse.h"' in src
    for name in ("k_seq_count", "k_seq_emit", "k_seq_row_first", "struct SeqJoiner"):
        assert ") " + name + "(" not in src and name + " {" not in src, name
    parse = open(os.path.join(CSRC, "od_parse.h")).read()
    assert '#include "vec_parse.h"' in parse and "vec_msb128(" in parse and "VEC_HD int vec_msb128" not in parse
    code = "\n".join(l.split("//")[0] for l in parse.splitlines())
    assert not re.search(r"\b(double|float)\b", code)                                       # integer arithmetic only
