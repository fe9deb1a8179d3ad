"""CPU: the flow table's text writers (dge_flows_to_text, dge_flows_write_text, dge_flows_time_series, dge_flows_time_series_text,
dge_flows_write_time_series) are part of the C ABI — declared, exported, bound — were added without moving the version or the trainer's build stamp, and refuse
every bad argument the header lists with DGE_ERR_ARG and a message before they look for a device and before they touch a path."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "embedding_amd", "csrc")
ENTRIES = ("dge_flows_to_text", "dge_flows_write_text", "dge_flows_time_series", "dge_flows_time_series_text", "dge_flows_write_time_series")
OD, LAYERED, MATRIX = 0, 1, 2


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
    assert re.search(r"\bdge_flow_text_info\b", h) and re.search(r"\bdge_flow_slices\b", h)
    assert re.search(r"DGE_FLOW_TEXT_OD = 0, DGE_FLOW_TEXT_OD_LAYERED = 1, DGE_FLOW_TEXT_MATRIX = 2", h)
    assert dge.lib.dge_version() == 106            # additions only: no bump
    for name in ("od_text", "write_od", "matrix_text", "write_matrix", "time_series", "time_series_text", "write_time_series", "to_od_bytes"):
        assert callable(getattr(dge.Flows, name))


def test_struct_layouts(dge):
    from embedding_amd._native import FlowSlices, FlowTextInfo
    assert C.sizeof(FlowTextInfo) == 56
    assert [f[0] for f in FlowTextInfo._fields_] == ["bytes", "lines", "edges", "zeros", "slices", "reserved", "kernel_ms", "write_ms"]
    assert [getattr(FlowTextInfo, f[0]).offset for f in FlowTextInfo._fields_] == [0, 8, 16, 24, 32, 36, 40, 48]
    assert C.sizeof(FlowSlices) == 24
    assert [(f[0], getattr(FlowSlices, f[0]).offset) for f in FlowSlices._fields_] == [("T", 0), ("mode", 4), ("K", 8), ("reserved", 12), ("win", 16)]


def test_flow_text_is_built_into_the_library_and_stays_out_of_the_stamp():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = next(l for l in mk.splitlines() if l.startswith("OBJS")).split()
    assert "flow_text.o" in objs and os.path.exists(os.path.join(CSRC, "flow_text.hip"))
    hash_lines = "".join(l for l in mk.splitlines() if "HASH" in l)
    assert "flow_text" not in hash_lines and "text_out_pump" not in hash_lines
    assert [l for l in mk.splitlines() if l.startswith("\t") and "flow_text" in l] == []      # the generic rule builds it
    # one pump, two writers
    for unit in ("seq_write.hip", "flow_text.hip"):
        src = open(os.path.join(CSRC, unit)).read()
        assert '#include "text_out_pump.h"' in src and "hipHostMalloc" not in src


def test_bad_arguments_are_argument_errors_without_a_device(dge, tmp_path):
    """Every form is decided by the arguments alone: status 1 with or without a GPU, the entry's name in the message, no file at the path, nothing written.
    The table handle of the forms that carry one is 256 zero bytes: plain values are checked before handles, so it is never read."""
    from embedding_amd._native import FlowSlices, FlowTextInfo, HourWindow
    lib = dge.lib
    f = C.create_string_buffer(256)
    info = FlowTextInfo(); n = C.c_int64(-7)
    text = C.create_string_buffer(b"\xAA" * 16, 16)
    path = os.fsencode(str(tmp_path / "never.od"))
    paths1 = (C.c_char_p * 1)(path)
    paths2 = (C.c_char_p * 2)(path, None)
    sel = C.create_string_buffer(8)
    slots = FlowSlices(1, 0, 0, 0, None)
    win = (HourWindow * 2)(HourWindow(0, 1), HourWindow(5, 24))
    wins = FlowSlices(0, 0, 2, 0, C.cast(win, C.POINTER(HourWindow)))
    badwin = (HourWindow * 1)(HourWindow(24, 1))

    def to_text(h=f, s=slots, kind=OD, k=0, select=None, sep=0, buf=text, cap=16, nb=C.byref(n)):
        return lambda: lib.dge_flows_to_text(h, C.byref(s) if s is not None else None, kind, k, select, sep, buf, cap, nb, C.byref(info))

    def write(h=f, s=slots, kind=OD, select=None, sep=0, arr=paths1, count=1):
        return lambda: lib.dge_flows_write_text(h, C.byref(s) if s is not None else None, kind, select, sep, arr, count, C.byref(info))

    forms = {
        "dge_flows_to_text": [
            (to_text(h=None), "null"), (to_text(s=None), "null"), (to_text(nb=None), "null"), (to_text(buf=None), "null"), (to_text(cap=-1), "null"), (to_text(k=-1), "null"),
            (to_text(kind=3), "kind"), (to_text(kind=-1), "kind"),
            (to_text(sep=ord(",")), "sep"), (to_text(select=sel), "select"), (to_text(kind=LAYERED, sep=ord(" ")), "sep"),
            (to_text(kind=MATRIX, sep=0), "sep"), (to_text(kind=MATRIX, sep=ord(";")), "sep"),
            (to_text(k=1), "slice"), (to_text(s=wins, k=2), "slice"), (to_text(s=wins, kind=LAYERED, k=1), "slice"),
            (to_text(s=FlowSlices(5, 0, 0, 0, None)), "divides 24"), (to_text(s=FlowSlices(25, 1, 0, 0, None)), "T"), (to_text(s=FlowSlices(1, 2, 0, 0, None)), "mode"),
            (to_text(s=FlowSlices(0, 0, -1, 0, None)), "K"), (to_text(s=FlowSlices(1, 0, 0, 9, None)), "reserved"),
            (to_text(s=FlowSlices(1, 0, 2, 0, C.cast(win, C.POINTER(HourWindow)))), "windows"), (to_text(s=FlowSlices(0, 1, 2, 0, C.cast(win, C.POINTER(HourWindow)))), "windows"),
            (to_text(s=FlowSlices(0, 0, 2, 0, None)), "null"), (to_text(s=FlowSlices(0, 0, 1, 0, C.cast(badwin, C.POINTER(HourWindow)))), "window 0")],
        "dge_flows_write_text": [
            (write(h=None), "null"), (write(s=None), "null"), (write(arr=None), "null"), (write(count=-1), "null"), (write(s=wins, arr=paths2, count=2), "null"),
            (write(kind=7), "kind"), (write(sep=ord(",")), "sep"), (write(select=sel), "select"), (write(kind=MATRIX, sep=ord("x")), "sep"),
            (write(s=FlowSlices(24, 0, 0, 0, None)), "n_paths"), (write(count=0), "n_paths"), (write(s=wins), "n_paths"), (write(s=wins, kind=LAYERED, arr=paths2, count=2), "null"),
            (write(s=FlowSlices(7, 0, 0, 0, None)), "divides 24")],
        "dge_flows_time_series": [
            (lambda: lib.dge_flows_time_series(None, None, None, None, None, 0, C.byref(n)), "null"),
            (lambda: lib.dge_flows_time_series(f, None, None, None, None, 0, None), "null"),
            (lambda: lib.dge_flows_time_series(f, None, None, None, None, -1, C.byref(n)), "null"),
            (lambda: lib.dge_flows_time_series(f, None, None, text, text, 1, C.byref(n)), "null")],
        "dge_flows_time_series_text": [
            (lambda: lib.dge_flows_time_series_text(None, None, text, 16, C.byref(n), None), "null"),
            (lambda: lib.dge_flows_time_series_text(f, None, text, 16, None, None), "null"),
            (lambda: lib.dge_flows_time_series_text(f, None, None, 16, C.byref(n), None), "null"),
            (lambda: lib.dge_flows_time_series_text(f, None, text, -1, C.byref(n), None), "null")],
        "dge_flows_write_time_series": [
            (lambda: lib.dge_flows_write_time_series(None, None, path, None), "null"),
            (lambda: lib.dge_flows_write_time_series(f, None, None, None), "null")],
    }
    for name, calls in forms.items():
        for k, (call, word) in enumerate(calls):
            assert call() == 1, (name, k)              # DGE_ERR_ARG
            msg = (lib.dge_last_error() or b"").decode()
            assert name in msg and word in msg, (name, k, msg)
    assert not os.path.exists(path) and text.raw == b"\xAA" * 16 and n.value == -7
    # a layered text over two windows wants ONE path
    both = (C.c_char_p * 2)(path, path)
    assert write(s=wins, kind=LAYERED, arr=both, count=2)() == 1 and "n_paths" in lib.dge_last_error().decode() and not os.path.exists(path)
