"""CPU: the .matrix reader (dge_flows_add_matrix_texts, dge_flows_add_matrix_files) is part of the C ABI — declared, exported, bound — was added without
moving the version or the trainer's build stamp, and refuses every bad plain argument the header lists with DGE_ERR_ARG and a message before it reads the
handle, looks for a device or opens a file."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "embedding_amd", "csrc")
ENTRIES = ("dge_flows_add_matrix_texts", "dge_flows_add_matrix_files")


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
    assert re.search(r"\bdge_matrix_read_options\b", h) and re.search(r"\bdge_matrix_read_info\b", h)
    assert dge.lib.dge_version() == 106            # additions only: no bump
    assert callable(dge.Flows.add_matrix) and callable(dge.Regions.from_ids)


def test_struct_layouts(dge):
    from embedding_amd._native import MatrixReadInfo, MatrixReadOptions
    assert C.sizeof(MatrixReadOptions) == 16
    assert [(f[0], getattr(MatrixReadOptions, f[0]).offset) for f in MatrixReadOptions._fields_] == [("sep", 0), ("reserved", 4), ("slab_bytes", 8)]
    assert C.sizeof(MatrixReadInfo) == 88
    assert [f[0] for f in MatrixReadInfo._fields_] == ["bytes", "lines", "rows", "values", "entries", "zeros", "total", "pieces", "n", "tile_bytes", "slabs", "read_ms",
                                                      "kernel_ms"]
    assert [getattr(MatrixReadInfo, f[0]).offset for f in MatrixReadInfo._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 68, 72, 80]


def test_matrix_read_is_built_into_the_library_and_stays_out_of_the_stamp():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = next(l for l in mk.splitlines() if l.startswith("OBJS")).split()
    hdrs = next(l for l in mk.splitlines() if l.startswith("HDRS")).split()
    assert "matrix_read.o" in objs and os.path.exists(os.path.join(CSRC, "matrix_read.hip"))
    assert "matrix_parse.h" in hdrs and "matrix_feed.h" in hdrs
    hash_lines = "".join(l for l in mk.splitlines() if "HASH" in l)
    assert "matrix_read" not in hash_lines and "matrix_parse" not in hash_lines and "matrix_feed" not in hash_lines
    assert [l for l in mk.splitlines() if l.startswith("\t") and "matrix_" in l] == []      # the generic rule builds it
    # the feeder is free of HIP, and the trip feeder was left alone
    feed = open(os.path.join(CSRC, "matrix_feed.h")).read()
    assert "hip" not in re.sub(r"//.*", "", feed).lower() and "struct MatrixFeeder" in feed
    assert "matrix" not in open(os.path.join(CSRC, "seq_pieces.h")).read().lower()
    # one commit, two callers
    for unit in ("flow_windows.hip", "matrix_read.hip"):
        assert "trip_commit_entries(" in open(os.path.join(CSRC, unit)).read()


def test_bad_arguments_are_argument_errors_without_a_device(dge, tmp_path):
    """Every form is decided by the plain arguments alone: status 1 with or without a GPU, the entry's name in the message, and the table handle — 256 zero
    bytes — is never read.  The path does not exist: had a file been looked for, the status would be DGE_ERR_IO."""
    from embedding_amd._native import MatrixReadInfo, MatrixReadOptions
    lib = dge.lib
    f = C.create_string_buffer(256)
    info = MatrixReadInfo()
    body = b"1,2\n3,4\n"
    texts = (C.c_char_p * 2)(body, body)
    null_text = (C.c_char_p * 2)(body, None)
    sizes = (C.c_int64 * 2)(len(body), len(body))
    neg_sizes = (C.c_int64 * 2)(len(body), -1)
    hours = (C.c_int32 * 2)(0, 23)
    path = os.fsencode(str(tmp_path / "never.matrix"))
    paths = (C.c_char_p * 2)(path, path)
    null_path = (C.c_char_p * 2)(path, None)
    good = MatrixReadOptions(ord(","), 0, 0)

    def texts_call(h=f, t=texts, s=sizes, hr=hours, n=2, opt=good):
        return lambda: lib.dge_flows_add_matrix_texts(h, t, s, hr, n, None, C.byref(opt) if opt is not None else None, C.byref(info))

    def files_call(h=f, p=paths, hr=hours, n=2, opt=good):
        return lambda: lib.dge_flows_add_matrix_files(h, p, hr, n, None, C.byref(opt) if opt is not None else None, C.byref(info))

    def options(call):
        return [(call(opt=MatrixReadOptions(ord(";"), 0, 0)), "sep"), (call(opt=MatrixReadOptions(0, 0, 0)), "sep"), (call(opt=MatrixReadOptions(ord(","), 7, 0)), "reserved"),
                (call(opt=MatrixReadOptions(ord(","), 0, -1)), "slab_bytes"), (call(opt=MatrixReadOptions(ord(","), 0, 255)), "slab_bytes"),
                (call(opt=MatrixReadOptions(ord(","), 0, (16 << 20) + 1)), "slab_bytes"),
                (call(hr=(C.c_int32 * 2)(0, 24)), "hour"), (call(hr=(C.c_int32 * 2)(-1, 0)), "hour"), (call(n=0), "n_pieces"), (call(n=-1), "null or negative"),
                (call(h=None), "null"), (call(hr=None), "null"), (call(opt=None), "null")]

    forms = {
        "dge_flows_add_matrix_texts": options(texts_call) + [(texts_call(t=None), "null"), (texts_call(s=None), "null"), (texts_call(t=null_text), "text 1"),
                                                             (texts_call(s=neg_sizes), "text 1")],
        "dge_flows_add_matrix_files": options(files_call) + [(files_call(p=None), "null"), (files_call(p=null_path), "path 1")],
    }
    for name, calls in forms.items():
        for k, (call, word) in enumerate(calls):
            assert call() == 1, (name, k)              # DGE_ERR_ARG
            msg = (lib.dge_last_error() or b"").decode()
            assert name in msg and word in msg, (name, k, msg)
    assert not os.path.exists(path)
    # the least slab the entries take lets a small text cross slabs
    assert int(re.search(r"#define MAT_SLAB_MIN (\d+)", open(os.path.join(CSRC, "matrix_feed.h")).read()).group(1)) <= 4096
    assert texts_call(opt=MatrixReadOptions(ord(","), 0, 255))() == 1
