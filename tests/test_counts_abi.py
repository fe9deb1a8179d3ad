"""CPU: the count tables (dge_counts_*) are part of the C ABI — declared, exported, bound — were added without moving the version or the trainer's build stamp,
and refuse every bad plain argument the header lists with DGE_ERR_ARG and a message before they read a handle, look for a device or open a file."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "embedding_amd", "csrc")
ENTRIES = ("dge_counts_create", "dge_counts_destroy", "dge_counts_info", "dge_counts_to_host", "dge_counts_add_entries", "dge_counts_add_table_texts",
           "dge_counts_add_table_files", "dge_counts_add_points", "dge_counts_merge", "dge_counts_vectors")


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
    assert re.search(r"\bdge_table_read_options\b", h) and re.search(r"\bdge_table_read_info\b", h) and re.search(r"\bstruct dge_counts_info\b", h)
    assert dge.lib.dge_version() == 106            # additions only: no bump
    for method in ("add_table", "add_entries", "add_points", "merge", "to_host", "info", "vectors", "close"):
        assert callable(getattr(dge.Counts, method))


def test_struct_layouts(dge):
    from embedding_amd._native import CountsInfo, TableReadInfo, TableReadOptions
    assert C.sizeof(TableReadOptions) == 56
    assert [(f[0], getattr(TableReadOptions, f[0]).offset) for f in TableReadOptions._fields_] == [
        ("sep", 0), ("skip_lines", 4), ("key_field", 8), ("key_lo", 12), ("key_hi", 16), ("col_lo", 20), ("n_cols", 24), ("col_offset", 28), ("neg_col_offset", 32),
        ("reserved", 36), ("slab_bytes", 40), ("reserved2", 48)]
    assert C.sizeof(TableReadInfo) == 88
    assert [f[0] for f in TableReadInfo._fields_] == ["bytes", "lines", "skipped", "empty", "rows", "foreign", "values", "total", "pieces", "slabs", "read_ms", "kernel_ms"]
    assert [getattr(TableReadInfo, f[0]).offset for f in TableReadInfo._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 68, 72, 80]
    assert C.sizeof(CountsInfo) == 32 and [f[0] for f in CountsInfo._fields_] == ["regions", "cols", "nonzero", "total"]
    # the header states the same offsets
    h = open(os.path.join(ROOT, "include", "dge.h")).read()
    body = h[h.index("typedef struct dge_table_read_options {"):h.index("} dge_table_read_info;")]
    assert "/* 56 bytes */" in body and "/* 40: 0 = the default" in body and "/* 80 " in body


def test_table_read_is_built_into_the_library_and_stays_out_of_the_stamp():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = next(l for l in mk.splitlines() if l.startswith("OBJS")).split()
    hdrs = next(l for l in mk.splitlines() if l.startswith("HDRS")).split()
    assert "table_read.o" in objs and os.path.exists(os.path.join(CSRC, "table_read.hip"))
    assert "table_parse.h" in hdrs
    hash_lines = "".join(l for l in mk.splitlines() if "HASH" in l)
    assert "table_read" not in hash_lines and "table_parse" not in hash_lines
    assert [l for l in mk.splitlines() if l.startswith("\t") and "table_" in l] == []      # the generic rule builds it
    # the parser is free of HIP calls and of floating point; the trip feeder is still the only feeder of seq_pieces.h, and the reader uses it
    parse = re.sub(r"//.*", "", open(os.path.join(CSRC, "table_parse.h")).read())
    assert "hip/" not in parse and "double" not in parse and "float" not in parse
    pieces = open(os.path.join(CSRC, "seq_pieces.h")).read()
    assert re.findall(r"struct (\w*Feeder)\b", pieces) == ["TripFeeder"] and "table" not in pieces.lower()
    reader = open(os.path.join(CSRC, "table_read.hip")).read()
    assert "TripFeeder feed{" in reader and "struct TripFeeder" not in reader


def test_bad_arguments_are_argument_errors_without_a_device(dge, tmp_path):
    """Every form is decided by the plain arguments alone: status 1 with or without a GPU, the entry's name in the message, and the table handle — 256 zero
    bytes — is never read.  The path does not exist: had a file been looked for, the status would be DGE_ERR_IO."""
    from embedding_amd._native import TableReadInfo, TableReadOptions
    lib = dge.lib
    c = C.create_string_buffer(256)
    info = TableReadInfo()
    body = b"100,1,2\n200,3,4\n"
    texts = (C.c_char_p * 2)(body, body)
    null_text = (C.c_char_p * 2)(body, None)
    sizes = (C.c_int64 * 2)(len(body), len(body))
    neg_sizes = (C.c_int64 * 2)(len(body), -1)
    path = os.fsencode(str(tmp_path / "never.csv"))
    paths = (C.c_char_p * 2)(path, path)
    null_path = (C.c_char_p * 2)(path, None)

    def opts(**kw):
        f = dict(sep=ord(","), skip_lines=0, key_field=0, key_lo=0, key_hi=0, col_lo=1, n_cols=2, col_offset=0, neg_col_offset=-1, reserved=0, slab_bytes=0, reserved2=0)
        f.update(kw)
        return TableReadOptions(*[f[name] for name, _ in TableReadOptions._fields_])

    def texts_call(h=c, t=texts, s=sizes, n=2, opt=opts()):
        return lambda: lib.dge_counts_add_table_texts(h, t, s, n, C.byref(opt) if opt is not None else None, C.byref(info))

    def files_call(h=c, p=paths, n=2, opt=opts()):
        return lambda: lib.dge_counts_add_table_files(h, p, n, C.byref(opt) if opt is not None else None, C.byref(info))

    def options(call):
        return [(call(opt=opts(sep=ord(";"))), "sep"), (call(opt=opts(sep=0)), "sep"), (call(opt=opts(reserved=7)), "reserved"), (call(opt=opts(reserved2=7)), "reserved"),
                (call(opt=opts(skip_lines=-1)), "skip_lines"), (call(opt=opts(key_field=-1)), "key_field"), (call(opt=opts(key_lo=-1)), "key_lo"),
                (call(opt=opts(key_lo=5, key_hi=5)), "key_hi"), (call(opt=opts(key_hi=-1)), "key_hi"), (call(opt=opts(key_hi=2 ** 31 - 1)), "key_hi"),
                (call(opt=opts(key_lo=65537)), "key_lo"), (call(opt=opts(key_lo=65536, key_hi=65537)), "key_hi"), (call(opt=opts(col_lo=-1)), "col_lo"),
                (call(opt=opts(n_cols=0)), "n_cols"), (call(opt=opts(n_cols=1025)), "n_cols"), (call(opt=opts(key_field=2)), "key_field"),
                (call(opt=opts(col_offset=-1)), "col_offset"), (call(opt=opts(neg_col_offset=-2)), "neg_col_offset"), (call(opt=opts(slab_bytes=-1)), "slab_bytes"),
                (call(opt=opts(slab_bytes=131071)), "slab_bytes"), (call(n=0), "n_pieces"), (call(n=-1), "null or negative"), (call(h=None), "null"), (call(opt=None), "null")]

    forms = {
        "dge_counts_add_table_texts": options(texts_call) + [(texts_call(t=None), "null"), (texts_call(s=None), "null"), (texts_call(t=null_text), "text 1"),
                                                             (texts_call(s=neg_sizes), "text 1")],
        "dge_counts_add_table_files": options(files_call) + [(files_call(p=None), "null"), (files_call(p=null_path), "path 1")],
    }
    for name, calls in forms.items():
        for k, (call, word) in enumerate(calls):
            assert call() == 1, (name, k)              # DGE_ERR_ARG
            msg = (lib.dge_last_error() or b"").decode()
            assert name in msg and word in msg, (name, k, msg)
    assert not os.path.exists(path)
    # the other entries' plain arguments
    out = C.c_void_p(0)
    one = (C.c_int32 * 1)(0)
    val = (C.c_int64 * 1)(1)
    xy = (C.c_double * 2)(0.0, 0.0)
    others = [
        ("dge_counts_create", lambda: lib.dge_counts_create(None, 4, C.byref(out)), "null"), ("dge_counts_create", lambda: lib.dge_counts_create(c, 4, None), "null"),
        ("dge_counts_create", lambda: lib.dge_counts_create(c, 0, C.byref(out)), "n_cols"), ("dge_counts_create", lambda: lib.dge_counts_create(c, 1025, C.byref(out)), "n_cols"),
        ("dge_counts_info", lambda: lib.dge_counts_info(None, None), "null"), ("dge_counts_to_host", lambda: lib.dge_counts_to_host(None, None), "null"),
        ("dge_counts_add_entries", lambda: lib.dge_counts_add_entries(None, one, one, val, 1), "null"),
        ("dge_counts_add_entries", lambda: lib.dge_counts_add_entries(c, one, one, val, -1), "negative"),
        ("dge_counts_add_entries", lambda: lib.dge_counts_add_entries(c, None, one, val, 1), "null"),
        ("dge_counts_add_points", lambda: lib.dge_counts_add_points(None, xy, one, 1, None), "null"),
        ("dge_counts_add_points", lambda: lib.dge_counts_add_points(c, xy, None, 1, None), "null"),
        ("dge_counts_add_points", lambda: lib.dge_counts_add_points(c, xy, one, -1, None), "negative"),
        ("dge_counts_merge", lambda: lib.dge_counts_merge(c, c, one, None), "null"), ("dge_counts_merge", lambda: lib.dge_counts_merge(None, c, one, C.byref(out)), "null"),
        ("dge_counts_merge", lambda: lib.dge_counts_merge(c, None, one, C.byref(out)), "null"),
        ("dge_counts_vectors", lambda: lib.dge_counts_vectors(None, 0, 1, 1, 0, C.byref(out)), "null"),
        ("dge_counts_vectors", lambda: lib.dge_counts_vectors(c, 0, 1, 1, 0, None), "null"),
        ("dge_counts_vectors", lambda: lib.dge_counts_vectors(c, 0, 1, 1, 2, C.byref(out)), "present_mode"),
    ]
    for k, (name, call, word) in enumerate(others):
        assert call() == 1, (name, k)
        msg = (lib.dge_last_error() or b"").decode()
        assert name in msg and word in msg, (name, k, msg)
    lib.dge_counts_destroy(None)                       # a null handle is nothing to free
