"""CPU: the .vec reader's entries (dge_vectors_*, dge_model_load_vectors, dge_knn_cosine_vectors, dge_ndcg_at_k_vectors) are part of the C ABI — declared,
exported, bound — were added without moving the version or the trainer's build stamp, and refuse null / negative arguments before they look for a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "embedding_amd", "csrc")
ENTRIES = ("dge_vectors_from_vec_text", "dge_vectors_from_vec_files", "dge_vectors_from_host", "dge_vectors_info", "dge_vectors_to_host", "dge_vectors_free",
           "dge_model_load_vectors", "dge_knn_cosine_vectors", "dge_ndcg_at_k_vectors")


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
    assert re.search(r"\bdge_vec_info\b", h) and re.search(r"\bdge_vectors\b", h)
    assert dge.lib.dge_version() == 106            # additions only: no bump
    for cls, methods in ((dge.Vectors, ("from_vec", "from_host", "to_host", "present", "knn", "ndcg_against")), (dge.SgnsModel, ("load_vectors",))):
        for m in methods:
            assert callable(getattr(cls, m)), m
    from embedding_amd import evaluate
    assert callable(evaluate.knn_cosine_vectors) and callable(evaluate.ndcg_vectors)


def test_info_layout(dge):
    from embedding_amd._native import VecInfo
    assert C.sizeof(VecInfo) == 88
    assert [f[0] for f in VecInfo._fields_] == ["bytes", "lines", "rows", "values", "dropped", "missing", "names_added", "host_values", "dim", "reserved",
                                                "read_ms", "kernel_ms"]
    assert [getattr(VecInfo, f[0]).offset for f in VecInfo._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 68, 72, 80]
    h = open(os.path.join(ROOT, "include", "dge.h")).read()
    body = re.search(r"typedef struct dge_vec_info \{(.*?)\} dge_vec_info;", h, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+);", body) == [f[0] for f in VecInfo._fields_]


def test_null_and_negative_arguments_are_argument_errors_without_a_device(dge):
    from embedding_amd._native import VecInfo
    lib = dge.lib
    names = dge.Names(["a"])
    out = C.c_void_p(0); info = VecInfo(); n = C.c_int64(0); nd = C.c_double(0)
    path = (C.c_char_p * 1)(b"/nonexistent.vec")
    rows = (C.c_float * 4)(); idx = (C.c_int32 * 4)()
    text = b"a 1 2\n"
    calls = {
        "dge_vectors_from_vec_text": [lambda: lib.dge_vectors_from_vec_text(0, text, len(text), 0, None, 1, C.byref(out), C.byref(info)),
                                      lambda: lib.dge_vectors_from_vec_text(0, text, len(text), 0, names._h, 1, None, C.byref(info)),
                                      lambda: lib.dge_vectors_from_vec_text(0, None, len(text), 0, names._h, 1, C.byref(out), C.byref(info)),
                                      lambda: lib.dge_vectors_from_vec_text(0, text, -1, 0, names._h, 1, C.byref(out), C.byref(info))],
        "dge_vectors_from_vec_files": [lambda: lib.dge_vectors_from_vec_files(0, path, 1, 0, None, 1, C.byref(out), C.byref(info)),
                                       lambda: lib.dge_vectors_from_vec_files(0, path, 1, 0, names._h, 1, None, C.byref(info)),
                                       lambda: lib.dge_vectors_from_vec_files(0, None, 1, 0, names._h, 1, C.byref(out), C.byref(info)),
                                       lambda: lib.dge_vectors_from_vec_files(0, path, -1, 0, names._h, 1, C.byref(out), C.byref(info))],
        "dge_vectors_from_host": [lambda: lib.dge_vectors_from_host(0, rows, 2, 2, None, None),
                                  lambda: lib.dge_vectors_from_host(0, None, 2, 2, None, C.byref(out)),
                                  lambda: lib.dge_vectors_from_host(0, rows, -1, 2, None, C.byref(out)),
                                  lambda: lib.dge_vectors_from_host(0, rows, 2, -2, None, C.byref(out))],
        "dge_vectors_info": [lambda: lib.dge_vectors_info(None, C.byref(n), None, None, None)],
        "dge_vectors_to_host": [lambda: lib.dge_vectors_to_host(None, rows, None, 4)],
        "dge_model_load_vectors": [lambda: lib.dge_model_load_vectors(None, None, C.byref(n))],
        "dge_knn_cosine_vectors": [lambda: lib.dge_knn_cosine_vectors(None, 1, idx, rows, C.byref(nd))],
        "dge_ndcg_at_k_vectors": [lambda: lib.dge_ndcg_at_k_vectors(None, None, 1, C.byref(nd), C.byref(nd))],
    }
    for name, forms in calls.items():
        for k, call in enumerate(forms):
            assert call() == 1, (name, k)              # DGE_ERR_ARG, on a machine with or without a GPU
            msg = (lib.dge_last_error() or b"").decode()
            assert name in msg and "null" in msg, msg
    assert names.as_bytes() == [b"a"] and not out.value
    lib.dge_vectors_free(None)                         # like free(NULL)


def test_vec_read_is_built_into_the_library_and_stays_out_of_the_stamp():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = next(l for l in mk.splitlines() if l.startswith("OBJS")).split()
    assert "vec_read.o" in objs and os.path.exists(os.path.join(CSRC, "vec_read.hip")) and os.path.exists(os.path.join(CSRC, "vec_parse.h"))
    hash_lines = "".join(l for l in mk.splitlines() if "HASH" in l)
    for word in ("vec_read", "vec_parse", "seq_tokens", "sgns_io", "knn"):
        assert word not in hash_lines
    recipes = [l for l in mk.splitlines() if l.startswith("\t") and "vec_read" in l]
    assert recipes == []                               # the generic rule builds it
    # the tokeniser exists once: both readers include the header that holds it
    # (the joiner is host code and stands in seq_pieces.h, which seq_tokens.h includes)
    tok = open(os.path.join(CSRC, "seq_tokens.h")).read()
    assert '#include "seq_pieces.h"' in tok and "struct SeqJoiner" not in tok
    tok += open(os.path.join(CSRC, "seq_pieces.h")).read()
    for name in ("k_seq_count", "k_seq_emit", "k_seq_hash", "k_seq_intern", "k_seq_row_first", "struct SeqJoiner"):
        assert tok.count("void __launch_bounds__(SEQ_BLOCK) " + name + "(") == 1 or (name.startswith("struct") and tok.count(name) == 1), name
        for f in ("seq_ingest.hip", "vec_read.hip"):
            src = open(os.path.join(CSRC, f)).read()
            assert '#include "seq_tokens.h"' in src and ") " + name + "(" not in src and name + " {" not in src, (f, name)
