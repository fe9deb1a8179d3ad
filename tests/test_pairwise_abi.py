"""CPU: dge_pairwise_eval_vectors and dge_pairwise_ground_vectors are part of the C ABI — declared, exported, bound, added without moving the version, the knob
list or the trainer's build stamp — and refuse every bad argument of step 8 of the rule that needs no device before they look for one; the host helpers
evaluate.slice_rows / region_rows parse names as the reference does.

A resident-row handle cannot exist without a device, and the checks read only its host fields (device, rows, dim): the test hands the library a ctypes
mirror of struct dge_vectors (csrc/dge_internal.h) whose device pointers are null.  No call here gets as far as reading them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "embedding_amd", "csrc")
ENTRIES = ("dge_pairwise_eval_vectors", "dge_pairwise_ground_vectors")


class FakeVectors(C.Structure):
    """struct dge_vectors as csrc/dge_internal.h lays it out"""
    _fields_ = [("device", C.c_int), ("rows", C.c_int64), ("dim", C.c_int32), ("d", C.c_void_p), ("d_present", C.c_void_p), ("n_present", C.c_int64)]


def fake(rows, dim, device=0):
    return FakeVectors(device, rows, dim, None, None, rows)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_the_entries_are_declared_exported_and_bound(dge):
    h = open(os.path.join(ROOT, "include", "dge.h")).read()
    assert int(re.search(r"DGE_TUNE_COUNT\s*=\s*(\d+)", h).group(1)) == 22
    src = open(os.path.join(CSRC, "dge_internal.h")).read()
    body = re.search(r"struct dge_vectors \{(.*?)\};", src, flags=re.S).group(1)
    assert re.findall(r"\b(\w+)\s*=", body) == [f[0] for f in FakeVectors._fields_]         # the mirror above is the struct
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    declared = set(re.findall(r"\b(dge_[a-z0-9_]+)\s*\(", h))
    raw = C.CDLL(dge.LIB_PATH)
    from embedding_amd._native import SIGNATURES, PairwiseInfo
    for name in ENTRIES:
        assert name in declared and hasattr(raw, name) and name in SIGNATURES, name
        args = re.search(r"\b%s\s*\((.*?)\);" % name, h, flags=re.S).group(1)
        assert len(args.split(",")) == len(SIGNATURES[name][1]), name
    assert dge.lib.dge_version() == 106            # additions only: no bump
    assert C.sizeof(PairwiseInfo) == 56
    fields = ["regions", "members", "tested", "threshold_keys", "knn_ms", "ground_ms", "score_ms"]
    assert [f[0] for f in PairwiseInfo._fields_] == fields and [getattr(PairwiseInfo, f).offset for f in fields] == [0, 8, 16, 24, 32, 40, 48]
    body = re.search(r"typedef struct dge_pairwise_info \{(.*?)\} dge_pairwise_info;", open(os.path.join(ROOT, "include", "dge.h")).read(), flags=re.S).group(1)
    assert re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == fields
    import embedding_amd.evaluate as ev
    assert callable(dge.Vectors.pairwise_eval) and callable(dge.Vectors.pairwise_ground)
    assert callable(ev.pairwise_eval) and callable(ev.pairwise_ground) and callable(ev.slice_rows) and callable(ev.region_rows)
    assert ev.PAIRWISE_KS == (5, 10, 20, 30, 40, 50, 60, 70)


def test_bad_arguments_are_argument_errors_without_a_device(dge):
    from embedding_amd._native import PairwiseInfo
    lib = dge.lib
    n, V = 12, 30
    row_of = np.stack([np.arange(n), np.arange(n) + 12]).astype(np.int64)
    ks = np.array([1, 3, 5], np.int32)
    ndcg = np.full((2, 3), -7.0); prec = np.full((2, 3), -7.0); members = np.full(2, -7, np.int64); tested = np.full(2, -7, np.int64)
    info = PairwiseInfo(); info.regions = -5
    F, G = fake(V, 4), fake(n, 3)

    def call(f=F, g=G, ro=row_of, S=2, kk=ks, nk=3, rel_m=4, nd=ndcg, pr=prec, me=members, te=tested):
        rc = lib.dge_pairwise_eval_vectors(C.byref(f) if f is not None else None, C.byref(g) if g is not None else None, _p(ro), S, None, _p(kk), nk, rel_m,
                                           _p(nd), _p(pr), _p(me), _p(te), None, None, None, None, C.byref(info))
        return rc, (lib.dge_last_error() or b"").decode()

    def with_entry(s, i, v):
        r = row_of.copy(); r[s, i] = v
        return r

    cases = (
        ("no features", dict(f=None), ("null",)), ("no ground", dict(g=None), ("null",)), ("no row_of", dict(ro=None), ("null",)), ("no ks", dict(kk=None), ("null",)),
        ("no ndcg", dict(nd=None), ("null",)), ("no members", dict(me=None), ("null",)), ("no tested", dict(te=None), ("null",)),
        ("no sets", dict(S=0), ("n_sets = 0", "1 .. 64")), ("65 sets", dict(S=65), ("n_sets = 65",)), ("no k", dict(nk=0), ("n_k = 0", "1 .. 16")), ("17 k", dict(nk=17), ("n_k = 17",)),
        ("k 0", dict(kk=np.array([0, 3, 5], np.int32)), ("ks[0] = 0", "1 .. 128")), ("k 129", dict(kk=np.array([1, 3, 129], np.int32)), ("ks[2] = 129",)),
        ("unsorted", dict(kk=np.array([1, 5, 3], np.int32)), ("ks[2] = 3", "strictly ascending")), ("a k twice", dict(kk=np.array([1, 3, 3], np.int32)), ("strictly ascending",)),
        ("n - 1 < kmax", dict(kk=np.array([1, 3, 12], np.int32)), ("lists of 12", "11 other regions", "n - 1 < kmax")),
        ("one region", dict(g=fake(1, 3)), ("1 ground rows",)), ("ground dim 257", dict(g=fake(n, 257)), ("ground dim = 257", "1 .. 256")),
        ("dim 257", dict(f=fake(V, 257)), ("dim = 257", "1 .. 256")), ("dim 0", dict(f=fake(V, 0)), ("dim = 0",)), ("no rows", dict(f=fake(0, 4)), ("0 feature rows",)),
        ("rel_m n", dict(rel_m=12), ("rel_m = 12", "n - 1 = 11")), ("rel_m negative", dict(rel_m=-1), ("rel_m = -1",)),
        ("precision without rel_m", dict(rel_m=0), ("precision", "rel_m = 0")), ("rel_m without precision", dict(pr=None), ("precision", "rel_m = 4")),
        ("devices", dict(g=fake(n, 3, device=1)), ("devices 0 and 1",)),
        ("row_of V", dict(ro=with_entry(1, 7, V)), ("set 1, region 7", "row_of = 30", "-1 .. 29")), ("row_of -2", dict(ro=with_entry(0, 3, -2)), ("set 0, region 3", "row_of = -2")),
        ("named twice", dict(ro=with_entry(1, 2, 20)), ("set 1 names feature row 20 twice",)),
    )
    for what, kw, words in cases:
        rc, msg = call(**kw)
        assert rc == 1 and "dge_pairwise_eval_vectors" in msg, (what, rc, msg)
        for w in words:
            assert w in msg, (what, msg)
    # the same row in two DIFFERENT sets is nothing to refuse, nor is a missing region: the call goes on to look for a device.  The handles here hold no device
    # memory, so the call must be one that is still refused once a device is found, before anything is launched: with kmax = 11 set 1, 11 members, is short
    shared = row_of.copy(); shared[1] = row_of[0]; shared[1, 4] = -1
    rc, msg = call(ro=shared, kk=np.array([1, 3, 11], np.int32))
    assert rc == 6 or (rc == 1 and "set 1 has 11 members" in msg), (rc, msg)

    idx = np.full((n, 3), -7, np.int32); dist = np.full((n, 3), -7.0)
    for what, args, words in (("null", (None, 3, _p(idx), _p(dist)), ("null",)), ("no idx", (C.byref(G), 3, None, _p(dist)), ("null",)),
                              ("m 0", (C.byref(G), 0, _p(idx), _p(dist)), ("m = 0", "1 .. 128")), ("m 129", (C.byref(G), 129, _p(idx), _p(dist)), ("m = 129",)),
                              ("n - 1 < m", (C.byref(G), 12, _p(idx), _p(dist)), ("lists of 12", "n - 1 < kmax"))):
        rc = lib.dge_pairwise_ground_vectors(*args)
        msg = lib.dge_last_error().decode()
        assert rc == 1 and "dge_pairwise_ground_vectors" in msg, (what, rc, msg)
        for w in words:
            assert w in msg, (what, msg)
    assert (ndcg == -7).all() and (prec == -7).all() and (members == -7).all() and (tested == -7).all() and (idx == -7).all() and (dist == -7).all() and info.regions == -5


def test_slice_rows_and_region_rows():
    import embedding_amd.evaluate as ev
    ids = [10100, 10201, 10202, 10300]
    names = ["0-10100", b"1-10201", "2-10100", "0-99999", "1-10300", "0-10202", "1-10201", "7-10202", "0-10300"]
    row_of, counts = ev.slice_rows(names, ids, 2)
    assert row_of.dtype == np.int64 and row_of.tolist() == [[0, -1, 5, 8], [-1, 1, -1, 4]]
    assert counts == dict(foreign=2, unknown=1, duplicates=1)
    for bad in ("10100", "a-10100", "0-x", "0-1-2", "-1-10100"):
        with pytest.raises(ValueError):
            ev.slice_rows(["0-10100", bad], ids, 2)
    with pytest.raises(ValueError):
        ev.slice_rows(names, ids + [10100], 2)
    row_of, counts = ev.region_rows(["10300", "7", b"10100", "10300"], ids)
    assert row_of.tolist() == [[2, -1, -1, 0]] and counts == dict(unknown=1, duplicates=1)
    with pytest.raises(ValueError):
        ev.region_rows(["0-10100"], ids)


def test_the_python_view_checks_shapes_before_the_library(dge):
    class Shape:                                     # stands in for a Vectors: only .shape is read before the check fails
        shape = (12, 3)
    v = dge.Vectors(None, 0)
    with pytest.raises(ValueError):
        v.pairwise_eval(Shape(), np.zeros((2, 11), np.int64))
    with pytest.raises(ValueError):
        v.pairwise_eval(Shape(), np.zeros((2, 12), np.int64), ks=())
    with pytest.raises(ValueError):
        v.pairwise_eval(Shape(), np.zeros((2, 12), np.int64), test=np.ones(5))


def test_pairwise_is_built_into_the_library_and_stays_out_of_the_stamp():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = next(l for l in mk.splitlines() if l.startswith("OBJS")).split()
    hdrs = next(l for l in mk.splitlines() if l.startswith("HDRS")).split()
    assert "pairwise.o" in objs and "pairwise_rule.h" in hdrs
    hash_lines = "".join(l for l in mk.splitlines() if "HASH" in l)
    assert "pairwise" not in hash_lines
    assert [l for l in mk.splitlines() if l.startswith("\t") and "pairwise" in l] == []                  # the generic rule builds it
    src = open(os.path.join(CSRC, "pairwise.hip")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    for piece in ("pairwise_rule.h", "pw_step(", "pw_dist_rows(", "pw_key_less(", "pw_gain(", "pw_ratio(", "pw_disc_host(", "dge_knn_device("):
        assert piece in code, piece
    assert "fma(" not in code and "mfma" not in code.lower() and "log2" not in code and "printf" not in code and "assert(" not in code
    for m in re.finditer(r"atomicAdd\(([^,]+),", code):          # integer atomics only
        assert m.group(1).strip() == "&hist[lo]", m.group(0)
    rule = open(os.path.join(CSRC, "pairwise_rule.h")).read()
    assert "fma" not in "\n".join(l.split("//")[0] for l in rule.splitlines())
