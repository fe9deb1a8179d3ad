"""CPU: the k-means entries (dge_kmeans_vectors, dge_kmeans, dge_cluster_accuracy) are part of the C ABI — declared, exported, bound — were added without moving
the version or the trainer's build stamp, refuse bad arguments with DGE_ERR_ARG before they look for a device, and the accuracy needs no device at all."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kmeans_ref as ref  # noqa: E402

CSRC = os.path.join(ROOT, "embedding_amd", "csrc")
ENTRIES = ("dge_kmeans_vectors", "dge_kmeans", "dge_cluster_accuracy")


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


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
        args = re.search(r"\b%s\s*\((.*?)\);" % name, h, flags=re.S).group(1)
        assert len(args.split(",")) == len(SIGNATURES[name][1]), name
    assert dge.lib.dge_version() == 106            # additions only: no bump
    import embedding_amd.evaluate as ev
    assert callable(dge.Vectors.kmeans) and callable(ev.kmeans_gpu) and callable(ev.clustering_accuracy) and callable(ev.clustering_accuracy_vectors)


def test_struct_layouts(dge):
    from embedding_amd._native import KmeansCfg, KmeansInfo
    h = open(os.path.join(ROOT, "include", "dge.h")).read()
    for cls, name, size, fields, offsets in (
            (KmeansCfg, "dge_kmeans_cfg", 24, ["k", "n_init", "max_iter", "reserved", "seed"], [0, 4, 8, 12, 16]),
            (KmeansInfo, "dge_kmeans_info", 48, ["rows", "best_restart", "iterations", "total_iterations", "scale_bits", "empty", "inertia", "kernel_ms"],
             [0, 8, 12, 16, 24, 28, 32, 40])):
        assert C.sizeof(cls) == size
        assert [f[0] for f in cls._fields_] == fields and [getattr(cls, f).offset for f in fields] == offsets
        body = re.search(r"typedef struct %s \{(.*?)\} %s;\s*/\* %d bytes \*/" % (name, name, size), h, flags=re.S).group(1)
        assert re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == fields


def test_bad_arguments_are_argument_errors_without_a_device(dge):
    """dge_kmeans checks everything a host can check — nulls, the limits on k, n_init, max_iter and dim, k against the selected rows — before it looks for a
    device; dge_kmeans_vectors needs a handle, which cannot exist without a device: its NULL is refused.  Never DGE_ERR_DEVICE; the outputs stay untouched."""
    from embedding_amd._native import KmeansCfg, KmeansInfo
    lib = dge.lib
    X = np.ones((10, 3), np.float32)
    labels = np.full(10, -7, np.int32); centres = np.full((64, 3), 9.0, np.float32); info = KmeansInfo(); info.rows = -5

    def call(k=2, n_init=1, max_iter=5, rows=X, n=10, dim=3, select=None, cfg=True, lab=labels, cen=centres):
        c = KmeansCfg(k, n_init, max_iter, 0, 1)
        rc = lib.dge_kmeans(0, _p(rows), n, dim, _p(select), C.byref(c) if cfg else None, None, _p(lab), _p(cen), C.byref(info))
        return rc, (lib.dge_last_error() or b"").decode()

    few = np.zeros(10, np.uint8); few[3] = 1
    for what, kw, words in (("k 0", dict(k=0), ("k = 0", "1 .. 64")), ("k 65", dict(k=65), ("k = 65", "1 .. 64")), ("k negative", dict(k=-1), ("k = -1",)),
                            ("n_init 0", dict(n_init=0), ("n_init = 0",)), ("max_iter 0", dict(max_iter=0), ("max_iter = 0",)), ("dim 0", dict(dim=0), ("dim = 0", "1 .. 256")),
                            ("dim 257", dict(dim=257), ("dim = 257",)), ("k > n", dict(k=11), ("k = 11", "10 selected rows")), ("k > selected", dict(select=few), ("k = 2", "1 selected rows")),
                            ("no rows", dict(rows=None), ("null",)), ("no cfg", dict(cfg=False), ("null",)), ("no labels", dict(lab=None), ("null",)), ("no centres", dict(cen=None), ("null",)),
                            ("negative rows", dict(n=-1), ("negative",)), ("negative dim", dict(dim=-3), ("negative",))):
        rc, msg = call(**kw)
        assert rc == 1 and "dge_kmeans" in msg, (what, rc, msg)
        for w in words:
            assert w in msg, (what, msg)
    cfg = KmeansCfg(2, 1, 5, 0, 1)
    assert lib.dge_kmeans_vectors(None, None, C.byref(cfg), None, _p(labels), _p(centres), C.byref(info)) == 1
    assert "dge_kmeans_vectors" in lib.dge_last_error().decode() and "null" in lib.dge_last_error().decode()
    assert (labels == -7).all() and (centres == 9.0).all() and info.rows == -5


def test_cluster_accuracy_needs_no_device(dge):
    import embedding_amd.evaluate as ev
    rng = np.random.default_rng(21)
    cases = [(np.array([0, 0, 1, 1, 2, 2]), np.array([1, 1, 0, 0, 2, 2]), 3), (np.array([0, 0, 0, 1, 1, 1]), np.array([0, 1, 2, 0, 1, 2]), 3),
             (np.array([-1, -1, 1, 0]), np.array([0, 1, 1, -1]), 2), (np.zeros(0, int), np.zeros(0, int), 1)]
    for k in (1, 3, 8, 64):
        a = rng.integers(-1, k, 300); g = rng.integers(-1, k, 300)
        cases += [(a, g, k), (a, np.where(rng.random(300) < 0.8, a, g), k)]
    for a, g, k in cases:
        acc, cnt, m = ev.clustering_accuracy(a, g, k)
        want, wcnt, wmap = ref.clustering_accuracy(a, g, k)
        assert np.array_equal(cnt, wcnt) and np.array_equal(m, wmap), (a, g, k)
        assert (math.isnan(want) and math.isnan(acc)) or acc == want
    acc, cnt, m = ev.clustering_accuracy([0, 0, 1, 1, 2, 2], [1, 1, 0, 0, 2, 2], 3)
    assert acc == 1.0 and m.tolist() == [1, 0, 2] and cnt.tolist() == [[0, 2, 0], [2, 0, 0], [0, 0, 2]]
    assert math.isnan(ev.clustering_accuracy([0, 1], [-1, -1], 2)[0])                                  # a zero denominator: NaN, not an error
    lib = dge.lib
    a = np.array([0, 2], np.int32); acc = C.c_double(7.0)
    assert lib.dge_cluster_accuracy(_p(a), _p(a), 2, 2, None, None, C.byref(acc)) == 1 and "row 1" in lib.dge_last_error().decode() and acc.value == 7.0
    assert lib.dge_cluster_accuracy(_p(a), _p(a), 2, 0, None, None, C.byref(acc)) == 1 and "k = 0" in lib.dge_last_error().decode()
    assert lib.dge_cluster_accuracy(None, _p(a), 2, 3, None, None, C.byref(acc)) == 1 and "null" in lib.dge_last_error().decode()
    assert lib.dge_cluster_accuracy(_p(a), _p(a), 2, 3, None, None, C.byref(acc)) == 0 and acc.value == 1.0      # cnt and map may be NULL


def test_kmeans_is_built_into_the_library_and_stays_out_of_the_stamp():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = next(l for l in mk.splitlines() if l.startswith("OBJS")).split()
    hdrs = next(l for l in mk.splitlines() if l.startswith("HDRS")).split()
    assert "kmeans.o" in objs and "kmeans_rule.h" in hdrs and "cluster_match.h" in hdrs
    for f in ("kmeans.hip", "kmeans_rule.h", "cluster_match.h"):
        assert os.path.exists(os.path.join(CSRC, f))
    hash_lines = "".join(l for l in mk.splitlines() if "HASH" in l)
    assert "kmeans" not in hash_lines and "cluster_match" not in hash_lines
    assert [l for l in mk.splitlines() if l.startswith("\t") and "kmeans" in l] == []                    # the generic rule builds it
