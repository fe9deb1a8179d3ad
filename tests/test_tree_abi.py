"""CPU: the decision-tree entries (dge_tree_fit_vectors, dge_tree_predict_vectors, dge_tree_cv_vectors, dge_tree_fit, dge_tree_cv) are part of the C ABI —
declared, exported, bound — were added without moving the version or the trainer's build stamp, and refuse bad arguments before they look for a device."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "embedding_amd", "csrc")
ENTRIES = ("dge_tree_fit_vectors", "dge_tree_predict_vectors", "dge_tree_cv_vectors", "dge_tree_fit", "dge_tree_cv")


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
    assert callable(dge.Vectors.tree_fit) and callable(dge.Vectors.tree_predict) and callable(dge.Vectors.tree_cv)
    assert callable(ev.tree_cv_gpu) and callable(ev.tree_fit_gpu) and callable(ev.stratified_folds) and callable(ev.median_labels)
    assert dge.engine.TUNING_KNOBS["tree_batch"] == int(re.search(r"DGE_TUNE_TREE_BATCH\s*=\s*(\d+)", h).group(1))


def test_struct_layouts(dge):
    from embedding_amd._native import TreeCfg, TreeInfo
    h = open(os.path.join(ROOT, "include", "dge.h")).read()
    for cls, name, size, fields, offsets in (
            (TreeCfg, "dge_tree_cfg", 16, ["max_depth", "min_samples_split", "min_samples_leaf", "reserved"], [0, 4, 8, 12]),
            (TreeInfo, "dge_tree_info", 40, ["rows", "n_nodes", "depth", "levels", "trees", "batches", "kernel_ms"], [0, 8, 16, 20, 24, 28, 32])):
        assert C.sizeof(cls) == size
        assert [f[0] for f in cls._fields_] == fields and [getattr(cls, f).offset for f in fields] == offsets
        body = re.search(r"typedef struct %s \{(.*?)\} %s;\s*/\* %d bytes \*/" % (name, name, size), h, flags=re.S).group(1)
        assert re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == fields


def test_bad_arguments_are_argument_errors_without_a_device(dge):
    """dge_tree_fit and dge_tree_cv check everything a host can check — nulls, negative sizes, the limits, dim, n_folds, labels, fold numbers, a fold without
    training rows, no rows at all — before they look for a device; the *_vectors entries need a handle, which cannot exist without a device: their NULL is
    refused, as are their bad limits.  Never DGE_ERR_DEVICE; the outputs stay untouched."""
    from embedding_amd._native import TreeCfg, TreeInfo
    lib = dge.lib
    X = np.ones((10, 3), np.float32)
    y = (np.arange(10) % 2).astype(np.uint8)
    fold = (np.arange(10) % 5).astype(np.int32)
    cap = 19
    feature = np.full(cap, -7, np.int32); threshold = np.full(cap, 9.0); left = np.full(cap, -7, np.int32); count = np.full(cap, -7, np.int64); pos = np.full(cap, -7, np.int64)
    correct = np.full(64, -7, np.int64); tested = np.full(64, -7, np.int64); nodes = np.full(64, -7, np.int32); depth = np.full(64, -7, np.int32)
    info = TreeInfo(); info.rows = -5

    def fit(rows=X, n=10, dim=3, yy=y, select=None, cfg=(0, 2, 1), cap=cap, feat=feature, thr=threshold):
        c = TreeCfg(cfg[0], cfg[1], cfg[2], 0) if cfg else None
        rc = lib.dge_tree_fit(0, _p(rows), n, dim, _p(yy), _p(select), C.byref(c) if c else None, cap, _p(feat), _p(thr), _p(left), _p(count), _p(pos), C.byref(info))
        return rc, (lib.dge_last_error() or b"").decode()

    def cv(rows=X, n=10, dim=3, yy=y, fo=fold, F=5, cfg=(0, 2, 1), cor=correct, tes=tested):
        c = TreeCfg(cfg[0], cfg[1], cfg[2], 0)
        rc = lib.dge_tree_cv(0, _p(rows), n, dim, _p(yy), _p(fo), F, C.byref(c), _p(cor), _p(tes), _p(nodes), _p(depth), C.byref(info))
        return rc, (lib.dge_last_error() or b"").decode()

    y2 = y.copy(); y2[4] = 2
    none = np.zeros(10, np.uint8)
    for what, kw, words in (("max_depth", dict(cfg=(-1, 2, 1)), ("max_depth = -1",)), ("split 1", dict(cfg=(0, 1, 1)), ("min_samples_split = 1", "at least 2")),
                            ("leaf 0", dict(cfg=(0, 2, 0)), ("min_samples_leaf = 0", "at least 1")), ("dim 0", dict(dim=0), ("dim = 0", "1 .. 4096")),
                            ("dim 4097", dict(dim=4097), ("dim = 4097",)), ("no rows", dict(rows=None), ("null",)), ("no y", dict(yy=None), ("null",)),
                            ("no feature", dict(feat=None), ("null",)), ("no threshold", dict(thr=None), ("null",)), ("negative rows", dict(n=-1), ("negative",)),
                            ("negative dim", dict(dim=-3), ("negative",)), ("negative cap", dict(cap=-1), ("negative",)), ("label 2", dict(yy=y2), ("row 4", "label 2")),
                            ("nothing selected", dict(select=none), ("no row",)), ("zero rows", dict(n=0), ("no row",))):
        rc, msg = fit(**kw)
        assert rc == 1 and "dge_tree_fit" in msg, (what, rc, msg)
        for w in words:
            assert w in msg, (what, msg)

    f_bad = fold.copy(); f_bad[3] = 5
    f_low = fold.copy(); f_low[3] = -2
    f_one = np.zeros(10, np.int32)
    for what, kw, words in (("F 0", dict(F=0), ("n_folds = 0", "1 .. 64")), ("F 65", dict(F=65), ("n_folds = 65",)), ("fold 5", dict(fo=f_bad), ("row 3", "fold 5")),
                            ("fold -2", dict(fo=f_low), ("row 3", "fold -2")), ("no training rows", dict(fo=f_one, F=1), ("fold 0 has no training rows",)),
                            ("an empty fold's partner", dict(fo=np.full(10, 2, np.int32), F=5), ("fold 2 has no training rows",)),
                            ("max_depth", dict(cfg=(-3, 2, 1)), ("max_depth = -3",)), ("dim 0", dict(dim=0), ("dim = 0",)), ("label 2", dict(yy=y2), ("row 4", "label 2")),
                            ("no fold", dict(fo=None), ("null",)), ("no correct", dict(cor=None), ("null",)), ("no tested", dict(tes=None), ("null",)),
                            ("negative rows", dict(n=-2), ("negative",))):
        rc, msg = cv(**kw)
        assert rc == 1 and "dge_tree_cv" in msg, (what, rc, msg)
        for w in words:
            assert w in msg, (what, msg)

    cfg = TreeCfg(0, 2, 1, 0)
    bad = TreeCfg(0, 1, 1, 0)
    assert lib.dge_tree_fit_vectors(None, _p(y), None, C.byref(cfg), cap, _p(feature), _p(threshold), _p(left), _p(count), _p(pos), C.byref(info)) == 1
    assert "dge_tree_fit_vectors" in lib.dge_last_error().decode() and "null" in lib.dge_last_error().decode()
    assert lib.dge_tree_cv_vectors(None, _p(y), _p(fold), 5, C.byref(cfg), _p(correct), _p(tested), None, None, None) == 1
    assert "dge_tree_cv_vectors" in lib.dge_last_error().decode() and "null" in lib.dge_last_error().decode()
    assert lib.dge_tree_predict_vectors(None, 1, _p(feature), _p(threshold), _p(left), _p(count), _p(pos), _p(none)) == 1
    assert "dge_tree_predict_vectors" in lib.dge_last_error().decode() and "null" in lib.dge_last_error().decode()
    fake = C.c_void_p(1)                                          # never read: the limits are looked at first
    assert lib.dge_tree_fit_vectors(fake, _p(y), None, C.byref(bad), cap, _p(feature), _p(threshold), _p(left), _p(count), _p(pos), None) == 1
    assert "min_samples_split = 1" in lib.dge_last_error().decode()
    assert lib.dge_tree_cv_vectors(fake, _p(y), _p(fold), 0, C.byref(cfg), _p(correct), _p(tested), None, None, None) == 1 and "n_folds = 0" in lib.dge_last_error().decode()
    assert (feature == -7).all() and (threshold == 9.0).all() and (left == -7).all() and (count == -7).all() and (pos == -7).all()
    assert (correct == -7).all() and (tested == -7).all() and (nodes == -7).all() and (depth == -7).all() and info.rows == -5
    # a bad label on a row that is not used is nothing to refuse: the call goes on to look for a device
    sel = np.ones(10, np.uint8); sel[4] = 0
    f_out = fold.copy(); f_out[4] = -1
    for rc, msg in (fit(yy=y2, select=sel), cv(yy=y2, fo=f_out)):
        assert rc in (0, 6), (rc, msg)


def test_the_python_view_checks_shapes_before_the_library(dge):
    import embedding_amd.evaluate as ev
    import pytest
    with pytest.raises(ValueError):
        ev.tree_fit_gpu(np.ones((4, 2), np.float32), [0, 1, 0])
    with pytest.raises(ValueError):
        ev.tree_cv_gpu(np.ones((4, 2), np.float32), [0, 1, 0, 1], n_folds=2, fold=[0, 1, 0])
    with pytest.raises(ValueError):
        ev.tree_cv_gpu(np.ones((4, 2), np.float32), [0, 1, 0, 1], n_folds=2, fold=[0, 1, 0, 1], select=[1, 1, 1, 1])
    with pytest.raises(dge.DgeError) as ei:
        ev.tree_cv_gpu(np.ones((4, 2), np.float32), [0, 1, 0, 1], n_folds=2, max_depth=-1)
    assert ei.value.code == 1 and "max_depth" in str(ei.value)
    s = ev.cv_scores([3, 0, 5], [4, 0, 5])
    assert s["scores"][0] == 0.75 and np.isnan(s["scores"][1]) and s["scores"][2] == 1.0 and s["mean"] == np.array([0.75, 1.0]).mean()
    assert np.isnan(ev.cv_scores([0], [0])["mean"])


def test_tree_is_built_into_the_library_and_stays_out_of_the_stamp():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = next(l for l in mk.splitlines() if l.startswith("OBJS")).split()
    hdrs = next(l for l in mk.splitlines() if l.startswith("HDRS")).split()
    assert "tree.o" in objs and "tree_rule.h" in hdrs
    for f in ("tree.hip", "tree_rule.h"):
        assert os.path.exists(os.path.join(CSRC, f))
    hash_lines = "".join(l for l in mk.splitlines() if "HASH" in l)
    assert "tree" not in hash_lines
    assert [l for l in mk.splitlines() if l.startswith("\t") and "tree" in l] == []                      # the generic rule builds it
    src = open(os.path.join(CSRC, "tree.hip")).read()
    assert "tr_better(" in src and "tree_rule.h" in src and "atomicAdd(float" not in src and "__int128" not in src      # the comparator is tree_rule.h's
