"""CPU: the SVM entries (dge_svm_fit_vectors, dge_svm_decision_vectors, dge_svm_cv_vectors and their host-row forms) are part of the C ABI — declared,
exported, bound — were added without moving the version, the knob list or the trainer's build stamp, and refuse bad arguments before they look for a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "embedding_amd", "csrc")
ENTRIES = ("dge_svm_fit_vectors", "dge_svm_decision_vectors", "dge_svm_cv_vectors", "dge_svm_fit", "dge_svm_decision", "dge_svm_cv")


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_the_entries_are_declared_exported_and_bound(dge):
    h = open(os.path.join(ROOT, "include", "dge.h")).read()
    assert int(re.search(r"DGE_TUNE_COUNT\s*=\s*(\d+)", h).group(1)) == 22
    assert "DGE_TUNE_SVM" not in h                 # no knob of its own: what a test must force goes through dge_svm_cfg
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
    got = C.c_int64(0)
    assert dge.lib.dge_get_tuning(21, C.byref(got)) == 0 and dge.lib.dge_get_tuning(22, C.byref(got)) == 1
    assert len(dge.engine.TUNING_KNOBS) == 22
    import embedding_amd.evaluate as ev
    for name in ("svm_fit", "svm_decision", "svm_cv"):
        assert callable(getattr(dge.Vectors, name))
    assert callable(ev.svm_fit_gpu) and callable(ev.svm_cv_gpu) and callable(ev.svm_scores)


def test_struct_layout(dge):
    from embedding_amd._native import SvmCfg, SvmInfo
    h = open(os.path.join(ROOT, "include", "dge.h")).read()
    for cls, name, size, fields, offsets in (
            (SvmCfg, "dge_svm_cfg", 40, ["C", "gamma", "eps", "max_iter", "state", "launch_iters"], [0, 8, 16, 24, 32, 36]),
            (SvmInfo, "dge_svm_info", 72, ["rows", "problems", "iterations", "max_iterations", "not_converged", "support", "kernel_bytes", "launches", "kernel_ms"],
             [0, 8, 16, 24, 32, 40, 48, 56, 64])):
        assert C.sizeof(cls) == size
        assert [f[0] for f in cls._fields_] == fields and [getattr(cls, f).offset for f in fields] == offsets
        body = re.search(r"typedef struct %s \{(.*?)\} %s;\s*/\* %d bytes \*/" % (name, name, size), h, flags=re.S).group(1)
        assert re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == fields


def test_bad_arguments_are_argument_errors_without_a_device(dge):
    """dge_svm_fit, dge_svm_cv and dge_svm_decision check everything a host can check — nulls, negative sizes, dim, the numbers of labels and folds, every field
    of the configuration, labels, fold numbers, a fold without training rows, fewer than two used rows, more than 65 536, state = 1 on a set too large —
    before they look for a device; the *_vectors entries need a handle, which cannot exist without a device: their NULL is refused, as are their bad limits.
    Never DGE_ERR_DEVICE; the outputs stay untouched."""
    from embedding_amd._native import SvmCfg, SvmInfo
    lib = dge.lib
    X = np.ones((10, 3), np.float32)
    y = np.stack([np.arange(10) % 2, (np.arange(10) // 2) % 2]).astype(np.uint8)
    fold = (np.arange(10) % 5).astype(np.int32)
    coef = np.full((2, 10), -7.0); bias = np.full(2, -7.0); iters = np.full(2, -7, np.int64); conv = np.full(2, -7, np.int32)
    correct = np.full((2, 64), -7, np.int64); tested = np.full(64, -7, np.int64); its = np.full((2, 64), -7, np.int64); sup = np.full((2, 64), -7, np.int64)
    cnv = np.full((2, 64), -7, np.int32); dec = np.full((2, 10), -7.0); out = np.full((2, 10), -7.0)
    info = SvmInfo(); info.rows = -5
    good = dict(C=1.0, gamma=0.5, eps=1e-3, max_iter=100, state=0, launch_iters=0)

    def mk(**kw):
        c = dict(good); c.update(kw)
        return SvmCfg(c["C"], c["gamma"], c["eps"], c["max_iter"], c["state"], c["launch_iters"])

    def fit(rows=X, n=10, dim=3, yy=y, L=2, select=None, cfg=None, co=coef, bi=bias):
        c = cfg or mk()
        rc = lib.dge_svm_fit(0, _p(rows), n, dim, _p(yy), L, _p(select), C.byref(c), _p(co), _p(bi), _p(iters), _p(conv), C.byref(info))
        return rc, (lib.dge_last_error() or b"").decode()

    def cv(rows=X, n=10, dim=3, yy=y, L=2, fo=fold, F=5, cfg=None, cor=correct, tes=tested):
        c = cfg or mk()
        rc = lib.dge_svm_cv(0, _p(rows), n, dim, _p(yy), L, _p(fo), F, C.byref(c), _p(cor), _p(tes), _p(its), _p(sup), _p(cnv), _p(dec), C.byref(info))
        return rc, (lib.dge_last_error() or b"").decode()

    cfgs = (("C 0", mk(C=0.0), ("C = 0",)), ("C negative", mk(C=-1.0), ("C = -1",)), ("C inf", mk(C=np.inf), ("C = inf",)), ("C nan", mk(C=np.nan), ("C = ",)),
            ("gamma 0", mk(gamma=0.0), ("gamma = 0",)), ("gamma inf", mk(gamma=np.inf), ("gamma = inf",)), ("gamma nan", mk(gamma=np.nan), ("gamma",)),
            ("eps 0", mk(eps=0.0), ("eps = 0",)), ("eps nan", mk(eps=np.nan), ("eps",)), ("max_iter", mk(max_iter=-1), ("max_iter = -1",)),
            ("state 3", mk(state=3), ("state = 3", "0 .. 2")), ("state -1", mk(state=-1), ("state = -1",)), ("launch_iters", mk(launch_iters=-4), ("launch_iters = -4",)))
    y2 = y.copy(); y2[1, 4] = 2
    one = np.zeros(10, np.uint8); one[3] = 1
    big_y = np.zeros((1, 65537), np.uint8); big_X = np.zeros((65537, 1), np.float32)
    lds_y = np.zeros((1, 3585), np.uint8); lds_X = np.zeros((3585, 1), np.float32)
    for what, kw, words in tuple((w, dict(cfg=c), m) for w, c, m in cfgs) + (
            ("dim 0", dict(dim=0), ("dim = 0", "1 .. 4096")), ("dim 4097", dict(dim=4097), ("dim = 4097",)), ("no rows", dict(rows=None), ("null",)),
            ("no y", dict(yy=None), ("null",)), ("no coef", dict(co=None), ("null",)), ("no bias", dict(bi=None), ("null",)), ("negative rows", dict(n=-1), ("negative",)),
            ("negative dim", dict(dim=-3), ("negative",)), ("negative labels", dict(L=-1), ("negative",)), ("L 0", dict(L=0), ("n_labels = 0", "1 .. 64")),
            ("L 65", dict(L=65), ("n_labels = 65",)), ("label 2", dict(yy=y2), ("row 4", "label 2", "column 1")), ("one row", dict(select=one), ("1 used rows", "at least 2")),
            ("zero rows", dict(n=0), ("0 used rows",)), ("too many", dict(rows=big_X, n=65537, dim=1, yy=big_y, L=1), ("65537 used rows", "65536")),
            ("state 1 too large", dict(rows=lds_X, n=3585, dim=1, yy=lds_y, L=1, cfg=mk(state=1)), ("state = 1", "3584", "3585"))):
        rc, msg = fit(**kw)
        assert rc == (2 if what == "too many" else 1) and "dge_svm_fit" in msg, (what, rc, msg)
        for w in words:
            assert w in msg, (what, msg)

    f_bad = fold.copy(); f_bad[3] = 5
    f_low = fold.copy(); f_low[3] = -2
    for what, kw, words in tuple((w, dict(cfg=c), m) for w, c, m in cfgs) + (
            ("F 0", dict(F=0), ("n_folds = 0", "1 .. 64")), ("F 65", dict(F=65), ("n_folds = 65",)), ("negative folds", dict(F=-1), ("negative",)),
            ("fold 5", dict(fo=f_bad), ("row 3", "fold 5")), ("fold -2", dict(fo=f_low), ("row 3", "fold -2")),
            ("no training rows", dict(fo=np.zeros(10, np.int32), F=1), ("fold 0 has no training rows",)),
            ("an empty fold's partner", dict(fo=np.full(10, 2, np.int32), F=5), ("fold 2 has no training rows",)), ("dim 0", dict(dim=0), ("dim = 0",)),
            ("L 65", dict(L=65), ("n_labels = 65",)), ("label 2", dict(yy=y2), ("row 4", "label 2")), ("no fold", dict(fo=None), ("null",)),
            ("no correct", dict(cor=None), ("null",)), ("no tested", dict(tes=None), ("null",)), ("negative rows", dict(n=-2), ("negative",)),
            ("all out", dict(fo=np.full(10, -1, np.int32)), ("0 used rows",))):
        rc, msg = cv(**kw)
        assert rc == 1 and "dge_svm_cv" in msg, (what, rc, msg)
        for w in words:
            assert w in msg, (what, msg)

    def decide(sv=X, n=10, dim=3, co=coef, bi=bias, m=2, gamma=0.5, x=None, nx=0, o=out):
        rc = lib.dge_svm_decision(0, _p(sv), n, dim, _p(co), _p(bi), m, gamma, _p(x), nx, _p(o))
        return rc, (lib.dge_last_error() or b"").decode()

    for what, kw, words in (("no sv", dict(sv=None), ("null",)), ("no coef", dict(co=None), ("null",)), ("no bias", dict(bi=None), ("null",)), ("no out", dict(o=None), ("null",)),
                            ("negative rows", dict(n=-1), ("negative",)), ("negative x", dict(nx=-1), ("negative",)), ("dim 0", dict(dim=0), ("dim = 0",)),
                            ("models 0", dict(m=0), ("n_models = 0", "1 .. 4096")), ("models 4097", dict(m=4097), ("n_models = 4097",)),
                            ("gamma 0", dict(gamma=0.0), ("gamma = 0",)), ("gamma nan", dict(gamma=float("nan")), ("gamma",))):
        rc, msg = decide(**kw)
        assert rc == 1 and "dge_svm_decision" in msg, (what, rc, msg)
        for w in words:
            assert w in msg, (what, msg)

    def err():
        return lib.dge_last_error().decode()

    c = mk()
    assert lib.dge_svm_fit_vectors(None, _p(y), 2, None, C.byref(c), _p(coef), _p(bias), None, None, None) == 1 and "dge_svm_fit_vectors" in err() and "null" in err()
    assert lib.dge_svm_cv_vectors(None, _p(y), 2, _p(fold), 5, C.byref(c), _p(correct), _p(tested), None, None, None, None, None) == 1 and "dge_svm_cv_vectors" in err() and "null" in err()
    assert lib.dge_svm_decision_vectors(None, _p(coef), _p(bias), 2, 0.5, None, _p(out)) == 1 and "dge_svm_decision_vectors" in err() and "null" in err()
    fake = C.c_void_p(1)                                          # never read: the nulls and the counts are looked at first
    assert lib.dge_svm_fit_vectors(fake, None, 2, None, C.byref(c), _p(coef), _p(bias), None, None, None) == 1 and "null" in err()
    assert lib.dge_svm_fit_vectors(fake, _p(y), 0, None, C.byref(c), _p(coef), _p(bias), None, None, None) == 1 and "n_labels = 0" in err()
    assert lib.dge_svm_cv_vectors(fake, _p(y), 2, _p(fold), 0, C.byref(c), _p(correct), _p(tested), None, None, None, None, None) == 1 and "n_folds = 0" in err()
    assert lib.dge_svm_cv_vectors(fake, _p(y), 2, None, 5, C.byref(c), _p(correct), _p(tested), None, None, None, None, None) == 1 and "null" in err()
    assert lib.dge_svm_decision_vectors(fake, _p(coef), _p(bias), 0, 0.5, fake, _p(out)) == 1 and "n_models = 0" in err()
    assert lib.dge_svm_decision_vectors(fake, _p(coef), _p(bias), 2, -1.0, fake, _p(out)) == 1 and "gamma = -1" in err()
    assert lib.dge_svm_decision_vectors(fake, _p(coef), _p(bias), 2, 0.5, None, _p(out)) == 1 and "null" in err()
    assert (coef == -7).all() and (bias == -7).all() and (iters == -7).all() and (conv == -7).all() and (correct == -7).all() and (tested == -7).all()
    assert (its == -7).all() and (sup == -7).all() and (cnv == -7).all() and (dec == -7).all() and (out == -7).all() and info.rows == -5
    # a bad label on a row that is not used is nothing to refuse: the call goes on to look for a device
    sel = np.ones(10, np.uint8); sel[4] = 0
    f_out = fold.copy(); f_out[4] = -1
    for rc, msg in (fit(yy=y2, select=sel), cv(yy=y2, fo=f_out)):
        assert rc in (0, 6), (rc, msg)


def test_the_python_view_checks_shapes_before_the_library(dge):
    import embedding_amd.evaluate as ev
    X = np.ones((4, 2), np.float32)
    with pytest.raises(ValueError):
        ev.svm_fit_gpu(X, [0, 1, 0])
    with pytest.raises(ValueError):
        ev.svm_fit_gpu(np.ones(4, np.float32), [0, 1, 0, 1])
    with pytest.raises(ValueError):
        ev.svm_fit_gpu(X, [0, 1, 0, 1], select=[1, 1, 1])
    with pytest.raises(ValueError):
        ev.svm_cv_gpu(X, [0, 1, 0, 1], n_folds=2, fold=[0, 1, 0])
    with pytest.raises(ValueError):
        ev.svm_cv_gpu(X, [0, 1, 0, 1], n_folds=2, fold=[0, 1, 0, 1], select=[1, 1, 1, 1])
    with pytest.raises(dge.DgeError) as ei:
        ev.svm_cv_gpu(X, [0, 1, 0, 1], n_folds=2, C=-1.0)
    assert ei.value.code == 1 and "C = -1" in str(ei.value)
    s = ev.svm_scores([[3, 0, 5], [4, 0, 0]], [4, 0, 5])
    assert s["scores"][0, 0] == 0.75 and np.isnan(s["scores"][:, 1]).all() and s["scores"][1, 2] == 0.0
    assert s["mean"][0] == np.array([0.75, 1.0]).mean() and s["std"][1] == np.array([1.0, 0.0]).std()
    assert np.isnan(ev.svm_scores([[0]], [0])["mean"]).all()


def test_svm_is_built_into_the_library_and_stays_out_of_the_stamp():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = next(l for l in mk.splitlines() if l.startswith("OBJS")).split()
    hdrs = next(l for l in mk.splitlines() if l.startswith("HDRS")).split()
    assert "svm.o" in objs and "svm_rule.h" in hdrs
    for f in ("svm.hip", "svm_rule.h"):
        assert os.path.exists(os.path.join(CSRC, f))
    hash_lines = "".join(l for l in mk.splitlines() if "HASH" in l)
    assert "svm" not in hash_lines
    assert [l for l in mk.splitlines() if l.startswith("\t") and "svm" in l] == []                       # the generic rule builds it
    src = open(os.path.join(CSRC, "svm.hip")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    for piece in ("svm_rule.h", "sv_front_row(", "sv_pick_row(", "sv_step(", "sv_grad(", "sv_term(", "sv_kernel_of(", "km_dist_step("):
        assert piece in code, piece
    assert "fma(" not in code and "mfma" not in code.lower() and "printf" not in code and "assert(" not in code      # every fused step is a rule header's; no MFMA
    for m in re.finditer(r"atomicAdd\(([^,]+),", code):          # integer atomics only
        assert m.group(1).strip() in ("active", "&correct[p]"), m.group(0)
