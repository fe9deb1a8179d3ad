"""CPU: the ridge entries (dge_ridge_loo_vectors, dge_ridge_loo, dge_ridge_predict_vectors) are part of the C ABI — declared, exported, bound — were added
without moving the version or the trainer's build stamp, and refuse bad arguments before they look for a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "embedding_amd", "csrc")
ENTRIES = ("dge_ridge_loo_vectors", "dge_ridge_loo", "dge_ridge_predict_vectors")


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_the_entries_are_declared_exported_and_bound(dge):
    h = open(os.path.join(ROOT, "include", "dge.h")).read()
    knob = int(re.search(r"DGE_TUNE_RIDGE_CHUNK\s*=\s*(\d+)", h).group(1))
    assert knob == 21 and int(re.search(r"DGE_TUNE_COUNT\s*=\s*(\d+)", h).group(1)) == 22
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
    assert callable(dge.Vectors.ridge_loo) and callable(dge.Vectors.ridge_predict) and callable(ev.ridge_loo_gpu)
    assert dge.engine.TUNING_KNOBS["ridge_chunk"] == knob
    got = C.c_int64(0)
    assert dge.lib.dge_get_tuning(knob, C.byref(got)) == 0 and got.value == -1      # the library's own rule until someone sets it
    assert dge.lib.dge_get_tuning(knob + 1, C.byref(got)) == 1


def test_struct_layout(dge):
    from embedding_amd._native import RidgeInfo
    h = open(os.path.join(ROOT, "include", "dge.h")).read()
    fields = ["rows", "blocks", "chunks", "min_pivot", "max_leverage", "kernel_ms"]
    assert C.sizeof(RidgeInfo) == 48
    assert [f[0] for f in RidgeInfo._fields_] == fields and [getattr(RidgeInfo, f).offset for f in fields] == [0, 8, 16, 24, 32, 40]
    body = re.search(r"typedef struct dge_ridge_info \{(.*?)\} dge_ridge_info;\s*/\* 48 bytes \*/", h, flags=re.S).group(1)
    assert re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == fields


def test_bad_arguments_are_argument_errors_without_a_device(dge):
    """dge_ridge_loo checks everything a host can check — nulls, negative sizes, dim, the numbers of targets and penalties, every penalty, fewer than two used
    rows, a target that is not finite in a used row — before it looks for a device; the *_vectors entries need a handle, which cannot exist without a device:
    their NULL is refused, as are their bad limits.  Never DGE_ERR_DEVICE; the outputs stay untouched."""
    from embedding_amd._native import RidgeInfo
    lib = dge.lib
    X = np.ones((10, 3), np.float32)
    y = np.arange(20, dtype=np.float64).reshape(10, 2)
    lam = np.array([0.5, 1.0])
    mae = np.full((2, 2), -7.0); mre = np.full((2, 2), -7.0); beta = np.full((2, 2, 4), -7.0); pred = np.full((2, 2, 10), -7.0)
    info = RidgeInfo(); info.rows = -5

    def loo(rows=X, n=10, dim=3, yy=y, T=2, select=None, la=lam, nl=2, ma=mae, mr=mre):
        rc = lib.dge_ridge_loo(0, _p(rows), n, dim, _p(yy), T, _p(select), _p(la), nl, _p(ma), _p(mr), _p(beta), _p(pred), C.byref(info))
        return rc, (lib.dge_last_error() or b"").decode()

    y_nan = y.copy(); y_nan[4, 1] = np.nan
    y_inf = y.copy(); y_inf[6, 0] = -np.inf
    one = np.zeros(10, np.uint8); one[2] = 1
    for what, kw, words in (("dim 0", dict(dim=0), ("dim = 0", "1 .. 256")), ("dim 257", dict(dim=257), ("dim = 257",)), ("negative dim", dict(dim=-3), ("negative",)),
                            ("negative rows", dict(n=-1), ("negative",)), ("no rows", dict(rows=None), ("null",)), ("no y", dict(yy=None), ("null",)),
                            ("no lambda", dict(la=None), ("null",)), ("no mae", dict(ma=None), ("null",)), ("no mre", dict(mr=None), ("null",)),
                            ("T 0", dict(T=0), ("n_targets = 0", "1 .. 64")), ("T 65", dict(T=65), ("n_targets = 65",)),
                            ("L 0", dict(nl=0), ("n_lambda = 0", "1 .. 64")), ("L 65", dict(nl=65), ("n_lambda = 65",)),
                            ("negative lambda", dict(la=np.array([0.5, -1.0])), ("lambda[1]", "not a finite number >= 0")),
                            ("nan lambda", dict(la=np.array([np.nan, 1.0])), ("lambda[0]",)), ("inf lambda", dict(la=np.array([0.0, np.inf])), ("lambda[1]",)),
                            ("one used row", dict(select=one), ("1 used rows", "at least 2")), ("zero rows", dict(n=0), ("0 used rows",)),
                            ("nan target", dict(yy=y_nan), ("row 4", "not finite")), ("inf target", dict(yy=y_inf), ("row 6", "not finite"))):
        rc, msg = loo(**kw)
        assert rc == 1 and "dge_ridge_loo" in msg, (what, rc, msg)
        for w in words:
            assert w in msg, (what, msg)

    def err():
        return lib.dge_last_error().decode()

    assert lib.dge_ridge_loo_vectors(None, _p(y), 2, None, _p(lam), 2, _p(mae), _p(mre), None, None, None) == 1 and "dge_ridge_loo_vectors" in err() and "null" in err()
    assert lib.dge_ridge_predict_vectors(None, _p(beta), 4, _p(pred)) == 1 and "dge_ridge_predict_vectors" in err() and "null" in err()
    fake = C.c_void_p(1)                                          # never read: the nulls are looked at first
    assert lib.dge_ridge_loo_vectors(fake, None, 2, None, _p(lam), 2, _p(mae), _p(mre), None, None, None) == 1 and "null" in err()
    assert lib.dge_ridge_predict_vectors(fake, None, 4, _p(pred)) == 1 and "null" in err()
    assert lib.dge_ridge_predict_vectors(fake, _p(beta), 0, _p(pred)) == 1 and "n_models = 0" in err()
    assert lib.dge_ridge_predict_vectors(fake, _p(beta), 4097, _p(pred)) == 1 and "n_models = 4097" in err()
    assert (mae == -7).all() and (mre == -7).all() and (beta == -7).all() and (pred == -7).all() and info.rows == -5
    # a target that is not finite on a row that is not used is nothing to refuse: the call goes on to look for a device
    sel = np.ones(10, np.uint8); sel[4] = 0
    rc, msg = loo(yy=y_nan, select=sel)
    assert rc in (0, 6), (rc, msg)


def test_the_python_view_checks_shapes_before_the_library(dge):
    import embedding_amd.evaluate as ev
    X = np.ones((4, 2), np.float32)
    with pytest.raises(ValueError):
        ev.ridge_loo_gpu(X, [0.0, 1.0, 2.0], [1.0])
    with pytest.raises(ValueError):
        ev.ridge_loo_gpu(X, np.zeros((4, 2, 1)), [1.0])
    with pytest.raises(ValueError):
        ev.ridge_loo_gpu(X, [0.0, 1.0, 2.0, 3.0], [1.0], select=[1, 1, 1])
    with pytest.raises(ValueError):
        ev.ridge_loo_gpu(np.ones(4, np.float32), [0.0, 1.0, 2.0, 3.0], [1.0])
    with pytest.raises(dge.DgeError) as ei:
        ev.ridge_loo_gpu(X, [0.0, 1.0, 2.0, 3.0], [-1.0])
    assert ei.value.code == 1 and "lambda[0]" in str(ei.value)


def test_ridge_is_built_into_the_library_and_stays_out_of_the_stamp():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = next(l for l in mk.splitlines() if l.startswith("OBJS")).split()
    hdrs = next(l for l in mk.splitlines() if l.startswith("HDRS")).split()
    assert "ridge.o" in objs and "ridge_rule.h" in hdrs
    for f in ("ridge.hip", "ridge_rule.h"):
        assert os.path.exists(os.path.join(CSRC, f))
    hash_lines = "".join(l for l in mk.splitlines() if "HASH" in l)
    assert "ridge" not in hash_lines
    assert [l for l in mk.splitlines() if l.startswith("\t") and "ridge" in l] == []                     # the generic rule builds it
    src = open(os.path.join(CSRC, "ridge.hip")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert "ridge_rule.h" in src and "rg_sub_step(" in code and "rg_moment_step(" in code and "rg_lev_step(" in code and "rg_pred_step(" in code
    assert "fma(" not in code and "mfma" not in code.lower() and "atomicAdd" not in code      # every fused step is ridge_rule.h's; no MFMA, no floating-point atomic
