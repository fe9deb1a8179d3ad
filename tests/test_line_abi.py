"""CPU: the LINE entries (dge_line_coo, dge_line_flows) are part of the C ABI — declared, exported, bound — were added without moving the version or the trainer's
build stamp, and refuse null arguments and every limit violation with DGE_ERR_ARG before they look for a device (the calls name device 99), leaving the outputs
untouched."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CSRC = os.path.join(ROOT, "embedding_amd", "csrc")
ENTRIES = ("dge_line_coo", "dge_line_flows")


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
    assert callable(dge.Flows.line) and callable(dge.Vectors.from_line) and callable(ev.line_gpu) and callable(ev.line_features) and callable(ev.line_config)


def test_struct_layouts(dge):
    from embedding_amd._native import LineCfg, LineInfo
    h = open(os.path.join(ROOT, "include", "dge.h")).read()
    for cls, name, size, fields, offsets in (
            (LineCfg, "dge_line_cfg", 40, ["dim", "order", "negative", "batch", "samples", "rho0", "seed"], [0, 4, 8, 12, 16, 24, 32]),
            (LineInfo, "dge_line_info", 72, ["vertices", "entries", "zeros", "batches", "samples", "total_weight", "neg_total", "max_abs", "kernel_ms"], [0, 8, 16, 24, 32, 40, 48, 56, 64])):
        assert C.sizeof(cls) == size
        assert [f[0] for f in cls._fields_] == fields and [getattr(cls, f).offset for f in fields] == offsets
        body = re.search(r"typedef struct %s \{(.*?)\} %s;\s*/\* %d bytes \*/" % (name, name, size), h, flags=re.S).group(1)
        assert re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == fields


def test_bad_arguments_are_argument_errors_before_a_device_is_looked_for(dge):
    from embedding_amd._native import LineCfg, LineInfo
    lib = dge.lib
    src = np.array([0, 1, 2], np.int32); dst = np.array([1, 0, 2], np.int32); w = np.array([1.0, 2.0, 3.0])
    X = np.full((3, 256), 9.0); Y = np.full((3, 256), 7.0); touched = np.full(3, 5, np.uint8); info = LineInfo(); info.vertices = -5
    good = np.full((3, 2), 0.25)

    def call(dim=2, order=2, K=5, batch=64, samples=100, rho0=0.025, s=src, d=dst, v=w, ne=3, n=3, cfg=True, ix=None, iy=None, x=X, y=Y, t=touched):
        cf = LineCfg(dim, order, K, batch, samples, rho0, 1)
        rc = lib.dge_line_coo(99, _p(s), _p(d), _p(v), ne, n, C.byref(cf) if cfg else None, _p(ix), _p(iy), _p(x), _p(y), _p(t), C.byref(info))
        return rc, (lib.dge_last_error() or b"").decode()

    big = good.copy(); big[1, 1] = 256.0
    low = good.copy(); low[2, 1] = -256.0
    nan = good.copy(); nan[0, 1] = np.nan
    inf = good.copy(); inf[2, 0] = -np.inf
    for what, kw, words in (("dim 0", dict(dim=0), ("dim = 0", "1 .. 256")), ("dim 257", dict(dim=257), ("dim = 257", "1 .. 256")), ("dim negative", dict(dim=-1), ("dim = -1",)),
                            ("order 0", dict(order=0), ("order = 0",)), ("order 3", dict(order=3), ("order = 3",)),
                            ("K negative", dict(K=-1), ("negative = -1", "0 .. 32")), ("K 33", dict(K=33), ("negative = 33",)),
                            ("batch 0", dict(batch=0), ("batch = 0", "1 .. 65536")), ("batch 65537", dict(batch=65537), ("batch = 65537",)),
                            ("samples 0", dict(samples=0), ("samples = 0",)), ("samples 2^40 + 1", dict(samples=(1 << 40) + 1), ("samples = 1099511627777",)),
                            ("rho0 0", dict(rho0=0.0), ("rho0 = 0",)), ("rho0 above 1", dict(rho0=1.5), ("rho0 = 1.5",)), ("rho0 negative", dict(rho0=-0.1), ("rho0 = -0.1",)),
                            ("rho0 NaN", dict(rho0=float("nan")), ("rho0",)),
                            ("n 0", dict(n=0), ("n = 0",)), ("n 2^22 + 1", dict(n=(1 << 22) + 1), ("n = 4194305",)), ("n negative", dict(n=-4), ("n = -4",)),
                            ("no entries", dict(ne=0), ("n_entries = 0",)), ("negative entries", dict(ne=-1), ("n_entries = -1",)), ("2^31 entries", dict(ne=1 << 31), ("n_entries = 2147483648",)),
                            ("no src", dict(s=None), ("null",)), ("no dst", dict(d=None), ("null",)), ("no w", dict(v=None), ("null",)), ("no cfg", dict(cfg=False), ("null",)),
                            ("no X", dict(x=None), ("null",)), ("init_Y alone", dict(iy=good), ("null", "init_Y", "init_X")),
                            ("init_X at 256", dict(ix=big), ("init_X[3]",)), ("init_X at -256", dict(ix=low), ("init_X[5]",)), ("NaN init_X", dict(ix=nan), ("init_X[1]",)),
                            ("infinite init_Y", dict(ix=good, iy=inf), ("init_Y[4]",)), ("init_Y at 256", dict(ix=good, iy=big), ("init_Y[3]",))):
        rc, msg = call(**kw)
        assert rc == 1 and "dge_line_coo" in msg, (what, rc, msg)
        for word in words:
            assert word in msg, (what, msg)
    cf = LineCfg(2, 2, 5, 64, 100, 0.025, 1)
    index = np.full(4, -3, np.int64)
    rc = lib.dge_line_flows(None, 8, 0, 0, None, C.byref(cf), _p(X), _p(Y), _p(touched), _p(index), C.byref(info))        # a handle cannot exist without a device: its NULL is refused
    assert rc == 1 and "dge_line_flows" in lib.dge_last_error().decode() and "null" in lib.dge_last_error().decode()
    assert (X == 9.0).all() and (Y == 7.0).all() and (touched == 5).all() and info.vertices == -5 and (index == -3).all()
    for kw in (dict(), dict(y=None, t=None), dict(ix=good), dict(ix=good, iy=good), dict(dim=256, K=32, batch=65536, samples=1 << 40, rho0=1.0), dict(dim=1, K=0, batch=1, samples=1)):
        rc, msg = call(**kw)                                     # nothing wrong but the device: only now is it looked for
        assert rc != 0 and rc != 1, (kw, rc, msg)
    assert (X == 9.0).all() and (Y == 7.0).all() and (touched == 5).all() and info.vertices == -5


def test_the_python_entries_check_their_arguments(dge):
    import embedding_amd.evaluate as ev
    with pytest.raises(ValueError):
        ev.line_features(np.ones((4, 2)), np.ones(5))
    with pytest.raises(ValueError):
        ev.line_features(np.ones(4), np.ones(4))
    f = ev.line_features(np.arange(8.0).reshape(4, 2) + 1, np.array([1, 0, 1, 1]))
    assert f.dtype == np.float32 and f.tolist() == [[1.0, 2.0], [0.0, 0.0], [5.0, 6.0], [7.0, 8.0]]
    assert ev.line_features(np.ones((2, 3)), np.array([True, False]), dtype=np.float64).dtype == np.float64
    with pytest.raises(ValueError):
        ev.line_gpu([0], [0, 1], [1.0], 2)
    with pytest.raises(ValueError):
        ev.line_gpu([0], [0], [1.0], 2, dim=3, init=np.ones((2, 2)))
    with pytest.raises(ValueError):
        ev.line_gpu([0], [0], [1.0], 2, dim=3, init=(np.ones((2, 3)), np.ones((3, 3))))
    cfg = ev.line_config(seed=-1)
    assert (cfg.dim, cfg.order, cfg.negative, cfg.rho0, cfg.seed) == (20, 2, 5, 0.025, (1 << 64) - 1)


def test_line_is_built_into_the_library_and_stays_out_of_the_stamp():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = next(l for l in mk.splitlines() if l.startswith("OBJS")).split()
    hdrs = next(l for l in mk.splitlines() if l.startswith("HDRS")).split()
    assert "line.o" in objs and "line_rule.h" in hdrs
    for f in ("line.hip", "line_rule.h"):
        assert os.path.exists(os.path.join(CSRC, f))
    hash_lines = "".join(l for l in mk.splitlines() if "HASH" in l)
    assert "line" not in hash_lines
    assert [l for l in mk.splitlines() if l.startswith("\t") and "line" in l] == []                    # the generic rule builds it
