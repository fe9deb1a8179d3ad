"""CPU: the NMF entries (dge_nmf_coo, dge_nmf_flows) are part of the C ABI — declared, exported, bound — were added without moving the version or the trainer's
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
ENTRIES = ("dge_nmf_coo", "dge_nmf_flows")


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
    assert callable(dge.Flows.nmf) and callable(ev.nmf_gpu) and callable(ev.nmf_features)


def test_struct_layouts(dge):
    from embedding_amd._native import NmfCfg, NmfInfo
    h = open(os.path.join(ROOT, "include", "dge.h")).read()
    for cls, name, size, fields, offsets in (
            (NmfCfg, "dge_nmf_cfg", 24, ["rank", "max_iter", "update", "reserved", "seed"], [0, 4, 8, 12, 16]),
            (NmfInfo, "dge_nmf_info", 64, ["rows", "cols", "entries", "zeros", "iterations", "reserved", "vmax", "objective", "kernel_ms"], [0, 8, 16, 24, 32, 36, 40, 48, 56])):
        assert C.sizeof(cls) == size
        assert [f[0] for f in cls._fields_] == fields and [getattr(cls, f).offset for f in fields] == offsets
        body = re.search(r"typedef struct %s \{(.*?)\} %s;\s*/\* %d bytes \*/" % (name, name, size), h, flags=re.S).group(1)
        assert re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == fields


def test_bad_arguments_are_argument_errors_before_a_device_is_looked_for(dge):
    from embedding_amd._native import NmfCfg, NmfInfo
    lib = dge.lib
    rows = np.array([0, 1, 2], np.int32); cols = np.array([1, 0, 2], np.int32); vals = np.array([1.0, 2.0, 3.0])
    W = np.full((3, 32), 9.0); H = np.full((32, 4), 7.0); info = NmfInfo(); info.rows = -5
    good_w = np.ones((3, 2)); good_h = np.ones((2, 4))

    def call(rank=2, max_iter=3, update=0, r=rows, c=cols, v=vals, ne=3, n=3, m=4, cfg=True, iw=None, ih=None, w=W, h=H):
        cf = NmfCfg(rank, max_iter, update, 0, 1)
        rc = lib.dge_nmf_coo(99, _p(r), _p(c), _p(v), ne, n, m, C.byref(cf) if cfg else None, _p(iw), _p(ih), _p(w), _p(h), C.byref(info))
        return rc, (lib.dge_last_error() or b"").decode()

    bad_w = good_w.copy(); bad_w[1, 1] = -1.0
    nan_h = good_h.copy(); nan_h[0, 3] = np.nan
    inf_w = good_w.copy(); inf_w[2, 0] = np.inf
    for what, kw, words in (("rank 0", dict(rank=0), ("rank = 0", "1 .. 32")), ("rank 33", dict(rank=33), ("rank = 33", "1 .. 32")), ("rank negative", dict(rank=-1), ("rank = -1",)),
                            ("max_iter 0", dict(max_iter=0), ("max_iter = 0", "1 .. 10000")), ("max_iter 10001", dict(max_iter=10001), ("max_iter = 10001",)),
                            ("update 2", dict(update=2), ("update = 2",)), ("update -1", dict(update=-1), ("update = -1",)),
                            ("n 0", dict(n=0), ("n = 0",)), ("n 2^31", dict(n=1 << 31), ("n = 2147483648",)), ("m 0", dict(m=0), ("m = 0",)), ("m 2^31", dict(m=1 << 31), ("m = 2147483648",)),
                            ("m negative", dict(m=-4), ("m = -4",)), ("no entries", dict(ne=0), ("n_entries = 0",)), ("negative entries", dict(ne=-1), ("n_entries = -1",)),
                            ("2^31 entries", dict(ne=1 << 31), ("n_entries = 2147483648",)),
                            ("no rows", dict(r=None), ("null",)), ("no cols", dict(c=None), ("null",)), ("no vals", dict(v=None), ("null",)), ("no cfg", dict(cfg=False), ("null",)),
                            ("no W", dict(w=None), ("null",)), ("no H", dict(h=None), ("null",)), ("init_W alone", dict(iw=good_w), ("null", "init_W and init_H")),
                            ("init_H alone", dict(ih=good_h), ("null", "init_W and init_H")), ("negative init_W", dict(iw=bad_w, ih=good_h), ("init_W[3]",)),
                            ("NaN init_H", dict(iw=good_w, ih=nan_h), ("init_H[3]",)), ("infinite init_W", dict(iw=inf_w, ih=good_h), ("init_W[4]",))):
        rc, msg = call(**kw)
        assert rc == 1 and "dge_nmf_coo" in msg, (what, rc, msg)
        for w in words:
            assert w in msg, (what, msg)
    cf = NmfCfg(2, 3, 0, 0, 1)
    index = np.full(4, -3, np.int64)
    rc = lib.dge_nmf_flows(None, 8, 0, 0, None, C.byref(cf), _p(W), _p(H), _p(index), C.byref(info))        # a handle cannot exist without a device: its NULL is refused
    assert rc == 1 and "dge_nmf_flows" in lib.dge_last_error().decode() and "null" in lib.dge_last_error().decode()
    assert (W == 9.0).all() and (H == 7.0).all() and info.rows == -5 and (index == -3).all()
    rc, msg = call()                                         # nothing wrong but the device: only now is it looked for
    assert rc != 0 and rc != 1, (rc, msg)
    assert (W == 9.0).all() and (H == 7.0).all() and info.rows == -5


def test_the_python_entries_check_their_arguments(dge):
    import embedding_amd.evaluate as ev
    with pytest.raises(ValueError):
        ev.nmf_features(np.ones((4, 2)), np.ones((2, 5)))
    with pytest.raises(ValueError):
        ev.nmf_features(np.ones((4, 2)), np.ones((3, 4)))
    f = ev.nmf_features(np.arange(8.0).reshape(4, 2), np.arange(8.0).reshape(2, 4) + 10)
    assert f.shape == (4, 4) and f[1].tolist() == [2.0, 3.0, 11.0, 15.0]
    with pytest.raises(ValueError):
        ev.nmf_gpu([0], [0, 1], [1.0], (2, 2))
    with pytest.raises(ValueError):
        ev.nmf_gpu([0], [0], [1.0], (2, 2), update="kl")
    with pytest.raises(ValueError):
        ev.nmf_gpu([0], [0], [1.0], (2, 2), rank=2, init=(np.ones((2, 3)), np.ones((2, 2))))


def test_nmf_is_built_into_the_library_and_stays_out_of_the_stamp():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = next(l for l in mk.splitlines() if l.startswith("OBJS")).split()
    hdrs = next(l for l in mk.splitlines() if l.startswith("HDRS")).split()
    assert "nmf.o" in objs and "nmf_rule.h" in hdrs
    for f in ("nmf.hip", "nmf_rule.h"):
        assert os.path.exists(os.path.join(CSRC, f))
    hash_lines = "".join(l for l in mk.splitlines() if "HASH" in l)
    assert "nmf" not in hash_lines
    assert [l for l in mk.splitlines() if l.startswith("\t") and "nmf" in l] == []                    # the generic rule builds it
