"""Test infrastructure: tests/native/line_rule_harness.cpp built for the host and bound through ctypes.  Shared by tests/test_line_host.py,
tests/test_gpu_line.py and scripts/line_rate.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import line_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "line_rule_harness.cpp")
FLAGS = ["-std=c++17", "-Wall", "-ffp-contract=off"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def load_harness(so):
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC"] + FLAGS + ["-o", so, SRC])
    H = C.CDLL(so)
    u64, i64, dbl = C.c_uint64, C.c_int64, C.c_double
    for name, args, res in (("seed2", [u64], u64), ("u", [u64, u64], dbl), ("quant", [dbl], i64), ("value", [i64], dbl), ("init_cell", [u64, u64, C.c_int], i64),
                            ("search", [C.c_void_p, i64, u64, i64], i64), ("neg_weight", [i64], i64), ("draw", [u64, u64, u64], u64), ("rho", [dbl, i64, i64], dbl),
                            ("sig_entry", [C.c_int], dbl), ("sig", [dbl], dbl), ("dot", [C.c_void_p, C.c_void_p, C.c_int], dbl), ("term", [dbl, dbl], i64)):
        f = getattr(H, "harness_line_" + name)
        f.argtypes = args; f.restype = res
    H.harness_line.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, i64, i64, C.c_int, C.c_int, C.c_int, i64, i64, dbl, u64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.POINTER(i64)]
    H.harness_line.restype = C.c_int
    return H


def harness_line(H, src, dst, w, n, dim=20, order=2, negative=5, samples=1000, batch=64, rho0=0.025, seed=1, init=None):
    """the host loop of the harness -> dict of X, Y, touched and the counters; ref.BoundLeft when the rule's bound is left"""
    G = ref.Graph(src, dst, w, n)
    es = np.ascontiguousarray(G.es, np.int32); ed = np.ascontiguousarray(G.ed, np.int32); ew = np.ascontiguousarray(G.ew, np.int64)
    ix, iy = (None, None) if init is None else (init if isinstance(init, (tuple, list)) else (init, None))
    ix = None if ix is None else np.ascontiguousarray(ix, np.float64)
    iy = None if iy is None else np.ascontiguousarray(iy, np.float64)
    X = np.empty((n, dim)); Y = np.empty((n, dim)); touched = np.empty(n, np.uint8); totals = np.zeros(4, np.int64); over = C.c_int64(-1)
    rc = H.harness_line(_p(es), _p(ed), _p(ew), G.ne, n, dim, order, negative, batch, samples, rho0, seed & ref.MASK, _p(ix), _p(iy), _p(X), _p(Y), _p(touched), _p(totals),
                        C.byref(over))
    if rc == 2:
        raise ref.BoundLeft(over.value)
    assert rc == 0, rc
    return dict(X=X, Y=Y, touched=touched.astype(bool), vertices=n, entries=G.ne, zeros=G.zeros, batches=int(totals[3]), samples=samples, total_weight=int(totals[0]),
                neg_total=int(totals[1]), max_abs=float(totals[2]) * ref.UNFIX)
