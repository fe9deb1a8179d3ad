"""Test infrastructure: tests/native/nmf_rule_harness.cpp built for the host and bound through ctypes.  Shared by tests/test_nmf_host.py and
tests/test_gpu_nmf.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import nmf_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "nmf_rule_harness.cpp")
FLAGS = ["-std=c++17", "-Wall", "-ffp-contract=off"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def load_harness(so):
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC"] + FLAGS + ["-o", so, SRC])
    H = C.CDLL(so)
    H.harness_nmf_u.argtypes = [C.c_uint64, C.c_uint64]; H.harness_nmf_u.restype = C.c_double
    H.harness_nmf_floor.argtypes = [C.c_double]; H.harness_nmf_floor.restype = C.c_double
    H.harness_nmf_update.argtypes = [C.c_double] * 3; H.harness_nmf_update.restype = C.c_double
    H.harness_nmf_fma.argtypes = [C.c_double] * 3; H.harness_nmf_fma.restype = C.c_double
    H.harness_nmf_segment_sum.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]; H.harness_nmf_segment_sum.restype = C.c_double
    H.harness_nmf_blocked_sum.argtypes = [C.c_void_p, C.c_int64]; H.harness_nmf_blocked_sum.restype = C.c_double
    H.harness_nmf.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.POINTER(C.c_double)]
    return H


def harness_nmf(H, rows, cols, vals, shape, rank=10, max_iter=30, update=0, seed=1, init=None):
    """the host loop of the harness -> dict of W, H, vmax, entries, zeros"""
    E = ref.Entries(rows, cols, vals, shape)
    n, m = shape
    ri = np.ascontiguousarray(E.ri, np.int32); ci = np.ascontiguousarray(E.ci, np.int32); v = np.ascontiguousarray(E.v, np.float64)
    W = np.empty((n, rank)); Hm = np.empty((rank, m)); vmax = C.c_double(0)
    iw = None if init is None else np.ascontiguousarray(init[0], np.float64)
    ih = None if init is None else np.ascontiguousarray(init[1], np.float64)
    assert H.harness_nmf(_p(ri), _p(ci), _p(v), E.ne, n, m, rank, max_iter, update, seed, _p(iw), _p(ih), _p(W), _p(Hm), C.byref(vmax)) == 0
    return dict(W=W, H=Hm, vmax=vmax.value, entries=E.ne, zeros=E.zeros, rows=n, cols=m, iterations=max_iter)
