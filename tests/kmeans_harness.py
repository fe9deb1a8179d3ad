"""Test infrastructure: tests/native/kmeans_rule_harness.cpp built for the host and bound through ctypes, and the comparison of two clustering results
bit for bit.  Shared by tests/test_kmeans_host.py and tests/test_gpu_kmeans.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "kmeans_rule_harness.cpp")


class Result(C.Structure):
    _fields_ = [("rows", C.c_int64), ("total_iterations", C.c_int64), ("best_restart", C.c_int32), ("iterations", C.c_int32), ("scale_bits", C.c_int32),
                ("empty", C.c_int32), ("inertia", C.c_double)]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def load_harness(so):
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-Wall", "-ffp-contract=off", "-o", so, SRC])
    H = C.CDLL(so)
    H.harness_dist.argtypes = [C.c_void_p, C.c_void_p, C.c_int]; H.harness_dist.restype = C.c_double
    H.harness_dist_all.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    H.harness_fma_sq_add.argtypes = [C.c_double, C.c_double]; H.harness_fma_sq_add.restype = C.c_double
    H.harness_scale_bits.argtypes = [C.c_float, C.c_int64]
    H.harness_quantise.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    H.harness_centre_from_sum.argtypes = [C.c_int64, C.c_int64, C.c_int]; H.harness_centre_from_sum.restype = C.c_float
    H.harness_first_pick.argtypes = [C.c_uint64, C.c_int64, C.c_int, C.c_int64]; H.harness_first_pick.restype = C.c_int64
    H.harness_draw.argtypes = [C.c_uint64, C.c_int64, C.c_int, C.c_int]; H.harness_draw.restype = C.c_double
    H.harness_blocked_sum.argtypes = [C.c_void_p, C.c_int64]; H.harness_blocked_sum.restype = C.c_double
    H.harness_walk.argtypes = [C.c_void_p, C.c_int64, C.c_double]; H.harness_walk.restype = C.c_int64
    H.harness_pick.argtypes = [C.c_void_p, C.c_int64, C.c_double]; H.harness_pick.restype = C.c_int64
    H.harness_kmeans.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Result)]
    H.harness_accuracy.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
    return H


def harness_kmeans(H, X, k, seed=1, n_init=10, max_iter=300, init=None):
    """the host loop of the harness on float32 rows -> the dict kmeans_ref.kmeans gives"""
    X = np.ascontiguousarray(X, np.float32)
    n, dim = X.shape
    labels = np.empty(n, np.int32); centres = np.empty((k, dim), np.float32); res = Result()
    init = None if init is None else np.ascontiguousarray(init, np.float32)
    assert H.harness_kmeans(_p(X), n, dim, k, seed, n_init, max_iter, _p(init), _p(labels), _p(centres), C.byref(res)) == 0
    return dict(labels=labels, centres=centres, **{f[0]: getattr(res, f[0]) for f in Result._fields_})


FIELDS = ("inertia", "iterations", "best_restart", "total_iterations", "scale_bits", "empty", "rows")


def same_result(got, want):
    assert np.array_equal(got["labels"], want["labels"])
    assert np.array_equal(np.asarray(got["centres"], np.float32).view(np.uint32), np.asarray(want["centres"], np.float32).view(np.uint32))
    assert np.float64(got["inertia"]).view(np.uint64) == np.float64(want["inertia"]).view(np.uint64), (got["inertia"], want["inertia"])
    for f in FIELDS[1:]:
        assert got[f] == want[f], (f, got[f], want[f])
