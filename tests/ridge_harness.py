"""Test infrastructure: tests/native/ridge_rule_harness.cpp built for the host and bound through ctypes, and the comparison of two results bit for bit.
Shared by tests/test_ridge_host.py, tests/test_gpu_ridge.py and scripts/ridge_rate.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "ridge_rule_harness.cpp")
KINDS = {1: "pivot", 2: "leverage"}


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def load_harness(so):
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-Wall", "-ffp-contract=off", "-o", so, SRC])
    H = C.CDLL(so)
    H.harness_ridge.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 9
    H.harness_ridge_predict.argtypes = [C.c_void_p, C.c_void_p, C.c_int]; H.harness_ridge_predict.restype = C.c_double
    return H


def harness_ridge(H, X, Y, lambdas):
    """rg_solve_host on the used rows -> the dict ridge_ref.ridge_loo gives, or dict(refused=(kind, lambda index, index))"""
    X = np.ascontiguousarray(X, np.float32)
    Y = np.asarray(Y, np.float64)
    Y = np.ascontiguousarray(Y[:, None] if Y.ndim == 1 else Y)
    lam = np.ascontiguousarray(lambdas, np.float64)
    n, dim = X.shape
    T, nl, P = Y.shape[1], len(lam), dim + 1
    M = np.zeros((P, P + T)); d = np.zeros((nl, P)); L = np.zeros((nl, P, P)); beta = np.zeros((nl, T, P)); h = np.zeros((nl, n)); e = np.zeros((nl, T, n))
    mae = np.zeros((nl, T)); mre = np.zeros((nl, T)); why = np.zeros(3, np.int64)
    rc = H.harness_ridge(_p(X), _p(Y), n, dim, T, _p(lam), nl, _p(M), _p(d), _p(L), _p(beta), _p(h), _p(e), _p(mae), _p(mre), _p(why))
    assert rc >= 0, "arguments outside the limits"
    if rc:
        return dict(refused=(KINDS[int(why[0])], int(why[1]), int(why[2])))
    return dict(G=M[:, :P].copy(), c=M[:, P:].T.copy(), ysum=M[0, P:].copy(), d=d, L=L, beta=beta, h=h, e=e, loo_pred=Y.T[None, :, :] - e, mae=mae, mre=mre)


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_result(got, want, fields=("G", "c", "ysum", "d", "L", "beta", "h", "e", "loo_pred", "mae", "mre")):
    for f in fields:
        assert same_bits(got[f], want[f]), (f, np.asarray(got[f]).ravel()[:4], np.asarray(want[f]).ravel()[:4])
