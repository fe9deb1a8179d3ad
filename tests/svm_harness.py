"""Test infrastructure: tests/native/svm_rule_harness.cpp built for the host and bound through ctypes.  Shared by tests/test_svm_host.py and scripts/svm_rate.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "svm_rule_harness.cpp")


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def load_harness(so, opt="-O2"):
    subprocess.check_call(["g++", opt, "-shared", "-fPIC", "-std=c++17", "-Wall", "-ffp-contract=off", "-o", so, SRC])
    H = C.CDLL(so)
    H.harness_svm_exp.argtypes = [C.c_double]; H.harness_svm_exp.restype = C.c_double
    H.harness_svm_kernel.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_double, C.c_void_p]
    H.harness_svm_solve.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_double, C.c_int64] + [C.c_void_p] * 5
    H.harness_svm_decide.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_double, C.c_void_p]
    return H


def harness_kernel(H, X, gamma):
    X = np.ascontiguousarray(X, np.float32)
    n, dim = X.shape
    K = np.empty((n, n))
    assert H.harness_svm_kernel(_p(X), n, dim, float(gamma), _p(K)) == 0
    return K


def harness_solve(H, K, sgn, C_=1.0, eps=1e-3, max_iter=10_000_000):
    """svm_solve_host -> the dict svm_ref.solve gives"""
    K = np.ascontiguousarray(K, np.float64)
    sgn = np.ascontiguousarray(sgn, np.int8)
    n = len(sgn)
    alpha = np.empty(n); G = np.empty(n); coef = np.empty(n); bias = np.zeros(1); counts = np.zeros(3, np.int64)
    assert H.harness_svm_solve(_p(K), n, _p(sgn), float(C_), float(eps), int(max_iter), _p(alpha), _p(G), _p(coef), _p(bias), _p(counts)) == 0
    return dict(alpha=alpha, G=G, coef=coef, bias=float(bias[0]), iterations=int(counts[0]), converged=int(counts[1]), support=int(counts[2]))


def harness_decide(H, Kx, coef, bias):
    Kx = np.ascontiguousarray(Kx, np.float64)
    coef = np.ascontiguousarray(coef, np.float64)
    out = np.empty(Kx.shape[0])
    H.harness_svm_decide(_p(Kx), Kx.shape[0], Kx.shape[1], _p(coef), float(bias), _p(out))
    return out
