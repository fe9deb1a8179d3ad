"""CPU: embedding_amd/csrc/spatial_weight.h — the centroid chain and the weight E((-d) * scale) every lane of spatial.hip runs — built for the host
(tests/native/spatial_weight_harness.cpp, -ffp-contract=off) and held to the rule of include/dge.h: bit for bit equal to tests/spatial_ref.py, E within 1 ulp
of the true exponential (decimal, 60 digits) and never rising as its argument falls, the centroid against exact rational arithmetic; the same harness, built
stand-alone with -fsanitize=address,undefined, runs clean."""
import ctypes as C
import math
import os
import subprocess
import sys
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import spatial_ref as ref  # noqa: E402

SRC = os.path.join(ROOT, "tests", "native", "spatial_weight_harness.cpp")
HDR = os.path.join(ROOT, "embedding_amd", "csrc", "spatial_weight.h")
LN2 = math.log(2.0)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("spatial_weight_harness")), "libspatial_weight_harness.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-Wall", "-ffp-contract=off", "-o", so, SRC])
    H = C.CDLL(so)
    H.harness_exp_neg.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    H.harness_weight.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p]
    H.harness_centroid.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    H.harness_monotone_run.argtypes = [C.c_double, C.c_int64, C.c_void_p]
    H.harness_monotone_run.restype = C.c_int64
    return H


def steps(x, n):
    """x moved n doubles (n < 0: towards -inf)"""
    for _ in range(abs(n)):
        x = math.nextafter(x, math.inf if n > 0 else -math.inf)
    return x


def k_boundaries():
    """the arguments at which E changes its branch or its k: 2^-28, 0.5 ln2, 1.5 ln2, then every (m + 0.5) ln2; the scaling switch at k = -1021 / -1022; the cut to 0"""
    return [-ref.TINY, -ref.HALF_LN2, -ref.THREE_HALF_LN2] + [-(m + 0.5) * LN2 for m in (2, 3, 10, 100, 500, 1020, 1021, 1022, 1073, 1074)] + [ref.UNDER]


def inputs():
    rng = np.random.default_rng(20261018)
    xs = list(-750.0 * rng.random(3000)) + list(-np.exp(rng.uniform(math.log(1e-12), math.log(750.0), 1500)))
    for b in k_boundaries():
        xs += [steps(b, s) for s in range(-4, 5)]
    xs += [0.0, -0.0, -5e-324, -2.0 ** -1022, -1e-300, -707.9, -708.0, -708.3964185322641, -708.4, -709.0, -709.78, -709.79, -744.0, -744.44, -745.0, -745.13, -745.1332191019411,
           -745.1332191019412, -745.14, -746.0, -1e9, -1.7976931348623157e308, -math.inf]
    return np.array(xs, np.float64)


def true_exp(x):
    getcontext().prec = 60
    return Decimal(x).exp() if x != -math.inf else Decimal(0)


def ulp_of(v):
    """the spacing of binary64 at the exact value v (a Decimal >= 0): 2^-1074 in the subnormal range"""
    if v < Decimal(2) ** -1022:
        return Decimal(2) ** -1074
    e = math.frexp(float(v))[1] - 1                      # float(v) is within half an ulp of v: the exponent can only be off at a power of two, towards the larger ulp
    if Decimal(2) ** e > v:
        e -= 1
    return Decimal(2) ** (e - 52)


def test_the_constants_are_those_of_the_rule():
    h = open(HDR).read()
    for name, dec in (("SW_LN2_HI", "6.93147180369123816490e-01"), ("SW_LN2_LO", "1.90821492927058770002e-10"), ("SW_INV_LN2", "1.44269504088896338700e+00"),
                      ("SW_P1", "1.66666666666666019037e-01"), ("SW_P2", "-2.77777777770155933842e-03"), ("SW_P3", "6.61375632143793436117e-05"),
                      ("SW_P4", "-1.65339022054652515390e-06"), ("SW_P5", "4.13813679705723846039e-08")):
        import re
        m = re.search(r"#define %s \(?(-?0x[0-9a-f.]+p[+-]?\d+)\)?" % name, h)
        assert m and float.fromhex(m.group(1)) == float(dec), name
    assert (ref.LN2_HI, ref.LN2_LO, ref.P5) == (6.93147180369123816490e-01, 1.90821492927058770002e-10, 4.13813679705723846039e-08)
    assert "fma" not in "\n".join(l.split("//")[0] for l in h.splitlines())


def test_the_harness_equals_the_reference_bit_for_bit(harness):
    xs = inputs()
    out = np.empty_like(xs)
    harness.harness_exp_neg(_p(xs), len(xs), _p(out))
    want = np.array([ref.E(float(x)) for x in xs], np.float64)
    assert len(xs) > 4500 and np.array_equal(out.view(np.uint64), want.view(np.uint64))
    assert ref.E(0.0) == 1.0 and ref.E(-0.0) == 1.0 and ref.E(-math.inf) == 0.0 and ref.E(-746.0) == 0.0 and ref.E(-745.13) == 5e-324 and ref.E(-5e-324) == 1.0
    assert 0.0 < ref.E(-708.4) < 2.0 ** -1022 and ref.E(-708.0) > 2.0 ** -1022                         # subnormal and smallest normal results
    # the weight of two points, distance and sqrt included
    rng = np.random.default_rng(5)
    a = rng.random((2000, 2)) * 0.5 - np.array([87.6, -41.8]); b = rng.random((2000, 2)) * 0.5 - np.array([87.6, -41.8])
    a[:5] = b[:5]                                                                                        # d = 0: w = 1
    a[5] = (1e200, 0.0); b[5] = (-1e200, 0.0)                                                            # dx*dx overflows: d = inf, w = 0
    w = np.empty(2000)
    harness.harness_weight(_p(a), _p(b), 2000, 100.0, _p(w))
    want = np.array([ref.weight(tuple(p), tuple(q), 100.0) for p, q in zip(a.tolist(), b.tolist())])
    assert np.array_equal(w.view(np.uint64), want.view(np.uint64)) and (w[:5] == 1.0).all() and w[5] == 0.0


def test_E_is_within_one_ulp_of_the_exponential():
    """What Java asks of Math.exp.  The figure printed is the largest error met, in ulps of the true value."""
    worst = Decimal(0)
    for x in inputs().tolist():
        t = true_exp(x)
        err = abs(Decimal(ref.E(x)) - t) / ulp_of(t)
        worst = max(worst, err)
        assert err <= 1, (x, float(err))
    print("largest error of E: %.4f ulp" % float(worst))


def test_E_never_rises_as_its_argument_falls(harness):
    """Runs of adjacent doubles at several magnitudes and across every change of branch and of k: a few thousand pairs through the reference, a few million
    through the harness (the same function bit for bit, by the test above)."""
    starts = [steps(b, 150) for b in k_boundaries()] + [-1e-9, -1e-3, -0.1, -1.0, -3.0, -37.5, -300.0, -700.0, -720.0, -744.9]
    pairs = 0
    for x0 in starts:
        x, e = x0, ref.E(x0)
        for _ in range(300):
            y = math.nextafter(x, -math.inf)
            f = ref.E(y)
            assert f <= e, (x, y, e, f)
            x, e = y, f
            pairs += 1
    assert pairs >= 6000
    last = C.c_double(0)
    for x0 in starts:
        assert harness.harness_monotone_run(x0, 200_000, C.byref(last)) == 0, x0
    # and coarsely over the whole range: a descending sweep
    xs = np.linspace(0.0, -750.0, 20001)
    out = np.empty_like(xs)
    harness.harness_exp_neg(_p(xs), len(xs), _p(out))
    assert (np.diff(out) <= 0).all() and out[0] == 1.0 and out[-1] == 0.0


def test_the_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "spatial_weight_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    run = subprocess.run([exe, "200000", "7"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert " wrong 0" in run.stdout and "inputs 400000 " in run.stdout


# ------------------------------------------------------------------------------------------ centroids
square, reverse_all, DYADIC, ROUNDED = ref.square, ref.reverse_all, ref.DYADIC, ref.ROUNDED          # the fixtures live beside the reference: the GPU tests use them too


def exact_centroid(rings):
    F = Fraction
    bx, by = F(rings[0][0][0]), F(rings[0][0][1])
    cx = cy = A = F(0)
    for ring in rings:
        for (px, py), (qx, qy) in zip(ring[:-1], ring[1:]):
            px, py, qx, qy = F(px), F(py), F(qx), F(qy)
            a2 = (px - bx) * (qy - by) - (qx - bx) * (py - by)
            cx += a2 * (bx + px + qx); cy += a2 * (by + py + qy); A += a2
    return cx / 3 / A, cy / 3 / A


def segments(rings):
    return np.array([[p[0], p[1], q[0], q[1]] for ring in rings for p, q in zip(ring[:-1], ring[1:])], np.float64)


def test_the_centroid_rule_against_exact_arithmetic(harness):
    """The rule's centroid against the same formula in fractions.Fraction over the binary64 inputs — a sanity check of the formula.  The error is relative,
    per coordinate: |got - exact| / |exact|.  The largest figure met on the fixtures below is 3.11e-16 (the tract with a hole), so the bound is 4 x that,
    1.25e-15.  On the dyadic fixtures every product and sum of the chain is exact, so all rings reversed give the same bits there; with rounded coordinates a
    reversed ring is summed in another order and agrees to rounding only (held to the same bound, not to the bits)."""
    worst = 0.0
    for name, rings in list(DYADIC.items()) + list(ROUNDED.items()):
        for orient, rr in (("as given", rings), ("reversed", reverse_all(rings))):
            got = ref.centroid(rr)
            seg = segments(rr)
            xy = np.zeros(2)
            assert harness.harness_centroid(_p(seg), len(seg), _p(xy)) == 1 and (xy[0], xy[1]) == got, (name, orient)
            ex, ey = exact_centroid(rr)
            assert (ex, ey) == exact_centroid(rings)                                # exactly, orientation cancels
            err = float(max(abs(Fraction(got[0]) - ex) / abs(ex), abs(Fraction(got[1]) - ey) / abs(ey)))
            worst = max(worst, err)
            assert err <= 1.25e-15, (name, orient, err)
        if name in DYADIC:
            assert ref.centroid(reverse_all(rings)) == ref.centroid(rings), name
    print("largest relative error of the centroid rule: %.3g" % worst)
    assert ref.centroid(DYADIC["unit square"]) == (0.5, 0.5) and ref.centroid(DYADIC["square away from the origin"]) == (-87.875, 41.625)
    # zero area: no centroid
    flat = [[(0.0, 0.0), (1.0, 1.0), (2.0, 2.0), (0.0, 0.0)]]
    assert ref.centroid(flat) is None and harness.harness_centroid(_p(segments(flat)), 3, _p(np.zeros(2))) == 0
