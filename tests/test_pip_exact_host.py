"""CPU: embedding_amd/csrc/pip_exact.h — the side test and the ray-crossing step every lane of k_trip_locate (trip_map.hip) runs — built for the host
(tests/native/pip_exact_harness.cpp) and compared with exact rational arithmetic (fractions.Fraction over the doubles).  The ulp lattice is the case a plain
binary64 evaluation gets wrong: the segment (-12,-12)-(24,24) against the points (0.5 + i 2^-53, 0.5 + j 2^-53); the sign is that of j - i.  The same
program, built stand-alone with -fsanitize=address,undefined, runs clean."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pip_exact_harness.cpp")


def load_harness(tmp_dir):
    so = os.path.join(str(tmp_dir), "libpip_exact_harness.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", so, SRC])
    H = C.CDLL(so)
    H.harness_pip_side.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    H.harness_pip_side_plain.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    H.harness_pip_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    H.harness_pip_locate.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    H.harness_pip_selfcheck.argtypes = [C.c_int64, C.c_uint64, C.c_void_p]
    H.harness_pip_selfcheck.restype = C.c_int64
    return H


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def side(H, t):
    t = np.ascontiguousarray(t, np.float64).reshape(-1, 6)
    s = np.zeros(len(t), np.int8); e = np.zeros(len(t), np.uint8)
    H.harness_pip_side(p(t), len(t), p(s), p(e))
    return s, e


def step(H, seg, pts):
    seg = np.ascontiguousarray(seg, np.float64).reshape(-1, 4); pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 2)
    c = np.zeros(len(seg), np.uint8); b = np.zeros(len(seg), np.uint8); e = np.zeros(len(seg), np.uint8)
    H.harness_pip_step(p(seg), p(pts), len(seg), p(c), p(b), p(e))
    return c.tolist(), b.tolist()


def exact_sign(t):
    """the sign of the determinant over the rationals the six doubles are (float.as_integer_ratio, what Fraction(float) holds), on one common denominator."""
    r = [float(v).as_integer_ratio() for v in t]
    den = max(d for _, d in r)                                 # powers of two: the largest is a common denominator
    ax, ay, bx, by, px, py = (n * (den // d) for n, d in r)
    d = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
    return (d > 0) - (d < 0)


def test_exact_sign_is_fraction_arithmetic():
    rng = np.random.default_rng(1)
    for row in (rng.uniform(-1, 1, (2000, 6)) * 2.0 ** rng.integers(-40, 40, (2000, 6))).tolist():
        ax, ay, bx, by, px, py = (Fraction(v) for v in row)
        d = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
        assert exact_sign(row) == (d > 0) - (d < 0)


def lattice():
    i, j = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    t = np.zeros((64, 64, 6))
    t[..., 0:2] = -12.0; t[..., 2:4] = 24.0
    t[..., 4] = 0.5 + i * 2.0 ** -53; t[..., 5] = 0.5 + j * 2.0 ** -53
    return t.reshape(-1, 6), np.sign(j - i).reshape(-1)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return load_harness(tmp_path_factory.mktemp("pip_exact_harness"))


def test_the_ulp_lattice(harness):
    t, want = lattice()
    assert len(np.unique(t[:, 4])) == 64                       # every step of 2^-53 is a double of its own
    s, e = side(harness, t)
    assert np.array_equal(s, want)
    plain = np.zeros(len(t), np.int8)
    harness.harness_pip_side_plain(p(t), len(t), p(plain))
    wrong = int((plain != want).sum())
    print("a plain binary64 evaluation gets %d of 4096 wrong; %d went past the filter" % (wrong, int(e.sum())))
    assert wrong == 820                                        # the test has teeth
    crossed, boundary = step(harness, t[:, :4], t[:, 4:])
    assert [b == 1 for b in boundary] == (want == 0).tolist()  # the i == j points come out on the segment
    assert [c == 1 for c in crossed] == (want > 0).tolist()    # the upward segment is crossed by the ray of the points to its left


def test_a_million_random_triples_against_fraction(harness):
    rng = np.random.default_rng(20251018)
    n = 250_000
    base = np.array([-87.6, 41.8] * 3)
    # near Chicago, perturbed by 0 .. 3 ulps: nearly collinear, the filter cannot decide most of them
    a = np.tile(base, (n, 1)) + rng.uniform(-0.01, 0.01, (n, 1)) * np.array([1, 0.7] * 3)
    t1 = a.copy()
    t1[:, 2:4] += rng.uniform(-0.01, 0.01, (n, 1)) * np.array([1, 0.7]); t1[:, 4:6] += rng.uniform(-0.01, 0.01, (n, 1)) * np.array([1, 0.7])
    ulps = rng.integers(0, 4, (n, 6))
    t1 = (t1.view(np.int64) + ulps * rng.choice([-1, 1], (n, 6))).view(np.float64)
    # collinear triples of exactly representable integers, some moved one unit off
    a0 = rng.integers(-10 ** 6, 10 ** 6, (n, 2)); d = rng.integers(-1000, 1000, (n, 2)); m = rng.integers(-1000, 1000, (n, 1))
    t2 = np.concatenate([a0, a0 + d, a0 + m * d + (rng.integers(0, 3, (n, 2)) == 0) * rng.integers(-1, 2, (n, 2))], 1).astype(np.float64)
    # both ends of the domain: the same integers scaled by 2^-440 and 2^460 (exact), and random mantissas at 2^-450 and 2^499
    t3 = t2 * np.where(rng.integers(0, 2, (n, 1)) == 0, 2.0 ** -440, 2.0 ** 460)
    t4 = rng.uniform(1, 2, (n, 6)) * rng.choice([-1, 1], (n, 6)) * np.where(rng.integers(0, 2, (n, 1)) == 0, 2.0 ** -450, 2.0 ** 499)
    t4[:, 4:6] = t4[:, 0:2] + (t4[:, 2:4] - t4[:, 0:2]) * rng.uniform(0, 1, (n, 1))          # near the segment
    t4 = np.clip(np.abs(t4), 2.0 ** -450, 2.0 ** 500) * np.sign(t4)
    t = np.concatenate([t1, t2, t3, t4])
    assert len(t) == 1_000_000 and np.isfinite(t).all()
    s, e = side(harness, t)
    want = np.fromiter((exact_sign(row) for row in t.tolist()), np.int8, len(t))
    print("zeros %d, past the filter %d of %d" % (int((want == 0).sum()), int(e.sum()), len(t)))
    assert np.array_equal(s, want)
    assert (want == 0).sum() > 100_000 and e.sum() > 100_000 and e[:n].sum() > 0 and e[3 * n:].sum() > 0


def test_the_per_segment_step(harness):
    # (segment, point) -> (crossed, boundary)
    cases = [
        # p.y equal to a vertex's y: the apex of a peak touching the ray (both segments have no end above: none crossed) ...
        ((2, 0, 3, 1), (0, 1), (0, 0)), ((3, 1, 4, 0), (0, 1), (0, 0)),
        # ... the bottom of a valley touching the ray (each has one end above, the other on the line: both crossed, parity unchanged) ...
        ((2, 2, 3, 1), (0, 1), (1, 0)), ((3, 1, 4, 2), (0, 1), (1, 0)),
        # ... and a vertex the ray passes through (one segment crossed, the other not)
        ((2, 0, 3, 1), (0, 1), (0, 0)), ((3, 1, 4, 2), (0, 1), (1, 0)),
        # the same with the point behind the segments: nothing is crossed
        ((2, 2, 3, 1), (5, 1), (0, 0)), ((3, 1, 4, 2), (5, 1), (0, 0)),
        # horizontal segments on the ray's line, p left of, on (both ends, inside) and right of them; both directions
        ((2, 1, 4, 1), (0, 1), (0, 0)), ((2, 1, 4, 1), (2, 1), (0, 1)), ((2, 1, 4, 1), (3, 1), (0, 1)), ((2, 1, 4, 1), (4, 1), (0, 1)), ((2, 1, 4, 1), (5, 1), (0, 0)),
        ((4, 1, 2, 1), (3, 1), (0, 1)), ((4, 1, 2, 1), (1, 1), (0, 0)),
        # p equal to a vertex: either end, of a rising, a falling and a peak segment
        ((2, 0, 3, 1), (2, 0), (0, 1)), ((2, 0, 3, 1), (3, 1), (0, 1)), ((3, 1, 4, 0), (3, 1), (0, 1)), ((3, 1, 4, 0), (4, 0), (0, 1)),
        # p inside a segment, left and right of it, above and below its span
        ((0, 0, 4, 4), (2, 2), (0, 1)), ((0, 0, 4, 4), (1, 2), (1, 0)), ((0, 0, 4, 4), (3, 2), (0, 0)), ((4, 4, 0, 0), (1, 2), (1, 0)), ((4, 4, 0, 0), (3, 2), (0, 0)),
        ((0, 0, 4, 4), (1, 5), (0, 0)), ((0, 0, 4, 4), (-1, -1), (0, 0)), ((0, 0, 4, 4), (5, 5), (0, 0)),
        # a vertical segment
        ((1, 0, 1, 2), (1, 1), (0, 1)), ((1, 0, 1, 2), (0, 1), (1, 0)), ((1, 0, 1, 2), (2, 1), (0, 0)), ((1, 0, 1, 2), (0, 2), (0, 0)), ((1, 0, 1, 2), (0, 0), (1, 0)),
        # a segment of one point
        ((1, 1, 1, 1), (1, 1), (0, 1)), ((1, 1, 1, 1), (0, 1), (0, 0)),
    ]
    crossed, boundary = step(harness, [c[0] for c in cases], [c[1] for c in cases])
    assert list(zip(crossed, boundary)) == [c[2] for c in cases]


def test_the_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "pip_exact_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    run = subprocess.run([exe, "300000", "7"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert " wrong 0 " in run.stdout and " lattice_wrong 0 " in run.stdout and " plain_wrong 820 " in run.stdout
