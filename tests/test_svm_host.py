"""CPU: the host build of embedding_amd/csrc/svm_rule.h (tests/native/svm_rule_harness.cpp) gives the bits of tests/svm_ref.py, the rule of include/dge.h read
out in Python — kernel matrix, coefficients, bias, iterations, decision values — at the edges of the decision's blocks, on duplicated rows and on a one-class
set; the rule is right as well as self-consistent: the two-row problem has its closed form, the returned alpha alone satisfies the optimality conditions in
extended precision, and the dual objective agrees with scikit-learn's SVC where that is importable; the same harness, built stand-alone with
-fsanitize=address,undefined, runs clean."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import spatial_ref
import svm_ref as ref
from svm_harness import SRC, harness_decide, harness_kernel, harness_solve, load_harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "embedding_amd", "csrc")
EPS = 1e-3


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return load_harness(os.path.join(str(tmp_path_factory.mktemp("svm_rule_harness")), "libsvm_rule_harness.so"))


def same_solution(got, want):
    for f in ("coef", "alpha", "G"):
        assert ref.same_bits(got[f], want[f]), (f, got[f][:4], want[f][:4])
    assert ref.same_bits([got["bias"]], [want["bias"]]), (got["bias"], want["bias"])
    assert got["iterations"] == want["iterations"] and got["converged"] == want["converged"]


def test_the_array_exponential_is_the_scalar_one(harness):
    rng = np.random.default_rng(3)
    x = -np.concatenate([rng.random(4000) * 3.0, 10.0 ** rng.uniform(-12, 2.9, 4000), [0.0, 2.0 ** -28, 2.0 ** -29, spatial_ref.HALF_LN2, spatial_ref.THREE_HALF_LN2, 744.0, 745.2, 746.0, 708.4, 709.0]])
    got = ref.E_np(x)
    want = np.array([spatial_ref.E(float(v)) for v in x])
    assert ref.same_bits(got, want)
    assert ref.same_bits(got, np.array([harness.harness_svm_exp(float(v)) for v in x]))


@pytest.mark.parametrize("C_", [0.25, 1.0, 16.0])
@pytest.mark.parametrize("dim", [1, 3, 20])
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 255, 256, 257, 700])
def test_the_host_solver_is_the_rule_bit_for_bit(harness, n, dim, C_):
    X, y = ref.table(n, dim, 1000 * n + dim)
    gamma = 1.0 / dim
    K = ref.kernel_matrix(X, X, gamma)
    assert ref.same_bits(harness_kernel(harness, X, gamma), K)
    assert np.array_equal(K, K.T) and (np.diag(K) == 1.0).all()
    assert ref.same_bits(ref.kernel_matrix_sym(X, gamma, block=100), K)
    sgn = np.where(y != 0, 1, -1)
    want = ref.solve(K, sgn, C_, EPS)
    got = harness_solve(harness, K, sgn, C_, EPS)
    same_solution(got, want)
    assert want["converged"] == 1
    assert ref.same_bits(harness_decide(harness, K, got["coef"], got["bias"]), ref.decision(K, want["coef"], want["bias"]))
    check_optimality(K, sgn, want, C_)


def check_optimality(K, sgn, r, C_):
    """(b) from alpha alone, in extended precision: 0 <= alpha <= C; the violating-pair gap of the recomputed gradient is below
    eps + 64 n 2^-53 C n (first-order error of n fma steps on terms below C, the constant generous); |sum s alpha| <= 4 iterations C 2^-53 (two roundings of
    at most half an ulp of C an update)."""
    alpha = r["alpha"]
    n = len(alpha)
    tr = sgn != 0
    assert (alpha >= 0).all() and (alpha <= C_).all() and (alpha[~tr] == 0).all()
    s = sgn.astype(np.longdouble)
    z = s * alpha.astype(np.longdouble)
    G = s * (K.astype(np.longdouble) @ z) - np.longdouble(1.0)
    v = -s * G
    up = tr & (((sgn > 0) & (alpha < C_)) | ((sgn < 0) & (alpha > 0)))
    low = tr & (((sgn > 0) & (alpha > 0)) | ((sgn < 0) & (alpha < C_)))
    if up.any() and low.any():
        gap = float(v[up].max() - v[low].min())
        bound = EPS + 64.0 * n * 2.0 ** -53 * C_ * n
        assert gap < bound, (gap, bound)
    total = sum((Fraction(int(sg)) * Fraction(float(a)) for sg, a in zip(sgn, alpha)), Fraction(0))
    assert abs(total) <= Fraction(4 * r["iterations"]) * Fraction(C_) * Fraction(2) ** -53, (float(total), r["iterations"])


@pytest.mark.parametrize("C_", [0.25, 1.0, 16.0])
def test_two_rows_have_their_closed_form(harness, C_):
    """(a) one row per class: alpha = min(C, 1 / (1 - K12)) on both, up to the one rounding of 2 - 2K: the rule's value is min(C, RN(2 / RN(2 - 2 K12)))."""
    X = np.array([[0.0, 1.0], [1.5, -0.25]], np.float32)
    K = ref.kernel_matrix(X, X, 0.5)
    sgn = np.array([1, -1])
    got = harness_solve(harness, K, sgn, C_, EPS)
    same_solution(got, ref.solve(K, sgn, C_, EPS))
    want = min(C_, 2.0 / (2.0 - 2.0 * K[0, 1]))
    assert got["alpha"][0] == want and got["alpha"][1] == want and got["iterations"] == 1
    assert abs(want - min(C_, 1.0 / (1.0 - K[0, 1]))) <= 4 * np.spacing(want)
    assert abs(got["bias"]) < 1e-12                             # the two rows mirror each other


@pytest.mark.parametrize("n,dim,dup", [(64, 3, 8), (257, 1, 40), (130, 20, 65)])
def test_duplicated_rows_of_opposite_labels(harness, n, dim, dup):
    """rows that repeat another with the opposite label: K(i, j) = 1, a = 2 - 2K = 0, the a <= 0 branch; such a pair can only end at the bound"""
    X, y = ref.table(n, dim, 77 + n, dup=dup)
    K = ref.kernel_matrix(X, X, 1.0 / dim)
    assert (K[np.arange(dup), n - dup + np.arange(dup)] == 1.0).all()
    sgn = np.where(y != 0, 1, -1)
    for C_ in (0.25, 16.0):
        want = ref.solve(K, sgn, C_, EPS)
        got = harness_solve(harness, K, sgn, C_, EPS)
        same_solution(got, want)
        assert want["converged"] == 1
        assert (want["alpha"][:dup] == C_).any()
        check_optimality(K, sgn, want, C_)
        assert ref.same_bits(harness_decide(harness, K, got["coef"], got["bias"]), ref.decision(K, want["coef"], want["bias"]))


def test_a_one_class_set_and_rows_that_do_not_train(harness):
    X, y = ref.table(65, 3, 5)
    K = ref.kernel_matrix(X, X, 1.0 / 3)
    for label, bias in ((1, 1.0), (0, -1.0)):
        sgn = np.full(65, 1 if label else -1)
        got = harness_solve(harness, K, sgn)
        same_solution(got, ref.solve(K, sgn))
        assert got["iterations"] == 0 and got["converged"] == 1 and got["bias"] == bias and (got["alpha"] == 0).all() and got["support"] == 0
        assert (harness_decide(harness, K, got["coef"], got["bias"]) == bias).all()
    sgn = np.where(y != 0, 1, -1); sgn[::5] = 0                 # a fold's test rows
    got = harness_solve(harness, K, sgn)
    want = ref.solve(K, sgn)
    same_solution(got, want)
    assert (got["alpha"][::5] == 0).all() and (got["G"][::5] == -1.0).all() and want["converged"] == 1


def test_max_iter_stops_after_that_many_updates(harness):
    X, y = ref.table(255, 3, 9)
    K = ref.kernel_matrix(X, X, 1.0 / 3)
    sgn = np.where(y != 0, 1, -1)
    got = harness_solve(harness, K, sgn, 1.0, EPS, max_iter=5)
    same_solution(got, ref.solve(K, sgn, 1.0, EPS, max_iter=5))
    assert got["iterations"] == 5 and got["converged"] == 0
    got = harness_solve(harness, K, sgn, 1.0, EPS, max_iter=0)
    same_solution(got, ref.solve(K, sgn, 1.0, EPS, max_iter=0))
    assert got["iterations"] == 0 and got["converged"] == 0 and got["bias"] == 0.0


@pytest.mark.parametrize("n,dim,C_", [(77, 8, 1.0), (200, 20, 1.0), (400, 20, 10.0)])
def test_the_dual_objective_is_scikit_learns(harness, n, dim, C_):
    """(c) ours and SVC(C, gamma, tol=eps) are each feasible with a violating-pair gap below eps, hence each within eps C n of the optimum of the dual; the two
    objectives differ by at most eps C n.  Measured differences (absolute, of objectives 9.7, 11.5 and 13.6): 77 x 8, C 1: 6.2e-07 of 0.077 allowed; 200 x 20,
    C 1: 6.65e-07 of 0.2; 400 x 20, C 10: 1.26e-06 of 4."""
    svm = pytest.importorskip("sklearn.svm")
    X, y = ref.table(n, dim, 31 * n + dim)
    gamma = 1.0 / dim
    K = ref.kernel_matrix(X, X, gamma)
    sgn = np.where(y != 0, 1, -1)
    r = harness_solve(harness, K, sgn, C_, EPS)                   # the shipped svm_solve_host, not the reference
    assert r["converged"] == 1
    ours = ref.dual_objective(K, sgn, r["alpha"])
    m = svm.SVC(C=C_, kernel="rbf", gamma=gamma, tol=EPS, shrinking=False).fit(X.astype(np.float64), y)
    alpha = np.zeros(n); alpha[m.support_] = np.abs(m.dual_coef_[0])
    theirs = ref.dual_objective(K, sgn, alpha)
    print("%d x %d, C %g: ours %.10g (%d updates), scikit-learn %.10g, difference %.3g of %.3g allowed" % (n, dim, C_, ours, r["iterations"], theirs, abs(ours - theirs), EPS * C_ * n))
    assert abs(ours - theirs) <= EPS * C_ * n
    fx = ref.decision(K, r["coef"], r["bias"])
    assert ((fx > 0) == (m.decision_function(X.astype(np.float64)) > 0)).mean() > 0.98      # (not the check: the two biases differ by up to the gap)


def test_the_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "svm_rule_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    run = subprocess.run([exe, "2", "7"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert " wrong 0" in run.stdout and "rounds 2 " in run.stdout


def test_the_header_fuses_only_where_it_says_so():
    rule = open(os.path.join(CSRC, "svm_rule.h")).read()
    code = "\n".join(l.split("//")[0] for l in rule.splitlines())
    assert code.count("fma(") == 2                                # the two steps of the gradient chain (the distance chain is kmeans_rule.h's)
    assert "km_dist(" in code and "sw_exp_neg(" in code
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "-ffp-contract=off" in mk
