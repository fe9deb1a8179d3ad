"""CPU: the host build of embedding_amd/csrc/ridge_rule.h (tests/native/ridge_rule_harness.cpp) gives the bits of tests/ridge_ref.py, the rule of include/dge.h
read out in Python, for every quantity of the rule — moments, pivots, L, coefficients, leverages, left-out errors, the two figures — at the edges of the blocked
sums; the rule is right as well as self-consistent: on integer-lattice inputs its left-out predictions are those of the twelve refits solved in rational
arithmetic, to a bound from the system's condition number; the two refusals name their column and their row; the same harness, built stand-alone with
-fsanitize=address,undefined, runs clean."""
import os
import subprocess

import numpy as np
import pytest

import ridge_ref as ref
from ridge_harness import SRC, harness_ridge, load_harness, same_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "embedding_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return load_harness(os.path.join(str(tmp_path_factory.mktemp("ridge_rule_harness")), "libridge_rule_harness.so"))


def table(n, dim, T, seed):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n, dim)) * 10.0 ** rng.integers(-2, 3, dim)).astype(np.float32)
    Y = rng.standard_normal((n, T)) * 50.0 + 20.0
    return X, Y


@pytest.mark.parametrize("dim", [1, 3, 17])
@pytest.mark.parametrize("n", [2, 5, 255, 256, 257, 700])
def test_the_host_solver_is_the_rule_bit_for_bit(harness, n, dim):
    T = 2 if n < 255 else 1
    X, Y = table(n, dim, T, 1000 * n + dim)
    lambdas = [0.0, 0.5] if n > 4 * (dim + 1) else [0.5, 3.0]      # lambda = 0 needs more rows than columns
    want = ref.ridge_loo(X, Y, lambdas)
    got = harness_ridge(harness, X, Y, lambdas)
    assert "refused" not in got, got
    same_result(got, want)
    assert (want["d"] > 0).all() and (want["h"] < 1).all() and np.isfinite(want["mre"]).all()


def lattice(seed, n=12, dim=3):
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, (n, dim)).astype(np.float32), rng.integers(-20, 21, n).astype(np.float64)


@pytest.mark.parametrize("lam", [0.0, 0.5])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_left_out_predictions_are_those_of_the_refits(harness, seed, lam):
    """n = 12, dim = 3, features in -8 .. 8: the identity e = r / (1 - h) against twelve exact refits.  Tolerance: 64 * P * 2^-53 * cond_2(A) relative to
    max |prediction| — a first-order backward-error bound for LDL' and two triangular solves, the constant generous because the bound is first-order."""
    X, y = lattice(seed)
    exact = ref.exact_loo(X, y, lam)
    got = harness_ridge(harness, X, y, [lam])
    assert "refused" not in got, got
    same_result(got, ref.ridge_loo(X, y, [lam]))
    P = X.shape[1] + 1
    Z = np.concatenate([np.ones((len(X), 1)), X.astype(np.float64)], axis=1)
    A = Z.T @ Z + lam * np.diag([0.0] + [1.0] * (P - 1))           # integers and halves: exact
    tol = 64 * P * 2.0 ** -53 * np.linalg.cond(A, 2)
    scale = max(abs(float(v)) for v in exact)
    err = max(abs(ref.Fraction(float(p)) - v) for p, v in zip(got["loo_pred"][0, 0], exact))
    print("lattice seed %d lambda %g: cond %.3g, error %.3g of %.3g allowed" % (seed, lam, np.linalg.cond(A, 2), float(err) / scale, tol))
    assert float(err) <= tol * scale


def test_a_rank_deficient_system_is_refused_at_its_column(harness):
    X, y = lattice(5, n=12, dim=4)
    X[:, 3] = X[:, 2]                                             # column 4 of z repeats column 3: its chain is column 3's, L[4][3] = 1 and the pivot of j = 4 is exactly 0
    assert harness_ridge(harness, X, y, [0.5, 0.0]).get("refused") == ("pivot", 1, 4)
    assert harness_ridge(harness, X, y, [0.0]).get("refused") == ("pivot", 0, 4)
    assert "refused" not in harness_ridge(harness, X, y, [0.5, 2.0])
    with pytest.raises(ref.Refused) as ei:
        ref.ridge_loo(X, y, [0.5, 0.0])
    assert (ei.value.kind, ei.value.lam, ei.value.index) == ("pivot", 1, 4)


def test_a_row_nothing_else_predicts_is_refused_by_its_number(harness):
    """Row 3 is the only one with a non-zero second feature: under lambda = 0 the fit goes through it, h = 1 exactly (integers), g = 0."""
    X = np.array([[1, 0], [2, 0], [4, 0], [3, 5], [7, 0], [8, 0]], np.float32)
    y = np.array([1.0, 2.0, 0.0, 4.0, 5.0, 3.0])
    assert harness_ridge(harness, X, y, [1.0, 0.0]).get("refused") == ("leverage", 1, 3)
    with pytest.raises(ref.Refused) as ei:
        ref.ridge_loo(X, y, [1.0, 0.0])
    assert (ei.value.kind, ei.value.lam, ei.value.index) == ("leverage", 1, 3)
    assert "refused" not in harness_ridge(harness, X, y, [1.0])
    # a pivot's refusal goes before a leverage's, whatever the order of the lambdas
    Xd = np.concatenate([X, X[:, 1:]], axis=1)
    assert harness_ridge(harness, Xd, y, [0.0, 1.0]).get("refused") == ("pivot", 0, 3)


def test_the_prediction_chain(harness):
    rng = np.random.default_rng(4)
    for dim in (1, 3, 17, 64):
        x = rng.standard_normal(dim).astype(np.float32); beta = rng.standard_normal(dim + 1)
        got = harness.harness_ridge_predict(x.ctypes.data, beta.ctypes.data, dim)
        assert got == ref.predict(ref.design(x[None, :])[0], beta)


def test_the_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "ridge_rule_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    run = subprocess.run([exe, "3", "7"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert " wrong 0" in run.stdout and "rounds 3 " in run.stdout


def test_the_header_fuses_only_where_it_says_so():
    rule = open(os.path.join(CSRC, "ridge_rule.h")).read()
    code = "\n".join(l.split("//")[0] for l in rule.splitlines())
    assert code.count("fma(") == 4                                # the moment, substitution, leverage and prediction steps
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "-ffp-contract=off" in mk
