"""CPU: sanity checks of the NMF RULE (tests/nmf_ref.py, the Python reading of include/dge.h), not of the kernels: its two fma forms agree, its divergence
objective does not rise from iteration to iteration, and on a rank-2 product matrix it gets as close as scikit-learn's multiplicative-update solver from the same
initial factors."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nmf_ref as ref  # noqa: E402

# test_rank_two_product_against_sklearn: the rule's relative residual may exceed scikit-learn's by this factor.  Measured with this file's inputs (40 x 30 products
# of integer factors, seeds 1, 2, 3, both solvers from the rule's own initial factors, 50 iterations; DESIGN.md section 5.16 records it): residuals 0.0306 / 0.0415,
# 0.0571 / 0.0595 and 0.0157 / 0.0136 (rule / scikit-learn), ratios 0.74, 0.96 and 1.15 — both run Lee and Seung's update, the rule H first, scikit-learn W first.
# The comparison is made at 50 iterations because further on both residuals fall geometrically towards 0 and their ratio says nothing (at 200 iterations it was
# measured between 0.09 and 6.6 on the same inputs).
SKLEARN_MARGIN = 1.5
ITERATIONS = 50


def test_the_two_fma_forms_agree():
    rng = np.random.default_rng(2)
    n = 4000
    a = (rng.random(n) - 0.5) * 10.0 ** rng.integers(-30, 30, n)
    b = (rng.random(n) - 0.5) * 10.0 ** rng.integers(-30, 30, n)
    c = (rng.random(n) - 0.5) * 10.0 ** rng.integers(-30, 30, n)
    c[::3] = -(a[::3] * b[::3])                              # cancellation: the result is the product's rounding error
    c[1::7] = 0.0
    a[2::11] = np.round(a[2::11] * 2.0 ** 20) / 2.0 ** 20    # short significands: exact products, ties
    b[2::11] = 3.0
    c[2::11] = np.ldexp(1.0, -55) * a[2::11]
    got = ref.fma_np(a, b, c)
    want = np.array([ref.fma(x, y, z) for x, y, z in zip(a, b, c)])
    assert ref.same_bits(got, want)
    # the sizes the rule meets: values at the floor, tiny matrices
    a = np.array([ref.EPS, ref.EPS, 1e-300 * 37, 2.0 ** -52, 50.0]); b = np.array([ref.EPS, 1e-269, ref.EPS, 2.0 ** -52, 50.0]); c = np.array([0.0, 2.0 ** -104, 1e-290, 3 * 2.0 ** -104, 1e5])
    assert ref.same_bits(ref.fma_np(a, b, c), np.array([ref.fma(x, y, z) for x, y, z in zip(a, b, c)]))


@pytest.mark.parametrize("shape,density,rank,hub", [((60, 45), 0.1, 3, None), ((64, 48), 0.15, 10, (3, 5)), ((257, 130), 0.03, 10, None)])
def test_the_divergence_objective_does_not_rise(shape, density, rank, hub):
    r, c, v = ref.random_sparse(shape[0], shape[1], density, 7, hub=hub)
    trace = []
    res = ref.nmf(r, c, v, shape, rank=rank, max_iter=8, update=ref.DIVERGENCE, seed=12345, trace=trace)
    assert len(trace) == 8
    for k in range(1, 8):
        (prev, a0), (cur, a1) = trace[k - 1], trace[k]
        assert cur <= prev + ref.objective_bound(res["E"], rank, max(a0, a1)), (k, prev, cur)
    assert trace[-1][0] < trace[0][0] and trace[-1][0] >= -ref.objective_bound(res["E"], rank, trace[-1][1])


def test_rank_two_product_against_sklearn(capsys):
    decomposition = pytest.importorskip("sklearn.decomposition")
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        n, m = 40, 30
        V = rng.integers(1, 6, (n, 2)).astype(np.float64) @ rng.integers(1, 6, (2, m)).astype(np.float64)
        rows, cols = np.divmod(np.arange(n * m), m)
        W0, H0 = ref.init_factors(n, m, 2, seed, V.max())
        res = ref.nmf(rows, cols, V.ravel(), (n, m), rank=2, max_iter=ITERATIONS, update=ref.DIVERGENCE, init=(W0, H0))
        mine = np.linalg.norm(V - res["W"] @ res["H"]) / np.linalg.norm(V)
        model = decomposition.NMF(n_components=2, init="custom", solver="mu", beta_loss="kullback-leibler", max_iter=ITERATIONS, tol=0.0)
        Ws = model.fit_transform(V, W=W0.copy(), H=H0.copy())
        theirs = np.linalg.norm(V - Ws @ model.components_) / np.linalg.norm(V)
        with capsys.disabled():
            print("\nrank-2 product %d x %d, seed %d, %d iterations: relative residual of the rule %.6e, of scikit-learn's mu solver %.6e" % (n, m, seed, ITERATIONS, mine, theirs))
        assert mine <= SKLEARN_MARGIN * theirs and mine < 0.1, (mine, theirs)
