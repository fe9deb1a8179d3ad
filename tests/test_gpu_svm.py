"""GPU: dge_svm_fit*, dge_svm_decision* and dge_svm_cv* give the bits of tests/svm_ref.py, the rule of include/dge.h read out in Python, in every output —
coefficients, bias, iterations, convergence, decision values, per-fold counts — whatever the place of the solver's state (LDS or global memory) and the length
of a launch; at the edges of the wave, the workgroup and the decision's blocks, on duplicated rows, on absent and unselected rows, on a one-class training set,
an empty test fold and rows outside every fold; the refusals name their row and leave the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

import svm_ref as ref

pytestmark = pytest.mark.gpu
EPS = 1e-3
FORMS = [(1, 0), (1, 7), (2, 0), (2, 7)]          # (state, launch_iters): the four give the same bits


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def same_fit(got, want, what=""):
    assert ref.same_bits(got["coef"], want["coef"]), (what, "coef")
    assert ref.same_bits(got["bias"], want["bias"]), (what, got["bias"], want["bias"])
    assert np.array_equal(got["iterations"], want["iterations"]) and np.array_equal(got["converged"], want["converged"]), (what, got["iterations"], want["iterations"])
    assert got["info"]["support"] == int(want["support"].sum()) and got["info"]["iterations"] == int(want["iterations"].sum())


def check_fit(dge, X, Y, C_=1.0, present=None, select=None, forms=FORMS, **kw):
    """fit under every form and the decision on the rows themselves -> (the reference's fit, the Vectors)"""
    dim = X.shape[1]
    want = ref.fit(X, Y, present=present, select=select, C=C_, eps=EPS, **kw)
    v = dge.Vectors.from_host(X, present=present)
    for state, launch in forms:
        got = v.svm_fit(Y, select=select, C=C_, eps=EPS, state=state, launch_iters=launch, **kw)
        same_fit(got, want, (state, launch))
        assert got["gamma"] == 1.0 / dim and got["info"]["rows"] == len(want["used"]) and got["info"]["kernel_bytes"] == 8 * len(want["used"]) ** 2
        assert got["info"]["launches"] >= (1 if launch == 0 else int(want["iterations"].max()) // 7)
    return want, v


@pytest.mark.parametrize("dim", [1, 3, 20, 130])
@pytest.mark.parametrize("n", [2, 63, 64, 65, 255, 256, 257, 1025])
def test_fit_and_decision_are_the_rule_bit_for_bit(dge, n, dim):
    X, y = ref.table(n, dim, 1000 * n + dim)
    want, v = check_fit(dge, X, y)
    assert (want["converged"] == 1).all()
    got = v.svm_decision(want["coef"], want["bias"], want["gamma"])
    assert ref.same_bits(got, np.stack([ref.decision(want["K"], want["coef"][0], want["bias"][0])]))
    # other rows, one of them absent, against the same models
    Z, _ = ref.table(37, dim, 5 + n)
    pres = np.ones(37, bool); pres[11] = False
    Zg = Z.copy(); Zg[11] = np.nan                                # never read
    got = v.svm_decision(want["coef"], want["bias"], want["gamma"], dge.Vectors.from_host(Zg, present=pres))
    assert ref.same_bits(got, ref.decide(X, want["coef"], want["bias"], want["gamma"], Z, present=pres)) and np.isnan(got[0, 11])


@pytest.mark.parametrize("n,dim,lo,hi", [(400, 3, 256, 512), (1100, 1, 512, 768)])
def test_support_counts_across_the_blocks_of_the_decision(dge, n, dim, lo, hi):
    """a small C puts most rows at the bound: the support rows fill two and three blocks of 256"""
    X, y = ref.table(n, dim, 40 + n)
    Y = np.stack([y, 1 - y])
    want, v = check_fit(dge, X, Y, C_=0.05)
    assert lo < want["support"][0] <= hi, want["support"]
    got = v.svm_decision(want["coef"], want["bias"], want["gamma"])
    assert ref.same_bits(got, np.stack([ref.decision(want["K"], want["coef"][l], want["bias"][l]) for l in range(2)]))


def test_duplicated_rows_of_opposite_labels(dge):
    X, y = ref.table(257, 3, 91, dup=40)
    for C_ in (0.25, 16.0):
        want, v = check_fit(dge, X, y, C_=C_)
        assert (want["converged"] == 1).all() and (np.abs(want["coef"][0, :40]) == C_).any()
        assert ref.same_bits(v.svm_decision(want["coef"], want["bias"], want["gamma"])[0], ref.decision(want["K"], want["coef"][0], want["bias"][0]))


def test_absent_rows_and_a_select_mask(dge):
    rng = np.random.default_rng(17)
    X, y = ref.table(300, 8, 17)
    present = rng.random(300) < 0.8
    select = rng.random(300) < 0.7
    Xg = X.copy(); yg = y.copy()
    Xg[~present] = np.nan                                         # never read
    Xg[present & ~select] = np.inf
    yg[~(present & select)] = 9
    want = ref.fit(X, y, present=present, select=select, eps=EPS)
    v = dge.Vectors.from_host(Xg, present=present)
    for state, launch in FORMS:
        same_fit(v.svm_fit(yg, select=select, eps=EPS, state=state, launch_iters=launch), want, (state, launch))
    take = present & select
    assert np.isnan(want["coef"][0, ~take]).all() and not np.isnan(want["coef"][0, take]).any() and len(want["used"]) == take.sum()
    got = v.svm_decision(want["coef"], want["bias"], want["gamma"], dge.Vectors.from_host(X, present=present))
    assert ref.same_bits(got, ref.decide(X, want["coef"], want["bias"], want["gamma"], X, present=present))
    assert np.isnan(got[0, ~present]).all() and not np.isnan(got[0, present]).any()
    # the host-row entry equals the resident one (every row present there)
    import embedding_amd.evaluate as ev
    host = ev.svm_fit_gpu(np.where(np.isnan(Xg), np.float32(0.0), Xg), yg, select=take, eps=EPS)
    same_fit(host, want, "host rows")


def test_the_host_row_decision_is_the_resident_one(dge):
    """dge_svm_decision on the coef and bias of a fit (two models, more than 256 support rows each, NaN on the rows the fit did not take): with x_features NULL
    it decides the support rows themselves, whatever n_x says; with other rows it decides those; both give the bits of Vectors.svm_decision and of the rule"""
    lib = dge.lib
    X, y = ref.table(400, 3, 440)
    Y = np.stack([y, 1 - y])
    select = np.ones(400, bool); select[[3, 77, 78, 399]] = False
    want = ref.fit(X, Y, select=select, C=0.05, eps=EPS)
    assert (want["support"] > 256).all() and np.isnan(want["coef"][:, ~select]).all()
    v = dge.Vectors.from_host(X)
    fit = v.svm_fit(Y, select=select, C=0.05, eps=EPS)
    same_fit(fit, want)
    coef, bias, gamma = fit["coef"], fit["bias"], fit["gamma"]
    Z, _ = ref.table(37, 3, 441)

    def host_rows(x, n_x):
        out = np.full((2, 400 if x is None else len(x)), -7.0)
        rc = lib.dge_svm_decision(0, _p(X), 400, 3, _p(coef), _p(bias), 2, gamma, _p(x), n_x, _p(out))
        assert rc == 0, (lib.dge_last_error() or b"").decode()
        return out

    own = ref.decide(X, want["coef"], want["bias"], gamma)
    assert not np.isnan(own).any()
    for n_x in (0, 400, 5):                                       # without x_features the rows are sv's and n_x is not looked at
        got = host_rows(None, n_x)
        assert ref.same_bits(got, v.svm_decision(coef, bias, gamma)) and ref.same_bits(got, own), n_x
    got = host_rows(Z, 37)
    assert ref.same_bits(got, v.svm_decision(coef, bias, gamma, dge.Vectors.from_host(Z))) and ref.same_bits(got, ref.decide(X, want["coef"], want["bias"], gamma, Z))
    # a model without support rows decides by its bias alone
    zero = np.zeros((2, 400)); b2 = np.array([0.5, -0.25])
    out = np.full((2, 37), -7.0)
    assert lib.dge_svm_decision(0, _p(X), 400, 3, _p(zero), _p(b2), 2, gamma, _p(Z), 37, _p(out)) == 0
    assert (out[0] == 0.5).all() and (out[1] == -0.25).all()


# ------------------------------------------------------------------------------------------ cross-validation
def cv_table():
    """300 x 8, F = 10, five label columns.  Column 3 is 1 on the rows of fold 3 only: one-class inside that fold's training set.  Fold 9 has no test rows.
    Rows 5, 50, 150 have fold -1; rows 7 and 70 are absent."""
    X, y = ref.table(300, 8, 23)
    rng = np.random.default_rng(23)
    fold = (np.arange(300) % 9).astype(np.int32)
    fold[[5, 50, 150]] = -1
    Y = np.stack([y, 1 - y, (rng.random(300) < 0.3).astype(np.uint8), (fold == 3).astype(np.uint8), (X[:, 0] > 0).astype(np.uint8)])
    present = np.ones(300, bool); present[[7, 70]] = False
    Xg = X.copy(); Xg[~present] = np.nan
    Yg = Y.copy(); Yg[:, ~present] = 9; Yg[:, fold < 0] = 9      # rows that are not used may hold anything
    return X, Xg, Y, Yg, fold, present


@pytest.fixture(scope="module")
def cv_case():
    X, Xg, Y, Yg, fold, present = cv_table()
    return dict(X=X, Xg=Xg, Y=Y, Yg=Yg, fold=fold, present=present, want=ref.cv(X, Y, fold, 10, present=present, eps=EPS))


def same_cv(got, want, what=""):
    for f in ("correct", "tested", "iterations", "support", "converged"):
        assert np.array_equal(got[f], want[f]), (what, f, got[f], want[f])
    assert ref.same_bits(got["decision"], want["decision"]), what


def test_cross_validation_is_the_rule_bit_for_bit(dge, cv_case):
    c, want = cv_case, cv_case["want"]
    assert want["tested"][9] == 0 and (want["correct"][:, 9] == 0).all()
    assert want["iterations"][3, 3] == 0 and want["converged"][3, 3] == 1 and want["support"][3, 3] == 0 and want["correct"][3, 3] == 0      # one class: every vote is 0
    assert (want["converged"] == 1).all()
    v = dge.Vectors.from_host(c["Xg"], present=c["present"])
    for state, launch in FORMS:
        got = v.svm_cv(c["Yg"], c["fold"], 10, eps=EPS, state=state, launch_iters=launch, want_decision=True)
        same_cv(got, want, (state, launch))
        assert got["info"]["problems"] == 50 and got["info"]["not_converged"] == 0 and got["info"]["rows"] == 295
        assert got["info"]["iterations"] == want["iterations"].sum() and got["info"]["max_iterations"] == want["iterations"].max()
    assert np.isnan(got["scores"][:, 9]).all() and ref.same_bits(got["scores"][:, :9], want["correct"][:, :9] / want["tested"][None, :9].astype(np.float64))
    assert ref.same_bits(got["mean"], got["scores"][:, :9].mean(axis=1)) and ref.same_bits(got["std"], got["scores"][:, :9].std(axis=1))
    used = c["present"] & (c["fold"] >= 0)
    assert np.isnan(got["decision"][:, ~used]).all() and not np.isnan(got["decision"][:, used]).any()


def test_the_cross_validation_decides_as_a_fit_on_the_fold_does(dge, cv_case):
    """decision from cv equals svm_decision on the coef of a fit with the matching select; the host-row entry equals the resident one"""
    c, want = cv_case, cv_case["want"]
    v = dge.Vectors.from_host(c["Xg"], present=c["present"])
    for f in (0, 3, 9):
        select = (c["fold"] >= 0) & (c["fold"] != f)
        fit = v.svm_fit(c["Yg"], select=select, eps=EPS)
        assert ref.same_bits(fit["coef"], want["coef"][:, f, :]), f
        assert np.array_equal(fit["iterations"], want["iterations"][:, f])
        dec = v.svm_decision(fit["coef"], fit["bias"], fit["gamma"])
        test = c["present"] & (c["fold"] == f)
        assert ref.same_bits(dec[:, test], want["decision"][:, test]), f
    import embedding_amd.evaluate as ev
    keep = c["present"]
    host = ev.svm_cv_gpu(c["X"][keep], c["Y"][:, keep], n_folds=10, fold=c["fold"][keep], eps=EPS, want_decision=True)
    for f in ("correct", "tested", "iterations", "support", "converged"):
        assert np.array_equal(host[f], want[f]), f
    assert ref.same_bits(host["decision"], want["decision"][:, keep])


def test_max_iter_caps_every_two_class_problem(dge, cv_case):
    """the single cap case: max_iter = 5 stops every problem with two classes after 5 updates; the one-class problem (3, 3) has nothing to do"""
    c = cv_case
    want = ref.cv(c["X"], c["Y"], c["fold"], 10, present=c["present"], eps=EPS, max_iter=5)
    assert (want["iterations"] == 5).sum() == 49 and want["iterations"][3, 3] == 0
    got = dge.Vectors.from_host(c["Xg"], present=c["present"]).svm_cv(c["Yg"], c["fold"], 10, eps=EPS, max_iter=5, want_decision=True)
    same_cv(got, want)
    assert got["info"]["not_converged"] == 49 and (got["converged"] == 0).sum() == 49 and got["converged"][3, 3] == 1


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched(dge):
    from embedding_amd._native import SvmCfg, SvmInfo
    lib = dge.lib
    X, y = ref.table(100, 3, 3)
    Y = np.stack([y, 1 - y])
    coef = np.full((2, 100), -7.0); bias = np.full(2, -7.0); iters = np.full(2, -7, np.int64); conv = np.full(2, -7, np.int32)
    info = SvmInfo(); info.rows = -5

    def fit(rows, labels, cfg=None, n_labels=2, select=None, co=coef):
        v = dge.Vectors.from_host(rows)
        c = cfg or SvmCfg(1.0, 1.0 / 3, EPS, 1000000, 0, 0)
        rc = lib.dge_svm_fit_vectors(v._h, _p(labels), n_labels, _p(select), C.byref(c), _p(co), _p(bias), _p(iters), _p(conv), C.byref(info))
        return rc, (lib.dge_last_error() or b"").decode()

    Xb = X.copy(); Xb[40, 2] = np.inf; Xb[40, 1] = np.nan; Xb[77, 0] = np.nan
    rc, msg = fit(Xb, Y)
    assert rc == 1 and "row 40, column 1" in msg and "not finite" in msg, msg
    sel = np.ones(100, np.uint8); sel[40] = 0
    rc, msg = fit(Xb, Y, select=sel)
    assert rc == 1 and "row 77, column 0" in msg, msg
    Yb = Y.copy(); Yb[1, 63] = 3
    rc, msg = fit(X, Yb)
    assert rc == 1 and "row 63" in msg and "label 3" in msg and "column 1" in msg, msg
    big = np.zeros((ref.LDS_ROWS + 1, 1), np.float32); big[::2] = 1.0
    yb = (np.arange(len(big)) % 2).astype(np.uint8)
    cb = np.full((1, len(big)), -7.0)
    rc, msg = fit(big, yb, cfg=SvmCfg(1.0, 1.0, EPS, 10, 1, 0), n_labels=1, co=cb)
    assert rc == 1 and "state = 1" in msg and str(ref.LDS_ROWS) in msg, msg
    huge = np.zeros((ref.MAX_ROWS + 1, 1), np.float32)
    yh = np.zeros(len(huge), np.uint8)
    ch = np.full((1, len(huge)), -7.0)
    rc, msg = fit(huge, yh, n_labels=1, co=ch)
    assert rc == 2 and "65537 used rows" in msg, msg
    correct = np.full((2, 4), -7, np.int64); tested = np.full(4, -7, np.int64); dec = np.full((2, 100), -7.0)
    fold = (np.arange(100) % 4).astype(np.int32)
    v = dge.Vectors.from_host(Xb)
    c = SvmCfg(1.0, 1.0 / 3, EPS, 1000000, 0, 0)
    assert lib.dge_svm_cv_vectors(v._h, _p(Y), 2, _p(fold), 4, C.byref(c), _p(correct), _p(tested), None, None, None, _p(dec), C.byref(info)) == 1
    assert "row 40, column 1" in lib.dge_last_error().decode()
    assert (coef == -7).all() and (bias == -7).all() and (iters == -7).all() and (conv == -7).all() and (cb == -7).all() and (ch == -7).all() and info.rows == -5
    assert (correct == -7).all() and (tested == -7).all() and (dec == -7).all()
    # a coefficient on an absent support row is refused; on a present one with the other rows absent it is not
    pres = np.ones(100, bool); pres[9] = False
    vs = dge.Vectors.from_host(X, present=pres)
    co = np.zeros((1, 100)); co[0, 9] = 0.5
    with pytest.raises(dge.DgeError) as ei:
        vs.svm_decision(co, [0.0], 0.5)
    assert ei.value.code == 1 and "row 9" in str(ei.value) and "absent" in str(ei.value)
    co[0, 9] = np.nan; co[0, 10] = -0.5
    out = vs.svm_decision(co, [0.25], 0.5)
    assert np.isnan(out[0, 9]) and out[0, 10] == 0.25 + -0.5 * 1.0
