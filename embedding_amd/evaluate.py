"""Quality metric of the reference's evaluation scripts on the device (P/embeddingEvaluation_tract.py:169-196 pairwiseEstimator, :249-260
ndcg_atK): ctypes views of dge_knn_cosine / dge_ndcg_at_k.  Used as the statistical parity check between training schedules (in-order /
Hogwild / multi-GPU) on one slice; and the reference's second figure, clusteringAccuracy (:539-571), on a k-means that is a fully specified rule
(include/dge.h: dge_kmeans_vectors, dge_cluster_accuracy) instead of scikit-learn's randomised one; and the figures' "MF" baseline, NMF of a slice's flow matrix
(P/matrixFactorization_tract.py:26-45), likewise a rule (dge_nmf_coo, dge_nmf_flows) instead of nimfa's randomised runs; and their "LINE" baseline
(P/flowFeatureGeneration_tract.py:54-73), a rule as well (dge_line_coo, dge_line_flows) instead of a third-party tool's racing threads; and their third figure, the cross-validated accuracy of a decision
tree on median labels (:201-232, :34-47), again a rule (dge_tree_fit, dge_tree_cv) instead of scikit-learn's randomly tie-broken one; and the fourth, the leave-one-out
regression error of regression-eval.sh:43-49 (P/tf_linear_regression.py:61-83), a rule too (dge_ridge_loo: closed-form ridge, the leverage identity) instead of ten steps of TensorFlow's FTRL.  The float64 host restatement these kernels are checked against is test infrastructure: oracle/quality.py."""
import numpy as np


def knn_cosine_gpu(features, k, device=0):
    """The same KNN lists from libdge.so (dge_knn_cosine: exact-f32 MFMA tiles fused with top-k on the MI355X).
    -> (idx int32 [n x k], dist float32 [n x k], kernel_ms)."""
    import ctypes as C
    from ._native import check, lib
    f = np.ascontiguousarray(features, np.float32)
    n, D = f.shape
    idx = np.empty((n, k), np.int32); dist = np.empty((n, k), np.float32); ms = C.c_double(0)
    check(lib.dge_knn_cosine(int(device), f.ctypes.data_as(C.c_void_p), n, D, int(k), idx.ctypes.data_as(C.c_void_p),
                             dist.ctypes.data_as(C.c_void_p), C.byref(ms)))
    return idx, dist, ms.value


def ndcg_against_gpu(features, gnd_features, k=10, device=0):
    """ndcg_against wholly on the device (dge_ndcg_at_k): both KNN passes on MFMA, the relevance look-ups and the DCG sums in a
    kernel.  -> (nDCG@k, kernel ms of the two KNN passes)."""
    import ctypes as C
    from ._native import check, lib
    f = np.ascontiguousarray(features, np.float32); g = np.ascontiguousarray(gnd_features, np.float32)
    if len(f) != len(g):
        raise ValueError("features and gnd_features describe different numbers of regions")
    out = C.c_double(0); ms = C.c_double(0)
    check(lib.dge_ndcg_at_k(int(device), f.ctypes.data_as(C.c_void_p), f.shape[1], g.ctypes.data_as(C.c_void_p), g.shape[1], len(f), int(k),
                            C.byref(out), C.byref(ms)))
    return out.value, ms.value


def knn_cosine_vectors(vectors, k):
    """knn_cosine_gpu on resident rows (an engine.Vectors, e.g. from Vectors.from_vec): dge_knn_cosine_vectors, no host copy of the features."""
    return vectors.knn(k)


def ndcg_vectors(vectors, gnd_vectors, k=10):
    """ndcg_against_gpu on two resident row sets aligned by name (engine.Vectors): dge_ndcg_at_k_vectors."""
    return vectors.ndcg_against(gnd_vectors, k)


def _info_dict(inf, reserved=True):
    """the fields of a ctypes info struct; reserved=False: without the field of that name"""
    return {f[0]: getattr(inf, f[0]) for f in inf._fields_ if reserved or f[0] != "reserved"}


def _select_mask(select, n):
    """select -> uint8 [n], non-zero = take the row; None stays None"""
    if select is None:
        return None
    select = np.ascontiguousarray(np.asarray(select) != 0, np.uint8)
    if select.shape != (n,):
        raise ValueError("select must hold one entry per row")
    return select


def kmeans_gpu(features, k, seed=1, n_init=10, max_iter=300, select=None, init=None, device=0):
    """k-means of host rows [n x dim] on the device as the rule of include/dge.h (dge_kmeans).  -> (labels int32 [n], -1 on rows select leaves out;
    centres float32 [k x dim]; info: the fields of struct dge_kmeans_info)."""
    import ctypes as C
    from ._native import KmeansCfg, KmeansInfo, check, lib
    f = np.ascontiguousarray(features, np.float32)
    n, dim = f.shape
    k = int(k)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    select = _select_mask(select, n)
    if init is not None:
        init = np.ascontiguousarray(init, np.float32)
        if init.shape != (k, dim):
            raise ValueError("init must be [k x dim] = [%d x %d], not %s" % (k, dim, list(init.shape)))
    cfg = KmeansCfg(k, int(n_init), int(max_iter), 0, int(seed) & 0xFFFFFFFFFFFFFFFF)
    labels = np.empty(n, np.int32); centres = np.empty((max(k, 0), dim), np.float32); inf = KmeansInfo()
    check(lib.dge_kmeans(int(device), p(f), n, dim, p(select), C.byref(cfg), p(init), p(labels), p(centres), C.byref(inf)))
    return labels, centres, _info_dict(inf)


def clustering_accuracy(labels, gnd, k):
    """clusteringAccuracy of the reference (P/embeddingEvaluation_tract.py:544-571) from cluster labels and ground labels, both in [0, k) or -1
    (dge_cluster_accuracy; a host computation).  -> (accuracy, cnt int64 [k x k], map int32 [k])."""
    import ctypes as C
    from ._native import check, lib
    a = np.ascontiguousarray(labels, np.int32); g = np.ascontiguousarray(gnd, np.int32)
    if a.shape != g.shape or a.ndim != 1:
        raise ValueError("labels and gnd must be one-dimensional and of one length")
    k = int(k)
    cnt = np.zeros((max(k, 0), max(k, 0)), np.int64); m = np.full(max(k, 0), -1, np.int32); acc = C.c_double(0)
    check(lib.dge_cluster_accuracy(a.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p), len(a), k, cnt.ctypes.data_as(C.c_void_p),
                                   m.ctypes.data_as(C.c_void_p), C.byref(acc)))
    return acc.value, cnt, m


def clustering_accuracy_vectors(vectors, gnd_labels, k, seed=1, n_init=10, max_iter=300, select=None):
    """The reference's clusteringAccuracy on resident rows (an engine.Vectors): k-means by rule, then the accuracy of its labels against gnd_labels
    (one per row, -1 = no ground label).  Rows the embedding lacks count in the denominator, as in the reference.  -> (accuracy, labels, info)."""
    labels, _, info = vectors.kmeans(k, seed=seed, n_init=n_init, max_iter=max_iter, select=select)
    acc, cnt, m = clustering_accuracy(labels, gnd_labels, k)
    info = dict(info, cnt=cnt, map=m)
    return acc, labels, info


NMF_UPDATES = {"divergence": 0, "euclidean": 1}


def nmf_config(rank=10, max_iter=30, update="divergence", seed=1):
    """struct dge_nmf_cfg from the keywords nmf_gpu and Flows.nmf share; update: "divergence" / "euclidean" (nimfa's names) or 0 / 1."""
    from ._native import NmfCfg
    if isinstance(update, str):
        if update not in NMF_UPDATES:
            raise ValueError("update must be 'divergence' or 'euclidean', not %r" % (update,))
        update = NMF_UPDATES[update]
    return NmfCfg(int(rank), int(max_iter), int(update), 0, int(seed) & 0xFFFFFFFFFFFFFFFF)


def nmf_gpu(rows, cols, vals, shape, rank=10, max_iter=30, update="divergence", seed=1, init=None, device=0):
    """NMF of the sparse matrix V [n x m] = shape given as entries (rows[e], cols[e], vals[e]), on the device as the rule of include/dge.h (dge_nmf_coo): the
    same bits for the same entries in any order, shape, rank, max_iter, update and seed.  init: (W [n x rank], H [rank x m]) replaces the generated factors.
    -> (W float64 [n x rank], H float64 [rank x m], info: the fields of struct dge_nmf_info)."""
    import ctypes as C
    from ._native import NmfInfo, check, lib
    r = np.ascontiguousarray(rows, np.int32); c = np.ascontiguousarray(cols, np.int32); v = np.ascontiguousarray(vals, np.float64)
    if not (r.ndim == c.ndim == v.ndim == 1 and len(r) == len(c) == len(v)):
        raise ValueError("rows, cols and vals must be one-dimensional and of one length")
    n, m = int(shape[0]), int(shape[1])
    cfg = nmf_config(rank, max_iter, update, seed)
    rank = cfg.rank
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    iw = ih = None
    if init is not None:
        iw = np.ascontiguousarray(init[0], np.float64); ih = np.ascontiguousarray(init[1], np.float64)
        if iw.shape != (n, rank) or ih.shape != (rank, m):
            raise ValueError("init must be (W [%d x %d], H [%d x %d])" % (n, rank, rank, m))
    W = np.empty((max(n, 0), max(rank, 0)), np.float64); H = np.empty((max(rank, 0), max(m, 0)), np.float64); inf = NmfInfo()
    check(lib.dge_nmf_coo(int(device), p(r), p(c), p(v), len(v), n, m, C.byref(cfg), p(iw), p(ih), p(W), p(H), C.byref(inf)))
    return W, H, {k: v for k, v in _info_dict(inf).items() if k != "reserved"}


def nmf_features(W, H):
    """A region's MF feature as the reference forms it: concat(W, H^T) (P/matrixFactorization_tract.py:44).  Square matrices only."""
    W = np.asarray(W); H = np.asarray(H)
    if W.ndim != 2 or H.ndim != 2 or W.shape[1] != H.shape[0] or W.shape[0] != H.shape[1]:
        raise ValueError("nmf_features needs W [n x rank] and H [rank x n] of a square matrix, not %s and %s" % (list(W.shape), list(H.shape)))
    return np.concatenate([W, H.T], axis=1)


def line_config(dim=20, order=2, negative=5, samples=1000000, batch=4096, rho0=0.025, seed=1):
    """struct dge_line_cfg from the keywords line_gpu and Flows.line share."""
    from ._native import LineCfg
    return LineCfg(int(dim), int(order), int(negative), int(batch), int(samples), float(rho0), int(seed) & 0xFFFFFFFFFFFFFFFF)


def line_gpu(src, dst, w, n, dim=20, order=2, negative=5, samples=1000000, batch=4096, rho0=0.025, seed=1, init=None, device=0):
    """LINE on the directed weighted graph of n vertices given as entries (src[e], dst[e], w[e]), on the device as the rule of include/dge.h (dge_line_coo): the
    same bits for the same entries in any order, n, dim, order, negative, samples, batch, rho0 and seed.  init: X [n x dim], or (X, Y), replaces the generated
    tables.  -> (X float64 [n x dim], Y float64 [n x dim], touched bool [n], info: the fields of struct dge_line_info)."""
    import ctypes as C
    from ._native import LineInfo, check, lib
    s = np.ascontiguousarray(src, np.int32); d = np.ascontiguousarray(dst, np.int32); v = np.ascontiguousarray(w, np.float64)
    if not (s.ndim == d.ndim == v.ndim == 1 and len(s) == len(d) == len(v)):
        raise ValueError("src, dst and w must be one-dimensional and of one length")
    n = int(n)
    cfg = line_config(dim, order, negative, samples, batch, rho0, seed)
    dim = cfg.dim
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    ix = iy = None
    if init is not None:
        if isinstance(init, (tuple, list)):
            ix, iy = init
        else:
            ix = init
        ix = np.ascontiguousarray(ix, np.float64)
        iy = None if iy is None else np.ascontiguousarray(iy, np.float64)
        if ix.shape != (n, dim) or (iy is not None and iy.shape != (n, dim)):
            raise ValueError("init must be X [%d x %d] or (X, Y) of that shape" % (n, dim))
    X = np.empty((max(n, 0), max(dim, 0)), np.float64); Y = np.empty_like(X); touched = np.empty(max(n, 0), np.uint8); inf = LineInfo()
    check(lib.dge_line_coo(int(device), p(s), p(d), p(v), len(v), n, C.byref(cfg), p(ix), p(iy), p(X), p(Y), p(touched), C.byref(inf)))
    return X, Y, touched.astype(bool), _info_dict(inf)


def line_features(X, touched, dtype=np.float32):
    """A region's LINE feature as the reference forms it: the vertex row, and a row of zeros for a region the edge file never names — what
    getLINEembeddingFeatures inserts for missing regions (P/flowFeatureGeneration_tract.py:54-73)."""
    X = np.asarray(X); touched = np.asarray(touched)
    if X.ndim != 2 or touched.shape != (X.shape[0],):
        raise ValueError("line_features needs X [n x dim] and touched [n], not %s and %s" % (list(X.shape), list(touched.shape)))
    out = X.astype(dtype)
    out[touched == 0] = 0
    return out


def cv_scores(correct, tested):
    """Per-fold accuracies from counts: scores[t] = correct[t] / tested[t] in binary64, NaN where a fold tested nothing; mean: numpy's mean of the others (what
    cross_val_score(..).mean() is in the reference), NaN if there is none.  -> dict(scores, mean, correct, tested)."""
    correct = np.asarray(correct, np.int64); tested = np.asarray(tested, np.int64)
    scores = np.full(len(tested), np.nan, np.float64)
    ok = tested > 0
    scores[ok] = correct[ok].astype(np.float64) / tested[ok].astype(np.float64)
    return dict(scores=scores, mean=float(scores[ok].mean()) if ok.any() else float("nan"), correct=correct, tested=tested)


def median_labels(counts):
    """generatePOIlabel_helper of the reference (P/embeddingEvaluation_tract.py:34-47) on integer counts, decided in integers: label 1 iff val >= median, and the
    flag median >= 1 (the reference keeps a label only where it holds).  -> (labels uint8 [n], flag)."""
    c = np.asarray(counts)
    if c.ndim != 1 or len(c) == 0 or not np.issubdtype(c.dtype, np.integer):
        raise ValueError("counts must be a non-empty one-dimensional array of integers")
    s = sorted(int(v) for v in c)
    twice = 2 * s[len(s) // 2] if len(s) % 2 else s[len(s) // 2 - 1] + s[len(s) // 2]       # twice the median, an integer
    return np.array([1 if 2 * int(v) >= twice else 0 for v in c], np.uint8), twice >= 2


def stratified_folds(y, n_folds, select=None):
    """The folds of the tree's cross-validation as a rule: the j-th used row of its class, in row order, gets fold j mod n_folds; a row `select` leaves out gets -1.
    -> int32 [n]."""
    y = np.asarray(y)
    F = int(n_folds)
    if y.ndim != 1 or F < 1:
        raise ValueError("y must be one-dimensional and n_folds at least 1")
    use = np.ones(len(y), bool) if select is None else np.asarray(select) != 0
    if use.shape != y.shape:
        raise ValueError("select must hold one entry per row")
    fold = np.full(len(y), -1, np.int32)
    for cls in np.unique(y[use]):
        idx = np.flatnonzero(use & (y == cls))
        fold[idx] = np.arange(len(idx)) % F
    return fold


def _cv_folds(y, n_folds, fold, select):
    """The folds of a cross-validation on host rows: the caller's, or stratified_folds of the labels y [n] -> int32 [n]"""
    if fold is None:
        fold = stratified_folds(y, n_folds, select)
    elif select is not None:
        raise ValueError("give fold or select, not both: fold -1 leaves a row out")
    fold = np.ascontiguousarray(fold, np.int32)
    if fold.shape != y.shape:
        raise ValueError("fold must hold one entry per row")
    return fold


def _tree_args(features, y):
    f = np.ascontiguousarray(features, np.float32)
    if f.ndim != 2:
        raise ValueError("features must be [n x dim]")
    y = np.asarray(y)
    if y.shape != (len(f),):
        raise ValueError("y must hold one label per row")
    if y.dtype != np.uint8:
        y = np.where((y == 0) | (y == 1), y, 255).astype(np.uint8)
    return f, np.ascontiguousarray(y)


def tree_fit_gpu(features, y, select=None, max_depth=0, min_samples_split=2, min_samples_leaf=1, device=0):
    """A binary decision tree on host rows [n x dim] with labels y in {0, 1}, on the device as the rule of include/dge.h (dge_tree_fit).
    -> (tree: dict of feature, threshold, left, count, pos; info: the fields of struct dge_tree_info)."""
    import ctypes as C
    from ._native import TreeCfg, TreeInfo, check, lib
    f, y = _tree_args(features, y)
    n, dim = f.shape
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    select = _select_mask(select, n)
    cfg = TreeCfg(int(max_depth), int(min_samples_split), int(min_samples_leaf), 0)
    cap = max(2 * n - 1, 1)
    feature = np.empty(cap, np.int32); threshold = np.empty(cap, np.float64); left = np.empty(cap, np.int32); count = np.empty(cap, np.int64); pos = np.empty(cap, np.int64)
    inf = TreeInfo()
    check(lib.dge_tree_fit(int(device), p(f), n, dim, p(y), p(select), C.byref(cfg), cap, p(feature), p(threshold), p(left), p(count), p(pos), C.byref(inf)))
    m = inf.n_nodes
    tree = dict(feature=feature[:m].copy(), threshold=threshold[:m].copy(), left=left[:m].copy(), count=count[:m].copy(), pos=pos[:m].copy())
    return tree, _info_dict(inf)


def tree_cv_gpu(features, y, n_folds=10, fold=None, select=None, max_depth=0, min_samples_split=2, min_samples_leaf=1, device=0):
    """cross_val_score(DecisionTreeClassifier(), features, y, cv=n_folds) of the reference (P/embeddingEvaluation_tract.py:224-225) as the rule of include/dge.h
    (dge_tree_cv).  fold: one fold number per row, -1 = leave the row out (default: stratified_folds(y, n_folds, select)).
    -> dict(scores, mean, correct, tested, n_nodes, depth, info)."""
    import ctypes as C
    from ._native import TreeCfg, TreeInfo, check, lib
    f, y = _tree_args(features, y)
    n, dim = f.shape
    F = int(n_folds)
    fold = _cv_folds(y, F, fold, select)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    cfg = TreeCfg(int(max_depth), int(min_samples_split), int(min_samples_leaf), 0)
    correct = np.zeros(max(F, 0), np.int64); tested = np.zeros(max(F, 0), np.int64); nodes = np.zeros(max(F, 0), np.int32); depth = np.zeros(max(F, 0), np.int32)
    inf = TreeInfo()
    check(lib.dge_tree_cv(int(device), p(f), n, dim, p(y), p(fold), F, C.byref(cfg), p(correct), p(tested), p(nodes), p(depth), C.byref(inf)))
    return dict(cv_scores(correct, tested), n_nodes=nodes, depth=depth, info=_info_dict(inf))


def _ridge_args(n, y, lambdas, select):
    """y [n] or [n x T] -> float64 [n x T]; lambdas -> float64 [L]; select -> uint8 [n] or None.  The shapes are checked here, the values by the library."""
    y = np.asarray(y, np.float64)
    if y.ndim == 1:
        y = y[:, None]
    if y.ndim != 2 or y.shape[0] != n:
        raise ValueError("y must hold one row of targets per row: [%d] or [%d x n_targets], not %s" % (n, n, list(y.shape)))
    lam = np.ascontiguousarray(np.atleast_1d(np.asarray(lambdas, np.float64)))
    if lam.ndim != 1:
        raise ValueError("lambdas must be a number or one-dimensional")
    select = _select_mask(select, n)
    return np.ascontiguousarray(y), lam, select


def ridge_loo_gpu(features, y, lambdas, select=None, device=0):
    """Leave-one-out ridge regression of the targets y on host rows [n x dim], on the device as the rule of include/dge.h (dge_ridge_loo): the reference's
    regression figure (np.mean(mae), and that over mean(target)) per penalty and target.
    -> dict(mae, mre [n_lambda x n_targets]; beta [n_lambda x n_targets x (dim + 1)]; loo_pred [n_lambda x n_targets x n], NaN on rows select leaves out; info)."""
    import ctypes as C
    from ._native import RidgeInfo, check, lib
    f = np.ascontiguousarray(features, np.float32)
    if f.ndim != 2:
        raise ValueError("features must be [n x dim]")
    n, dim = f.shape
    y, lam, select = _ridge_args(n, y, lambdas, select)
    T, L = y.shape[1], len(lam)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    mae = np.empty((L, T), np.float64); mre = np.empty((L, T), np.float64); beta = np.empty((L, T, dim + 1), np.float64); pred = np.empty((L, T, n), np.float64)
    inf = RidgeInfo()
    check(lib.dge_ridge_loo(int(device), p(f), n, dim, p(y), T, p(select), p(lam), L, p(mae), p(mre), p(beta), p(pred), C.byref(inf)))
    return dict(mae=mae, mre=mre, beta=beta, loo_pred=pred, info=_info_dict(inf))


def svm_scores(correct, tested):
    """Per-label, per-fold accuracies from counts: scores[l][f] = correct[l][f] / tested[f], NaN where a fold tested nothing; mean, std [n_labels]: numpy's over
    the other folds (scores.mean(), scores.std() of the reference's printed line).  -> dict(scores, mean, std, correct, tested)."""
    correct = np.asarray(correct, np.int64); tested = np.asarray(tested, np.int64)
    scores = np.full(correct.shape, np.nan, np.float64)
    ok = tested > 0
    scores[:, ok] = correct[:, ok].astype(np.float64) / tested[ok].astype(np.float64)
    if ok.any():
        mean = scores[:, ok].mean(axis=1); std = scores[:, ok].std(axis=1)
    else:
        mean = np.full(len(correct), np.nan); std = np.full(len(correct), np.nan)
    return dict(scores=scores, mean=mean, std=std, correct=correct, tested=tested)


def _svm_args(features, y):
    f = np.ascontiguousarray(features, np.float32)
    if f.ndim != 2:
        raise ValueError("features must be [n x dim]")
    y = np.asarray(y)
    if y.ndim == 1:
        y = y[None, :]
    if y.ndim != 2 or y.shape[1] != len(f) or y.shape[0] < 1:
        raise ValueError("y must hold one label per row: [n] or [n_labels x n]")
    if y.dtype != np.uint8:
        y = np.where((y == 0) | (y == 1), y, 255).astype(np.uint8)
    return f, np.ascontiguousarray(y)


def svm_fit_gpu(features, y, select=None, C=1.0, gamma=None, eps=1e-3, max_iter=10_000_000, state=0, launch_iters=0, device=0):
    """An RBF C-SVC per label column on host rows [n x dim] with labels y [n] or [n_labels x n] in {0, 1}, on the device as the rule of include/dge.h
    (dge_svm_fit).  gamma: default 1 / dim.  -> dict(coef [n_labels x n], bias, iterations, converged [n_labels], gamma, info)."""
    import ctypes as Ct
    from ._native import SvmCfg, SvmInfo, check, lib
    f, y = _svm_args(features, y)
    n, dim = f.shape
    L = y.shape[0]
    p = lambda a: None if a is None else a.ctypes.data_as(Ct.c_void_p)      # noqa: E731
    select = _select_mask(select, n)
    cfg = SvmCfg(float(C), 1.0 / max(dim, 1) if gamma is None else float(gamma), float(eps), int(max_iter), int(state), int(launch_iters))
    coef = np.empty((L, n), np.float64); bias = np.empty(L, np.float64); iters = np.zeros(L, np.int64); conv = np.zeros(L, np.int32); inf = SvmInfo()
    check(lib.dge_svm_fit(int(device), p(f), n, dim, p(y), L, p(select), Ct.byref(cfg), p(coef), p(bias), p(iters), p(conv), Ct.byref(inf)))
    return dict(coef=coef, bias=bias, iterations=iters, converged=conv, gamma=cfg.gamma, info=_info_dict(inf))


def svm_cv_gpu(features, y, n_folds=10, fold=None, select=None, C=1.0, gamma=None, eps=1e-3, max_iter=10_000_000, state=0, launch_iters=0, want_decision=False,
               device=0):
    """cross_val_score(svm.SVC(), features, y, cv=n_folds) of the reference (P/binaryClassification_CA.py:38,55-57) for every label column at once, as the rule
    of include/dge.h (dge_svm_cv).  fold: one fold number per row, -1 = leave the row out (default: stratified_folds of the FIRST label column — one set of
    folds serves all columns of a call).  -> dict(scores [n_labels x n_folds], mean, std [n_labels], correct, tested, iterations, support, converged,
    decision, gamma, info)."""
    import ctypes as Ct
    from ._native import SvmCfg, SvmInfo, check, lib
    f, y = _svm_args(features, y)
    n, dim = f.shape
    L, F = y.shape[0], int(n_folds)
    fold = _cv_folds(y[0], F, fold, select)
    p = lambda a: None if a is None else a.ctypes.data_as(Ct.c_void_p)      # noqa: E731
    cfg = SvmCfg(float(C), 1.0 / max(dim, 1) if gamma is None else float(gamma), float(eps), int(max_iter), int(state), int(launch_iters))
    shape = (L, max(F, 0))
    correct = np.zeros(shape, np.int64); tested = np.zeros(max(F, 0), np.int64); iters = np.zeros(shape, np.int64); support = np.zeros(shape, np.int64)
    conv = np.zeros(shape, np.int32); inf = SvmInfo()
    decision = np.empty((L, n), np.float64) if want_decision else None
    check(lib.dge_svm_cv(int(device), p(f), n, dim, p(y), L, p(fold), F, Ct.byref(cfg), p(correct), p(tested), p(iters), p(support), p(conv), p(decision), Ct.byref(inf)))
    return dict(svm_scores(correct, tested), iterations=iters, support=support, converged=conv, decision=decision, gamma=cfg.gamma,
                info=_info_dict(inf))


PAIRWISE_KS = (5, 10, 20, 30, 40, 50, 60, 70)      # the x-axis of the reference's figure (P/embeddingEvaluation_tract.py:789-792)


def _as_vectors(rows, device=0):
    """an engine.Vectors as it is (owned = False), host rows [n x dim] as a new one"""
    from .engine import Vectors
    if isinstance(rows, Vectors):
        return rows, False
    return Vectors.from_host(rows, device=device), True


def pairwise_eval(features, gnd, row_of, ks=PAIRWISE_KS, rel_m=0, test=None, want_rows=False, want_lists=False, device=0):
    """The reference's per-slice pairwise figure (evalute_by_pairwise_similarity, P/embeddingEvaluation_tract.py:285-367) as the rule of include/dge.h
    (dge_pairwise_eval_vectors), one call per method: features [V x D] and gnd [n x g] are engine.Vectors or host rows; row_of int64 [n_sets x n] (or [n]: one
    set) names the feature row of every region in every set (slice), -1 = the set lacks the region (slice_rows / region_rows make it from names).
    -> dict(ndcg [n_sets x n_k]; precision, the same shape, None with rel_m = 0; members, tested [n_sets]; coverage = members / n; ks; info; with want_rows
    ratio float64, hits int32 [n_sets x n_k x n] and ideal [n_k x n]; with want_lists lists int32 [n_sets x n x kmax], -1 rows for non-members)."""
    made = []                                     # the resident rows this call uploads: closed on every way out, a failed second upload included
    try:
        f, own = _as_vectors(features, device)
        if own:
            made.append(f)
        g, own = _as_vectors(gnd, device)
        if own:
            made.append(g)
        return f.pairwise_eval(g, row_of, ks=ks, rel_m=rel_m, test=test, want_rows=want_rows, want_lists=want_lists)
    finally:
        for v in made:
            v.close()


def pairwise_ground(gnd, m, device=0):
    """The ground's own m <= 128 nearest regions of every region by the rule's keys (dge_pairwise_ground_vectors): generatePairWiseGT's lists (:63-103) as far as a
    list goes.  -> (idx int32 [n x m], dist float64 [n x m])."""
    g, own = _as_vectors(gnd, device)
    try:
        return g.pairwise_ground(m)
    finally:
        if own:
            g.close()


def _region_index(region_ids):
    ids = [int(r) for r in region_ids]
    index = {r: i for i, r in enumerate(ids)}
    if len(index) != len(ids):
        raise ValueError("region_ids holds an id twice")
    return index


def _text(name):
    return name.decode("utf-8", "replace") if isinstance(name, (bytes, bytearray)) else str(name)


def slice_rows(names, region_ids, n_slices):
    """The rows of a cross-interval embedding by slice, as retrieveCrossIntervalEmbeddings reads its names (P/embeddingEvaluation_tract.py:149-160): names[i],
    "h-id", is the name of feature row i (a Names, or any sequence of str / bytes); region_ids: the n regions in ground order.  A name of a slice outside
    0 .. n_slices-1 or of a region that is not in region_ids is ignored and counted, as is the later row of a name that comes twice; a name that is not two
    integers around one "-" is a ValueError.  -> (row_of int64 [n_slices x n], -1 = no row; dict(foreign, unknown, duplicates))."""
    index = _region_index(region_ids)
    n_slices = int(n_slices)
    row_of = np.full((max(n_slices, 0), len(index)), -1, np.int64)
    counts = dict(foreign=0, unknown=0, duplicates=0)
    for i, name in enumerate(names):
        parts = _text(name).split("-")
        try:
            if len(parts) != 2:
                raise ValueError
            h, rid = int(parts[0]), int(parts[1])
        except ValueError:
            raise ValueError("row %d: %r is not a name of the form h-id" % (i, name)) from None
        if not 0 <= h < n_slices:
            counts["foreign"] += 1
        elif rid not in index:
            counts["unknown"] += 1
        elif row_of[h, index[rid]] >= 0:
            counts["duplicates"] += 1
        else:
            row_of[h, index[rid]] = i
    return row_of, counts


def region_rows(names, region_ids):
    """slice_rows for an embedding whose names are plain region ids, one set: the taxi-all.vec column of the reference (:352-355).
    -> (row_of int64 [1 x n]; dict(unknown, duplicates))."""
    index = _region_index(region_ids)
    row_of = np.full((1, len(index)), -1, np.int64)
    counts = dict(unknown=0, duplicates=0)
    for i, name in enumerate(names):
        try:
            rid = int(_text(name))
        except ValueError:
            raise ValueError("row %d: %r is not a region id" % (i, name)) from None
        if rid not in index:
            counts["unknown"] += 1
        elif row_of[0, index[rid]] >= 0:
            counts["duplicates"] += 1
        else:
            row_of[0, index[rid]] = i
    return row_of, counts
