"""Test infrastructure: the decision-tree rule of include/dge.h read out literally in Python — per node, per column: sort, scan, compare — on Python integers
(scores are compared by cross-multiplication, which Python does exactly at any size) and Python floats (binary64; a float32 value converts exactly).  It shares no
code with csrc/tree.hip or csrc/tree_rule.h and is the yardstick of tests/test_gpu_tree.py and tests/test_tree_host.py."""
import math

import numpy as np


def used_rows(n, present=None, select=None):
    return [i for i in range(n) if (present is None or present[i]) and (select is None or select[i])]


def _fit(rows, labels, max_depth, min_samples_split, min_samples_leaf):
    """rows: lists of Python floats, labels: 0 / 1.  -> the five arrays as lists, and the depth."""
    dim = len(rows[0]) if rows else 0
    feature, threshold, left, count, pos = [-1], [0.0], [-1], [len(rows)], [sum(labels)]
    level = [(0, list(range(len(rows))))]
    depth = d = 0
    while level:
        nxt = []
        for node, idx in level:                                   # node order
            n, p = count[node], pos[node]
            if p == 0 or p == n or n < min_samples_split or (max_depth > 0 and d == max_depth):
                continue
            best = None                                           # (N, Dn, f, a, b)
            for f in range(dim):
                col = sorted((rows[i][f], labels[i]) for i in idx)
                pL = 0
                for j in range(n - 1):
                    pL += col[j][1]
                    a, b = col[j][0], col[j + 1][0]
                    if not a < b:
                        continue
                    nL = j + 1
                    nR = n - nL
                    if nL < min_samples_leaf or nR < min_samples_leaf:
                        continue
                    qL, pR = nL - pL, p - pL
                    qR = nR - pR
                    N = (pL * pL + qL * qL) * nR + (pR * pR + qR * qR) * nL
                    Dn = nL * nR
                    if best is None or N * best[1] > best[0] * Dn:      # strictly greater: among equals the first stays, the least f, then the least a
                        best = (N, Dn, f, a, b)
            if best is None:
                continue
            _, _, f, a, b = best
            m = (a + b) * 0.5
            assert a <= m < b
            li = [i for i in idx if rows[i][f] <= m]
            ri = [i for i in idx if not rows[i][f] <= m]
            assert all(rows[i][f] <= a for i in li) and all(rows[i][f] >= b for i in ri)
            feature[node], threshold[node], left[node] = f, m, len(feature)
            for ch in (li, ri):
                nxt.append((len(feature), ch))
                feature.append(-1); threshold.append(0.0); left.append(-1); count.append(len(ch)); pos.append(sum(labels[i] for i in ch))
        if nxt:
            depth = d + 1
        level = nxt
        d += 1
    return feature, threshold, left, count, pos, depth


def _rows(X):
    X = np.asarray(X, np.float32)
    return [[float(v) for v in r] for r in X]


def tree_fit(X, y, present=None, select=None, max_depth=0, min_samples_split=2, min_samples_leaf=1, rows=None):
    """-> dict(feature int32, threshold float64, left int32, count int64, pos int64, n_nodes, depth, rows)"""
    R = _rows(X)
    use = used_rows(len(R), present, select) if rows is None else list(rows)
    y = [int(v) for v in y]
    f, t, l, c, p, depth = _fit([R[i] for i in use], [y[i] for i in use], max_depth, min_samples_split, min_samples_leaf)
    return dict(feature=np.array(f, np.int32), threshold=np.array(t, np.float64), left=np.array(l, np.int32), count=np.array(c, np.int64), pos=np.array(p, np.int64),
                n_nodes=len(f), depth=depth, rows=len(use))


def predict_row(tree, row):
    k = 0
    while tree["feature"][k] >= 0:
        k = int(tree["left"][k]) + (0 if float(row[int(tree["feature"][k])]) <= float(tree["threshold"][k]) else 1)
    return 1 if 2 * int(tree["pos"][k]) > int(tree["count"][k]) else 0


def tree_predict(tree, X, present=None):
    X = np.asarray(X, np.float32)
    out = np.full(len(X), 255, np.uint8)
    for i in range(len(X)):
        if present is None or present[i]:
            out[i] = predict_row(tree, X[i])
    return out


def tree_cv(X, y, fold, n_folds, present=None, **limits):
    """-> dict(correct, tested, n_nodes, depth: int64 / int32 [n_folds]; scores float64, NaN for a fold without test rows; mean over the others)"""
    X = np.asarray(X, np.float32)
    use = [i for i in used_rows(len(X), present) if fold[i] >= 0]
    correct, tested, nodes, depth = [], [], [], []
    for t in range(n_folds):
        train = [i for i in use if fold[i] != t]
        test = [i for i in use if fold[i] == t]
        assert train, "fold %d has no training rows" % t
        tr = tree_fit(X, y, rows=train, **limits)
        correct.append(sum(1 for i in test if predict_row(tr, X[i]) == int(y[i])))
        tested.append(len(test)); nodes.append(tr["n_nodes"]); depth.append(tr["depth"])
    return dict(cv_scores(correct, tested), n_nodes=np.array(nodes, np.int32), depth=np.array(depth, np.int32))


def cv_scores(correct, tested):
    correct = np.array(correct, np.int64); tested = np.array(tested, np.int64)
    scores = np.array([c / t if t else math.nan for c, t in zip(correct.tolist(), tested.tolist())], np.float64)
    ok = scores[~np.isnan(scores)]
    mean = float(ok.mean()) if len(ok) else math.nan              # numpy's mean, as cross_val_score(..).mean() in the reference
    return dict(correct=correct, tested=tested, scores=scores, mean=mean)


def stratified_folds(y, n_folds, select=None):
    """the j-th used row of its class, in row order, gets fold j mod F; a row that is not used gets -1"""
    seen = {}
    out = []
    for i, v in enumerate(y):
        if select is not None and not select[i]:
            out.append(-1)
            continue
        j = seen.get(int(v), 0)
        seen[int(v)] = j + 1
        out.append(j % n_folds)
    return np.array(out, np.int32)


def median_labels_numpy(counts):
    """generatePOIlabel_helper of the reference (P/embeddingEvaluation_tract.py:34-47) as it is written there: np.median and a comparison in binary64"""
    counts = [int(c) for c in counts]
    median = np.median(counts)
    return np.array([1 if val >= median else 0 for val in counts], np.uint8), bool(median >= 1)
