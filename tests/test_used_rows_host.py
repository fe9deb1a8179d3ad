"""embedding_amd/csrc/used_rows.h on the host: the one intake of k-means, the tree, ridge and the SVM — which rows of a table are used, the first offence of the
walk, the gathers and the way back — against the selection rule restated below.  tests/native/used_rows_harness.cpp, built with g++ and bound through ctypes; no
device."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "used_rows_harness.cpp")
ROWS = 37
NONE, FOLD, LABEL, TARGET = 0, 1, 2, 3


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("used_rows") / "used_rows_harness.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-Wall", "-ffp-contract=off", "-o", so, SRC])
    H = C.CDLL(so)
    H.harness_used_rows.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 10
    H.harness_used_rows.restype = None
    H.harness_outside.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p]
    return H


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def reference(rows, present, select, fold, n_folds):
    """the selection rule: a row is used iff it is present, and select is absent or non-zero, and fold is absent or >= 0"""
    use = np.ones(rows, bool)
    if present is not None:
        use &= present != 0
    if select is not None:
        use &= select != 0
    if fold is not None:
        use &= fold >= 0
    used = np.flatnonzero(use)
    fu = fold[used] if fold is not None else np.full(len(used), -1, np.int32)
    tested = np.bincount(fu, minlength=n_folds)[:n_folds] if fold is not None else np.zeros(0, np.int64)
    return used, len(used) == rows, fu, tested


def intake(H, rows, present=None, select=None, fold=None, n_folds=0, labels=None, targets=None):
    """-> dict of everything the header gives; the values that go back are 100 + t (int32) and t + 0.5 (float64) for the t-th used row"""
    L = 0 if labels is None else labels.shape[0]
    T = 0 if targets is None else targets.shape[1]
    used = np.full(rows, -7, np.int64); fo = np.full(rows, -7, np.int32); tested = np.zeros(max(n_folds, 1), np.int64); meta = np.zeros(6, np.int64)
    yu = np.zeros(max(L * rows, 1), np.uint8); tu = np.zeros(max(rows * T, 1), np.float64)
    vd = np.arange(rows) + 0.5; od = np.full(rows, 9.0); vi = (100 + np.arange(rows)).astype(np.int32); oi = np.full(rows, 9, np.int32)
    H.harness_used_rows(rows, _p(present), _p(select), _p(fold), n_folds, _p(labels), L, _p(targets), T, _p(used), _p(fo), _p(tested), _p(meta), _p(yu), _p(tu), _p(vd), _p(od), _p(vi), _p(oi))
    n = int(meta[0])
    return dict(n=n, all=bool(meta[1]), kind=int(meta[2]), bad_row=int(meta[3]), bad_col=int(meta[4]), bad_value=int(meta[5]), used=used[:n], fold=fo[:n],
                tested=tested[:n_folds] if fold is not None else tested[:0], yu=yu[:L * n].reshape(L, n), tu=tu[:n * T].reshape(n, T), out_d=od, out_i=oi)


def masks(kind):
    """the rows a mask leaves out: none, one in the middle, the first, the last, every row"""
    keep = np.ones(ROWS, bool)
    if kind == "one":
        keep[17] = False
    elif kind == "first":
        keep[0] = False
    elif kind == "last":
        keep[ROWS - 1] = False
    elif kind == "every":
        keep[:] = False
    return keep


@pytest.mark.parametrize("n_folds", [1, 3])
@pytest.mark.parametrize("drop", ["none", "one", "first", "last", "every"])
def test_the_used_rows_the_gathers_and_the_way_back_are_the_rules(harness, drop, n_folds):
    rng = np.random.default_rng(5 + n_folds)
    keep = masks(drop)
    labels3 = rng.integers(0, 2, (3, ROWS)).astype(np.uint8)
    targets = np.ascontiguousarray(rng.integers(-50, 50, (ROWS, 2)) / 4.0)
    for with_p, with_s, with_f in itertools.product([False, True], repeat=3):
        # each array that is given leaves out the mask's rows; with all three, each a different rotation of them, so that the three conditions are told apart
        present = np.roll(keep, 0).astype(np.uint8) if with_p else None
        select = (np.roll(keep, 5) * 3).astype(np.uint8) if with_s else None             # any non-zero value selects
        fold = np.where(np.roll(keep, 11), rng.integers(0, n_folds, ROWS), -1).astype(np.int32) if with_f else None
        used, all_, fu, tested = reference(ROWS, present, select, fold, n_folds)
        for labels in (labels3[:1], labels3):
            got = intake(harness, ROWS, present, select, fold, n_folds if with_f else 0, np.ascontiguousarray(labels), targets)
            assert got["kind"] == NONE and got["n"] == len(used) and got["all"] == all_
            assert (got["used"] == used).all() and (got["fold"] == fu).all() and (got["tested"] == tested).all()
            assert (got["yu"] == labels[:, used]).all() and (got["tu"] == targets[used]).all()
            want_i = np.full(ROWS, -1, np.int32); want_i[used] = 100 + np.arange(len(used))
            want_d = np.full(ROWS, np.nan); want_d[used] = np.arange(len(used)) + 0.5
            assert (got["out_i"] == want_i).all() and np.array_equal(got["out_d"], want_d, equal_nan=True)
        if not (with_p or with_s or with_f) or drop == "none":
            assert all_                                               # the shortcut of the way back: one copy
    got = intake(harness, ROWS)                                       # nothing to leave a row out and nothing to check: k-means' call on a whole table
    assert got["n"] == ROWS and got["all"] and got["kind"] == NONE and (got["used"] == np.arange(ROWS)).all() and (got["fold"] == -1).all()
    assert (got["out_i"] == 100 + np.arange(ROWS)).all() and (got["out_d"] == np.arange(ROWS) + 0.5).all()


def test_the_first_offence_in_row_order_is_the_one_reported(harness):
    labels = np.zeros((3, ROWS), np.uint8)
    fold = (np.arange(ROWS) % 3).astype(np.int32)
    labels[1, 3] = 2; fold[7] = 3                                     # a bad fold after a bad label
    got = intake(harness, ROWS, fold=fold, n_folds=3, labels=labels)
    assert (got["kind"], got["bad_row"], got["bad_col"], got["bad_value"]) == (LABEL, 3, 1, 2)
    labels[:] = 0; labels[1, 7] = 2; fold[7] = 1; fold[3] = -2        # and the other way round
    got = intake(harness, ROWS, fold=fold, n_folds=3, labels=labels)
    assert (got["kind"], got["bad_row"], got["bad_value"]) == (FOLD, 3, -2)
    fold[3] = 3                                                        # the range's other end, on a row that select leaves out: every row's fold is checked
    select = np.ones(ROWS, np.uint8); select[3] = 0
    got = intake(harness, ROWS, select=select, fold=fold, n_folds=3, labels=labels)
    assert (got["kind"], got["bad_row"], got["bad_value"]) == (FOLD, 3, 3)


def test_a_bad_value_on_a_row_that_is_not_used_is_no_offence(harness):
    labels = np.zeros((2, ROWS), np.uint8); labels[0, 4] = 255; labels[1, 9] = 7; labels[1, 20] = 2
    targets = np.zeros((ROWS, 2)); targets[4, 1] = np.nan; targets[9, 0] = np.inf; targets[20, 0] = -np.inf
    present = np.ones(ROWS, np.uint8); present[4] = 0
    select = np.ones(ROWS, np.uint8); select[9] = 0
    fold = np.zeros(ROWS, np.int32); fold[20] = -1
    got = intake(harness, ROWS, present, select, fold, 1, labels, targets)
    assert got["kind"] == NONE and got["n"] == ROWS - 3
    got = intake(harness, ROWS, present, None, fold, 1, labels, targets)         # row 9 is used now
    assert (got["kind"], got["bad_row"], got["bad_col"], got["bad_value"]) == (LABEL, 9, 1, 7) and got["n"] == ROWS - 2      # the walk goes on: n is the table's
    got = intake(harness, ROWS, present, None, fold, 1, None, targets)
    assert (got["kind"], got["bad_row"], got["bad_col"]) == (TARGET, 9, 0)


def test_the_least_column_of_a_row_with_two_offences(harness):
    labels = np.zeros((3, ROWS), np.uint8); labels[2, 6] = 9; labels[1, 6] = 5; labels[0, 8] = 3
    got = intake(harness, ROWS, labels=labels)
    assert (got["kind"], got["bad_row"], got["bad_col"], got["bad_value"]) == (LABEL, 6, 1, 5)
    targets = np.zeros((ROWS, 2)); targets[6, 1] = np.nan; targets[6, 0] = np.inf
    got = intake(harness, ROWS, targets=targets)
    assert (got["kind"], got["bad_row"], got["bad_col"]) == (TARGET, 6, 0)
    got = intake(harness, ROWS, labels=labels, targets=targets)                  # labels before targets
    assert got["kind"] == LABEL


def test_the_range_check_words_the_refusal(harness):
    msg = C.create_string_buffer(192)
    assert harness.harness_outside(b"dge_svm_cv", b"n_folds", 0, 64, msg) == 1 and msg.value == b"dge_svm_cv: n_folds = 0 is outside 1 .. 64"
    assert harness.harness_outside(b"dge_kmeans", b"dim", 4097, 4096, msg) == 1 and msg.value == b"dge_kmeans: dim = 4097 is outside 1 .. 4096"
    assert harness.harness_outside(b"w", b"dim", 1, 4096, msg) == 0 and harness.harness_outside(b"w", b"dim", 4096, 4096, msg) == 0


def test_the_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "used_rows_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    run = subprocess.run([exe, "40", "7"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert "rounds 40 wrong 0" in run.stdout
