"""Wall time of one cross-validated decision tree on the device (include/dge.h: dge_tree_cv_vectors) at the shape of one cfg3 slice — 41 667 x 128 generated
blobs, labels by evaluate.median_labels of a generated count, 10 folds by evaluate.stratified_folds, default limits — next to scikit-learn's
cross_val_score(DecisionTreeClassifier(), ..., cv=10) where it is importable, each leg by its own rule.

    python scripts/tree_rate.py [--rows 41667] [--dim 128] [--folds 10] [--out profiles/tree.txt]

Every leg is a process of its own (this file with --leg), under its own time limit:
  device    Vectors.from_host once, then Vectors.tree_cv: a warm-up call and three more; the median wall time, the call's kernel_ms, levels, nodes and batches;
  sequence  the same with the trees grown one after another (tuning(tree_batch=1)): the same counts, by the rule;
  cpu       scikit-learn on the same folds (its own tie-breaking and float32 thresholds): once, with n_jobs = the folds on the threads the machine gives.
The closeness of the two mean accuracies and node counts is reported, not asserted: ties are broken differently (include/dge.h, "NOT scikit-learn").  The script
stops at the first leg that dies, hangs or fails, with what it has written: nothing more is started on a device that a leg has just failed on.  Numbers from
one run on one device, not a distribution."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def table(rows, dim, folds):
    import numpy as np
    import embedding_amd.evaluate as ev
    rng = np.random.default_rng(20261019)
    mu = rng.uniform(-1.0, 1.0, (8, dim)).astype(np.float32)
    blob = rng.integers(0, 8, rows)
    X = (mu[blob] + 0.5 * rng.standard_normal((rows, dim), np.float32)).astype(np.float32)
    counts = np.maximum(0, np.rint(4 + 3 * X[:, 0] - 2 * X[:, dim // 2] + (blob % 3) + rng.standard_normal(rows))).astype(np.int64)
    y, _ = ev.median_labels(counts)
    return X, y, ev.stratified_folds(y, folds)


def leg_device(a, batch):
    import embedding_amd as E
    X, y, fold = table(a.rows, a.dim, a.folds)
    v = E.Vectors.from_host(X)
    times, r = [], None
    knobs = dict(tree_batch=batch) if batch else {}
    with E.tuning(**knobs):
        for i in range(4):
            t = time.perf_counter()
            r = v.tree_cv(y, fold, a.folds)
            if i:
                times.append(time.perf_counter() - t)
    print("seconds %.6f kernel_ms %.3f levels %d nodes %d depth %d batches %d mean %.17g correct %d"
          % (statistics.median(times), r["info"]["kernel_ms"], r["info"]["levels"], r["info"]["n_nodes"], r["info"]["depth"], r["info"]["batches"], r["mean"], int(r["correct"].sum())))


def leg_cpu(a):
    import numpy as np
    from sklearn.model_selection import PredefinedSplit, cross_validate
    from sklearn.tree import DecisionTreeClassifier
    X, y, fold = table(a.rows, a.dim, a.folds)
    threads = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    jobs = max(1, min(a.folds, threads, int(os.environ.get("OMP_NUM_THREADS", "16"))))
    t = time.perf_counter()
    r = cross_validate(DecisionTreeClassifier(random_state=0), X, y, cv=PredefinedSplit(fold), n_jobs=jobs, return_estimator=True)
    dt = time.perf_counter() - t
    nodes = sum(e.tree_.node_count for e in r["estimator"]); depth = max(e.tree_.max_depth for e in r["estimator"])
    print("seconds %.6f what scikit-learn_%d_jobs nodes %d depth %d mean %.17g" % (dt, jobs, nodes, depth, float(np.mean(r["test_score"]))))


def run_leg(a, kind):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", kind, "--rows", str(a.rows), "--dim", str(a.dim), "--folds", str(a.folds)]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
    except subprocess.TimeoutExpired:
        return False, "ran past %d s" % a.limit
    line = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    if out.returncode != 0 or not line.startswith("seconds "):
        return False, "exit status %d: %s" % (out.returncode, line or out.stderr.strip()[-300:])
    f = line.split()
    return True, dict(zip(f[0::2], f[1::2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=41667)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--folds", type=int, default=10)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree.txt"))
    ap.add_argument("--leg", choices=("device", "sequence", "cpu"))
    a = ap.parse_args()
    if a.leg:
        if a.leg == "cpu":
            leg_cpu(a)
        else:
            leg_device(a, 1 if a.leg == "sequence" else 0)
        return
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    def finish(code):
        open(a.out, "w").write("\n".join(lines) + "\n")
        sys.exit(code)

    say("# scripts/tree_rate.py: %d x %d float32 blobs, median labels, %d stratified folds, default limits; wall seconds of one cross-validation, rows resident (device) or in "
        "host memory (cpu); one run on one device" % (a.rows, a.dim, a.folds))
    dev = None
    for kind, what in (("device", "Vectors.tree_cv, the trees together"), ("sequence", "Vectors.tree_cv, tree_batch = 1")):
        ok, r = run_leg(a, kind)
        if not ok:
            say("%s  STOPPED, no further leg was started: %s" % (kind, r))
            finish(1)
        say("%-8s  %s  %s s (median of 3 after a warm-up), kernel_ms %s, %s level passes, %s nodes, depth %s, %s batch(es), mean accuracy %s (%s rows right)"
            % (kind, what, r["seconds"], r["kernel_ms"], r["levels"], r["nodes"], r["depth"], r["batches"], r["mean"], r["correct"]))
        if dev is not None and (r["mean"], r["nodes"], r["correct"]) != (dev["mean"], dev["nodes"], dev["correct"]):
            say("sequence  DIFFERS from the trees grown together")
            finish(1)
        dev = dev or r
    import importlib.util
    if importlib.util.find_spec("sklearn") is None:
        say("cpu       scikit-learn is not importable here: no CPU leg, no ratio")
        finish(0)
    ok, r = run_leg(a, "cpu")
    if not ok:
        say("cpu  STOPPED: %s" % r)
        finish(1)
    say("cpu       %s, the same folds, its own tie-breaking  %s s (once), %s nodes, depth %s, mean accuracy %s" % (r["what"], r["seconds"], r["nodes"], r["depth"], r["mean"]))
    say("# mean accuracy %s (rule) against %s (scikit-learn); nodes %s against %s; %.1f x the wall time" % (dev["mean"], r["mean"], dev["nodes"], r["nodes"], float(r["seconds"]) / float(dev["seconds"])))
    finish(0)


if __name__ == "__main__":
    main()
