"""Wall time of one 10-fold, 12-label SVM cross-validation on the device (include/dge.h: dge_svm_cv_vectors) at 801 x 20, at 6 000 x 128 (the solver's state
in global memory and several launches, still cheap for the host leg, so the bits are compared there) and at the shape of one cfg3 slice —
41 667 x 128 generated rows, inside the limit of 65 536 used rows; the kernel matrix is 13.9 GB there — next to the one-thread host solver of csrc/svm_rule.h
(svm_kernel_host, svm_solve_host, sv_decide through tests/native/svm_rule_harness.cpp), which runs the same rule one element after another, and, where it is
importable, next to scikit-learn's SVC on the same folds, each leg by its own rule.

    python scripts/svm_rate.py [--rows 41667] [--mid-rows 6000] [--dim 128] [--labels 12] [--folds 10] [--big-host] [--out profiles/svm.txt]

Every leg is a process of its own (this file with --leg), under its own time limit:
  device   Vectors.from_host once, then Vectors.svm_cv: a warm-up call and three more; the median wall time and the call's kernel_ms, iterations, launches;
  host     the host solver on the same table, once, one thread (at the large shape only with --big-host: its kernel matrix alone is 2e11 chain steps);
  sklearn  cross_val_score's work: SVC(C, gamma, tol=eps).fit on every fold's training rows, .predict on its test rows, one process.
The device's counts and decision values are compared with the host's as a checksum, and that is reported.  No time and no ratio is promised.  The script stops
at the first leg that dies, hangs or fails, with what it has written: nothing more is started on a device that a leg has just failed on.  Numbers from one run
on one device, not a distribution."""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
EPS = 1e-3


def table(rows, dim, labels, folds):
    import numpy as np
    rng = np.random.default_rng(20261019)
    X = rng.standard_normal((rows, dim), np.float32)
    W = rng.standard_normal((dim, labels))
    score = X.astype(np.float64) @ W + 0.5 * np.sqrt(dim) * rng.standard_normal((rows, labels))      # overlapping classes: labels from a noisy linear score
    Y = np.ascontiguousarray((score > np.median(score, axis=0)).T.astype(np.uint8))
    from embedding_amd.evaluate import stratified_folds
    return X, Y, stratified_folds(Y[0], folds)


def digest(r):
    import numpy as np
    h = hashlib.sha1()
    for f, t in (("correct", np.int64), ("iterations", np.int64), ("support", np.int64), ("converged", np.int64), ("decision", np.float64)):
        h.update(np.ascontiguousarray(r[f], t).tobytes())
    return h.hexdigest()[:16]


def leg_device(a):
    import embedding_amd as E
    X, Y, fold = table(a.rows, a.dim, a.labels, a.folds)
    v = E.Vectors.from_host(X)
    times, r = [], None
    for i in range(4):
        t = time.perf_counter()
        r = v.svm_cv(Y, fold, a.folds, eps=EPS, want_decision=True)
        if i:
            times.append(time.perf_counter() - t)
    inf = r["info"]
    print("seconds %.6f kernel_ms %.3f problems %d iterations %d max_iterations %d not_converged %d support %d launches %d kernel_bytes %d mean %.6f bits %s"
          % (statistics.median(times), inf["kernel_ms"], inf["problems"], inf["iterations"], inf["max_iterations"], inf["not_converged"], inf["support"], inf["launches"],
             inf["kernel_bytes"], float(r["mean"].mean()), digest(r)))


def leg_host(a):
    import numpy as np
    from svm_harness import harness_decide, harness_kernel, harness_solve, load_harness
    X, Y, fold = table(a.rows, a.dim, a.labels, a.folds)
    L, F, n = a.labels, a.folds, a.rows
    r = dict(correct=np.zeros((L, F), np.int64), iterations=np.zeros((L, F), np.int64), support=np.zeros((L, F), np.int64), converged=np.zeros((L, F), np.int64),
             decision=np.full((L, n), np.nan))
    with tempfile.TemporaryDirectory() as d:
        H = load_harness(os.path.join(d, "libsvm_rule_harness.so"), "-O3")
        t = time.perf_counter()
        K = harness_kernel(H, X, 1.0 / a.dim)
        for l in range(L):
            for f in range(F):
                test = fold == f
                s = harness_solve(H, K, np.where(test, 0, np.where(Y[l] != 0, 1, -1)), 1.0, EPS)
                r["iterations"][l, f] = s["iterations"]; r["support"][l, f] = s["support"]; r["converged"][l, f] = s["converged"]
                if test.any():
                    fx = harness_decide(H, K[test], s["coef"], s["bias"])
                    r["decision"][l, test] = fx
                    r["correct"][l, f] = int(((fx > 0.0) == (Y[l, test] != 0)).sum())
        dt = time.perf_counter() - t
    print("seconds %.6f iterations %d support %d bits %s" % (dt, r["iterations"].sum(), r["support"].sum(), digest(r)))


def leg_sklearn(a):
    import numpy as np
    from sklearn import svm
    X, Y, fold = table(a.rows, a.dim, a.labels, a.folds)
    Xd = X.astype(np.float64)
    t = time.perf_counter()
    acc = []
    for l in range(a.labels):
        for f in range(a.folds):
            test = fold == f
            m = svm.SVC(C=1.0, kernel="rbf", gamma=1.0 / a.dim, tol=EPS).fit(Xd[~test], Y[l, ~test])
            acc.append(float((m.predict(Xd[test]) == Y[l, test]).mean()))
    print("seconds %.6f mean %.6f" % (time.perf_counter() - t, float(np.mean(acc))))


def run_leg(a, kind, rows, dim):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", kind, "--rows", str(rows), "--dim", str(dim), "--labels", str(a.labels), "--folds", str(a.folds)]
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
    ap.add_argument("--mid-rows", type=int, default=6000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--labels", type=int, default=12)
    ap.add_argument("--folds", type=int, default=10)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--big-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svm.txt"))
    ap.add_argument("--leg", choices=("device", "host", "sklearn"))
    a = ap.parse_args()
    if a.leg:
        {"device": leg_device, "host": leg_host, "sklearn": leg_sklearn}[a.leg](a)
        return
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    def finish(code):
        open(a.out, "w").write("\n".join(lines) + "\n")
        sys.exit(code)

    try:
        import sklearn  # noqa: F401
        have_sklearn = True
    except ImportError:
        have_sklearn = False
    say("# scripts/svm_rate.py: wall seconds of one %d-fold cross-validation of %d label columns (RBF C-SVC, C 1, gamma 1 / dim, eps %g): rows resident (device) or in "
        "host memory (host, sklearn); one run on one device" % (a.folds, a.labels, EPS))
    code = 0
    # the middle shape is the largest at which the host leg is cheap: above the rows that fit in LDS, so the state is in global memory, and several launches long
    for rows, dim, host, other in ((801, 20, True, True), (a.mid_rows, a.dim, True, False), (a.rows, a.dim, a.big_host, a.big_host)):
        say("## %d x %d float32 rows" % (rows, dim))
        ok, dev = run_leg(a, "device", rows, dim)
        if not ok:
            say("device   STOPPED, no further leg was started: %s" % dev)
            finish(1)
        say("device   Vectors.svm_cv  %s s (median of 3 after a warm-up), kernel_ms %s, %s problems, %s iterations in all (the longest %s), %s not converged, %s support rows, "
            "%s launches, kernel matrix %s bytes, mean accuracy %s, bits %s" % (dev["seconds"], dev["kernel_ms"], dev["problems"], dev["iterations"], dev["max_iterations"],
                                                                               dev["not_converged"], dev["support"], dev["launches"], dev["kernel_bytes"], dev["mean"], dev["bits"]))
        if host:
            ok, r = run_leg(a, "host", rows, dim)
            if not ok:
                say("host     STOPPED: %s" % r)
                finish(1)
            same = r["bits"] == dev["bits"]
            say("host     svm_kernel_host + svm_solve_host + sv_decide, one thread  %s s (once), %s iterations, %s support rows, bits %s" % (r["seconds"], r["iterations"], r["support"], r["bits"]))
            say("# the device's counts and decision values %s the host solver's, bit for bit" % ("ARE" if same else "ARE NOT"))
            code = code or (0 if same else 1)
        else:
            say("host     not run at this shape (--big-host runs it)")
        if have_sklearn and other:
            ok, r = run_leg(a, "sklearn", rows, dim)
            say("sklearn  SVC by its own rule (libsvm: shrinking, a cache, its own exp), one process  %s" % ("%s s (once), mean accuracy %s" % (r["seconds"], r["mean"]) if ok else "STOPPED: %s" % r))
        else:
            say("sklearn  not run at this shape" if have_sklearn else "sklearn  not importable here")
    finish(code)


if __name__ == "__main__":
    main()
