"""Wall time of k-means on the device (include/dge.h: dge_kmeans_vectors) on a table of the size of the metric's (1 000 008 x 128), next to a CPU k-means.

    python scripts/kmeans_rate.py [--rows 1000008] [--dim 128] [--ks 4,64] [--n-init 1] [--max-iter 20] [--out profiles/kmeans.txt]

Every leg is a process of its own (this file with --leg), under its own time limit:
  device  Vectors.from_host once, then Vectors.kmeans: a warm-up call and three more; the median wall time, the call's kernel_ms and its pass count;
  cpu     scikit-learn's KMeans (init="k-means++", algorithm="lloyd", tol=0, the same n_init and max_iter) where it is importable, else a numpy Lloyd loop
          on one thread started from the first k rows; once.
The two do not run the same number of passes (their seedings differ), so the seconds divided by the assignment passes are reported next to the totals
(the seeding's time is inside the seconds of both).  The legs run in the
order device, cpu for each k; the script stops at the first leg that dies, hangs or fails, with what it has written: nothing more is started on a device
that a leg has just failed on.  Numbers from one run on one device, not a distribution."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def table(rows, dim, k):
    import numpy as np
    rng = np.random.default_rng(20261018)
    mu = rng.uniform(-1.0, 1.0, (max(k, 8), dim)).astype(np.float32)
    X = np.empty((rows, dim), np.float32)
    for lo in range(0, rows, 65536):
        hi = min(rows, lo + 65536)
        X[lo:hi] = mu[rng.integers(0, len(mu), hi - lo)] + 0.5 * rng.standard_normal((hi - lo, dim), np.float32)
    return X


def leg_device(a, k):
    import embedding_amd as E
    X = table(a.rows, a.dim, k)
    v = E.Vectors.from_host(X)
    times, info = [], None
    for i in range(4):
        t = time.perf_counter()
        _, _, info = v.kmeans(k, seed=1, n_init=a.n_init, max_iter=a.max_iter)
        if i:
            times.append(time.perf_counter() - t)
    print("seconds %.6f kernel_ms %.3f passes %d inertia %.9g" % (statistics.median(times), info["kernel_ms"], info["total_iterations"], info["inertia"]))


def leg_cpu(a, k):
    import numpy as np
    X = table(a.rows, a.dim, k)
    try:
        from sklearn.cluster import KMeans
    except ImportError:
        KMeans = None
    t = time.perf_counter()
    if KMeans is not None:
        km = KMeans(n_clusters=k, init="k-means++", n_init=a.n_init, max_iter=a.max_iter, tol=0.0, algorithm="lloyd", random_state=1).fit(X)
        what, passes, inertia = "scikit-learn", int(km.n_iter_) * a.n_init, float(km.inertia_)
    else:
        C = X[:k].astype(np.float64)
        labels = np.full(len(X), -1)
        passes = 0
        while passes < a.max_iter:
            d = (X.astype(np.float64) ** 2).sum(1)[:, None] - 2.0 * X @ C.T + (C ** 2).sum(1)[None]
            new = d.argmin(1)
            passes += 1
            if (new == labels).all():
                break
            labels = new
            for c in range(k):
                if (labels == c).any():
                    C[c] = X[labels == c].mean(0)
        what, inertia = "numpy Lloyd", float(d.min(1).sum())
    print("seconds %.6f what %s passes %d inertia %.9g" % (time.perf_counter() - t, what.replace(" ", "_"), passes, inertia))


def run_leg(a, kind, k):
    """-> (True, fields) | (False, message)"""
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", kind, "--k", str(k), "--rows", str(a.rows), "--dim", str(a.dim), "--n-init", str(a.n_init),
           "--max-iter", str(a.max_iter)]
    env = dict(os.environ)
    if kind == "cpu":
        import importlib.util
        if importlib.util.find_spec("sklearn") is None:      # the numpy loop is the one-thread baseline
            env.update(OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit, env=env)
    except subprocess.TimeoutExpired:
        return False, "ran past %d s" % a.limit
    line = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    if out.returncode != 0 or not line.startswith("seconds "):
        return False, "exit status %d: %s" % (out.returncode, line or out.stderr.strip()[-300:])
    f = line.split()
    return True, dict(zip(f[0::2], f[1::2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000008)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--ks", default="4,64")
    ap.add_argument("--n-init", type=int, default=1)
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--limit", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans.txt"))
    ap.add_argument("--leg", choices=("device", "cpu"))
    ap.add_argument("--k", type=int, default=4)
    a = ap.parse_args()
    if a.leg:
        (leg_device if a.leg == "device" else leg_cpu)(a, a.k)
        return
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    def finish(code):
        open(a.out, "w").write("\n".join(lines) + "\n")
        sys.exit(code)

    say("# scripts/kmeans_rate.py: %d x %d float32, n_init = %d, max_iter = %d; wall seconds of one clustering, rows resident (device) or in host memory (cpu); one run on one device"
        % (a.rows, a.dim, a.n_init, a.max_iter))
    for k in [int(x) for x in a.ks.split(",")]:
        ok, dev = run_leg(a, "device", k)
        if not ok:
            say("k %2d  device  STOPPED, no further leg was started: %s" % (k, dev))
            finish(1)
        say("k %2d  device  Vectors.kmeans  %s s (median of 3 after a warm-up), kernel_ms %s, %s passes, %.6f s a pass, inertia %s"
            % (k, dev["seconds"], dev["kernel_ms"], dev["passes"], float(dev["seconds"]) / int(dev["passes"]), dev["inertia"]))
        ok, cpu = run_leg(a, "cpu", k)
        if not ok:
            say("k %2d  cpu  STOPPED, no further leg was started: %s" % (k, cpu))
            finish(1)
        say("k %2d  cpu     %s  %s s (once), %s passes, %.6f s a pass, inertia %s"
            % (k, cpu["what"], cpu["seconds"], cpu["passes"], float(cpu["seconds"]) / max(int(cpu["passes"]), 1), cpu["inertia"]))
    finish(0)


if __name__ == "__main__":
    main()
