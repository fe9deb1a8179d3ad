"""Wall time of one NMF on the device (include/dge.h: dge_nmf_coo) on a matrix of the shape of one cfg3 slice (41 667 x 41 667, about 4.2 million entries), next
to scikit-learn's multiplicative-update solver on the same entries.

    python scripts/nmf_rate.py [--regions 41667] [--entries 4200000] [--rank 10] [--max-iter 30] [--updates divergence,euclidean] [--out profiles/nmf.txt]

Every leg is a process of its own (this file with --leg), under its own time limit:
  device  evaluate.nmf_gpu: a warm-up call and three more; the median wall time (upload, the two sorts, max_iter iterations, the objective, read-back) and the
          call's kernel_ms;
  cpu     scikit-learn's NMF(solver="mu", beta_loss="kullback-leibler" or "frobenius", init="random", tol=0, the same rank and max_iter) on the scipy CSR
          matrix, once; without scikit-learn the leg says so and the script goes on.
Each leg runs its own rule (the initial factors and the order of the two updates differ), so the seconds are times of a factorisation each, not of the same
arithmetic.  These are memory-bound sparse passes; the script reports seconds and promises no rate.  It stops at the first device leg that dies, hangs or
fails, with what it has written: nothing more is started on a device that a leg has just failed on.  Numbers from one run on one device, not a distribution."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def matrix(regions, entries):
    """flows as a slice has them: a few hub regions take a large share of the trips, integer weights"""
    import numpy as np
    rng = np.random.default_rng(20261018)
    p = 1.0 / np.arange(1, regions + 1) ** 0.8                # region popularity: a Zipf law over a shuffled order
    p = rng.permutation(p / p.sum())
    cells = np.zeros(0, np.int64)
    while len(cells) < entries:                              # distinct (source, destination) pairs of trips drawn by popularity
        draw = rng.choice(regions, 2 * (entries - len(cells)) + 1024, p=p).astype(np.int64)
        cells = np.union1d(cells, draw[0::2] * regions + draw[1::2])
    cells = rng.permutation(cells)[:entries]
    rng.shuffle(cells)
    return (cells // regions).astype(np.int32), (cells % regions).astype(np.int32), rng.geometric(0.3, len(cells)).astype(np.float64)


def leg_device(a, update):
    import embedding_amd.evaluate as ev
    r, c, v = matrix(a.regions, a.entries)
    times, info = [], None
    for i in range(4):
        t = time.perf_counter()
        _, _, info = ev.nmf_gpu(r, c, v, (a.regions, a.regions), rank=a.rank, max_iter=a.max_iter, update=update, seed=1)
        if i:
            times.append(time.perf_counter() - t)
    print("seconds %.6f kernel_ms %.3f entries %d objective %.9g" % (statistics.median(times), info["kernel_ms"], info["entries"], info["objective"]))


def leg_cpu(a, update):
    try:
        import scipy.sparse as sp
        from sklearn.decomposition import NMF
    except ImportError as e:
        print("seconds nan what missing:%s entries 0 objective nan" % e.name)
        return
    r, c, v = matrix(a.regions, a.entries)
    V = sp.csr_matrix((v, (r, c)), shape=(a.regions, a.regions))
    t = time.perf_counter()
    model = NMF(n_components=a.rank, init="random", solver="mu", beta_loss="kullback-leibler" if update == "divergence" else "frobenius", max_iter=a.max_iter, tol=0.0, random_state=1)
    model.fit(V)
    print("seconds %.6f what scikit-learn_mu entries %d objective %.9g" % (time.perf_counter() - t, V.nnz, model.reconstruction_err_))


def run_leg(a, kind, update):
    """-> (True, fields) | (False, message)"""
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", kind, "--update", update, "--regions", str(a.regions), "--entries", str(a.entries), "--rank", str(a.rank),
           "--max-iter", str(a.max_iter)]
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
    ap.add_argument("--regions", type=int, default=41667)
    ap.add_argument("--entries", type=int, default=4200000)
    ap.add_argument("--rank", type=int, default=10)
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--updates", default="divergence,euclidean")
    ap.add_argument("--limit", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nmf.txt"))
    ap.add_argument("--leg", choices=("device", "cpu"))
    ap.add_argument("--update", default="divergence")
    a = ap.parse_args()
    if a.leg:
        (leg_device if a.leg == "device" else leg_cpu)(a, a.update)
        return
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    def finish(code):
        open(a.out, "w").write("\n".join(lines) + "\n")
        sys.exit(code)

    say("# scripts/nmf_rate.py: %d x %d, %d entries asked for, rank %d, max_iter %d; wall seconds of one factorisation from entries in host memory; one run on one device"
        % (a.regions, a.regions, a.entries, a.rank, a.max_iter))
    for update in a.updates.split(","):
        ok, dev = run_leg(a, "device", update)
        if not ok:
            say("%-10s device  STOPPED, no further leg was started: %s" % (update, dev))
            finish(1)
        say("%-10s device  evaluate.nmf_gpu  %s s (median of 3 after a warm-up), kernel_ms %s, %s entries, objective %s" % (update, dev["seconds"], dev["kernel_ms"], dev["entries"], dev["objective"]))
        ok, cpu = run_leg(a, "cpu", update)
        if not ok:
            say("%-10s cpu     did not finish: %s" % (update, cpu))
        else:
            say("%-10s cpu     %s  %s s (once), %s entries, its own reconstruction error %s" % (update, cpu["what"], cpu["seconds"], cpu["entries"], cpu["objective"]))
    finish(0)


if __name__ == "__main__":
    main()
