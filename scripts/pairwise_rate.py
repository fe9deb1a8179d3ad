"""Wall time of one per-slice pairwise evaluation on the device (include/dge.h: dge_pairwise_eval_vectors) at the reference's size — the 801 tracts of
tests/golden/poi_tract_counts.npy, 24 sets, the figure's eight k, rel_m = 300 — and at the size of a cfg3 slice — 41 667 generated regions, g = 10, D = 128,
24 sets — next to the numpy reading of tests/pairwise_ref.py at the reference's size only (its distance matrix alone is 14 GB at the other).

    python scripts/pairwise_rate.py [--regions 41667] [--dim 128] [--sets 24] [--out profiles/pairwise.txt]

Every leg is a process of its own (this file with --leg), under its own time limit:
  device   both tables resident (Vectors.from_host) once, then Vectors.pairwise_eval: a warm-up call and three more; the median wall time and the call's
           knn_ms, ground_ms, score_ms, and ground_ms of one more call with rel_m = 0 (no rank pass);
  numpy    pairwise_ref.evaluate on the lists the device leg's features imply (tests/knn_ref.py), once; the lists' time apart.
At the reference's size the device's ndcg and precision are compared with the reading's as a checksum, and that is reported.  No time and no ratio is promised.
The script stops at the first leg that dies, hangs or fails, with what it has written: nothing more is started on a device that a leg has just failed on.
Numbers from one run on one device, not a distribution."""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REL_M = 300


def tables(regions, dim, sets):
    """regions == 801: the fixture's counts and lattice features (the lists are then exact); else generated counts and Gaussian features.  Every set drops
    about a tenth of the regions; the sets' rows are shuffled into one table."""
    import numpy as np
    import knn_ref
    import pairwise_ref as ref
    rng = np.random.default_rng(20261020)
    if regions == 801:
        gnd = ref.fixture()[1]
    else:
        gnd = rng.poisson(rng.gamma(1.0, 8.0, (regions, 1)) * rng.dirichlet(np.ones(10), regions)).astype(np.float32)
    V = sets * regions
    features = knn_ref.lattice(V, dim, seed=3) if regions == 801 else rng.standard_normal((V, dim), np.float32)
    rows = rng.permutation(V)
    row_of = np.full((sets, regions), -1, np.int64)
    for s in range(sets):
        keep = rng.random(regions) >= 0.1
        row_of[s, keep] = rows[s * regions:(s + 1) * regions][keep]
    return gnd, features, row_of


def digest(r):
    import numpy as np
    h = hashlib.sha1()
    for f in ("ndcg", "precision"):
        h.update(np.ascontiguousarray(r[f], np.float64).tobytes())
    return h.hexdigest()[:16]


def leg_device(a):
    import embedding_amd as E
    gnd, features, row_of = tables(a.regions, a.dim, a.sets)
    F = E.Vectors.from_host(features); G = E.Vectors.from_host(gnd)
    times, r = [], None
    for i in range(4):
        t = time.perf_counter()
        r = F.pairwise_eval(G, row_of, rel_m=REL_M)
        if i:
            times.append(time.perf_counter() - t)
    inf = r["info"]
    ideal_ms = F.pairwise_eval(G, row_of, rel_m=0)["info"]["ground_ms"]          # without precision there is no rank pass: the norms and the ideal pass alone
    print("seconds %.6f knn_ms %.3f ground_ms %.3f ideal_ms %.3f score_ms %.3f members %d tested %d threshold_keys %d ndcg_at_70 %.6f precision_at_70 %.6f bits %s"
          % (statistics.median(times), inf["knn_ms"], inf["ground_ms"], ideal_ms, inf["score_ms"], inf["members"], inf["tested"], inf["threshold_keys"],
             float(r["ndcg"][:, -1].mean()), float(r["precision"][:, -1].mean()), digest(r)))


def leg_numpy(a):
    import pairwise_ref as ref
    gnd, features, row_of = tables(a.regions, a.dim, a.sets)
    t = time.perf_counter()
    lists, _ = ref.estimated_lists(features, row_of, None, 70)
    t_lists = time.perf_counter() - t
    t = time.perf_counter()
    r = ref.evaluate(gnd, lists, None, ref.PAPER_KS, REL_M)
    print("seconds %.6f lists_seconds %.6f bits %s" % (time.perf_counter() - t, t_lists, digest(r)))


def run_leg(a, kind, regions, dim):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", kind, "--regions", str(regions), "--dim", str(dim), "--sets", str(a.sets)]
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
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--sets", type=int, default=24)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairwise.txt"))
    ap.add_argument("--leg", choices=("device", "numpy"))
    a = ap.parse_args()
    if a.leg:
        {"device": leg_device, "numpy": leg_numpy}[a.leg](a)
        return
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    def finish(code):
        open(a.out, "w").write("\n".join(lines) + "\n")
        sys.exit(code)

    say("# scripts/pairwise_rate.py: wall seconds of one pairwise evaluation of %d sets at k = 5 .. 70 with rel_m = %d, both tables resident (device) or in host "
        "memory (numpy); one run on one device" % (a.sets, REL_M))
    code = 0
    for regions, dim, host in ((801, 20, True), (a.regions, a.dim, False)):
        say("## %d regions, ground rows of 10 counts, feature rows of %d floats, %d sets" % (regions, dim, a.sets))
        ok, dev = run_leg(a, "device", regions, dim)
        if not ok:
            say("device   STOPPED, no further leg was started: %s" % dev)
            finish(1)
        say("device   Vectors.pairwise_eval  %s s (median of 3 after a warm-up), knn_ms %s (the strip kernels of all sets), ground_ms %s (norms, ideal and rank passes; %s in a call with rel_m = 0, which has no rank pass), score_ms %s, "
            "%s members and %s tested regions over the sets, %s threshold slots a region, mean nDCG@70 %s, mean precision@70 %s, bits %s"
            % (dev["seconds"], dev["knn_ms"], dev["ground_ms"], dev["ideal_ms"], dev["score_ms"], dev["members"], dev["tested"], dev["threshold_keys"], dev["ndcg_at_70"],
               dev["precision_at_70"], dev["bits"]))
        if host:
            ok, r = run_leg(a, "numpy", regions, dim)
            if not ok:
                say("numpy    STOPPED: %s" % r)
                finish(1)
            same = r["bits"] == dev["bits"]
            say("numpy    pairwise_ref.evaluate  %s s (once; the lists by tests/knn_ref.py before it: %s s), bits %s" % (r["seconds"], r["lists_seconds"], r["bits"]))
            say("# the device's ndcg and precision %s the numpy reading's, bit for bit" % ("ARE" if same else "ARE NOT"))
            code = code or (0 if same else 1)
        else:
            say("numpy    not run at this size (the distance matrix alone is %.1f GB)" % (regions * regions * 8 / 1e9))
    finish(code)


if __name__ == "__main__":
    main()
