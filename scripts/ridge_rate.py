"""Wall time of one leave-one-out ridge regression on the device (include/dge.h: dge_ridge_loo_vectors) at the shape of one cfg3 slice — 41 667 x 128 generated
rows, 4 targets, 8 penalties — next to the one-thread host solver of csrc/ridge_rule.h (rg_solve_host through tests/native/ridge_rule_harness.cpp), which runs
the same rule one element after another.

    python scripts/ridge_rate.py [--rows 41667] [--dim 128] [--targets 4] [--lambdas 8] [--out profiles/ridge.txt]

Every leg is a process of its own (this file with --leg), under its own time limit:
  device   Vectors.from_host once, then Vectors.ridge_loo: a warm-up call and three more; the median wall time and the call's kernel_ms, blocks and chunks;
  chunks   the same with the moments taken three blocks at a time (tuning(ridge_chunk=3)): the same bits, by the rule;
  host     rg_solve_host on the same table, once, one thread.
The device's figures are compared with the host's bit for bit, and that is reported.  The useful work is about n x P^2 fused multiply-adds, a fraction of a
millisecond of arithmetic: no rate and no ratio is promised.  The script stops at the first leg that dies, hangs or fails, with what it has written: nothing
more is started on a device that a leg has just failed on.  Numbers from one run on one device, not a distribution."""
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


def table(rows, dim, targets, lambdas):
    import numpy as np
    rng = np.random.default_rng(20261019)
    X = rng.standard_normal((rows, dim), np.float32)
    w = rng.standard_normal((dim, targets))
    Y = 50.0 + X.astype(np.float64) @ w + 3.0 * rng.standard_normal((rows, targets))
    return X, Y, [0.0] + [2.0 ** (k - 3) for k in range(1, lambdas)]


def digest(r):
    import numpy as np
    h = hashlib.sha1()
    for f in ("mae", "mre", "beta", "loo_pred"):
        h.update(np.ascontiguousarray(r[f], np.float64).tobytes())
    return h.hexdigest()[:16]


def leg_device(a, chunk):
    import embedding_amd as E
    X, Y, lam = table(a.rows, a.dim, a.targets, a.lambdas)
    v = E.Vectors.from_host(X)
    times, r = [], None
    with E.tuning(**(dict(ridge_chunk=chunk) if chunk else {})):
        for i in range(4):
            t = time.perf_counter()
            r = v.ridge_loo(Y, lam)
            if i:
                times.append(time.perf_counter() - t)
    print("seconds %.6f kernel_ms %.3f blocks %d chunks %d min_pivot %.6g max_leverage %.6g mae %.17g bits %s"
          % (statistics.median(times), r["info"]["kernel_ms"], r["info"]["blocks"], r["info"]["chunks"], r["info"]["min_pivot"], r["info"]["max_leverage"], r["mae"][0, 0], digest(r)))


def leg_host(a):
    from ridge_harness import harness_ridge, load_harness
    X, Y, lam = table(a.rows, a.dim, a.targets, a.lambdas)
    with tempfile.TemporaryDirectory() as d:
        H = load_harness(os.path.join(d, "libridge_rule_harness.so"))
        t = time.perf_counter()
        r = harness_ridge(H, X, Y, lam)
        dt = time.perf_counter() - t
    print("seconds %.6f mae %.17g bits %s" % (dt, r["mae"][0, 0], digest(r)))


def run_leg(a, kind):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", kind, "--rows", str(a.rows), "--dim", str(a.dim), "--targets", str(a.targets), "--lambdas", str(a.lambdas)]
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
    ap.add_argument("--targets", type=int, default=4)
    ap.add_argument("--lambdas", type=int, default=8)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ridge.txt"))
    ap.add_argument("--leg", choices=("device", "chunks", "host"))
    a = ap.parse_args()
    if a.leg:
        if a.leg == "host":
            leg_host(a)
        else:
            leg_device(a, 3 if a.leg == "chunks" else 0)
        return
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    def finish(code):
        open(a.out, "w").write("\n".join(lines) + "\n")
        sys.exit(code)

    say("# scripts/ridge_rate.py: %d x %d float32 rows, %d targets, %d penalties (0 among them); wall seconds of one leave-one-out ridge regression, rows resident "
        "(device) or in host memory (host); one run on one device" % (a.rows, a.dim, a.targets, a.lambdas))
    dev = None
    for kind, what in (("device", "Vectors.ridge_loo"), ("chunks", "Vectors.ridge_loo, ridge_chunk = 3")):
        ok, r = run_leg(a, kind)
        if not ok:
            say("%s  STOPPED, no further leg was started: %s" % (kind, r))
            finish(1)
        say("%-7s  %s  %s s (median of 3 after a warm-up), kernel_ms %s, %s blocks in %s chunk(s), least pivot %s, greatest leverage %s, mae[0][0] %s, bits %s"
            % (kind, what, r["seconds"], r["kernel_ms"], r["blocks"], r["chunks"], r["min_pivot"], r["max_leverage"], r["mae"], r["bits"]))
        if dev is not None and r["bits"] != dev["bits"]:
            say("chunks   DIFFERS from the default chunk")
            finish(1)
        dev = dev or r
    ok, r = run_leg(a, "host")
    if not ok:
        say("host  STOPPED: %s" % r)
        finish(1)
    say("host     rg_solve_host, one thread  %s s (once), mae[0][0] %s, bits %s" % (r["seconds"], r["mae"], r["bits"]))
    say("# the device's mae, mre, beta and left-out predictions %s the host solver's, bit for bit" % ("ARE" if r["bits"] == dev["bits"] else "ARE NOT"))
    finish(0 if r["bits"] == dev["bits"] else 1)


if __name__ == "__main__":
    main()
