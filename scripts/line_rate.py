"""Wall time of one LINE run on the device (include/dge.h: dge_line_coo) on a graph of the shape of one cfg3 slice (41 667 vertices, about 4.2 million edges),
next to the one-thread host loop of tests/native/line_rule_harness.cpp, which computes the same bits.

    python scripts/line_rate.py [--regions 41667] [--entries 4200000] [--dims 20,128] [--batches 4096,65536] [--negative 5] [--samples 10000000] [--out profiles/line.txt]

Every leg is a process of its own (this file with --leg), under its own time limit:
  device  evaluate.line_gpu, order 2: a warm-up call of 100 000 samples, then one call of --samples; its wall time (upload, the sort, the two prefix sums, the
          draws, two launches a batch, read-back) and the call's kernel_ms.  Graphs: "slice" — edges between regions drawn by a Zipf popularity, as flows are;
          "hub" — every vertex points at each of 8 vertices, so the target adds of all positive samples of a batch fall on 8 rows (dim 20 and the first batch size
          only): what contention on the 64-bit integer atomics costs next to the spread case.
  host    the harness's loop, one thread, the same configuration on the "slice" graph, once; the device leg of the same configuration must give the same bits,
          which the leg checks through a checksum of X and Y.
The script reports seconds and samples per second and promises no rate.  A run that leaves the rule's bound is an error return
(DGE_ERR_ARG naming the batch); the script writes it down and goes on.  It stops at the first device leg that dies, hangs or fails, with what it has written:
nothing more is started on a device that a leg has just failed on.  Numbers from one run on one device, not a distribution."""
import argparse
import os
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def graph(kind, regions, entries):
    import numpy as np
    rng = np.random.default_rng(20261019)
    if kind == "hub":
        hubs = rng.permutation(regions)[:8].astype(np.int64)
        src = np.repeat(np.arange(regions, dtype=np.int64), 8); dst = np.tile(hubs, regions)
        return src.astype(np.int32), dst.astype(np.int32), rng.geometric(0.3, len(src)).astype(np.float64)
    p = 1.0 / np.arange(1, regions + 1) ** 0.8                # region popularity: a Zipf law over a shuffled order
    p = rng.permutation(p / p.sum())
    cells = np.zeros(0, np.int64)
    while len(cells) < entries:                              # distinct (source, destination) pairs of trips drawn by popularity
        draw = rng.choice(regions, 2 * (entries - len(cells)) + 1024, p=p).astype(np.int64)
        cells = np.union1d(cells, draw[0::2] * regions + draw[1::2])
    cells = rng.permutation(cells)[:entries]
    return (cells // regions).astype(np.int32), (cells % regions).astype(np.int32), rng.geometric(0.3, len(cells)).astype(np.float64)


def checksum(X, Y):
    return zlib.crc32(Y.tobytes(), zlib.crc32(X.tobytes()))


def config(a):
    return dict(dim=a.dim, order=2, negative=a.negative, samples=a.samples, batch=a.batch, rho0=0.025, seed=1)


def leg_device(a):
    import embedding_amd.evaluate as ev
    s, d, w = graph(a.graph, a.regions, a.entries)
    ev.line_gpu(s, d, w, a.regions, **dict(config(a), samples=min(a.samples, 100000)))
    t = time.perf_counter()
    try:
        X, Y, _, info = ev.line_gpu(s, d, w, a.regions, **config(a))
    except ev_error() as e:
        if e.code != 1:
            raise
        print("seconds nan refused %s" % str(e).split(": ", 2)[-1].replace(" ", "_"))          # an argument error — the rule's bound is left — is an answer, not a failure
        return
    print("seconds %.6f kernel_ms %.3f entries %d max_abs %.6g crc %08x" % (time.perf_counter() - t, info["kernel_ms"], info["entries"], info["max_abs"], checksum(X, Y)))


def ev_error():
    from embedding_amd._native import DgeError
    return DgeError


def leg_host(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from line_harness import harness_line, load_harness
    from line_ref import BoundLeft
    s, d, w = graph(a.graph, a.regions, a.entries)
    with tempfile.TemporaryDirectory() as tmp:
        H = load_harness(os.path.join(tmp, "libline_rule_harness.so"))
        t = time.perf_counter()
        try:
            r = harness_line(H, s, d, w, a.regions, **config(a))
        except BoundLeft as e:
            print("seconds nan refused the_bound_is_left_after_%s" % str(e).replace(" ", "_"))
            return
        print("seconds %.6f kernel_ms nan entries %d max_abs %.6g crc %08x" % (time.perf_counter() - t, r["entries"], r["max_abs"], checksum(r["X"], r["Y"])))


def run_leg(a, kind, graph_kind, dim, batch):
    """-> (True, fields) | (False, message)"""
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", kind, "--graph", graph_kind, "--dim", str(dim), "--batch", str(batch), "--regions", str(a.regions), "--entries", str(a.entries),
           "--negative", str(a.negative), "--samples", str(a.samples)]
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
    ap.add_argument("--dims", default="20,128")
    ap.add_argument("--batches", default="4096,65536")
    ap.add_argument("--negative", type=int, default=5)
    ap.add_argument("--samples", type=int, default=10000000)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line.txt"))
    ap.add_argument("--leg", choices=("device", "host"))
    ap.add_argument("--graph", default="slice")
    ap.add_argument("--dim", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4096)
    a = ap.parse_args()
    if a.leg:
        (leg_device if a.leg == "device" else leg_host)(a)
        return
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    def finish(code):
        open(a.out, "w").write("\n".join(lines) + "\n")
        sys.exit(code)

    def rate(f):
        return "%.3g samples/s" % (a.samples / float(f["seconds"]))

    dims = [int(x) for x in a.dims.split(",")]; batches = [int(x) for x in a.batches.split(",")]
    say("# scripts/line_rate.py: %d vertices, %d edges asked for, order 2, K %d, %d samples, rho0 0.025; wall seconds of one call from entries in host memory; one run on one device"
        % (a.regions, a.entries, a.negative, a.samples))
    crc = {}
    for gk, dim, batch in [("slice", dm, b) for dm in dims for b in batches] + [("hub", dims[0], batches[0])]:
        ok, dev = run_leg(a, "device", gk, dim, batch)
        if not ok:
            say("%-5s dim %-3d batch %-5d device  STOPPED, no further leg was started: %s" % (gk, dim, batch, dev))
            finish(1)
        if "refused" in dev:
            crc[(gk, dim, batch)] = None
            say("%-5s dim %-3d batch %-5d device  evaluate.line_gpu  refused the run: %s" % (gk, dim, batch, dev["refused"].replace("_", " ")))
            continue
        crc[(gk, dim, batch)] = dev["crc"]
        say("%-5s dim %-3d batch %-5d device  evaluate.line_gpu  %s s (one call after a warm-up), kernel_ms %s, %s, %s edges, max_abs %s, crc %s"
            % (gk, dim, batch, dev["seconds"], dev["kernel_ms"], rate(dev), dev["entries"], dev["max_abs"], dev["crc"]))
    for dim in ([] if a.no_host else dims):
        ok, host = run_leg(a, "host", "slice", dim, batches[0])
        if not ok or "refused" in host:
            say("slice dim %-3d batch %-5d host    did not finish: %s" % (dim, batches[0], host))
        else:
            say("slice dim %-3d batch %-5d host    one-thread loop of the harness  %s s (once), %s, crc %s (%s the device's)"
                % (dim, batches[0], host["seconds"], rate(host), host["crc"], "equals" if host["crc"] == crc[("slice", dim, batches[0])] else "DIFFERS FROM"))
    finish(0)


if __name__ == "__main__":
    main()
