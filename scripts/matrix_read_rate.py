"""Time of the .matrix reader (include/dge.h: dge_flows_add_matrix_files) on a cfg3-slice-shaped matrix, and on a smaller one next to the reference's way and
to one host thread running the same per-lane code.

    python scripts/matrix_read_rate.py [--regions 41667] [--entries 4200000] [--small 4096] [--dir DIR] [--parts large,small] [--out profiles/matrix_read.txt]

  large   `regions` regions, `entries` entries in one hour: the .matrix is written by Flows.write_matrix and read back by Flows.add_matrix; the table read must
          equal the table written, else the script fails
  small   a `small` x `small` matrix at the same density, three ways: the device call; np.loadtxt, np.nonzero and Flows.add_entries (what
          P/matrixFactorization_tract.py:35 does, and the only way in before this reader); tests/native/matrix_parse_harness.cpp's `rate` mode, one host
          thread over csrc/matrix_parse.h (built here with g++ -O2).  The host loop's checksum of (row, column, value) must equal the device table's.

Files go to DIR (default: /dev/shm when there is one, so that the file is memory-backed; else the system's temporary directory) and are removed afterwards.  Wall
clock around the call; read_ms and kernel_ms are the library's own split (struct dge_matrix_read_info).  One process, one run on one device, not a
distribution; no time and no ratio is promised anywhere."""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def table(E, R, N, hour, seed):
    rng = np.random.default_rng(seed)
    pair = rng.choice(R * R, N, replace=False)
    f = E.Flows(E.Regions.from_ids(np.arange(R, dtype=np.int64) * 100 + 17031000000))
    f.add_entries(np.full(N, hour, np.int32), (pair // R).astype(np.int32), (pair % R).astype(np.int32), np.minimum(rng.geometric(0.05, N), 2 ** 40).astype(np.int64))
    return f


def fnv(rows, cols, vals):
    h = 1469598103934665603
    for r, c, v in zip(rows, cols, vals):
        for x in (r, c, v):
            h = ((h ^ x) * 1099511628211) & (2 ** 64 - 1)
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=41667)
    ap.add_argument("--entries", type=int, default=4_200_000)
    ap.add_argument("--small", type=int, default=4096)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--parts", default="large,small")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_read.txt"))
    a = ap.parse_args()
    import embedding_amd as E
    parts = a.parts.split(",")
    d = tempfile.mkdtemp(prefix="matrix_read_rate_", dir=a.dir or ("/dev/shm" if os.path.isdir("/dev/shm") else None))
    lines = ["# scripts/matrix_read_rate.py --regions %d --entries %d --small %d: one run on one device, files in %s\n"
             % (a.regions, a.entries, a.small, "memory (/dev/shm)" if d.startswith("/dev/shm") else "the file system's cache")]

    def say(text):
        lines.append(text)
        print(text, end="", flush=True)
        open(a.out, "w").write("".join(lines))

    def row(name, wall, info):
        return "%-40s %8.3f s  read_ms %9.1f  kernel_ms %8.1f  slabs %4d  %13d bytes  %9d entries\n" % (name, wall, info["read_ms"], info["kernel_ms"], info["slabs"], info["bytes"],
                                                                                                        info["entries"])

    try:
        warm = table(E, 64, 100, 8, 0)
        E.Flows(warm.regions).add_matrix(warm.matrix_text(0, windows=[(8, 1)]), 8)                 # a warm-up: streams, pinned buffers, code objects
        if "large" in parts:
            R, N = a.regions, a.entries
            f = table(E, R, N, 8, 1)
            p = os.path.join(d, "taxi-h8.matrix")
            t0 = time.perf_counter()
            w = f.write_matrix([p], windows=[(8, 1)])
            say("large: %d x %d, %d entries; written by write_matrix in %.3f s (%d bytes)\n" % (R, R, N, time.perf_counter() - t0, w["bytes"]))
            g = E.Flows(f.regions)
            t0 = time.perf_counter()
            info = g.add_matrix(p, 8)
            wall = time.perf_counter() - t0
            os.remove(p)
            assert all(np.array_equal(x, y) for x, y in zip(f.to_host(), g.to_host())), "the table read is not the table written"
            say(row("  add_matrix, one file", wall, info))
            say("  the table read equals the table written\n")
            f.close(); g.close()
        if "small" in parts:
            R = a.small
            N = max(1, int(round(a.entries / a.regions ** 2 * R * R)))
            f = table(E, R, N, 8, 2)
            p = os.path.join(d, "small.matrix")
            f.write_matrix([p], windows=[(8, 1)])
            g = E.Flows(f.regions)
            t0 = time.perf_counter()
            info = g.add_matrix(p, 8)
            dev_t = time.perf_counter() - t0
            say("small: %d x %d, %d entries, %d bytes\n" % (R, R, N, info["bytes"]))
            say(row("  add_matrix, one file", dev_t, info))
            h = E.Flows(f.regions)
            t0 = time.perf_counter()
            dense = np.loadtxt(p, delimiter=",")
            load_t = time.perf_counter() - t0
            r, c = np.nonzero(dense)
            h.add_entries(np.full(len(r), 8, np.int32), r.astype(np.int32), c.astype(np.int32), dense[r, c].astype(np.int64))
            ref_t = time.perf_counter() - t0
            assert all(np.array_equal(x, y) for x, y in zip(g.to_host(), h.to_host())), "the two ways disagree"
            say("  %-38s %8.3f s  (np.loadtxt alone: %.3f s)\n" % ("np.loadtxt, np.nonzero, add_entries", ref_t, load_t))
            say("  the device call takes %.4f of the reference's way's time (%.1f times as fast)\n" % (dev_t / ref_t, ref_t / dev_t))
            bin_dir = tempfile.mkdtemp(prefix="matrix_read_rate_bin_")                             # (a memory-backed directory may not run programs)
            exe = os.path.join(bin_dir, "matrix_parse_harness")
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "native", "matrix_parse_harness.cpp")])
            out = subprocess.run([exe, "rate", p, str(ord(",")), str(R)], capture_output=True, text=True, check=True).stdout.split()
            _, src, dst, count = g.to_host()
            assert int(out[1]) == len(count) and int(out[3]) == fnv(src.tolist(), dst.tolist(), count.tolist()) and int(out[5]) == 0, "the host loop and the device disagree"
            say("  %-38s %8.3f s  (csrc/matrix_parse.h by lanes, the text already in memory; checksum equal to the device table's)\n" % ("one host thread, g++ -O2", float(out[7]) / 1e3))
            os.remove(p)
            shutil.rmtree(bin_dir, ignore_errors=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
