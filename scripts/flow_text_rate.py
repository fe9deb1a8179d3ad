"""Time of the flow table's text writers (include/dge.h: dge_flows_write_text, dge_flows_to_text) on a cfg3-shaped table, and next to the only writer a user had
before them, Flows.to_od_bytes — a Python loop over slot_edges.

    python scripts/flow_text_rate.py [--regions 41667] [--entries 100000000] [--small 1000000] [--dir DIR] [--parts small,od,layered,matrix] [--out profiles/flow_text.txt]

  small     a table of `small` edges (2 000 regions, one hour): Flows.od_text(T=1) and Flows.to_od_bytes(1); the two texts must be equal, else the script fails
  od        `regions` regions, `entries` table entries put in through add_entries in chunks, 24 one-hour windows: the 24 .od files by one write_od call
  layered   the same slices as ONE layered text into a file
  matrix    one regions x regions .matrix (the window of hour 8) into a file, comma-separated

Files go to DIR (default: a fresh directory under the system's temporary directory) and are removed as soon as they are measured.  Wall clock around the call;
kernel_ms and write_ms are the library's own split (struct dge_flow_text_info): the device passes — edges, sizing, every slab's emit — and the slab loops
that bring the bytes to the file.  One process, one run on one device, not a distribution; no time and no ratio is promised anywhere."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def squares(E, R):
    """R squares of 1e-3 degrees on a grid, under eleven-digit ids, as census tract ids are"""
    import trip_ref
    side = int(np.ceil(np.sqrt(R)))
    rings = []
    for i in range(R):
        x, y = (i % side) * 1e-3, (i // side) * 1e-3
        rings.append([[(x, y), (x + 1e-3, y), (x + 1e-3, y + 1e-3), (x, y + 1e-3), (x, y)]])
    ids = (17031000000 + 100 * np.random.default_rng(3).permutation(R)).tolist()
    return E.Regions.from_arrays(*trip_ref.Regions(ids, rings).arrays())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=41667)
    ap.add_argument("--entries", type=int, default=100_000_000)
    ap.add_argument("--small", type=int, default=1_000_000)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--parts", default="small,od,layered,matrix")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_text.txt"))
    a = ap.parse_args()
    import embedding_amd as E
    parts = a.parts.split(",")
    d = a.dir or tempfile.mkdtemp(prefix="flow_text_rate_")
    os.makedirs(d, exist_ok=True)
    lines = ["# scripts/flow_text_rate.py --regions %d --entries %d --small %d: files under %s; one run on one device\n" % (a.regions, a.entries, a.small, os.path.dirname(d) or d)]

    def say(text):
        lines.append(text)
        print(text, end="", flush=True)
        open(a.out, "w").write("".join(lines))

    def size_of(paths):
        n = sum(os.path.getsize(p) for p in paths)
        for p in paths:
            os.remove(p)
        return n

    def row(name, wall, info, extra=""):
        return "%-34s %8.3f s  kernel_ms %10.1f  write_ms %10.1f  %14d bytes  %11d lines%s\n" % (name, wall, info["kernel_ms"], info["write_ms"], info["bytes"], info["lines"], extra)

    try:
        if "small" in parts:
            R = 2000
            rng = np.random.default_rng(1)
            pair = rng.choice(R * R, a.small, replace=False)
            f = E.Flows(squares(E, R))
            f.add_entries(np.full(a.small, 8, np.int32), (pair // R).astype(np.int32), (pair % R).astype(np.int32), rng.integers(1, 500, a.small).astype(np.int64))
            f.od_text(T=1)                                                                          # a warm-up: streams, pinned buffers, code objects
            t0 = time.perf_counter()
            (text,) = f.od_text(T=1)
            new_t = time.perf_counter() - t0
            p = os.path.join(d, "small.od")
            t0 = time.perf_counter()
            info = f.write_od([p], T=1)
            file_t = time.perf_counter() - t0
            t0 = time.perf_counter()
            (old,) = f.to_od_bytes(1)
            old_t = time.perf_counter() - t0
            assert old == text and open(p, "rb").read() == text, "the writers disagree"
            os.remove(p)
            say("small: %d edges, %d bytes\n" % (a.small, len(text)))
            say(row("  write_od, one file", file_t, info))
            say("  %-32s %8.3f s  (a size query and the text: the edges are formed twice)\n" % ("od_text(T=1), into memory", new_t))
            say("  %-32s %8.3f s  (the parent's only writer: a Python loop over slot_edges)\n" % ("to_od_bytes(1)", old_t))
            f.close()
        if {"od", "layered", "matrix"} & set(parts):
            R, N = a.regions, a.entries
            rng = np.random.default_rng(2)
            f = E.Flows(squares(E, R))
            t0 = time.perf_counter()
            chunk = 25_000_000
            for lo in range(0, N, chunk):
                n = min(chunk, N - lo)
                f.add_entries(rng.integers(0, 24, n).astype(np.int32), rng.integers(0, R, n).astype(np.int32), rng.integers(0, R, n).astype(np.int32),
                              np.minimum(rng.geometric(0.3, n), 2 ** 40).astype(np.int64))
            say("table: %d regions, %d entries drawn, %d held, put in through add_entries in %.1f s\n" % (R, N, f.info()["entries"], time.perf_counter() - t0))
            windows = [(h, 1) for h in range(24)]
            if "od" in parts:
                paths = [os.path.join(d, "taxi-%d.od" % h) for h in range(24)]
                t0 = time.perf_counter()
                info = f.write_od(paths, windows=windows)
                wall = time.perf_counter() - t0
                assert size_of(paths) == info["bytes"]
                say(row("24 .od files, one write_od call", wall, info))
            if "layered" in parts:
                p = os.path.join(d, "taxi-crossInterval.od")
                t0 = time.perf_counter()
                info = f.write_od(p, windows=windows, layered=True)
                wall = time.perf_counter() - t0
                assert size_of([p]) == info["bytes"]
                say(row("the layered text, one file", wall, info))
            if "matrix" in parts:
                p = os.path.join(d, "taxi-8.matrix")
                t0 = time.perf_counter()
                info = f.write_matrix([p], windows=[(8, 1)])
                wall = time.perf_counter() - t0
                assert size_of([p]) == info["bytes"]
                say(row("one %d x %d .matrix" % (R, R), wall, info, "  %d entries, %d zeros" % (info["edges"], info["zeros"])))
            f.close()
    finally:
        if not a.dir:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
