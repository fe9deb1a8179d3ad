"""How fast .od flow files become the layered graph in device memory: the two host loaders as they stand — io.read_od_slices (np.loadtxt, np.unique,
searchsorted) and a one-thread C++ `ifstream >>` loop shaped like embedding_host.hpp: CrossTimeGraph::constructGraphFromOD's, each followed by what a host
does next (the region ranks, then dge_graph_add_edges / reserve_vertices / set_sources for the Python one) — against the device ingest
(dge_graph_add_od_files), one process per leg, page cache warm, the median of five runs after one warm-up with all five printed.  Every number stands next to
the size of the files it was measured on.  Writes profiles/od_read.txt.

    python scripts/od_read_rate.py [--shapes ca,tract,large] [--out profiles/od_read.txt] [--tmp DIR]

The inputs are generated here, spelled as the reference's writers spell them ("%d %d %d\\n"), one file per slice:
    ca     24 slices x 77 regions, every pair a flow (zeros included, as J/CommunityAreas.java:178 writes them)
    tract  24 slices x 801 regions, 40 000 flows a slice
    large  24 slices x 41 667 regions (cfg3's), 250 000 flows a slice: 6e6 flows, a sixteenth of cfg3's 9.95e7 edges; cfg3 itself is not measured here
A child process is a leg:  --leg device|python --files F0 F1 ..
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"ca": (24, 77, 0), "tract": (24, 801, 40_000), "large": (24, 41_667, 250_000)}

HOST_READER = r"""
#include <chrono>
#include <cstdio>
#include <fstream>
#include <map>
#include <set>
#include <string>
#include <vector>
struct Flow { int h; long long a, b; double w; };
int main(int argc, char** argv) {
    for (int run = 0; run < 6; run++) {
        auto t0 = std::chrono::steady_clock::now();
        std::vector<Flow> flows;
        std::set<long long> seen;
        for (int h = 1; h < argc; h++) {                     // constructGraphFromOD's loop
            std::ifstream in(argv[h]);
            if (!in) return 1;
            long long a, b; double w;
            while (in >> a >> b >> w) {
                flows.push_back({h - 1, a, b, w});
                if (w > 0) { seen.insert(a); seen.insert(b); }
            }
        }
        std::map<long long, int> rank;                       // ... and the ranks and the edge list a host hands to dge_graph_add_edges
        for (long long r : seen) { int i = (int)rank.size(); rank[r] = i; }
        const int R = (int)rank.size(), T = argc - 1;
        std::vector<int> src, dst; std::vector<double> wt;
        for (const Flow& f : flows) if (f.w > 0) { src.push_back(f.h * R + rank[f.a]); dst.push_back(((f.h + 1) % T) * R + rank[f.b]); wt.push_back(f.w); }
        double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("%s %.3f s flows=%zu edges=%zu regions=%d\n", run ? "run" : "warm-up", s, flows.size(), src.size(), R);
        std::fflush(stdout);
    }
    return 0;
}
"""


def write_inputs(tmp, shape):
    T, R, n = SHAPES[shape]
    rng = np.random.default_rng(R)
    ids = np.sort(rng.choice(np.arange(10_000, 10_000 + 40 * R), R, replace=False))
    paths, size = [], 0
    for h in range(T):
        if n == 0:
            s = np.repeat(ids, R); d = np.tile(ids, R); w = rng.integers(0, 50, R * R)
        else:
            s = rng.choice(ids, n); d = rng.choice(ids, n); w = rng.integers(1, 2000, n)
        path = os.path.join(tmp, "%s-%d.od" % (shape, h))
        np.savetxt(path, np.stack([s, d, w], 1), fmt="%d")
        paths.append(path); size += os.path.getsize(path)
    return paths, size


def five(fn):
    fn()                                            # warm-up
    return [fn() for _ in range(5)]


def fmt(vals, unit="s"):
    return "median %.3f %s  [%s]" % (statistics.median(vals), unit, ", ".join("%.3f" % v for v in vals))


def leg(args):
    import embedding_amd as E
    size = sum(os.path.getsize(p) for p in args.files)
    if args.leg == "device":
        infos = []

        def run():
            t0 = time.perf_counter()
            g, names, info = E.DeviceGraph.from_od(args.files, names=False)
            dt = time.perf_counter() - t0
            infos.append(info)
            g.close()
            return dt
        wall = five(run)
        infos = infos[1:]
        print("  wall      %s   = %.2f GB/s, %.1f M flows/s" % (fmt(wall), size / statistics.median(wall) / 1e9, infos[0]["flows"] / statistics.median(wall) / 1e6))
        print("  read_ms   %s" % fmt([i["read_ms"] for i in infos], "ms"))
        k = [i["kernel_ms"] for i in infos]
        print("  kernel_ms %s   = %.1f GB/s of text through the kernels" % (fmt(k, "ms"), size / statistics.median(k) / 1e6))
        print("  (wall also holds the CSR build and the source table of dge_graph_set_sources, which neither read_ms nor kernel_ms counts)")
        print("  flows %d, edges %d, dropped %d, regions %d, sources %d, host_values %d" % tuple(infos[0][k] for k in ("flows", "edges", "dropped", "regions", "sources", "host_values")))
    elif args.leg == "python":
        from embedding_amd import io
        parts = []

        def run():
            t0 = time.perf_counter()
            d = io.read_od_slices(args.files)
            t1 = time.perf_counter()
            g = E.DeviceGraph(0)
            g.add_edges(d["src"], d["dst"], d["w"]); g.reserve_vertices(d["T"] * d["R"]); g.set_sources(d["sources"])
            t2 = time.perf_counter()
            g.close()
            parts.append(t1 - t0)
            return t2 - t0
        wall = five(run)
        print("  wall      %s   = %.1f MB/s" % (fmt(wall), size / statistics.median(wall) / 1e6))
        print("  of it io.read_od_slices  %s" % fmt(parts[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ca,tract,large")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "od_read.txt"))
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--leg"); ap.add_argument("--files", nargs="*")
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    tmp = args.tmp or tempfile.mkdtemp(prefix="od_read_")
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)
    exe = os.path.join(tmp, "host_reader")
    open(exe + ".cpp", "w").write(HOST_READER)
    subprocess.check_call(["g++", "-O2", "-std=c++17", exe + ".cpp", "-o", exe])
    say("# scripts/od_read_rate.py --shapes %s : one MI355X box, one process per leg, page cache warm, medians of five after a warm-up" % args.shapes)
    for shape in args.shapes.split(","):
        T, R, n = SHAPES[shape]
        paths, size = write_inputs(tmp, shape)
        say("\n## %s: %d slices x %d regions, %.3f GB of text in %d files" % (shape, T, R, size / 1e9, T))
        out = subprocess.run([exe] + paths, capture_output=True, text=True, check=True).stdout
        vals = [float(l.split()[1]) for l in out.splitlines() if l.startswith("run")]
        say("(a) one thread, `ifstream >>` per field, std::set / std::map for the regions, g++ -O2 (constructGraphFromOD's loop; the edges stay on the host)  [%.3f GB]" % (size / 1e9))
        say("  wall      %s   = %.1f MB/s  (%s)" % (fmt(vals), size / statistics.median(vals) / 1e6, out.splitlines()[-1].split(" s ")[1]))
        for name, title in (("python", "(b) io.read_od_slices, then add_edges / reserve_vertices / set_sources"), ("device", "(c) dge_graph_add_od_files")):
            say("%s  [%.3f GB]" % (title, size / 1e9))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--files"] + paths, capture_output=True, text=True, timeout=900)
            if out.returncode != 0:                 # nothing more is started on a device that a leg has just failed on
                say("  FAILED (exit %d): %s" % (out.returncode, out.stderr[-2000:]))
                open(args.out, "w").write("\n".join(lines) + "\n")
                sys.exit(1)
            say(out.stdout.rstrip())
        for p in paths:
            os.remove(p)
    open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
