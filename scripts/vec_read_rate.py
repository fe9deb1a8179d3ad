"""How fast a .vec file becomes resident float32 rows: a single-thread C++ strtof loop (the fair host baseline) and io.read_vec (the Python loop) against the
device reader (dge_vectors_from_vec_files / dge_vectors_from_vec_text), one process per leg, page cache warm, the median of five runs after one warm-up
with all five printed.  Writes profiles/vec_read.txt.

    python scripts/vec_read_rate.py [--shapes tract,slice,cfg3] [--out profiles/vec_read.txt] [--tmp DIR]

The inputs are spelled by dge_write_vec itself: a model of V rows x D (counts all 2, so every row is in the vocabulary) whose syn0 is loaded with N(0, 0.3)
values through dge_model_load_vectors, written with the vertex ids as names:
    tract  6 408 x 20      the reference's tract shape
    slice  41 667 x 128    one cfg3 slice
    cfg3   1 000 008 x 128 the cfg3 .vec, about 1.67 GB
A child process is a leg:  --leg files|text|python --file F
Not a leg yet: the kernels one by one (rocprofv3 --kernel-trace --stats on the `files` leg gives that).
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
SHAPES = {"tract": (6408, 20), "slice": (41667, 128), "cfg3": (1000008, 128)}

HOST_READER = r"""
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
int main(int argc, char** argv) {
    for (int run = 0; run < 6; run++) {
        auto t0 = std::chrono::steady_clock::now();
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) return 1;
        std::fseek(f, 0, SEEK_END); long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
        std::vector<char> text((size_t)n + 1);
        if (std::fread(text.data(), 1, (size_t)n, f) != (size_t)n) return 1;
        std::fclose(f);
        text[(size_t)n] = 0;
        std::vector<std::string> names; std::vector<float> rows;
        char* p = text.data();
        char* end = p + n;
        while (p < end) {                                   // a line: name, then strtof until the newline
            while (p < end && (*p == ' ' || *p == '\r' || *p == '\t')) p++;
            if (p < end && *p == '\n') { p++; continue; }
            char* q = p;
            while (q < end && *q != ' ' && *q != '\n') q++;
            names.emplace_back(p, q);
            p = q;
            for (;;) {
                while (p < end && (*p == ' ' || *p == '\r' || *p == '\t')) p++;
                if (p >= end || *p == '\n') break;
                char* e; rows.push_back(std::strtof(p, &e)); p = e;
            }
        }
        double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("%s %.3f s rows=%zu values=%zu\n", run ? "run" : "warm-up", s, names.size(), rows.size());
        std::fflush(stdout);
    }
    return 0;
}
"""


def write_input(path, V, D):
    import torch

    import embedding_amd as E
    counts = torch.full((V,), 2, dtype=torch.int64, device="cuda:0")
    m = E.SgnsModel.create(E.make_config(D, 8, V, workers=1, table_size=10007), counts)
    rng = np.random.default_rng(V)
    m.load_vectors(E.Vectors.from_host(rng.normal(0, 0.3, (V, D)).astype(np.float32)))
    m.write_vec(path)
    m.close()
    return os.path.getsize(path)


def five(fn):
    fn()                                            # warm-up
    return [fn() for _ in range(5)]


def fmt(vals, unit="s"):
    return "median %.3f %s  [%s]" % (statistics.median(vals), unit, ", ".join("%.3f" % v for v in vals))


def leg(args):
    import embedding_amd as E
    size = os.path.getsize(args.file)
    if args.leg in ("files", "text"):
        data = open(args.file, "rb").read() if args.leg == "text" else None
        infos = []

        def run():
            t0 = time.perf_counter()
            vec, names, info = E.Vectors.from_vec(data if data is not None else args.file)
            dt = time.perf_counter() - t0
            infos.append(info)
            vec.close(); names.close()
            return dt
        wall = five(run)
        infos = infos[1:]
        print("  wall      %s   = %.2f GB/s, %.1f M values/s" % (fmt(wall), size / statistics.median(wall) / 1e9, infos[0]["values"] / statistics.median(wall) / 1e6))
        print("  read_ms   %s" % fmt([i["read_ms"] for i in infos], "ms"))
        k = [i["kernel_ms"] for i in infos]
        print("  kernel_ms %s   = %.1f GB/s of text through the kernels" % (fmt(k, "ms"), size / statistics.median(k) / 1e6))
        print("  rows %d, dim %d, values %d, host_values %d" % (infos[0]["rows"], infos[0]["dim"], infos[0]["values"], infos[0]["host_values"]))
    elif args.leg == "python":
        from embedding_amd import io

        def run():
            t0 = time.perf_counter()
            io.read_vec(args.file)
            return time.perf_counter() - t0
        wall = five(run)
        print("  wall      %s   = %.1f MB/s" % (fmt(wall), size / statistics.median(wall) / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="tract,slice,cfg3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vec_read.txt"))
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--leg"); ap.add_argument("--file")
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    tmp = args.tmp or tempfile.mkdtemp(prefix="vec_read_")
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)
    exe = os.path.join(tmp, "host_reader")
    open(exe + ".cpp", "w").write(HOST_READER)
    subprocess.check_call(["g++", "-O2", "-std=c++17", exe + ".cpp", "-o", exe])
    say("# scripts/vec_read_rate.py --shapes %s : one MI355X box, one process per leg, page cache warm, medians of five after a warm-up" % args.shapes)
    for shape in args.shapes.split(","):
        V, D = SHAPES[shape]
        path = os.path.join(tmp, shape + ".vec")
        size = write_input(path, V, D)
        say("\n## %s: %d rows x %d, %.3f GB as dge_write_vec spells it" % (shape, V, D, size / 1e9))
        out = subprocess.run([exe, path], capture_output=True, text=True, check=True).stdout
        vals = [float(l.split()[1]) for l in out.splitlines() if l.startswith("run")]
        say("(a) one thread, strtof per value, g++ -O2 (the host baseline)")
        say("  wall      %s   = %.1f MB/s  (%s)" % (fmt(vals), size / statistics.median(vals) / 1e6, out.splitlines()[-1].split(" s ")[1]))
        legs = [("files", "(c) dge_vectors_from_vec_files"), ("text", "(d) dge_vectors_from_vec_text, bytes in host memory")]
        if shape != "cfg3":
            legs.insert(0, ("python", "(b) io.read_vec"))
        for name, title in legs:
            say(title)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--file", path], capture_output=True, text=True, timeout=600)
            if out.returncode != 0:                 # nothing more is started on a device that a leg has just failed on
                say("  FAILED (exit %d): %s" % (out.returncode, out.stderr[-2000:]))
                open(args.out, "w").write("\n".join(lines) + "\n")
                sys.exit(1)
            say(out.stdout.rstrip())
        os.remove(path)
    open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
