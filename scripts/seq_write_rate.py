"""How fast a resident walk corpus of the reference's tract shape becomes .seq text: the host mirror's former writer loop (the yardstick) against the device
writer (dge_walks_write_seq / dge_walks_to_seq_text), one process per leg, the median of five runs after one warm-up with all five printed.  Writes
profiles/seq_write.txt.

    python scripts/seq_write_rate.py [--tenths 10] [--out profiles/seq_write.txt] [--tmp DIR]

The corpus: tenths x 1.56 M walks x 8 ids over 6 408 names "h-17xxxx" (801 regions x 8 slices) — the text scripts/seq_ingest_rate.py reads; a second corpus
draws the regions from a Zipf distribution.  A child process is a leg:
    (a) HOST_WRITER below: the loop CrossTimeGraph::write_seq ran before the device writer existed, copied verbatim — per token nameOfDeviceId and
        std::string +=, per line an ofstream <<, in chunks of 2^18 walks.  The walks already lie in host memory (the loop's device-to-host copy of each chunk
        is NOT in its time).
    (b) --leg file   dge_walks_write_seq into a file
    (c) --leg text   dge_walks_to_seq_text into host memory (the size is known: one call, no size query)
"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LINES_PER_TENTH, T, R = 1_560_000, 8, 801

HOST_WRITER = r"""
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>
static std::vector<std::string> names;
static const std::string& nameOfDeviceId(int32_t id) { return names[(size_t)id]; }
// CrossTimeGraph::write_seq as it stood, with the chunk taken from `all` instead of from the sampler
static void write_seq(const std::vector<int32_t>& all, const std::string& path, int64_t n, int L, bool positionPrefix) {
    std::ofstream out(path);
    const int64_t chunk = 1 << 18;
    for (int64_t done = 0; done < n; done += chunk) {
        int64_t m = std::min(chunk, n - done);
        const int32_t* w = all.data() + (size_t)done * L;
        std::string line;
        for (int64_t i = 0; i < m; i++) {
            line.clear();
            for (int j = 0; j < L && w[(size_t)i * L + j] >= 0; j++) {
                if (j) line += ' ';
                if (positionPrefix) { line += std::to_string(j); line += '-'; }   // J/SpatialGraph.java:105-108
                line += nameOfDeviceId(w[(size_t)i * L + j]);
            }
            line += '\n';
            out << line;
        }
    }
}
int main(int argc, char** argv) {
    const int L = 8, R = 801;
    for (int h = 0; h < L; h++) for (int r = 0; r < R; r++) names.push_back(std::to_string(h) + "-" + std::to_string(170000 + 7 * r));
    std::ifstream in(argv[1], std::ios::binary | std::ios::ate);
    const int64_t n = (int64_t)in.tellg() / (4 * L);
    std::vector<int32_t> all((size_t)n * L);
    in.seekg(0); in.read((char*)all.data(), (std::streamsize)all.size() * 4);
    for (int run = 0; run < 6; run++) {
        auto t0 = std::chrono::steady_clock::now();
        write_seq(all, argv[2], n, L, false);
        double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("%s %.3f s rows=%lld\n", run ? "run" : "warm-up", s, (long long)n);
        std::fflush(stdout);
    }
    return 0;
}
"""


def make_walks(path, tenths, zipf):
    rng = np.random.default_rng(7 if zipf else 3)
    p = None
    if zipf:
        p = 1.0 / np.arange(1, R + 1) ** 1.1; p /= p.sum()
    with open(path, "wb") as f:
        for _ in range(tenths):
            reg = rng.choice(R, (LINES_PER_TENTH, T), p=p) if zipf else rng.integers(0, R, (LINES_PER_TENTH, T))
            f.write((reg + np.arange(T) * R).astype(np.int32).tobytes())


def names_list():
    return ["%d-%d" % (h, 170000 + 7 * r) for h in range(T) for r in range(R)]


def fmt(vals, unit="s"):
    return "median %.3f %s  [%s]" % (statistics.median(vals), unit, ", ".join("%.3f" % v for v in vals))


def leg(args):
    import embedding_amd as E
    from embedding_amd._native import SeqOutInfo
    walks = np.fromfile(args.file, np.int32).reshape(-1, T)
    corpus = E.WalkCorpus.from_host(walks)
    names = E.Names(names_list())
    need = C.c_int64(0)
    E._native.check(E.lib.dge_walks_to_seq_text(corpus._h, 0, len(walks), names._h, 0, None, 0, C.byref(need), None))
    size = need.value
    buf = np.empty(size, np.uint8) if args.leg == "text" else None
    if buf is not None:
        buf[:] = 0                                  # the pages exist before the clock starts
    wall, infos = [], []
    for run in range(6):
        inf = SeqOutInfo()
        t0 = time.perf_counter()
        if args.leg == "file":
            E._native.check(E.lib.dge_walks_write_seq(corpus._h, 0, len(walks), names._h, 0, os.fsencode(args.target), 0, C.byref(inf)))
        else:
            E._native.check(E.lib.dge_walks_to_seq_text(corpus._h, 0, len(walks), names._h, 0, buf.ctypes.data_as(C.c_void_p), size, C.byref(need), C.byref(inf)))
        dt = time.perf_counter() - t0
        if run:
            wall.append(dt); infos.append(inf)
    k = [i.kernel_ms for i in infos]
    print("  wall      %s   = %.2f GB/s, %.1f M tokens/s" % (fmt(wall), size / statistics.median(wall) / 1e9, infos[0].tokens / statistics.median(wall) / 1e6))
    print("  kernel_ms %s   = %.1f GB/s of text through the kernels" % (fmt(k, "ms"), size / statistics.median(k) / 1e6))
    print("  write_ms  %s" % fmt([i.write_ms for i in infos], "ms"))
    print("  bytes %d, lines %d, tokens %d, empty lines %d" % (infos[0].bytes, infos[0].lines, infos[0].tokens, infos[0].empty_lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tenths", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_write.txt"))
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--leg"); ap.add_argument("--file"); ap.add_argument("--target")
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    tmp = args.tmp or tempfile.mkdtemp(prefix="seq_write_")
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)
    exe = os.path.join(tmp, "host_writer")
    open(exe + ".cpp", "w").write(HOST_WRITER)
    subprocess.check_call(["g++", "-O2", "-std=c++17", exe + ".cpp", "-o", exe])
    say("# scripts/seq_write_rate.py --tenths %d : one MI355X box, one process per leg, medians of five after a warm-up" % args.tenths)
    for zipf in (False, True):
        ids = os.path.join(tmp, "zipf.i32" if zipf else "flat.i32")
        target = os.path.join(tmp, "out.seq")
        make_walks(ids, args.tenths, zipf)
        say("\n## %s names: %d walks x %d ids over %d names" % ("Zipf-popular" if zipf else "flat", args.tenths * LINES_PER_TENTH, T, T * R))
        out = subprocess.run([exe, ids, target], capture_output=True, text=True, check=True).stdout
        vals = [float(l.split()[1]) for l in out.splitlines() if l.startswith("run")]
        size = os.path.getsize(target)
        say("(a) the former CrossTimeGraph::write_seq loop, g++ -O2 (the yardstick), %.3f GB of text" % (size / 1e9))
        say("  wall      %s   = %.1f MB/s" % (fmt(vals), size / statistics.median(vals) / 1e6))
        for name, title in (("file", "(b) dge_walks_write_seq into a file"), ("text", "(c) dge_walks_to_seq_text into host memory")):
            say(title)
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--file", ids, "--target", target], capture_output=True, text=True)
            say(o.stdout.rstrip() if o.returncode == 0 else "  FAILED: " + o.stderr[-2000:])
        os.remove(ids); os.remove(target)
    open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
