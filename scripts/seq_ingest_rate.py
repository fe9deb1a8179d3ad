"""How fast a .seq corpus of the reference's tract shape becomes a resident walk corpus: the host mirror's stream reader (DeepWalk::readSentencesHost, the
yardstick) against the device ingest (dge_walks_from_seq_files / dge_walks_from_seq_text), one process per leg, page cache warm, the median of five runs
after one warm-up with all five printed.  Writes profiles/seq_ingest.txt.

    python scripts/seq_ingest_rate.py [--tenths 10] [--out profiles/seq_ingest.txt] [--tmp DIR]

The file: tenths x 1.56 M lines x 8 tokens over 6 408 names "h-17xxxx" (the reference's "3-170400") (801 regions x 8 slices), single blanks, one '\\n' a line — what io.write_seq
writes; a second file draws the regions from a Zipf distribution (the popular names stress the one-address atomic chain).  A child process is a leg:
    --leg files|text|train  --file F
Not a leg yet: the kernels one by one (rocprofv3 --kernel-trace --stats on the `files` leg gives that) and learnEmbedding end to end.
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
LINES_PER_TENTH, T, R = 1_560_000, 8, 801

HOST_READER = r"""
#include <chrono>
#include <cstdio>
#include "%s/embedding_amd/host/embedding_host.hpp"
int main(int argc, char** argv) {
    for (int run = 0; run < 6; run++) {
        std::unordered_map<std::string, int> ids; std::vector<std::string> names; std::vector<int32_t> walks; size_t L = 1;
        auto t0 = std::chrono::steady_clock::now();
        size_t n = embedding::DeepWalk::readSentencesHost({argv[1]}, true, ids, names, walks, L);
        double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("%%s %%.3f s rows=%%zu names=%%zu\n", run ? "run" : "warm-up", s, n, names.size());
        std::fflush(stdout);
    }
    return 0;
}
"""


def write_corpus(path, tenths, zipf):
    rng = np.random.default_rng(7 if zipf else 3)
    names = np.array([b"%d-%d%s" % (h, 170000 + 7 * r, b"\n" if h == T - 1 else b" ") for h in range(T) for r in range(R)], "S10").reshape(T, R)
    p = None
    if zipf:
        p = 1.0 / np.arange(1, R + 1) ** 1.1; p /= p.sum()
    with open(path, "wb") as f:
        for _ in range(tenths):
            reg = rng.choice(R, (LINES_PER_TENTH, T), p=p) if zipf else rng.integers(0, R, (LINES_PER_TENTH, T))
            cell = np.zeros((LINES_PER_TENTH, T), "S10")
            for h in range(T):
                cell[:, h] = names[h][reg[:, h]]
            flat = cell.view(np.uint8).ravel()
            f.write(flat[flat != 0].tobytes())
    return os.path.getsize(path)


def five(fn):
    fn()                                            # warm-up
    vals = [fn() for _ in range(5)]
    return vals


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
            corpus, names, info = E.WalkCorpus.from_seq(data if data is not None else args.file)
            dt = time.perf_counter() - t0
            infos.append((info, len(names)))
            corpus.close(); names.close()
            return dt
        wall = five(run)
        infos = infos[1:]
        print("  wall      %s   = %.2f GB/s, %.1f M tokens/s" % (fmt(wall), size / statistics.median(wall) / 1e9, infos[0][0]["tokens"] / statistics.median(wall) / 1e6))
        print("  read_ms   %s" % fmt([i["read_ms"] for i, _ in infos], "ms"))
        k = [i["kernel_ms"] for i, _ in infos]
        print("  kernel_ms %s   = %.1f GB/s of text through the kernels" % (fmt(k, "ms"), size / statistics.median(k) / 1e6))
        print("  rows %d, tokens %d, names %d, max_len %d" % (infos[0][0]["rows"], infos[0][0]["tokens"], infos[0][1], infos[0][0]["max_len"]))
    elif args.leg == "train":
        corpus, names, info = E.WalkCorpus.from_seq(args.file)
        cfg = E.make_config(20, T, len(names), table_size=0)

        def run():
            t0 = time.perf_counter()
            m = E.SgnsModel.fit(corpus, cfg)
            dt = time.perf_counter() - t0
            run.pairs = m.stats()["pairs"]; m.close()
            return dt
        wall = five(run)
        print("  dge_train_sgns_device, D = 20, no tree term: %s   (%.3g pairs)" % (fmt(wall), run.pairs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tenths", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_ingest.txt"))
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--leg"); ap.add_argument("--file")
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    tmp = args.tmp or tempfile.mkdtemp(prefix="seq_ingest_")
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)
    exe = os.path.join(tmp, "host_reader")
    open(exe + ".cpp", "w").write(HOST_READER % ROOT)
    libdir = os.path.join(ROOT, "embedding_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", exe + ".cpp", "-o", exe, "-L" + libdir, "-l:libdge.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    say("# scripts/seq_ingest_rate.py --tenths %d : one MI355X box, one process per leg, page cache warm, medians of five after a warm-up" % args.tenths)
    for zipf in (False, True):
        path = os.path.join(tmp, "zipf.seq" if zipf else "flat.seq")
        size = write_corpus(path, args.tenths, zipf)
        say("\n## %s names: %d lines x %d tokens over %d names, %.3f GB" % ("Zipf-popular" if zipf else "flat", args.tenths * LINES_PER_TENTH, T, T * R, size / 1e9))
        legs = [("files", "(b) dge_walks_from_seq_files"), ("text", "(c) dge_walks_from_seq_text, bytes in host memory")]
        if not zipf:
            out = subprocess.run([exe, path], capture_output=True, text=True, check=True).stdout
            vals = [float(l.split()[1]) for l in out.splitlines() if l.startswith("run")]
            say("(a) DeepWalk::readSentencesHost, g++ -O2 (the yardstick)")
            say("  wall      %s   = %.1f MB/s  (%s)" % (fmt(vals), size / statistics.median(vals) / 1e6, out.splitlines()[-1].split(" s ")[1]))
            legs.append(("train", "(e) training that corpus"))
        for name, title in legs:
            say(title)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--file", path], capture_output=True, text=True)
            say(out.stdout.rstrip() if out.returncode == 0 else "  FAILED: " + out.stderr[-2000:])
        os.remove(path)
    open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
