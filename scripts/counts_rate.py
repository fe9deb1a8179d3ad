"""Time of the count-table reader (include/dge.h: dge_counts_add_table_texts / _files) on a RAC-shaped text, next to one host thread running the same
per-line code and to the reference-shaped Python loop.

    python scripts/counts_rate.py [--lines 300000] [--tracts 3100] [--wanted 801] [--dir DIR] [--out profiles/counts.txt]

The text is generated: a header and `lines` block lines of 43 fields, "17031" + tract + block in front, 42 numbers behind it, the tracts in sorted runs of about
lines / tracts lines each as the census files have them; `wanted` of the tracts are regions, the others foreign.  Three legs, one table each, whose checksums
(the sum of (cell index + 1) * cell, mod 2^64) must agree, else the script fails:
  device   Counts.add_table on the bytes and on a file, three calls each; and once on the same lines shuffled, where no run combines
  host     tests/native/table_parse_harness.cpp's `time` mode, one thread over csrc/table_parse.h (built here with g++ -O2), the text already in memory
  python   the loop of getLEHDfeatures_helper (P/embeddingEvaluation_tract.py:512-536): split, int(ls[0][5:11]), `tid in keys` over a list, ls[8:28]

Files go to DIR (default: /dev/shm when there is one; else the system's temporary directory) and are removed afterwards.  Wall clock around the call; read_ms and
kernel_ms are the library's own split (struct dge_table_read_info).  One process, one run on one device, not a distribution; no time and no ratio is promised
anywhere."""
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
OPT = dict(sep=",", skip_lines=1, key_field=0, key=(5, 11), cols=(8, 20))


def make_text(n_lines, n_tracts, seed, shuffled=False):
    rng = np.random.default_rng(seed)
    tracts = np.sort(rng.choice(np.arange(10100, 990000), n_tracts, replace=False))
    tails = [",".join(map(str, row)) for row in rng.integers(0, 400, (min(n_lines, 20000), 42)).tolist()]
    picks = np.sort(rng.integers(0, n_tracts, n_lines))
    lines = ["17031%06d%04d,%s" % (tracts[t], i % 10000, tails[i % len(tails)]) for i, t in enumerate(picks.tolist())]
    if shuffled:
        lines = [lines[i] for i in rng.permutation(n_lines)]
    header = ",".join("f%d" % i for i in range(43))
    return ("\n".join([header] + lines) + "\n").encode(), tracts


def checksum(table):
    t = table.reshape(-1).astype(np.uint64)
    with np.errstate(over="ignore"):
        return int((t * (np.arange(len(t), dtype=np.uint64) + np.uint64(1))).sum(dtype=np.uint64))


def reference_loop(text, keys):
    acs = {}
    lines = text.decode().split("\n")
    for l in lines[1:]:
        if not l:
            continue
        ls = l.strip().split(",")
        tid = int(ls[0][5:11])
        if tid in keys:
            vec = np.array([int(e) for e in ls[8:28]])
            if tid not in acs:
                acs[tid] = vec
            else:
                for idx, val in enumerate(vec):
                    acs[tid][idx] += val
    return acs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=300000)
    ap.add_argument("--tracts", type=int, default=3100)
    ap.add_argument("--wanted", type=int, default=801)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "counts.txt"))
    a = ap.parse_args()
    import embedding_amd as E
    d = tempfile.mkdtemp(prefix="counts_rate_", dir=a.dir or ("/dev/shm" if os.path.isdir("/dev/shm") else None))
    lines = ["# scripts/counts_rate.py --lines %d --tracts %d --wanted %d: one run on one device, files in %s\n"
             % (a.lines, a.tracts, a.wanted, "memory (/dev/shm)" if d.startswith("/dev/shm") else "the file system's cache")]

    def say(text):
        lines.append(text)
        print(text, end="", flush=True)
        open(a.out, "w").write("".join(lines))

    def row(name, wall, info):
        return "  %-38s %8.4f s  read_ms %7.2f  kernel_ms %7.2f  slabs %3d  rows %7d  foreign %7d\n" % (name, wall, info["read_ms"], info["kernel_ms"], info["slabs"], info["rows"],
                                                                                                      info["foreign"])

    try:
        text, tracts = make_text(a.lines, a.tracts, 1)
        wanted = np.sort(np.random.default_rng(2).choice(tracts, a.wanted, replace=False))
        rg = E.Regions.from_ids(wanted)
        say("text: %d lines of 43 fields, %d bytes; %d tracts in sorted runs, %d of them regions\n" % (a.lines, len(text), a.tracts, a.wanted))
        E.Counts(rg, 20).add_table(text[:text.index(b"\n", 200000) + 1], **OPT)      # a warm-up: streams, pinned buffers, code objects
        path = os.path.join(d, "rac.csv")
        with open(path, "wb") as f:
            f.write(text)
        sums = []
        for name, source in (("add_table, the bytes", text), ("add_table, one file", path)):
            for k in range(3):
                c = E.Counts(rg, 20)
                t0 = time.perf_counter()
                info = c.add_table(source, return_info=True, **OPT)
                wall = time.perf_counter() - t0
                say(row("%s, call %d" % (name, k + 1), wall, info))
                sums.append(checksum(c.to_host()))
                c.close()
        mixed, _ = make_text(a.lines, a.tracts, 1, shuffled=True)
        c = E.Counts(rg, 20)
        t0 = time.perf_counter()
        info = c.add_table(mixed, return_info=True, **OPT)
        say(row("add_table, the lines shuffled", time.perf_counter() - t0, info))
        sums.append(checksum(c.to_host()))
        bin_dir = tempfile.mkdtemp(prefix="counts_rate_bin_")                  # (a memory-backed directory may not run programs)
        exe = os.path.join(bin_dir, "table_parse_harness")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "native", "table_parse_harness.cpp")])
        ids_path = os.path.join(d, "ids.txt")
        with open(ids_path, "w") as f:
            f.write("\n".join(map(str, wanted.tolist())) + "\n")
        out = subprocess.run([exe, "time", path, ids_path, "20", str(ord(",")), "1", "0", "5", "11", "8", "20", "0", "-1"], capture_output=True, text=True, check=True).stdout.split()
        sums.append(int(out[-1]))
        say("  %-38s %8.4f s  (csrc/table_parse.h line by line, the text already in memory)\n" % ("one host thread, g++ -O2", float(out[-3]) / 1e3))
        shutil.rmtree(bin_dir, ignore_errors=True)
        t0 = time.perf_counter()
        acs = reference_loop(text, wanted.tolist())
        ref_t = time.perf_counter() - t0
        table = np.zeros((a.wanted, 20), np.int64)
        for i, tid in enumerate(wanted.tolist()):
            if tid in acs:
                table[i] = acs[tid]
        sums.append(checksum(table))
        say("  %-38s %8.4f s  (the loop of getLEHDfeatures_helper, `tid in keys` over a list of %d)\n" % ("reference-shaped Python loop", ref_t, a.wanted))
        assert len(set(sums)) == 1, "the legs' tables disagree: %r" % (sums,)
        say("  all %d tables have the checksum %d\n" % (len(sums), sums[0]))
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
