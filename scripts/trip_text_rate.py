"""Rate of reading taxi trip text (include/dge.h: dge_flows_add_trip_files / dge_flows_add_trip_texts) next to the host path a caller has without it.

    python scripts/trip_text_rate.py [--lines 20000000] [--mesh 12] [--out profiles/trip_text.txt]

A Type 3 file of `lines` well-formed lines (tests/trip_text_ref.py makes a block of 20 000, written over and over) is read three ways, one process per leg:
  (a) host   tests/native/trip_parse_harness.cpp built with g++ -O2: one thread reads the file, cuts lines and runs the host build of csrc/trip_parse.h — what a
             caller does today in front of dge_flows_add_trips (the harness reads the whole file first; its time includes that);
  (b) files  dge_flows_add_trip_files;
  (c) texts  dge_flows_add_trip_texts on the file's bytes already in memory.
Every leg runs once as a warm-up and five times more; the medians are reported, with the library's own read_ms and kernel_ms and the GB/s of text through the
text kernels.  Numbers from one run on one device, not a distribution."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
RUNS = 5


def leg(kind, path, mesh):
    """one leg in this process -> a JSON line"""
    import numpy as np
    if kind == "host":
        exe = os.path.join(os.path.dirname(path), "trip_parse_harness")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "trip_parse_harness.cpp")])
        times, out = [], ""
        for _ in range(RUNS + 1):
            t0 = time.perf_counter()
            out = subprocess.check_output([exe, path, "3", "0"], text=True)
            times.append(time.perf_counter() - t0)
        print(json.dumps(dict(kind=kind, seconds=float(np.median(times[1:])), ok=int(out.split(" ok ")[1].split()[0]))))
        return
    import trip_ref

    import embedding_amd as E
    rg = E.Regions.from_arrays(*trip_ref.quad_mesh(mesh, 20251018)[0].arrays())
    data = open(path, "rb").read() if kind == "texts" else None
    times, infos = [], []
    for _ in range(RUNS + 1):
        f = E.Flows(rg)
        t0 = time.perf_counter()
        info = f.add_trip_files(path, 3, header=False) if kind == "files" else f.add_trip_text(data, 3, header=False)
        times.append(time.perf_counter() - t0)
        infos.append(dict(info, flows_kernel_ms=f.info()["kernel_ms"], mapped=f.info()["mapped"]))
    med = lambda k: float(np.median([i[k] for i in infos[1:]]))  # noqa: E731
    print(json.dumps(dict(kind=kind, seconds=float(np.median(times[1:])), ok=infos[-1]["ok"], mapped=infos[-1]["mapped"], bytes=infos[-1]["bytes"], slabs=infos[-1]["slabs"],
                          read_ms=med("read_ms"), kernel_ms=med("kernel_ms"), flows_kernel_ms=med("flows_kernel_ms"))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=20_000_000)
    ap.add_argument("--mesh", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trip_text.txt"))
    ap.add_argument("--leg", default=None)
    ap.add_argument("--path", default=None)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.path, a.mesh)
    import trip_text_ref as T
    block = b"\n".join(T.corpus_lines(3, 20_000, 61, mutated=0)) + b"\n"
    d = tempfile.mkdtemp()
    path = os.path.join(d, "trips.csv")
    reps = max(a.lines // 20_000, 1)
    with open(path, "wb") as f:
        for _ in range(reps):
            f.write(block)
    size = os.path.getsize(path)
    res = {}
    for kind in ("host", "files", "texts"):
        out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--leg", kind, "--path", path, "--mesh", str(a.mesh)], text=True)
        res[kind] = json.loads(out.strip().splitlines()[-1])
    os.remove(path)
    text = "# scripts/trip_text_rate.py: Type 3, %d lines, %d bytes, %d x %d regions; medians of %d after a warm-up, one run on one device\n" % (reps * 20_000, size, a.mesh, a.mesh, RUNS)
    text += "host   one thread, trip_parse.h   %.3f s  %.3f GB/s  ok %d  (parsing only: the trips still have to go through dge_flows_add_trips)\n" % (
        res["host"]["seconds"], size / res["host"]["seconds"] / 1e9, res["host"]["ok"])
    for kind, name in (("files", "dge_flows_add_trip_files"), ("texts", "dge_flows_add_trip_texts")):
        r = res[kind]
        text += "%s  %s  %.3f s  %.3f GB/s  read_ms %.1f  kernel_ms %.1f (%.2f GB/s through the text kernels)  flow table kernels %.1f ms  slabs %d  ok %d  mapped %d\n" % (
            kind, name, r["seconds"], size / r["seconds"] / 1e9, r["read_ms"], r["kernel_ms"], size / max(r["kernel_ms"], 1e-9) / 1e6, r["flows_kernel_ms"], r["slabs"], r["ok"], r["mapped"])
    print(text, end="")
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
