"""Wall time of the spatial graph built on the device (include/dge.h: dge_graph_add_spatial_points) next to the path it replaces.

    python scripts/spatial_graph_rate.py [--sizes 801,4096,16384] [--alone 41667] [--k 10] [--out profiles/spatial_graph.txt]

scripts/spatial_graph_rate.cpp is built with g++ -O2 -ffp-contract=off and run once per leg and size, a process each:
  old   a one-thread C++ double loop shaped like J/SpatialGraph.java:43-49 fills the R x R weight matrix, then dge_graph_add_edges of the R^2 edges,
        dge_graph_keep_top_k and dge_graph_set_sources — what a host did before;
  new   dge_graph_add_spatial_points: centroids in, graph out.
Both start from R centroids in host memory and end with a graph ready for dge_graph_build_alias.  The sizes are tried in ascending order; the old path ends at
the first size it refuses cleanly (exit status 1 with the program's own "FAILED ... rc" line: a DGE error, or no host memory for the matrix) and the largest that
worked is reported.  Anything else — a time limit, a signal, another status, a failure of the new call — ends the script at once with what it has written: no
further process is started on a device that one has just failed, died or hung on.  --alone is run through the new call
only.  Every leg runs once as a warm-up and five times more (three from 16 384 regions on for the old path); medians are reported.  Numbers from one run on one
device, not a distribution."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def leg(exe, kind, R, k, runs, limit):
    """-> ("ok", result) | ("cannot hold", message) | ("stop", message).  Only the program's own clean refusal — exit status 1 with its "FAILED ... rc" line, a
    DGE error or host memory for the matrix — means that the size cannot be held.  A time limit, a signal or any other status is "stop"."""
    try:
        out = subprocess.run([exe, kind, str(R), str(k), str(runs)], capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return "stop", "ran past %d s" % limit
    line = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    if out.returncode == 0 and " seconds " in line:
        fields = line.split(" seconds ")[1].split()
        return "ok", dict(seconds=statistics.median([float(x) for x in fields[:runs]]), rest=" ".join(fields[runs:]))
    if out.returncode == 1 and line.startswith("FAILED ") and " rc " in line:
        return "cannot hold", line
    return "stop", "exit status %d: %s" % (out.returncode, line or out.stderr.strip()[-200:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="801,4096,16384")
    ap.add_argument("--alone", type=int, default=41667)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--limit", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spatial_graph.txt"))
    a = ap.parse_args()
    libdir = os.path.join(ROOT, "embedding_amd")
    exe = os.path.join(tempfile.mkdtemp(), "spatial_graph_rate")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "scripts", "spatial_graph_rate.cpp"), "-o", exe,
                           "-L" + libdir, "-l:libdge.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    def finish(code):
        open(a.out, "w").write("\n".join(lines) + "\n")
        sys.exit(code)

    def stop(what, msg):                # nothing more is started on a device that a leg has just failed, died or hung on
        say("%s  STOPPED, no further leg was started: %s" % (what, msg))
        finish(1)

    say("# scripts/spatial_graph_rate.py: k = %d, scale = 100; wall seconds from centroids in host memory to a graph ready for build_alias; medians after a warm-up, one run on one device" % a.k)
    old_alive = True
    for R in [int(x) for x in a.sizes.split(",")]:
        what = "R %6d  new  dge_graph_add_spatial_points" % R
        status, new = leg(exe, "new", R, a.k, 5, a.limit)
        if status != "ok":              # the new call has no size it may refuse here: any failure ends the script
            stop(what, new)
        say("%s  %.6f s  %s" % (what, new["seconds"], new["rest"]))
        if not old_alive:
            continue
        what = "R %6d  old  matrix loop + add_edges + keep_top_k + set_sources" % R
        status, old = leg(exe, "old", R, a.k, 5 if R < 16384 else 3, a.limit)
        if status == "stop":
            stop(what, old)
        if status == "cannot hold":
            say("%s  could not be held: %s" % (what, old))
            old_alive = False
        else:
            say("%s  %.6f s  (%.1f x the new call)" % (what, old["seconds"], old["seconds"] / new["seconds"]))
    what = "R %6d  new  alone" % a.alone
    status, new = leg(exe, "new", a.alone, a.k, 5, a.limit)
    if status != "ok":
        stop(what, new)
    say("%s  %.6f s  %s" % (what, new["seconds"], new["rest"]))
    finish(0)


if __name__ == "__main__":
    main()
