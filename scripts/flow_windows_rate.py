"""Time of the triplet search and of the cross-time graph's window sums (include/dge.h: dge_flows_triplets, dge_flows_window_edges) next to a one-thread C++
loop shaped like the Java one: a hash map per region and hour, getFlowTo(dst, lo, hi) as a loop of look-ups over the hours, the triplet search as
Tracts.bruteForceSearchCase writes it (J/Tracts.java:380-406) — R^3 triplets, the ten conditions in its order behind its short-circuit `||` — and the graph's
sums as CrossTimeGraph.constructGraph_tract asks for them (J/CrossTimeGraph.java:33-41).

    python scripts/flow_windows_rate.py [--regions 801] [--planted 200] [--noise 400] [--out profiles/flow_windows.txt]

The table is generated: `planted` disjoint triples with the counts of tests/flow_ref.py's base pattern (every fourth with one condition broken), and
noise * R entries between random pairs in random hours.  Device: wall clock around the call, median of three after a warm-up; kernel_ms is the library's own
event time.  Host: built here with g++ -O2, run once.  Both legs must give the same triplets and the same number of window edges, else the script fails.  One
process; numbers from one run on one device, not a distribution; no time and no ratio is promised anywhere."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HOST_LOOP = r"""
#include <stdint.h>
#include <unordered_map>
#include <vector>
typedef std::vector<std::unordered_map<int32_t, int32_t>> Region;      // taxiFlows: one map per hour, destination -> count
static std::vector<Region> regions;
static inline int64_t flow(int32_t src, int32_t dst, int lo, int hi) {     // Tract.getFlowTo(dst, lo, hi): inclusive high
    int64_t cnt = 0;
    for (int h = lo; h <= hi; h++) { auto it = regions[src][h].find(dst); if (it != regions[src][h].end()) cnt += it->second; }
    return cnt;
}
extern "C" void host_load(const int32_t* hour, const int32_t* src, const int32_t* dst, const int64_t* count, int64_t n, int32_t R) {
    regions.assign(R, Region(24));
    for (int64_t i = 0; i < n; i++) regions[src[i]][hour[i]][dst[i]] += (int32_t)count[i];
}
extern "C" int64_t host_triplets(int32_t R, int32_t* out, int64_t cap) {
    int64_t pos = 0;
    for (int32_t t1 = 0; t1 < R; t1++)
        for (int32_t t2 = 0; t2 < R; t2++) {
            if (t2 == t1) continue;
            for (int32_t t3 = 0; t3 < R; t3++) {
                if (t3 == t1 || t3 == t2) continue;
                if (flow(t1, t2, 7, 9) <= 30 || flow(t3, t1, 17, 23) <= 70 || flow(t2, t3, 17, 23) <= 70 || flow(t1, t2, 7, 9) <= 2 * flow(t2, t1, 7, 9) ||
                    flow(t1, t3, 17, 22) <= 2 * flow(t1, t3, 7, 12) || flow(t2, t1, 17, 22) <= 2 * flow(t1, t2, 17, 22) || flow(t2, t3, 17, 22) <= 2 * flow(t2, t3, 7, 12) ||
                    flow(t3, t1, 17, 23) <= 2 * flow(t3, t1, 7, 13) || flow(t3, t1, 17, 23) <= 2 * flow(t3, t2, 17, 23) || flow(t3, t1, 17, 23) <= 2 * flow(t1, t3, 17, 23))
                    continue;
                if (pos < cap) { out[3 * pos] = t1; out[3 * pos + 1] = t2; out[3 * pos + 2] = t3; }
                pos++;
            }
        }
    return pos;
}
extern "C" int64_t host_cross_time(int32_t R, int32_t T, int64_t* weight_sum) {      // the edges constructGraph_tract adds
    int64_t edges = 0, sum = 0;
    const int step = 24 / T;
    for (int h = 0; h < T; h++)
        for (int32_t s = 0; s < R; s++)
            for (int32_t d = 0; d < R; d++) { const int64_t w = flow(s, d, h, h + step - 1); if (w > 0) { edges++; sum += w; } }
    *weight_sum = sum;
    return edges;
}
"""


def generate(R, planted, noise, seed=1):
    import flow_ref
    rng = np.random.default_rng(seed)
    perm = rng.permutation(R).tolist()
    c = Counter()
    for q in range(planted):
        t = perm[3 * q: 3 * q + 3]
        base = flow_ref._base(*t)
        if q % 4 == 3:
            broken = sorted(base)[(q // 4) % len(base)]
            h, s, e, w = base[broken]
            base[broken] = (h, s, e, w // 4 if broken in ("a12", "c21", "b31", "c13", "b23") else 4 * w)
        for h, s, e, w in base.values():
            c[(h, s, e)] += w
    n = noise * R
    for h, s, e, w in zip(rng.integers(0, 24, n).tolist(), rng.integers(0, R, n).tolist(), rng.integers(0, R, n).tolist(), rng.integers(1, 20, n).tolist()):
        c[(h, s, e)] += w
    return dict(c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=801)
    ap.add_argument("--planted", type=int, default=200)
    ap.add_argument("--noise", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_windows.txt"))
    a = ap.parse_args()
    import flow_ref
    import trip_ref

    import embedding_amd as E
    R = a.regions
    assert 3 * a.planted <= R
    c = generate(R, a.planted, a.noise)
    side = int(np.ceil(np.sqrt(R)))
    squares = [[[(x, y), (x + 1.0, y), (x + 1.0, y + 1.0), (x, y + 1.0), (x, y)]] for x, y in ((float(i % side), float(i // side)) for i in range(R))]
    rg = E.Regions.from_arrays(*trip_ref.Regions(list(range(R)), squares).arrays())             # id = index: the host leg's triplets compare as they are
    f = E.Flows(rg)
    hour, src, dst, count = flow_ref.arrays(c)
    f.add_entries(hour, src, dst, count)
    windows = E.Flows.windows_cross_time(8)

    def timed(call):
        times = []
        for _ in range(4):
            t0 = time.perf_counter()
            out = call()
            times.append(time.perf_counter() - t0)
        return out, float(np.median(times[1:]))

    (trip, info), trip_t = timed(lambda: f.triplets(return_info=True))
    edges, edge_t = timed(lambda: f.window_edges(windows))

    d = tempfile.mkdtemp()
    cpp = os.path.join(d, "host_loop.cpp")
    open(cpp, "w").write(HOST_LOOP)
    so = os.path.join(d, "libhost_loop.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-o", so, cpp])
    H = C.CDLL(so)
    H.host_triplets.restype = C.c_int64
    H.host_cross_time.restype = C.c_int64
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    H.host_load(p(hour), p(src), p(dst), p(count), C.c_int64(len(hour)), C.c_int32(R))
    out = np.zeros((max(len(trip), 1) + 16, 3), np.int32)
    t0 = time.perf_counter()
    n_host = H.host_triplets(C.c_int32(R), p(out), C.c_int64(len(out)))
    host_trip_t = time.perf_counter() - t0
    wsum = C.c_int64(0)
    t0 = time.perf_counter()
    host_edges = H.host_cross_time(C.c_int32(R), C.c_int32(8), C.byref(wsum))
    host_edge_t = time.perf_counter() - t0
    assert n_host == len(trip) and np.array_equal(out[:n_host].astype(np.int64), trip), "the two legs disagree on the triplets"
    assert host_edges == len(edges[0]) and wsum.value == int(edges[3].sum()), "the two legs disagree on the window edges"
    text = ("# scripts/flow_windows_rate.py: %d regions, %d table entries, %d planted triples, noise %d x R; one run on one device\n"
            "device  triplets()                 %.4f s (kernels %.4f s)  %d triplets, %d candidates, pairs %d / %d / %d\n"
            "host    one-thread R^3 loop        %.3f s  %d triplets\n"
            "device  window_edges(cross_time 8) %.4f s  %d edges\n"
            "host    one-thread T x R^2 loop    %.3f s  %d edges\n") % (R, len(c), a.planted, a.noise, trip_t, info["kernel_ms"] / 1e3, len(trip), info["candidates"], info["pairs_12"],
                                                                       info["pairs_23"], info["pairs_31"], host_trip_t, n_host, edge_t, len(edges[0]), host_edge_t, host_edges)
    print(text, end="")
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
