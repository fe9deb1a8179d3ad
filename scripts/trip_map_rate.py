"""Rate of mapping trips into regions (include/dge.h: dge_flows_add_trips_device) next to a one-thread C++ loop shaped like Tracts.mapTripsIntoTracts
(J/Tracts.java:71-102): every region in turn, a bounding-box reject, then the same csrc/pip_exact.h test, until both ends are found.

    python scripts/trip_map_rate.py [--mesh 28] [--subdivide 50] [--trips 20000000] [--host-trips 200000] [--out profiles/trip_map.txt]

The regions are the quad mesh of tests/trip_ref.py with every edge cut into `subdivide` pieces (28 x 28 quads of about 200 segments: the tract workload's
shape).  Device: the trips are generated on the host, copied once, and add_trips_device is timed with the wall clock around a synchronised call, median of
three after a warm-up; kernel_ms is the library's own event time.  Host: the loop is built here with g++ -O2 and timed on a smaller number of trips (it is
slow); rates are per point (two points a trip).  One process; numbers from one run on one device, not a distribution."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HOST_LOOP = r"""
#include <stdint.h>
#include <vector>
#include "%s"
extern "C" int64_t host_map(const double* seg, const int64_t* seg_first, const double* box, int64_t R, const double* s, const double* e, int64_t n, int64_t* mapped) {
    int64_t m = 0;
    for (int64_t i = 0; i < n; i++) {
        int64_t rs = -1, re = -1;
        for (int64_t r = 0; r < R && (rs < 0 || re < 0); r++) {
            const double* b = box + 4 * r;
            for (int end = 0; end < 2; end++) {
                const double px = end ? e[2 * i] : s[2 * i], py = end ? e[2 * i + 1] : s[2 * i + 1];
                if ((end ? re : rs) >= 0 || !(px >= b[0] && px <= b[2] && py >= b[1] && py <= b[3])) continue;
                pip_state st = {0, 0, 0};
                for (int64_t k = seg_first[r]; k < seg_first[r + 1]; k++) pip_step(seg[4 * k], seg[4 * k + 1], seg[4 * k + 2], seg[4 * k + 3], px, py, &st);
                if (!st.boundary && st.parity) (end ? re : rs) = r;
            }
        }
        m += rs >= 0 && re >= 0;
    }
    *mapped = m;
    return 0;
}
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", type=int, default=28)
    ap.add_argument("--subdivide", type=int, default=50)
    ap.add_argument("--trips", type=int, default=20_000_000)
    ap.add_argument("--host-trips", type=int, default=200_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trip_map.txt"))
    a = ap.parse_args()
    import torch
    import trip_ref

    import embedding_amd as E
    ref, _ = trip_ref.quad_mesh(a.mesh, 1, subdivide=a.subdivide)
    seg, seg_first = ref.segments()
    rg = E.Regions.from_arrays(*ref.arrays())
    rng = np.random.default_rng(2)
    s = np.stack([rng.uniform(-87.9, -87.4, a.trips), rng.uniform(41.6, 42.1, a.trips)], 1)
    e = np.stack([rng.uniform(-87.9, -87.4, a.trips), rng.uniform(41.6, 42.1, a.trips)], 1)
    h = rng.integers(0, 24, a.trips).astype(np.int32)
    ds, de, dh = torch.from_numpy(s).cuda(), torch.from_numpy(e).cuda(), torch.from_numpy(h).cuda()
    times, kernel = [], []
    for _ in range(4):
        f = E.Flows(rg)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f.add_trips(ds, de, dh)
        times.append(time.perf_counter() - t0)
        kernel.append(f.info()["kernel_ms"] / 1e3)
        mapped = f.info()["mapped"]
    dev_t, dev_k = float(np.median(times[1:])), float(np.median(kernel[1:]))
    d = tempfile.mkdtemp()
    src = os.path.join(d, "host_loop.cpp")
    open(src, "w").write(HOST_LOOP % os.path.join(ROOT, "embedding_amd", "csrc", "pip_exact.h"))
    so = os.path.join(d, "libhost_loop.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-o", so, src])
    H = C.CDLL(so)
    box = np.array([[sg[:, [0, 2]].min(), sg[:, [1, 3]].min(), sg[:, [0, 2]].max(), sg[:, [1, 3]].max()] for sg in (seg[seg_first[r]:seg_first[r + 1]] for r in range(len(ref.ids)))])
    m = C.c_int64(0)
    n = min(a.host_trips, a.trips)
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    t0 = time.perf_counter()
    H.host_map(p(seg), p(seg_first), p(box), len(ref.ids), p(s), p(e), n, C.byref(m))
    host_t = time.perf_counter() - t0
    dev_rate, host_rate = 2 * a.trips / dev_t, 2 * n / host_t
    text = ("# scripts/trip_map_rate.py: %d x %d regions, %d segments, grid %d; one run on one device\n"
            "device  add_trips_device  %d trips  %.3f s (kernels %.3f s, %.0f %%)  %.3e points/s  mapped %d\n"
            "host    one-thread loop   %d trips  %.3f s  %.3e points/s  mapped %d\n"
            "ratio   device / host     %.1f\n") % (a.mesh, a.mesh, len(seg), rg.info()["grid"], a.trips, dev_t, dev_k, 100 * dev_k / dev_t, dev_rate, mapped, n, host_t, host_rate, m.value,
                                                  dev_rate / host_rate)
    print(text, end="")
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
