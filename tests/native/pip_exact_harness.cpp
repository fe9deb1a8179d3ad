// Host build of embedding_amd/csrc/pip_exact.h (the per-lane routines of k_trip_locate, trip_map.hip) for tests/test_pip_exact_host.py and
// tests/test_gpu_trip_map.py:
//   g++ -O2 -shared -fPIC -std=c++17 -ffp-contract=off -o libpip_exact_harness.so pip_exact_harness.cpp        the entries below, called through ctypes
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -o pip_exact_harness pip_exact_harness.cpp && ./pip_exact_harness [n_random [seed]]
//                                                         a stand-alone self-check against __int128 arithmetic on integer triples; exit 0 = all equal
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../embedding_amd/csrc/pip_exact.h"

// n triples of 6 doubles (ax ay bx by px py) -> sign[n] in {-1, 0, 1}, went_exact[n] in {0, 1}
extern "C" void harness_pip_side(const double* t, int64_t n, int8_t* sign, uint8_t* went_exact) {
    for (int64_t k = 0; k < n; k++) {
        uint64_t e = 0;
        sign[k] = (int8_t)pip_side(t[6 * k], t[6 * k + 1], t[6 * k + 2], t[6 * k + 3], t[6 * k + 4], t[6 * k + 5], &e);
        went_exact[k] = (uint8_t)e;
    }
}

// the filter alone: what a plain binary64 evaluation of the determinant says
extern "C" void harness_pip_side_plain(const double* t, int64_t n, int8_t* sign) {
    for (int64_t k = 0; k < n; k++) {
        const double* q = t + 6 * k;
        const double det = (q[2] - q[0]) * (q[5] - q[1]) - (q[3] - q[1]) * (q[4] - q[0]);
        sign[k] = det > 0 ? 1 : (det < 0 ? -1 : 0);
    }
}

// one ring-crossing step per (segment, point) pair: n segments of 4 doubles, n points of 2 -> parity flip, boundary, exact
extern "C" void harness_pip_step(const double* seg, const double* p, int64_t n, uint8_t* crossed, uint8_t* boundary, uint8_t* went_exact) {
    for (int64_t k = 0; k < n; k++) {
        pip_state st = {0, 0, 0};
        pip_step(seg[4 * k], seg[4 * k + 1], seg[4 * k + 2], seg[4 * k + 3], p[2 * k], p[2 * k + 1], &st);
        crossed[k] = (uint8_t)st.parity; boundary[k] = (uint8_t)st.boundary; went_exact[k] = (uint8_t)st.exact;
    }
}

// every point against every segment of every region whose bounding box contains it (no index): region[i] = the least interior region or -1,
// counters = located, on_boundary, multi, outside, exact — what dge_locate_info reports
extern "C" void harness_pip_locate(const double* seg, const int64_t* seg_first, int64_t R, const double* xy, int64_t n, int32_t* region, int64_t* counters) {
    std::vector<double> box((size_t)R * 4);
    for (int64_t r = 0; r < R; r++) {
        double b[4] = {1, 1, -1, -1};
        for (int64_t s = seg_first[r]; s < seg_first[r + 1]; s++)
            for (int e = 0; e < 2; e++) {
                const double x = seg[4 * s + 2 * e], y = seg[4 * s + 2 * e + 1];
                if (b[0] > b[2]) { b[0] = b[2] = x; b[1] = b[3] = y; }
                if (x < b[0]) b[0] = x;
                if (x > b[2]) b[2] = x;
                if (y < b[1]) b[1] = y;
                if (y > b[3]) b[3] = y;
            }
        memcpy(&box[(size_t)r * 4], b, sizeof(b));
    }
    for (int k = 0; k < 5; k++) counters[k] = 0;
    for (int64_t i = 0; i < n; i++) {
        const double px = xy[2 * i], py = xy[2 * i + 1];
        int32_t result = -1;
        int interior = 0, on = 0, in_any = 0;
        if (pip_in_domain(px) && pip_in_domain(py))
            for (int64_t r = 0; r < R; r++) {
                const double* b = &box[(size_t)r * 4];
                if (!(px >= b[0] && px <= b[2] && py >= b[1] && py <= b[3])) continue;
                in_any = 1;
                pip_state st = {0, 0, 0};
                for (int64_t s = seg_first[r]; s < seg_first[r + 1]; s++) pip_step(seg[4 * s], seg[4 * s + 1], seg[4 * s + 2], seg[4 * s + 3], px, py, &st);
                counters[4] += (int64_t)st.exact;
                if (st.boundary) on = 1;
                else if (st.parity) { if (result < 0) result = (int32_t)r; interior++; }
            }
        region[i] = result;
        counters[0] += result >= 0; counters[1] += result < 0 && on; counters[2] += interior > 1; counters[3] += !in_any;
    }
}

namespace {

struct Rng {      // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    int64_t within(int64_t m) { return (int64_t)(next() % (uint64_t)(2 * m + 1)) - m; }
};

}  // namespace

// integer coordinates below 2^30 in magnitude: the determinant is exact in __int128.  Half the triples are made collinear or one unit off.
extern "C" int64_t harness_pip_selfcheck(int64_t n, uint64_t seed, int64_t* counts) {
    Rng rng{seed};
    int64_t wrong = 0;
    counts[0] = counts[1] = counts[2] = 0;      // triples, went past the filter, zeros
    for (int64_t k = 0; k < n; k++) {
        const int64_t M = (k & 1) ? 1000 : (int64_t)1 << 29;
        int64_t ax = rng.within(M), ay = rng.within(M), dx = rng.within(1000), dy = rng.within(1000), m = rng.within(1000);
        int64_t bx = ax + dx, by = ay + dy, px = ax + m * dx, py = ay + m * dy;
        const int kind = (int)(rng.next() % 4);
        if (kind == 1) px += rng.within(1);
        if (kind == 2) py += rng.within(1);
        if (kind == 3) { px = rng.within(M); py = rng.within(M); }
        const __int128 det = (__int128)(bx - ax) * (py - ay) - (__int128)(by - ay) * (px - ax);
        const int want = det > 0 ? 1 : (det < 0 ? -1 : 0);
        // scaled by a power of two to both ends of the domain: exact, the sign is unchanged
        const double scale[3] = {1.0, 0x1p-440, 0x1p460};
        for (int sc = 0; sc < 3; sc++) {
            uint64_t e = 0;
            const double f = scale[sc];
            const int got = pip_side((double)ax * f, (double)ay * f, (double)bx * f, (double)by * f, (double)px * f, (double)py * f, &e);
            wrong += got != want;
            counts[0]++; counts[1] += (int64_t)e; counts[2] += want == 0;
        }
    }
    return wrong;
}

int main(int argc, char** argv) {
    const int64_t n = argc > 1 ? atoll(argv[1]) : 300000;
    const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    int64_t counts[3];
    const int64_t wrong = harness_pip_selfcheck(n, seed, counts);
    // the ulp lattice: segment (-12,-12)-(24,24), points (0.5 + i 2^-53, 0.5 + j 2^-53): the sign is that of j - i
    int64_t lattice_wrong = 0, plain_wrong = 0;
    for (int i = 0; i < 64; i++)
        for (int j = 0; j < 64; j++) {
            const double t[6] = {-12, -12, 24, 24, 0.5 + i * 0x1p-53, 0.5 + j * 0x1p-53};
            int8_t s, p;
            uint8_t e;
            harness_pip_side(t, 1, &s, &e);
            harness_pip_side_plain(t, 1, &p);
            const int want = j > i ? 1 : (j < i ? -1 : 0);
            lattice_wrong += s != want; plain_wrong += p != want;
            const double seg[4] = {-12, -12, 24, 24};
            uint8_t c, b, x;
            harness_pip_step(seg, t + 4, 1, &c, &b, &x);
            lattice_wrong += (b != 0) != (i == j);
        }
    printf("triples %lld past_filter %lld zeros %lld wrong %lld lattice_wrong %lld plain_wrong %lld \n", (long long)counts[0], (long long)counts[1], (long long)counts[2], (long long)wrong,
           (long long)lattice_wrong, (long long)plain_wrong);
    return wrong == 0 && lattice_wrong == 0 ? 0 : 1;
}
