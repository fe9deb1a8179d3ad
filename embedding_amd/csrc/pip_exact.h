// pip_exact.h — the exact point-in-polygon predicate of trip_map.hip, compilable for the host (tests/native/pip_exact_harness.cpp, scripts/trip_map_rate.py)
// and the device.  Outside the build stamp: no training launch reads anything decided here.
//
//   pip_in_domain(v)        v is finite and either 0 or of magnitude in [2^-450, 2^500]: no exact product below can overflow or lose bits to underflow
//   pip_side(a, b, p)       the sign of (b.x-a.x)(p.y-a.y) - (b.y-a.y)(p.x-a.x) in EXACT arithmetic over the six binary64 inputs: > 0 when p lies to the
//                           left of the line a -> b, 0 when on it.  Stage A is Shewchuk's filter (Adaptive Precision Floating-Point Arithmetic and Fast Robust
//                           Geometric Predicates, 1997, orient2d): the determinant of the rounded differences decides when it exceeds (3 + 16 eps) eps
//                           (|left| + |right|), eps = 2^-53, or when the two products differ in sign.  Otherwise the determinant is expanded over the inputs —
//                           ax*ay cancels, six products remain —, every product is taken as an exact (hi, lo) pair by an fma (two-product), and the twelve
//                           words are added into one non-overlapping expansion by grow-expansion (two-sum); the sign is that of its leading non-zero word.
//                           In the domain the differences are at least 2^-502 or 0, the products of the filter at least 2^-1004, the low words of the exact
//                           products multiples of 2^-1004 and every sum below 2^1004: nothing underflows, nothing overflows, every step is exact.
//   pip_step(a, b, p, st)   one segment of one ring in the ray-crossing rule (what JTS's RayCrossingCounter decides, J/Tracts.java:71-102 through
//                           MultiPolygon.contains): p on the segment, its ends included, sets st.boundary; the segment is CROSSED by the ray from p towards +x
//                           when exactly one of a.y, b.y is > p.y and p lies strictly on the ray's side of the line, and a crossing flips st.parity.
//                           st.exact counts the side tests that went past the filter.
//   pip_cell(v, v0, inv, n) the index cell of a coordinate: ONE monotone function for building the cell lists and for looking points up.
//
// The translation units that include this are compiled with -ffp-contract=off; the only fused operations are the fma calls written out below.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PIP_HD __host__ __device__ inline
#else
#define PIP_HD static inline
#endif

struct pip_state { int parity; int boundary; uint64_t exact; };

PIP_HD bool pip_in_domain(double v) {
    const double m = fabs(v);
    return v == 0.0 || (m >= 0x1p-450 && m <= 0x1p500);        // (a NaN fails both)
}

PIP_HD void pip_two_sum(double a, double b, double* s, double* e) {      // a + b = s + e exactly (Knuth)
    const double x = a + b, bv = x - a, av = x - bv;
    *s = x;
    *e = (a - av) + (b - bv);
}

// e[0 .. n) non-overlapping, increasing in magnitude; adds b: e[0 .. n]
PIP_HD void pip_grow(double* e, int n, double b) {
    double q = b;
    for (int i = 0; i < n; i++) { double s, lo; pip_two_sum(q, e[i], &s, &lo); e[i] = lo; q = s; }
    e[n] = q;
}

PIP_HD int pip_side_exact(double ax, double ay, double bx, double by, double px, double py) {
    // (bx-ax)(py-ay) - (by-ay)(px-ax) = bx*py - bx*ay - ax*py - by*px + by*ax + ay*px
    const double f[6][2] = {{bx, py}, {-bx, ay}, {-ax, py}, {-by, px}, {by, ax}, {ay, px}};
    double e[12];
    int n = 0;
    for (int k = 0; k < 6; k++) {
        const double hi = f[k][0] * f[k][1];
        const double lo = fma(f[k][0], f[k][1], -hi);
        pip_grow(e, n, lo); n++;
        pip_grow(e, n, hi); n++;
    }
    for (int i = n - 1; i >= 0; i--) {
        if (e[i] > 0.0) return 1;
        if (e[i] < 0.0) return -1;
    }
    return 0;
}

PIP_HD int pip_side(double ax, double ay, double bx, double by, double px, double py, uint64_t* exact) {
    const double left = (bx - ax) * (py - ay), right = (by - ay) * (px - ax);
    const double det = left - right;
    double sum;
    if (left > 0.0) { if (right <= 0.0) return det > 0.0 ? 1 : (det < 0.0 ? -1 : 0); sum = left + right; }
    else if (left < 0.0) { if (right >= 0.0) return det > 0.0 ? 1 : (det < 0.0 ? -1 : 0); sum = -left - right; }
    else return right < 0.0 ? 1 : (right > 0.0 ? -1 : 0);      // left == 0: a factor is an exact 0, the sign is that of -right, which is exact in sign
    const double bound = (3.0 + 16.0 * 0x1p-53) * 0x1p-53 * sum;
    if (det >= bound) return 1;
    if (-det >= bound) return -1;
    ++*exact;
    return pip_side_exact(ax, ay, bx, by, px, py);
}

PIP_HD void pip_step(double ax, double ay, double bx, double by, double px, double py, pip_state* st) {
    if ((px == ax && py == ay) || (px == bx && py == by)) { st->boundary = 1; return; }
    if (ay == py && by == py) {                                 // on the ray's line: p is on it or it is not crossed
        const double lo = ax < bx ? ax : bx, hi = ax < bx ? bx : ax;
        if (px >= lo && px <= hi) st->boundary = 1;
        return;
    }
    if ((ay > py) == (by > py)) return;                         // both ends above the ray's line, or neither: not crossed, and p (not an end) is not on it
    if (ax < px && bx < px) return;                             // wholly behind the ray's origin
    if (ax > px && bx > px) { st->parity ^= 1; return; }        // wholly in front of it, one end above the line and one not: crossed
    int s = pip_side(ax, ay, bx, by, px, py, &st->exact);
    if (s == 0) { st->boundary = 1; return; }                   // on the line, between the ends' ordinates: on the segment
    if (by < ay) s = -s;                                        // the segment taken upwards: the crossing lies towards +x when p is to its left
    if (s > 0) st->parity ^= 1;
}

// v0 = the low edge of the index, inv = cells per unit (0 for an index without extent), n >= 1 cells.  Monotone in v: the subtraction and the product by a
// non-negative constant are, and so are the clamps.
PIP_HD int32_t pip_cell(double v, double v0, double inv, int32_t n) {
    const double t = (v - v0) * inv;
    if (!(t > 0.0)) return 0;
    if (t >= (double)n) return n - 1;
    return (int32_t)t;
}
