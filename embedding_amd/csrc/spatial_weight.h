// spatial_weight.h — the spatial graph's geometry and edge weight, written once for the kernels of spatial.hip and for the host
// (tests/native/spatial_weight_harness.cpp): the centroid chain of one region, the distance of two centroids and w = E((-d) * scale) of include/dge.h.
//
// Every operation is a rounded binary64 + - * / or sqrt in the order written; compile with -ffp-contract=off and write no fma, so that the device, the
// host harness and tests/spatial_ref.py (Python floats) give the same bits.  Outside the build stamp: nothing here is read by a training launch.
//
// E(x) for x <= 0 is shaped like fdlibm's e_exp (the algorithm java.lang.StrictMath.exp is defined by, as recalled — its source is not consulted here):
//   x < SW_UNDER                 0                       (exp(x) < 2^-1075; -inf included)
//   x >= -2^-28                  1 + x                   (-0.0 and 0 give 1)
//   x >= -SW_HALF_LN2            k = 0, r = x, hi = x, lo = 0
//   x >  -SW_3HALF_LN2           k = -1, hi = x + ln2HI, lo = -ln2LO
//   else                         k = (int)(invln2 * x - 0.5) (truncated), hi = x - k * ln2HI, lo = k * ln2LO
//   r = hi - lo;  t = r * r;  c = r - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))))
//   k == 0:  y = 1 - ((r * c) / (c - 2) - r);   else  y = 1 - ((lo - (r * c) / (2 - c)) - hi)
//   k >= -1021:  y * 2^k (exact);   else  (y * 2^(k + 1000)) * 2^-1000 (the first product exact, the second rounds once into the subnormal range)
// Within 1 ulp of exp(x) and non-increasing as x falls: tests/test_spatial_host.py holds it to both.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SW_HD __host__ __device__ inline
#else
#define SW_HD inline
#endif

#define SW_LN2_HI 0x1.62e42feep-1            /* 6.93147180369123816490e-01 */
#define SW_LN2_LO 0x1.a39ef35793c76p-33      /* 1.90821492927058770002e-10 */
#define SW_INV_LN2 0x1.71547652b82fep+0      /* 1.44269504088896338700e+00 */
#define SW_P1 0x1.555555555553ep-3           /* 1.66666666666666019037e-01 */
#define SW_P2 (-0x1.6c16c16bebd93p-9)        /* -2.77777777770155933842e-03 */
#define SW_P3 0x1.1566aaf25de2cp-14          /* 6.61375632143793436117e-05 */
#define SW_P4 (-0x1.bbd41c5d26bf1p-20)       /* -1.65339022054652515390e-06 */
#define SW_P5 0x1.6376972bea4d0p-25          /* 4.13813679705723846039e-08 */
#define SW_UNDER (-0x1.74910d52d3051p+9)     /* -7.45133219101941108420e+02: below it the result is 0 */
#define SW_HALF_LN2 0x1.62e42fefa39efp-2     /* 0.5 ln2 */
#define SW_3HALF_LN2 0x1.0a2b23f3bab73p+0    /* 1.5 ln2 */
#define SW_TINY 0x1p-28
#define SW_TWOM1000 0x1p-1000

SW_HD double sw_pow2(int k) {                // 2^k for -1022 <= k <= 1023, from its bits
    const uint64_t b = (uint64_t)(k + 1023) << 52;
    double v;
    memcpy(&v, &b, 8);
    return v;
}

// E(x), x <= 0 (x = -0.0 and x = -inf included); see the head of the file
SW_HD double sw_exp_neg(double x) {
    if (x < SW_UNDER) return 0.0;
    if (x >= -SW_TINY) return 1.0 + x;
    double hi = x, lo = 0.0;
    int k = 0;
    if (x < -SW_HALF_LN2) {
        if (x > -SW_3HALF_LN2) { hi = x + SW_LN2_HI; lo = -SW_LN2_LO; k = -1; }
        else {
            k = (int)(SW_INV_LN2 * x - 0.5);
            const double t = (double)k;
            hi = x - t * SW_LN2_HI;
            lo = t * SW_LN2_LO;
        }
    }
    const double r = hi - lo;
    const double t = r * r;
    const double c = r - t * (SW_P1 + t * (SW_P2 + t * (SW_P3 + t * (SW_P4 + t * SW_P5))));
    if (k == 0) return 1.0 - ((r * c) / (c - 2.0) - r);
    const double y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi);
    if (k >= -1021) return y * sw_pow2(k);
    return (y * sw_pow2(k + 1000)) * SW_TWOM1000;
}

// d(i, j) squared, before the square root: dx*dx + dy*dy (may be +inf: finite centroids can overflow it)
SW_HD double sw_dist2(double xi, double yi, double xj, double yj) {
    const double dx = xi - xj, dy = yi - yj;
    return dx * dx + dy * dy;
}

// w(i, j) from the squared distance: E((-sqrt(d2)) * scale); sqrt is correctly rounded on the host and on the device
SW_HD double sw_weight(double d2, double scale) { return sw_exp_neg((-sqrt(d2)) * scale); }

// The centroid chain of one region over its segments (ax ay bx by each, rings in order, the segments of a ring in order); the base point is the first
// vertex of the first ring.  Returns 0 when the area sum is 0 or the centroid is not finite (xy is then not to be used).
SW_HD int sw_centroid(const double* seg, int64_t n_segs, double* cx_out, double* cy_out) {
    if (n_segs <= 0) { *cx_out = 0.0; *cy_out = 0.0; return 0; }
    const double bx = seg[0], by = seg[1];
    double cx = 0.0, cy = 0.0, A = 0.0;
    for (int64_t s = 0; s < n_segs; s++) {
        const double px = seg[4 * s], py = seg[4 * s + 1], qx = seg[4 * s + 2], qy = seg[4 * s + 3];
        const double a2 = (px - bx) * (qy - by) - (qx - bx) * (py - by);
        cx += a2 * (bx + px + qx);
        cy += a2 * (by + py + qy);
        A += a2;
    }
    const double x = cx / 3.0 / A, y = cy / 3.0 / A;
    *cx_out = x; *cy_out = y;
    return (A != 0.0 && (x - x) == 0.0 && (y - y) == 0.0) ? 1 : 0;
}
