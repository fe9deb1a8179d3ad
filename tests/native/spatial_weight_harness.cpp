// Host build of embedding_amd/csrc/spatial_weight.h: what every lane of the kernels of spatial.hip runs for a centroid and for a weight, handed to
// tests/test_spatial_host.py through ctypes.  Build with -ffp-contract=off.  Built as a program (its own main) with -fsanitize=address,undefined it walks
// E over the edge values and a few hundred thousand inputs and the centroid chain over generated rings, and prints what it saw.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../embedding_amd/csrc/spatial_weight.h"

extern "C" {
void harness_exp_neg(const double* x, int64_t n, double* out) { for (int64_t i = 0; i < n; i++) out[i] = sw_exp_neg(x[i]); }
void harness_weight(const double* xi, const double* xj, int64_t n, double scale, double* out) {
    for (int64_t i = 0; i < n; i++) out[i] = sw_weight(sw_dist2(xi[2 * i], xi[2 * i + 1], xj[2 * i], xj[2 * i + 1]), scale);
}
// one region: its segments (ax ay bx by), rings in order
int harness_centroid(const double* seg, int64_t n_segs, double* xy) { return sw_centroid(seg, n_segs, xy, xy + 1); }
// pairs of adjacent doubles x > x' (x' the next double below) with E(x') > E(x), over `n` steps down from x0
int64_t harness_monotone_run(double x0, int64_t n, double* last) {
    int64_t wrong = 0;
    double x = x0, e = sw_exp_neg(x0);
    for (int64_t i = 0; i < n; i++) {
        const double y = nextafter(x, -INFINITY), f = sw_exp_neg(y);
        if (f > e) wrong++;
        x = y; e = f;
    }
    *last = x;
    return wrong;
}
}

int main(int argc, char** argv) {
    const int64_t n = argc > 1 ? atoll(argv[1]) : 200000;
    uint64_t s = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    auto next = [&]() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(s >> 11) * 0x1.0p-53; };
    const double edges[] = {0.0, -0.0, -0x1p-1074, -0x1p-28, -0x1p-29, -SW_HALF_LN2, -SW_3HALF_LN2, -1.0, -708.0, -708.4, -709.78, -745.13, SW_UNDER, -745.14, -1e300, -INFINITY};
    int64_t bad = 0;
    for (double x : edges) { const double e = sw_exp_neg(x); if (!(e >= 0.0 && e <= 1.0)) bad++; }
    if (sw_exp_neg(-INFINITY) != 0.0 || sw_exp_neg(-0.0) != 1.0 || sw_exp_neg(0.0) != 1.0 || sw_exp_neg(-746.0) != 0.0) bad++;
    double prev = 2.0;
    for (int64_t i = 0; i < n; i++) {                      // a descending sweep: the results never rise
        const double x = -750.0 * (double)i / (double)n, e = sw_exp_neg(x);
        if (!(e <= prev) || !(e >= 0.0)) bad++;
        prev = e;
    }
    int64_t zero = 0;
    for (int64_t i = 0; i < n; i++) {
        const double a[2] = {next() * 1e3, next() * 1e3}, b[2] = {next() * 1e3, next() * 1e3};
        const double w = sw_weight(sw_dist2(a[0], a[1], b[0], b[1]), 100.0 * next());
        if (!(w >= 0.0 && w <= 1.0)) bad++;
        if (w == 0.0) zero++;
    }
    if (sw_weight(sw_dist2(1e200, 0, -1e200, 0), 100.0) != 0.0) bad++;         // dx*dx overflows: d = inf, w = 0
    int64_t rings = 0;
    for (int m = 4; m < 400; m += 7) {                     // a ring of m vertices round a circle, closed
        std::vector<double> v, seg;
        for (int i = 0; i < m - 1; i++) { const double t = 6.283185307179586 * i / (m - 1); v.push_back(3.0 + cos(t)); v.push_back(-2.0 + sin(t)); }
        v.push_back(v[0]); v.push_back(v[1]);
        for (int i = 0; i + 1 < m; i++) for (int c = 0; c < 4; c++) seg.push_back(v[2 * i + c]);
        double xy[2];
        if (!sw_centroid(seg.data(), (int64_t)seg.size() / 4, xy, xy + 1) || fabs(xy[0] - 3.0) > 1e-9 || fabs(xy[1] + 2.0) > 1e-9) bad++;
        rings++;
    }
    double xy[2];
    const double flat[8] = {0, 0, 1, 1, 1, 1, 0, 0};
    if (sw_centroid(flat, 2, xy, xy + 1) != 0 || sw_centroid(flat, 0, xy, xy + 1) != 0) bad++;       // zero area, no segment
    printf("inputs %lld zero_weights %lld rings %lld wrong %lld\n", (long long)(2 * n), (long long)zero, (long long)rings, (long long)bad);
    return bad ? 1 : 0;
}
