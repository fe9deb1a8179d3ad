// tree_rule.h — the per-element pieces of the decision-tree rule of include/dge.h, compiled for host and device: the order-preserving key of a float32 value,
// the score of a candidate split as a rational of integers and the ONE comparator that decides between two candidates, the threshold between two
// neighbouring values, the leaf test and the leaf vote.  Nothing here is floating point except tr_threshold's two operations and tr_goes_left's comparison.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TR_HD __host__ __device__ __forceinline__
#else
#define TR_HD static inline
#endif

#define TR_MAX_ROWS (1LL << 20)      // rows that train one tree, at most: N <= 2^58 and Dn <= 2^38 below, their cross products fit 128 bits
#define TR_MAX_FOLDS 64

// the bits of a finite float as an unsigned integer that orders as the value does; -0.0 and +0.0 share one key
TR_HD uint32_t tr_key_bits(uint32_t bits) {
    if (bits == 0x80000000u) bits = 0u;
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
TR_HD uint32_t tr_unkey_bits(uint32_t key) { return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key; }
TR_HD bool tr_finite_bits(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u; }
#if !defined(__HIP_DEVICE_COMPILE__)
static inline uint32_t tr_key(float x) { uint32_t b; memcpy(&b, &x, 4); return tr_key_bits(b); }
static inline float tr_unkey(uint32_t key) { const uint32_t b = tr_unkey_bits(key); float x; memcpy(&x, &b, 4); return x; }
#endif

// the score S = (pL^2 + qL^2) / nL + (pR^2 + qR^2) / nR of the cut of a node (n rows, p of label 1) that sends nL rows, pL of label 1, left: S = N / Dn.
// 1 <= nL < n <= 2^20: pL^2 + qL^2 <= nL^2, so N <= nL nR n <= 2^58, and Dn <= n^2 / 4 <= 2^38.
TR_HD void tr_score(int64_t n, int64_t p, int64_t nL, int64_t pL, uint64_t* N, uint64_t* Dn) {
    const uint64_t nR = (uint64_t)(n - nL), pR = (uint64_t)(p - pL), qL = (uint64_t)(nL - pL), qR = nR - pR;
    *N = ((uint64_t)pL * (uint64_t)pL + qL * qL) * nR + (pR * pR + qR * qR) * (uint64_t)nL;
    *Dn = (uint64_t)nL * nR;
}

// the 128-bit product of two uint64 as (hi, lo)
TR_HD void tr_mul128(uint64_t a, uint64_t b, uint64_t* hi, uint64_t* lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    *hi = __umul64hi(a, b);
    *lo = a * b;
#else
    const unsigned __int128 r = (unsigned __int128)a * b;
    *hi = (uint64_t)(r >> 64);
    *lo = (uint64_t)r;
#endif
}

// -1 / 0 / +1 as N1 / D1 is less than / equal to / greater than N2 / D2 (D1, D2 > 0): N1 D2 against N2 D1 in 128 bits
TR_HD int tr_score_cmp(uint64_t N1, uint64_t D1, uint64_t N2, uint64_t D2) {
    uint64_t h1, l1, h2, l2;
    tr_mul128(N1, D2, &h1, &l1);
    tr_mul128(N2, D1, &h2, &l2);
    if (h1 != h2) return h1 < h2 ? -1 : 1;
    if (l1 != l2) return l1 < l2 ? -1 : 1;
    return 0;
}

// a candidate: its score, its feature and the key of a, the greatest value that goes left.  D = 0: no candidate.
struct tr_cand {
    uint64_t N, D;
    int32_t f;
    uint32_t a;
};

// THE comparator: does x win against y?  The greater score, then the lesser feature, then the lesser a.  A total order on candidates that differ in (f, a);
// no candidate loses against any candidate.
TR_HD bool tr_better(const tr_cand& x, const tr_cand& y) {
    if (x.D == 0) return false;
    if (y.D == 0) return true;
    const int c = tr_score_cmp(x.N, x.D, y.N, y.D);
    if (c) return c > 0;
    if (x.f != y.f) return x.f < y.f;
    return x.a < y.a;
}

// m = RN(RN((double)a + (double)b) * 0.5) for float32 a < b.  a <= m < b: 2a and 2b are binary64 values and rounding is monotone, so 2a <= RN(a + b) <= 2b;
// halving a binary64 value is exact unless it is subnormal, and a sum of two float32 values (multiples of 2^-149) that is not zero is at least 2^-149 in
// magnitude, far from binary64's subnormals: a <= m <= b.  m = b would need RN(a + b) = 2b, that is b - a at most half a binary64 ulp of 2b, about 2^-52 |b|;
// but a float32 a < b lies at least one float32 step below b, about 2^-24 |b| (and for b = 0 the sum is a itself, m = a / 2 < 0).  So m < b.
TR_HD double tr_threshold(float a, float b) {
    const double s = (double)a + (double)b;
    return s * 0.5;
}
TR_HD bool tr_goes_left(float x, double m) { return (double)x <= m; }

// the limits of struct dge_tree_cfg as the rule reads them (0 = no depth limit)
struct tr_limits {
    int32_t max_depth, min_samples_split, min_samples_leaf;
};
// a node that cannot split whatever its rows hold
TR_HD bool tr_is_leaf(int64_t n, int64_t p, int32_t depth, const tr_limits& lim) {
    return p == 0 || p == n || n < (int64_t)lim.min_samples_split || (lim.max_depth > 0 && depth >= lim.max_depth);
}
TR_HD bool tr_valid_cut(int64_t n, int64_t nL, const tr_limits& lim) { return nL >= (int64_t)lim.min_samples_leaf && n - nL >= (int64_t)lim.min_samples_leaf; }
TR_HD uint8_t tr_vote(int64_t n, int64_t p) { return 2 * p > n ? 1 : 0; }
