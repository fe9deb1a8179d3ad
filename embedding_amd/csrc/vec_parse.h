// vec_parse.h — one value token of a .vec file to the binary32 nearest its exact decimal value, ties to even: what glibc's strtof returns in the "C" locale
// (include/dge.h: dge_vectors_from_vec_text).  Plain C++ for host and device, integer arithmetic only — no floating-point operation decides a bit.  The
// device kernel (vec_read.hip: k_vec_parse) runs it a lane per token; tests/native/vec_parse_harness.cpp builds it with g++ and compares it with strtof.
//
// A token is   [+-] digits [ . digits ] [ (e|E) [+-] digits ]   with at least one mantissa digit,  or  [+-] (inf | infinity | nan)  in any letter case.
// Everything else — hex floats, nan(...), "1e", ".", a trailing letter — is VEC_PARSE_BAD.
//
// The value.  Leading zeros go; the first 19 significant digits make w < 10^19 < 2^64 and a decimal exponent e, so that the token says w * 10^e when no
// digit behind the 19th is non-zero.  10^e = 5^e * 2^e: the power of two only moves the binary exponent, so the value is (Num / Den) * 2^e with
//   e >= 0:  Num = w * 5^e,  Den = 1          e < 0:  Num = w,  Den = 5^-e
// both held in 128 bits.  A shift-and-subtract division of the two, each normalised to bit 126, gives the first 28 bits of the quotient and whether anything
// is left behind them: more than the 24 bits (fewer in the denormals) and the sticky bit that round-half-even needs, exactly.
// Decided here: every zero, inf and nan; every token of at most 19 significant digits whose Num and Den stay below 2^127 (e >= 0: bits(w) + bits(5^e) <= 127,
// which admits e <= 27 for any w and e <= 41 for nine digits; e < 0: e >= -54) — that contains every such token with |value| in [1e-10, 1e10], the writer's
// whole fast range; and every token that is far outside the format whatever its digits say: >= 1e39 is +-inf, < 1e-46 is +-0.
// Everything else is VEC_PARSE_HOST: well-formed, finished by the caller with strtof.  A result never depends on which path took a token: both are the
// correctly rounded value.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VEC_HD __host__ __device__ inline
#else
#define VEC_HD static inline
#endif

enum { VEC_PARSE_OK = 0, VEC_PARSE_HOST = 1, VEC_PARSE_BAD = 2 };

typedef unsigned __int128 vec_u128;

VEC_HD int vec_msb128(vec_u128 x) {          // position of the highest set bit; x != 0
    const uint64_t hi = (uint64_t)(x >> 64), lo = (uint64_t)x;
    return hi ? 127 - __builtin_clzll(hi) : 63 - __builtin_clzll(lo);
}

// (q + f) * 2^X with 2^26 <= q < 2^28 and 0 <= f < 1, f != 0 exactly when sticky: the bits of the nearest binary32, ties to even; overflow gives inf
VEC_HD uint32_t vec_round_f32(uint32_t q, bool sticky, int64_t X) {
    const int h = 31 - __builtin_clz(q);
    const int64_t E2 = h + X;                               // 2^E2 <= value < 2^(E2 + 1)
    if (E2 >= 128) return 0x7F800000u;
    int64_t shift = h - 23;                                 // normal: 24 bits stay
    if (-149 - X > shift) shift = -149 - X;                 // denormal: the last bit kept weighs 2^-149
    if (shift > 40) return 0u;                              // below 2^-160
    const uint64_t Q = q;
    const uint64_t m = shift >= 32 ? 0 : (Q >> shift), rem = Q - (m << shift), half = 1ull << (shift - 1);
    uint32_t mant = (uint32_t)m;
    if (rem > half || (rem == half && (sticky || (mant & 1u)))) mant++;
    const int64_t biased = E2 + 126 > 0 ? E2 + 126 : 0;     // a mantissa that reaches 2^24 (or 2^23 in the denormals) carries into the exponent by itself
    const uint64_t bits = ((uint64_t)biased << 23) + mant;
    return bits >= 0x7F800000ull ? 0x7F800000u : (uint32_t)bits;
}

VEC_HD bool vec_word_is(const uint8_t* p, int64_t n, const char* lower, int64_t len) {
    if (n != len) return false;
    for (int64_t i = 0; i < n; i++) if ((p[i] | 0x20u) != (uint8_t)lower[i]) return false;
    return true;
}

// p[0 .. n): the token's bytes (no whitespace among them).  VEC_PARSE_OK: *bits is the value.
VEC_HD int vec_parse_f32(const uint8_t* p, int64_t n, uint32_t* bits) {
    int64_t i = 0;
    uint32_t sign = 0;
    if (i < n && (p[i] == '+' || p[i] == '-')) { sign = p[i] == '-' ? 0x80000000u : 0u; i++; }
    if (i >= n) return VEC_PARSE_BAD;
    if ((p[i] | 0x20u) == 'i' || (p[i] | 0x20u) == 'n') {
        if (vec_word_is(p + i, n - i, "inf", 3) || vec_word_is(p + i, n - i, "infinity", 8)) { *bits = sign | 0x7F800000u; return VEC_PARSE_OK; }
        if (vec_word_is(p + i, n - i, "nan", 3)) { *bits = sign | 0x7FC00000u; return VEC_PARSE_OK; }
        return VEC_PARSE_BAD;
    }
    // ---- mantissa: w = the first 19 significant digits, dec = the power of ten that goes with them, tail = a non-zero digit was left out
    uint64_t w = 0;
    int nd = 0;                      // significant digits in w
    int64_t dec = 0, digits = 0;
    bool tail = false, point = false;
    for (; i < n; i++) {
        const uint32_t c = p[i];
        if (c == '.') { if (point) return VEC_PARSE_BAD; point = true; continue; }
        const uint32_t d = c - '0';
        if (d > 9u) break;
        digits++;
        if (nd == 0 && d == 0) { if (point) dec--; continue; }          // a leading zero
        if (nd < 19) { w = w * 10u + d; nd++; if (point) dec--; }
        else { if (d) tail = true; if (!point) dec++; }
    }
    if (digits == 0) return VEC_PARSE_BAD;
    if (i < n) {
        if ((p[i] | 0x20u) != 'e') return VEC_PARSE_BAD;
        i++;
        bool neg = false;
        if (i < n && (p[i] == '+' || p[i] == '-')) { neg = p[i] == '-'; i++; }
        if (i >= n) return VEC_PARSE_BAD;
        int64_t x = 0;
        for (; i < n; i++) {
            const uint32_t d = (uint32_t)p[i] - '0';
            if (d > 9u) return VEC_PARSE_BAD;
            if (x < 1000000000000000LL) x = x * 10 + d;                // beyond any exponent that matters: stays huge
        }
        dec += neg ? -x : x;
    }
    if (nd == 0) { *bits = sign; return VEC_PARSE_OK; }                // zero, whatever the exponent
    // 10^(nd - 1 + dec) <= |value| < 10^(nd + dec), the left-out digits included
    if (nd - 1 + dec >= 39) { *bits = sign | 0x7F800000u; return VEC_PARSE_OK; }      // >= 1e39: above the largest float by more than half a step
    if (nd + dec <= -46) { *bits = sign; return VEC_PARSE_OK; }                      // < 1e-46: below half of the least denormal (7.0e-46)
    if (tail) return VEC_PARSE_HOST;
    const int64_t k = dec < 0 ? -dec : dec;
    if (k > 54) return VEC_PARSE_HOST;                                  // 5^54 < 2^126 < 5^55
    vec_u128 p5 = 1;
    for (int64_t j = 0; j < k; j++) p5 *= 5u;
    vec_u128 num, den;
    if (dec >= 0) {
        if ((64 - __builtin_clzll(w)) + (vec_msb128(p5) + 1) > 127) return VEC_PARSE_HOST;
        num = (vec_u128)w * p5; den = 1;
    } else { num = w; den = p5; }
    const int mn = vec_msb128(num), md = vec_msb128(den);
    vec_u128 a = num << (126 - mn);
    const vec_u128 b = den << (126 - md);
    uint32_t q = 0;
    for (int s = 0; s < 28; s++) {                                      // a < 2 b throughout: a - b < b, doubled it is < 2 b < 2^128
        q <<= 1;
        if (a >= b) { a -= b; q |= 1u; }
        a <<= 1;
    }
    // num / den = (a0 / b) * 2^(mn - md) and q = floor((a0 / b) * 2^27), a0 / b in (1/2, 2): q >= 2^26
    *bits = sign | vec_round_f32(q, a != 0, (int64_t)mn - md - 27 + dec);
    return VEC_PARSE_OK;
}
