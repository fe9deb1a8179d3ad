// od_parse.h — the two kinds of token of a .od flow line "src dst w" (include/dge.h: dge_graph_add_od_texts): a region id to its int64 and a weight to the
// binary64 nearest its exact decimal value, ties to even — what glibc's strtoll and strtod return in the "C" locale.  Plain C++ for host and device, integer
// arithmetic only — no floating-point operation decides a bit.  The device kernel (od_read.hip: k_od_parse) runs it a lane per line;
// tests/native/od_parse_harness.cpp builds it with g++ and compares it with strtoll and strtod.
//
// An id token is   [+-] digits   with a value in the int64 range; leading zeros are allowed ("007" is 7).  Everything else is no id.
//
// A weight token is a value token of the .vec grammar (vec_parse.h):   [+-] digits [ . digits ] [ (e|E) [+-] digits ]   with at least one mantissa digit,  or
// [+-] (inf | infinity | nan)  in any letter case; everything else is VEC_PARSE_BAD.  The value is found as in vec_parse_f32 — the first 19 significant digits
// make w < 10^19 and a decimal exponent e; the value is (Num / Den) * 2^e with Num = w * 5^e, Den = 1 (e >= 0) or Num = w, Den = 5^-e (e < 0), both held in
// 128 bits — only the shift-and-subtract division of the two, each normalised to bit 126, is carried further: 56 bits of quotient and whether anything is
// left behind them, which is more than the 53 bits (fewer in the denormals), the guard bit and the sticky bit that round-half-even needs, exactly.
// Decided here: every zero, inf and nan; every token of at most 19 significant digits whose Num and Den stay below 2^127 (e >= 0: bits(w) + bits(5^e) <= 127,
// which admits e <= 27 for any w; e < 0: e >= -54) — that contains every integer of up to 19 digits, all a "%d" writer writes; and every token that is far
// outside the format whatever its digits say: >= 1e309 is +-inf (the largest binary64 is 1.797..e308), < 1e-324 is +-0 (half the least denormal is 2.47e-324).
// Everything else is VEC_PARSE_HOST: well-formed, finished by the caller with strtod.  A result never depends on which path took a token: both are the
// correctly rounded value.
#pragma once
#include "vec_parse.h"

// p[0 .. n): the token's bytes.  true: *out is the id
VEC_HD bool od_parse_id(const uint8_t* p, int64_t n, int64_t* out) {
    int64_t i = 0;
    bool neg = false;
    if (i < n && (p[i] == '+' || p[i] == '-')) { neg = p[i] == '-'; i++; }
    if (i >= n) return false;
    uint64_t v = 0;
    int nd = 0;                      // significant digits in v
    for (; i < n; i++) {
        const uint32_t d = (uint32_t)p[i] - '0';
        if (d > 9u) return false;
        if (nd == 0 && d == 0) continue;                                // a leading zero
        if (++nd > 19) return false;                                    // 10^19 > 2^63; 19 digits stay below 2^64
        v = v * 10u + d;
    }
    if (v > (neg ? 0x8000000000000000ull : 0x7FFFFFFFFFFFFFFFull)) return false;
    *out = (int64_t)(neg ? 0ull - v : v);
    return true;
}

// (q + f) * 2^X with 2^54 <= q < 2^56 and 0 <= f < 1, f != 0 exactly when sticky: the bits of the nearest binary64, ties to even; overflow gives inf
VEC_HD uint64_t od_round_f64(uint64_t q, bool sticky, int64_t X) {
    const int h = 63 - __builtin_clzll(q);
    const int64_t E2 = h + X;                               // 2^E2 <= value < 2^(E2 + 1)
    if (E2 >= 1024) return 0x7FF0000000000000ull;
    int64_t shift = h - 52;                                 // normal: 53 bits stay (shift is 2 or 3)
    if (-1074 - X > shift) shift = -1074 - X;               // denormal: the last bit kept weighs 2^-1074
    if (shift > 60) return 0ull;                            // below 2^-1078
    const uint64_t m = q >> shift, rem = q - (m << shift), half = 1ull << (shift - 1);
    uint64_t mant = m;
    if (rem > half || (rem == half && (sticky || (mant & 1ull)))) mant++;
    const int64_t biased = E2 + 1022 > 0 ? E2 + 1022 : 0;   // a mantissa that reaches 2^53 (or 2^52 in the denormals) carries into the exponent by itself
    const uint64_t bits = ((uint64_t)biased << 52) + mant;
    return bits >= 0x7FF0000000000000ull ? 0x7FF0000000000000ull : bits;
}

// p[0 .. n): the token's bytes (no whitespace among them).  VEC_PARSE_OK: *bits is the value (inf and nan included: the caller decides what they mean).
VEC_HD int od_parse_f64(const uint8_t* p, int64_t n, uint64_t* bits) {
    int64_t i = 0;
    uint64_t sign = 0;
    if (i < n && (p[i] == '+' || p[i] == '-')) { sign = p[i] == '-' ? 0x8000000000000000ull : 0ull; i++; }
    if (i >= n) return VEC_PARSE_BAD;
    if ((p[i] | 0x20u) == 'i' || (p[i] | 0x20u) == 'n') {
        if (vec_word_is(p + i, n - i, "inf", 3) || vec_word_is(p + i, n - i, "infinity", 8)) { *bits = sign | 0x7FF0000000000000ull; return VEC_PARSE_OK; }
        if (vec_word_is(p + i, n - i, "nan", 3)) { *bits = sign | 0x7FF8000000000000ull; return VEC_PARSE_OK; }
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
    if (nd - 1 + dec >= 309) { *bits = sign | 0x7FF0000000000000ull; return VEC_PARSE_OK; }      // >= 1e309: above the largest double by more than half a step
    if (nd + dec <= -324) { *bits = sign; return VEC_PARSE_OK; }                               // < 1e-324: below half of the least denormal (2.47e-324)
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
    uint64_t q = 0;
    for (int s = 0; s < 56; s++) {                                      // a < 2 b throughout: a - b < b, doubled it is < 2 b < 2^128
        q <<= 1;
        if (a >= b) { a -= b; q |= 1ull; }
        a <<= 1;
    }
    // num / den = (a0 / b) * 2^(mn - md) and q = floor((a0 / b) * 2^55), a0 / b in (1/2, 2): q >= 2^54
    *bits = sign | od_round_f64(q, a != 0, (int64_t)mn - md - 55 + dec);
    return VEC_PARSE_OK;
}
