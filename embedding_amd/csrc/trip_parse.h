// trip_parse.h — one line of a taxi trip file to its record: status, hour, start point, end point (include/dge.h: dge_trips_parse_texts states the rule; the
// reference reads these lines in TaxiTrip(String line) and ShortDate, J/TaxiTrip.java:39-78,199-223).  Plain C++ for host and device, integer arithmetic only —
// no floating-point operation decides a bit: a coordinate is od_parse.h's correctly rounded binary64.  The device kernel (trip_text.hip: k_trip_parse) runs it a
// lane per line; tests/native/trip_parse_harness.cpp builds it with g++ and compares it with tests/trip_text_ref.py.
//
// Nothing here allocates: a split walks the bytes once and notes where its first pieces lie (at most TRIP_MAX_PIECES + 1 of them are ever looked at), then says
// how many pieces there are once the trailing empty ones are gone.
//
// A coordinate od_parse_f64 hands back (VEC_PARSE_HOST) is not decided here: its bit in host_mask is set and where[] says where its bytes lie, so that the
// caller — on the host — finishes it with strtod (trip_finish_host below) whichever side ran the parse.
#pragma once
#include <locale.h>
#include <stdlib.h>

#include <string>

#include "od_parse.h"

enum { TRIP_OK = 0, TRIP_BAD_FIELDS = 1, TRIP_BAD_PARSE = 2, TRIP_TOO_LONG = 3 };
enum { TRIP_SET_COMMA = 0, TRIP_SET_TAB, TRIP_SET_DATE1, TRIP_SET_SLASH, TRIP_SET_TIME };
constexpr int32_t TRIP_MAX_LINE = 65535;       // bytes; a longer line is TRIP_TOO_LONG whatever it holds
constexpr int TRIP_MAX_PIECES = 21;

struct trip_rec {
    int32_t status, hour;
    uint64_t xy[4];              // start x, start y, end x, end y: the doubles' bits
    uint32_t host_mask;          // bit k: xy[k] is left to the host
    int32_t where[4][2];         // coordinate k's bytes (blanks stripped): first byte in the line, length
};

VEC_HD bool trip_is_sep(uint32_t c, int set) {
    switch (set) {
        case TRIP_SET_COMMA: return c == ',';
        case TRIP_SET_TAB: return c == '\t';
        case TRIP_SET_DATE1: return c == '/' || c == ' ' || c == ':';
        case TRIP_SET_SLASH: return c == '/';
        default: return c == ' ' || c == ':';
    }
}

// s[0 .. n) cut at every byte of the set (plus: a run of them cuts once).  lo[i], hi[i]: piece i = s[lo[i] .. hi[i]), for the first cap pieces.
// Returns the number of pieces with the trailing empty ones gone; a text in which nothing cuts is one piece, the empty text too.
VEC_HD int trip_split(const uint8_t* s, int32_t n, int set, bool plus, int32_t* lo, int32_t* hi, int cap) {
    int count = 0, kept = 0;
    int32_t start = 0;
    bool cut = false;
    for (int32_t i = 0; i < n; i++) {
        if (!trip_is_sep(s[i], set)) continue;
        cut = true;
        if (count < cap) { lo[count] = start; hi[count] = i; }
        count++;
        if (i > start) kept = count;
        if (plus) while (i + 1 < n && trip_is_sep(s[i + 1], set)) i++;
        start = i + 1;
    }
    if (count < cap) { lo[count] = start; hi[count] = n; }
    count++;
    if (n > start) kept = count;
    return cut ? kept : 1;
}

// [+-] digits, at least one digit, the value inside [lo, hi]
VEC_HD bool trip_int(const uint8_t* s, int32_t n, int64_t lo, int64_t hi, int64_t* out) {
    int32_t i = 0;
    bool neg = false;
    if (i < n && (s[i] == '+' || s[i] == '-')) { neg = s[i] == '-'; i++; }
    if (i >= n) return false;
    int64_t v = 0;
    for (; i < n; i++) {
        const uint32_t d = (uint32_t)s[i] - '0';
        if (d > 9u) return false;
        if (v < 100000000000LL) v = v * 10 + d;                // beyond every range asked for: stays beyond
    }
    if (neg) v = -v;
    if (v < lo || v > hi) return false;
    *out = v;
    return true;
}
VEC_HD bool trip_byte(const uint8_t* s, int32_t n, int64_t* out) { return trip_int(s, n, -128, 127, out); }

// the coordinate in line[at .. at + n): blanks (bytes <= 0x20) stripped, od_parse.h's value grammar without its words, a finite value
VEC_HD bool trip_coord(const uint8_t* line, int32_t at, int32_t n, int k, trip_rec* r) {
    while (n > 0 && line[at] <= 0x20u) { at++; n--; }
    while (n > 0 && line[at + n - 1] <= 0x20u) n--;
    r->where[k][0] = at; r->where[k][1] = n;
    for (int32_t i = 0; i < n; i++) {                           // inf, infinity, nan: the only letters of the grammar besides e
        const uint32_t c = line[at + i] | 0x20u;
        if (c == 'i' || c == 'n') return false;
    }
    uint64_t bits = 0;
    const int rc = od_parse_f64(line + at, n, &bits);
    if (rc == VEC_PARSE_BAD) return false;
    if (rc == VEC_PARSE_HOST) { r->host_mask |= 1u << k; return true; }
    if ((bits & 0x7FFFFFFFFFFFFFFFull) >= 0x7FF0000000000000ull) return false;
    r->xy[k] = bits;
    return true;
}

// "M/D/Y H:M..." cut at '/', ' ' and ':': at least 5 pieces; pieces 0, 1, 3 and 4 are bytes; the hour is piece 3 as it stands
VEC_HD bool trip_date1(const uint8_t* s, int32_t n, int64_t* hour) {
    int32_t lo[5], hi[5];
    if (trip_split(s, n, TRIP_SET_DATE1, false, lo, hi, 5) < 5) return false;
    int64_t v;
    return trip_byte(s + lo[0], hi[0] - lo[0], &v) && trip_byte(s + lo[1], hi[1] - lo[1], &v) && trip_byte(s + lo[4], hi[4] - lo[4], &v) &&
           trip_byte(s + lo[3], hi[3] - lo[3], hour);
}

// date "M/D..." and time "H:M:S PM": the hour on the 24-hour clock, the remainder truncating as Java's
VEC_HD bool trip_date2(const uint8_t* d, int32_t nd, const uint8_t* t, int32_t nt, int64_t* hour) {
    int32_t lo[4], hi[4];
    int64_t v, h;
    if (trip_split(d, nd, TRIP_SET_SLASH, false, lo, hi, 2) < 2) return false;
    if (!trip_byte(d + lo[0], hi[0] - lo[0], &v) || !trip_byte(d + lo[1], hi[1] - lo[1], &v)) return false;
    if (trip_split(t, nt, TRIP_SET_TIME, false, lo, hi, 4) < 4) return false;
    if (!trip_byte(t + lo[1], hi[1] - lo[1], &v) || !trip_byte(t + lo[0], hi[0] - lo[0], &h)) return false;
    const bool pm = hi[3] - lo[3] == 2 && t[lo[3]] == 'P' && t[lo[3] + 1] == 'M';
    *hour = h % 12 + (pm ? 12 : 0);
    return true;
}

// cut at the first blank only: one piece or two
VEC_HD bool trip_split2(const uint8_t* s, int32_t n, int32_t* second) {
    for (int32_t i = 0; i < n; i++) if (s[i] == ' ') { *second = i + 1; return true; }
    return false;
}

// "(lat,lon)": first and last byte go, then y = piece 0, x = piece 1 of what is left cut at ','
VEC_HD bool trip_gps(const uint8_t* line, int32_t at, int32_t n, int kx, trip_rec* r) {
    if (n < 2) return false;
    int32_t lo[2], hi[2];
    if (trip_split(line + at + 1, n - 2, TRIP_SET_COMMA, false, lo, hi, 2) < 2) return false;
    const bool y = trip_coord(line, at + 1 + lo[0], hi[0] - lo[0], kx + 1, r);
    const bool x = trip_coord(line, at + 1 + lo[1], hi[1] - lo[1], kx, r);
    return x && y;
}

// line[0 .. n): the line without its terminator.  format: DGE_TRIPS_TYPE1 .. 3 (1 .. 3)
VEC_HD void trip_parse_line(const uint8_t* line, int64_t n64, int format, trip_rec* r) {
    r->status = TRIP_OK; r->hour = -1; r->host_mask = 0;
    for (int k = 0; k < 4; k++) { r->xy[k] = 0; r->where[k][0] = 0; r->where[k][1] = 0; }
    if (n64 > TRIP_MAX_LINE) { r->status = TRIP_TOO_LONG; return; }
    const int32_t n = (int32_t)n64;
    int32_t lo[TRIP_MAX_PIECES + 1], hi[TRIP_MAX_PIECES + 1];
    const int want = format == 1 ? 13 : (format == 2 ? 17 : 21);
    const int got = trip_split(line, n, format == 3 ? TRIP_SET_COMMA : TRIP_SET_TAB, format == 1, lo, hi, TRIP_MAX_PIECES + 1);
    if (got != want) { r->status = TRIP_BAD_FIELDS; return; }
#define TRIP_P(i) (line + lo[i]), (hi[i] - lo[i])
    int64_t hour = 0, v;
    bool ok;
    if (format == 1) {
        ok = trip_date1(TRIP_P(7), &hour);
        ok = trip_date1(TRIP_P(8), &v) && ok;
        ok = trip_gps(line, lo[9], hi[9] - lo[9], 0, r) && ok;
        ok = trip_gps(line, lo[10], hi[10] - lo[10], 2, r) && ok;
        ok = trip_int(TRIP_P(2), -2147483648LL, 2147483647LL, &v) && ok;
    } else if (format == 2) {
        ok = trip_date2(TRIP_P(0), TRIP_P(1), &hour);
        ok = trip_date1(TRIP_P(2), &v) && ok;
        for (int k = 0; k < 4; k++) ok = trip_coord(line, lo[9 + k], hi[9 + k] - lo[9 + k], k, r) && ok;
        ok = trip_int(TRIP_P(15), -2147483648LL, 2147483647LL, &v) && ok;
    } else {
        int32_t a = 0, b = 0;
        ok = trip_split2(TRIP_P(0), &a) && trip_split2(TRIP_P(1), &b);
        if (ok) {
            ok = trip_date2(line + lo[0], a - 1, line + lo[0] + a, hi[0] - lo[0] - a, &hour);
            ok = trip_date2(line + lo[1], b - 1, line + lo[1] + b, hi[1] - lo[1] - b, &v) && ok;
        }
        ok = trip_coord(line, lo[16], hi[16] - lo[16], 0, r) && ok;
        ok = trip_coord(line, lo[15], hi[15] - lo[15], 1, r) && ok;
        ok = trip_coord(line, lo[19], hi[19] - lo[19], 2, r) && ok;
        ok = trip_coord(line, lo[18], hi[18] - lo[18], 3, r) && ok;
        ok = trip_int(TRIP_P(2), -2147483648LL, 2147483647LL, &v) && ok;
    }
#undef TRIP_P
    if (!ok) { r->status = TRIP_BAD_PARSE; r->hour = -1; r->host_mask = 0; for (int k = 0; k < 4; k++) r->xy[k] = 0; return; }
    r->hour = (int32_t)hour;
}

// ---- host only
// the coordinates left to the host: strtod in the "C" locale on the token's own bytes.  Returns how many it finished; a value that is not finite makes the line bad
static inline int trip_finish_host(const uint8_t* line, trip_rec* r, locale_t c_locale) {
    int n = 0;
    bool finite = true;
    for (int k = 0; k < 4; k++) {
        if (!(r->host_mask >> k & 1u)) continue;
        const std::string tok(reinterpret_cast<const char*>(line) + r->where[k][0], (size_t)r->where[k][1]);
        const double d = strtod_l(tok.c_str(), nullptr, c_locale);
        __builtin_memcpy(&r->xy[k], &d, 8);
        n++;
        if ((r->xy[k] & 0x7FFFFFFFFFFFFFFFull) >= 0x7FF0000000000000ull) finite = false;
    }
    if (!finite) { r->status = TRIP_BAD_PARSE; r->hour = -1; for (int j = 0; j < 4; j++) r->xy[j] = 0; }
    r->host_mask = 0;
    return n;
}
