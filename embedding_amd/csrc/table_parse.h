// table_parse.h — one line of a delimited count table to its key and the place of its values (include/dge.h: dge_counts_add_table_texts states the rule; the
// reference reads these lines with line.split in getLEHDfeatures_helper, P/embeddingEvaluation_tract.py:512-536, and its siblings).  Plain C++ for host and
// device, integer arithmetic only.  The device kernel (table_read.hip: k_tab_parse) runs it a lane per line; tests/native/table_parse_harness.cpp builds it
// with g++ and compares it with tests/counts_ref.py.
//
// Nothing here allocates and nothing is stored per value: tab_parse_line walks the line once, checks the key and every value field and notes where the first
// value field starts; tab_next_value then hands out the values one by one from there.  An offence is (place << 4 | kind): the least of them is the one at the
// least place and, at one place, the first in the header's list.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TAB_HD __host__ __device__ inline
#else
#define TAB_HD static inline
#endif

enum { TAB_SHORT_LINE = 1, TAB_SHORT_KEY, TAB_BAD_KEY, TAB_KEY_SIGN, TAB_EMPTY_VALUE, TAB_BAD_VALUE_BYTE, TAB_LONG_VALUE, TAB_BIG_VALUE, TAB_LONG_LINE, TAB_KINDS };
constexpr int32_t TAB_MAX_LINE = 65536;                      // bytes; a longer line is TAB_LONG_LINE whatever it holds
constexpr uint64_t TAB_MAX_VALUE = (uint64_t)1 << 40;
constexpr uint64_t TAB_NO_OFFENCE = ~(uint64_t)0;
constexpr int TAB_MAX_COLS = 1024;

struct tab_rule { int32_t sep, key_field, key_lo, key_hi, col_lo, n_cols, neg_ok; };

struct tab_line {
    uint64_t offence;            // TAB_NO_OFFENCE, or (offset in the line << 4 | kind)
    int64_t key;                 // the key's digits as a number
    int32_t neg;                 // a '-' stood in front of them
    int32_t val_at;              // offset of the first value field
};

TAB_HD void tab_offend(tab_line* L, int32_t at, int kind) {
    const uint64_t o = (uint64_t)(uint32_t)at << 4 | (uint64_t)kind;
    if (o < L->offence) L->offence = o;
}

// the key field s[lo .. hi).  key_lo and key_hi are compared with the field's length before they are added to anything: whatever their size, no sum leaves the line
TAB_HD void tab_key(const uint8_t* s, int32_t lo, int32_t hi, const tab_rule& r, tab_line* L) {
    const int32_t len = hi - lo;
    if (len <= r.key_lo) { tab_offend(L, lo, TAB_SHORT_KEY); return; }
    int32_t a = lo + r.key_lo;
    const int32_t b = r.key_hi && r.key_hi < len ? lo + r.key_hi : hi;
    if (s[a] == '-') {
        if (!r.neg_ok) { tab_offend(L, a, TAB_KEY_SIGN); return; }
        L->neg = 1;
        a++;
    }
    if (a == b) { tab_offend(L, a, TAB_BAD_KEY); return; }
    int64_t k = 0;
    for (int32_t p = a; p < b; p++) {
        const uint32_t d = (uint32_t)s[p] - '0';
        if (d > 9u || p - a == 18) { tab_offend(L, p, TAB_BAD_KEY); return; }
        k = k * 10 + (int64_t)d;
    }
    L->key = k;
}

// a value field s[lo .. hi)
TAB_HD void tab_check_value(const uint8_t* s, int32_t lo, int32_t hi, tab_line* L) {
    if (lo == hi) { tab_offend(L, lo, TAB_EMPTY_VALUE); return; }
    uint64_t v = 0;
    for (int32_t p = lo; p < hi; p++) {
        const uint32_t d = (uint32_t)s[p] - '0';
        if (d > 9u) { tab_offend(L, p, TAB_BAD_VALUE_BYTE); return; }
        if (p - lo == 19) { tab_offend(L, p, TAB_LONG_VALUE); return; }
        v = v * 10 + d;                                        // 19 digits stay below 2^64
    }
    if (v > TAB_MAX_VALUE) tab_offend(L, lo, TAB_BIG_VALUE);
}

// the line s[0 .. n), its terminator gone, n >= 1
TAB_HD void tab_parse_line(const uint8_t* s, int32_t n, const tab_rule& r, tab_line* L) {
    L->offence = TAB_NO_OFFENCE; L->key = 0; L->neg = 0; L->val_at = 0;
    if (n > TAB_MAX_LINE) { tab_offend(L, 0, TAB_LONG_LINE); return; }
    const int32_t col_hi = r.col_lo + r.n_cols;
    const int32_t last = r.key_field > col_hi - 1 ? r.key_field : col_hi - 1;        // the last field anything is asked of
    int32_t f = 0, start = 0;
    for (int32_t i = 0; i <= n; i++) {
        if (i < n && s[i] != (uint8_t)r.sep) continue;
        if (f == r.key_field) tab_key(s, start, i, r, L);
        if (f >= r.col_lo && f < col_hi) {
            if (f == r.col_lo) L->val_at = start;
            tab_check_value(s, start, i, L);
        }
        if (f == last) return;
        f++;
        start = i + 1;
    }
    tab_offend(L, n, TAB_SHORT_LINE);
}

// the value that starts at s[*at] of a line tab_parse_line found no offence in; *at moves behind the sep that follows it
TAB_HD uint64_t tab_next_value(const uint8_t* s, int32_t n, int32_t sep, int32_t* at) {
    uint64_t v = 0;
    int32_t p = *at;
    while (p < n && s[p] != (uint8_t)sep) v = v * 10 + (uint64_t)(s[p++] - '0');
    *at = p + 1;
    return v;
}
