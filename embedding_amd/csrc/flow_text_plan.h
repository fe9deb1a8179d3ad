// flow_text_plan.h — the arithmetic of the flow-table text writer (flow_text.hip), free of HIP so that tests/native/flow_text_plan_harness.cpp builds it with
// g++: how an int64 is sized and spelled as %lld spells it, and how a .matrix row is laid out WITHOUT its zeros being stored anywhere — the length of a row, the
// byte a column starts at, and the way back from a byte offset to (column, character).  Integers only; nothing here touches a device.
//
// A matrix slice of n rows and columns is given by its M kept entries in (row, column) order:
//   col[j]   the column of entry j                         w[j]   its weight, > 0
//   P[j]     the sum of (digits(w) - 1) over the entries in front of j, P[M] the sum over all: an entry takes 2 + (P[j + 1] - P[j]) bytes, a zero takes 2
//   rowb[i]  the first entry of row i, rowb[n] = M
// Row i is bytes [ftp_row_start(i), ftp_row_start(i + 1)) of the text; every column gives its decimal and ONE byte behind it, the separator or, in column
// n - 1, the newline.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FTP_HD __host__ __device__ __forceinline__
#else
#define FTP_HD static inline
#endif

// ------------------------------------------------------------------------------------------ decimals
// decimal digits of v, by comparison: 1 .. 20
FTP_HD int ftp_digits_u(uint64_t v) {
    int n = 1;
    uint64_t p = 10u;
    while (n < 20 && v >= p) { n++; p = n < 20 ? p * 10u : p; }
    return n;
}
// |v| without overflow at -2^63
FTP_HD uint64_t ftp_mag(int64_t v) { return v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v; }
// bytes of "%lld" of v: a '-' when negative, no '+', no leading zeros
FTP_HD int ftp_len(int64_t v) { return (v < 0 ? 1 : 0) + ftp_digits_u(ftp_mag(v)); }
// the q-th byte (0 = the first) of "%lld" of v, 0 <= q < ftp_len(v)
FTP_HD uint8_t ftp_char(int64_t v, int q) {
    if (v < 0) { if (q == 0) return (uint8_t)'-'; q--; }
    const uint64_t m = ftp_mag(v);
    uint64_t p = 1;
    for (int k = ftp_digits_u(m) - 1 - q; k > 0; k--) p *= 10u;
    return (uint8_t)('0' + (m / p) % 10u);
}

// ------------------------------------------------------------------------------------------ a matrix row without its zeros
FTP_HD int64_t ftp_row_len(int64_t n, const int64_t* P, int64_t b, int64_t e) { return 2 * n + (P[e] - P[b]); }
FTP_HD int64_t ftp_row_start(int64_t n, const int64_t* P, const int64_t* rowb, int64_t i) { return 2 * n * i + P[rowb[i]]; }
// the byte of its row at which entry j of the row's entries [b, e) starts
FTP_HD int64_t ftp_entry_start(const int32_t* col, const int64_t* P, int64_t b, int64_t j) { return 2 * (int64_t)col[j] + (P[j] - P[b]); }
// the byte of its row at which column c starts, 0 <= c <= n (c = n: the row's length)
FTP_HD int64_t ftp_col_start(const int32_t* col, const int64_t* P, int64_t b, int64_t e, int64_t c) {
    int64_t lo = b, hi = e;                      // the first entry whose column is >= c
    while (lo < hi) { const int64_t mid = lo + (hi - lo) / 2; if ((int64_t)col[mid] < c) lo = mid + 1; else hi = mid; }
    return 2 * c + (P[lo] - P[b]);
}
// the row byte t of the text lies in: the largest i < rows with ftp_row_start(i) <= t (rows are never empty, so the starts rise strictly); rows >= 1 (the
// writer's matrices are square: rows = n), t >= 0
FTP_HD int64_t ftp_find_row(int64_t rows, int64_t n, const int64_t* P, const int64_t* rowb, int64_t t) {
    int64_t lo = 0, hi = rows;
    while (hi - lo > 1) { const int64_t mid = lo + (hi - lo) / 2; if (ftp_row_start(n, P, rowb, mid) <= t) lo = mid; else hi = mid; }
    return lo;
}
// the last entry of [b, e) whose bytes start at or before byte q of the row; b - 1 when there is none
FTP_HD int64_t ftp_find_entry(const int32_t* col, const int64_t* P, int64_t b, int64_t e, int64_t q) {
    int64_t lo = b - 1, hi = e;
    while (hi - lo > 1) { const int64_t mid = lo + (hi - lo) / 2; if (ftp_entry_start(col, P, b, mid) <= q) lo = mid; else hi = mid; }
    return lo;
}
// byte q of the row -> its character and, in *column, its column.  j = ftp_find_entry(.., q).  Either q lies inside entry j (a digit, or the byte behind the
// digits), or in the run of "0<sep>" pairs behind it (in front of the first entry when j = b - 1).
FTP_HD uint8_t ftp_row_char(const int32_t* col, const int64_t* P, const int64_t* w, int64_t n, uint8_t sep, int64_t b, int64_t j, int64_t q, int64_t* column) {
    int64_t c, t;
    if (j < b) { c = q >> 1; t = q & 1; }
    else {
        const int64_t s = ftp_entry_start(col, P, b, j), len = 2 + (P[j + 1] - P[j]);
        if (q < s + len) {
            c = col[j]; t = q - s;
            if (t < len - 1) { *column = c; return ftp_char(w[j], (int)t); }
            t = 1;
        } else { c = (int64_t)col[j] + 1 + ((q - s - len) >> 1); t = (q - s - len) & 1; }
    }
    *column = c;
    return t == 0 ? (uint8_t)'0' : c == n - 1 ? (uint8_t)'\n' : sep;
}

// a place in the text that moves forward a byte at a time: the row, its entries [b, e), the offset q inside it and the entry j of ftp_find_entry
struct ftp_cursor { int64_t row, b, e, j, q; };
FTP_HD void ftp_seek(ftp_cursor& c, int64_t rows, int64_t n, const int32_t* col, const int64_t* P, const int64_t* rowb, int64_t t) {
    c.row = ftp_find_row(rows, n, P, rowb, t);
    c.b = rowb[c.row]; c.e = rowb[c.row + 1];
    c.q = t - ftp_row_start(n, P, rowb, c.row);
    c.j = ftp_find_entry(col, P, c.b, c.e, c.q);
}
// the character under the cursor; the cursor moves on, into the next row behind a newline (row = rows behind the last)
FTP_HD uint8_t ftp_next(ftp_cursor& c, int64_t rows, int64_t n, const int32_t* col, const int64_t* P, const int64_t* w, const int64_t* rowb, uint8_t sep) {
    if (c.j + 1 < c.e && ftp_entry_start(col, P, c.b, c.j + 1) <= c.q) c.j++;
    int64_t column;
    const uint8_t ch = ftp_row_char(col, P, w, n, sep, c.b, c.j, c.q, &column);
    if (++c.q == ftp_row_len(n, P, c.b, c.e)) {
        c.row++; c.q = 0; c.b = c.e;
        if (c.row < rows) c.e = rowb[c.row + 1];
        c.j = c.b - 1;
    }
    return ch;
}
