// matrix_parse.h — the per-element pieces of the .matrix reader's rule (include/dge.h: dge_flows_add_matrix_texts), compiled for host and device: the byte
// classes of a lane's 32 bytes as 32-bit masks, what follows from them and the neighbour lane's by bit operations (terminators, line starts, empty values, the
// 20th digit of a run, the values > 0 that end here), the lane's summary and the segmented operator the scans run, the column of a byte, and the lane's part of
// the emit pass.  matrix_read.hip runs these in its two kernels; mat_host_slab runs the same lanes one after the other on one host thread
// (tests/native/matrix_parse_harness.cpp, scripts/matrix_read_rate.py).  Integer arithmetic only.
//
// A SLAB is n bytes of one piece at text[0 .. n), with MAT_LEAD bytes in front of them (zeros, and the byte before the slab at text[-1]: '\n' when the slab
// opens its piece) and behind them the byte that follows (0 when the piece ends) and zeros up to whole lanes and one byte more.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MP_HD __host__ __device__ inline
#define MP_MEMBER __host__ __device__
#else
#define MP_HD static inline
#define MP_MEMBER
#endif

#define MAT_LANE 32                          // bytes a lane takes
#define MAT_BLOCK 256                        // lanes of a workgroup
#define MAT_TILE (MAT_LANE * MAT_BLOCK)      // bytes a workgroup takes
#define MAT_LEAD 32                          // bytes in front of a slab
#define MAT_MAX_TILES 2048                   // tiles of a slab, at most: one workgroup scans their aggregates
#define MAT_MAX_VALUE (1ULL << 40)
#define MAT_MAX_DIGITS 19

// the offences, in the order that decides between two at one place
enum { MAT_BAD_BYTE = 1, MAT_EMPTY_VALUE = 2, MAT_LONG_VALUE = 3, MAT_BIG_VALUE = 4, MAT_RAGGED = 5, MAT_ROWS_MANY = 6, MAT_ROWS_FEW = 7 };
#define MAT_NO_OFFENCE (~0ULL)

struct MatRaw { uint32_t dig, nz, sep, nl, cr; };      // bit i: byte i is a digit, a digit 1 .. 9, the separator, '\n', '\r'

// the lane's bytes as eight little-endian words
MP_HD MatRaw mat_raw(const uint32_t (&w)[8], uint32_t sep) {
    MatRaw r = {0, 0, 0, 0, 0};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 32; i++) {
        const uint32_t c = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
        r.dig |= (uint32_t)(c - 48u < 10u) << i;
        r.nz |= (uint32_t)(c - 49u < 9u) << i;
        r.sep |= (uint32_t)(c == sep) << i;
        r.nl |= (uint32_t)(c == 10u) << i;
        r.cr |= (uint32_t)(c == 13u) << i;
    }
    return r;
}

MP_HD MatRaw mat_raw_bytes(const uint8_t* p, uint32_t sep) {
    uint32_t w[8];
    for (int i = 0; i < 8; i++) w[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 | (uint32_t)p[4 * i + 3] << 24;
    return mat_raw(w, sep);
}

// What a lane knows of its bytes once it has the lane's before it and the byte behind it; every mask is cut to the lane's valid bytes.
struct MatLane {
    uint32_t nl, sep;
    uint32_t start;          // a non-empty line opens: the byte before is '\n' and this one is no terminator
    uint32_t term;           // the first byte of a non-empty line's terminator
    uint32_t ends;           // the last digit of a value > 0
    uint32_t bad, empty, lng;
    uint64_t dig64;          // digits of the lane before (low half) and of this one (high half)
};

MP_HD uint32_t mat_below(int i) { return i <= 0 ? 0u : (i >= 32 ? ~0u : ~0u >> (32 - i)); }       // bits 0 .. i-1

// c: this lane, p: the lane before, after: the byte behind the lane, valid: 0 .. 32 bytes of the lane belong to the slab
MP_HD MatLane mat_lane(const MatRaw& c, const MatRaw& p, uint32_t after, int valid) {
    MatLane L;
    const uint32_t V = mat_below(valid);
    const uint32_t nl_next = (c.nl >> 1) | ((uint32_t)(after == 10u) << 31);
    const uint32_t dig_next = (c.dig >> 1) | ((uint32_t)(after - 48u < 10u) << 31);
    const uint32_t crok = c.cr & nl_next;                                            // a '\r' directly before a '\n': half of a terminator
    const uint32_t prev_nl = (c.nl << 1) | (p.nl >> 31), prev_sep = (c.sep << 1) | (p.sep >> 31);
    const uint32_t prev_crok = (crok << 1) | ((p.cr >> 31) & c.nl & 1u);
    const uint32_t tfirst = crok | (c.nl & ~prev_crok);                             // the first byte of a terminator
    L.nl = c.nl & V;
    L.sep = c.sep & V;
    L.start = prev_nl & ~tfirst & V;
    L.term = tfirst & ~prev_nl & V;
    L.bad = ~(c.dig | c.sep | c.nl | crok) & V;
    L.empty = ((c.sep & (prev_nl | prev_sep)) | (tfirst & prev_sep)) & V;
    L.dig64 = (uint64_t)c.dig << 32 | p.dig;
    const uint64_t r2 = L.dig64 & (L.dig64 << 1), r4 = r2 & (r2 << 2), r8 = r4 & (r4 << 4), r16 = r8 & (r8 << 8);      // bit i: a run of 2^k digits ends at i
    L.lng = (uint32_t)((r16 & (r4 << 16)) >> 32) & V;                                // 16 + 4: the 20th digit of a run, and every digit behind it
    // a carry runs from the lowest digit 1 .. 9 of a run to the place behind the run's end, and no further: that place holds no digit
    const uint64_t nz64 = (uint64_t)c.nz << 32 | p.nz, sum = L.dig64 + nz64;
    const uint32_t pos = (uint32_t)((sum & ~L.dig64) >> 33) | ((uint32_t)(sum < L.dig64) << 31);
    L.ends = c.dig & ~dig_next & pos & V;
    return L;
}

// (lines ended, separators since the last line end, non-empty lines opened, values > 0 ended)
template <typename I>
struct MatSumT { I nl, cols, rows, emits; };
typedef MatSumT<int32_t> MatSum;
typedef MatSumT<int64_t> MatSum64;

MP_HD int mat_popc(uint32_t x) { return __builtin_popcount(x); }
MP_HD uint32_t mat_through_top(uint32_t x) { return x ? ~0u >> __builtin_clz(x) : 0u; }           // bits 0 .. the highest set bit of x

MP_HD MatSum mat_summary(const MatLane& L) {
    MatSum s;
    s.nl = mat_popc(L.nl);
    s.cols = mat_popc(L.sep & ~mat_through_top(L.nl));
    s.rows = mat_popc(L.start);
    s.emits = mat_popc(L.ends);
    return s;
}

// a then b.  Associative; (0, 0, 0, 0) is its identity
template <typename A, typename B>
MP_HD MatSumT<A> mat_combine(const MatSumT<A>& a, const MatSumT<B>& b) {
    MatSumT<A> r;
    r.nl = a.nl + (A)b.nl;
    r.cols = b.nl ? (A)b.cols : a.cols + (A)b.cols;
    r.rows = a.rows + (A)b.rows;
    r.emits = a.emits + (A)b.emits;
    return r;
}
struct MatCombine {
    template <typename A>
    MP_MEMBER MatSumT<A> operator()(const MatSumT<A>& a, const MatSumT<A>& b) const { return mat_combine(a, b); }
};

// separators between the start of the line that holds byte i of the lane (i = 0 .. 32) and that byte; cols_in: at the lane's first byte
MP_HD int64_t mat_col_at(const MatLane& L, int64_t cols_in, int i) {
    const uint32_t below = mat_below(i), nlb = L.nl & below;
    return nlb ? (int64_t)mat_popc(L.sep & below & ~mat_through_top(nlb)) : cols_in + mat_popc(L.sep & below);
}

MP_HD uint64_t mat_offence(int64_t offset, int kind) { return (uint64_t)offset << 3 | (uint64_t)kind; }

struct MatSlab {
    const uint8_t* text;     // the slab's first byte (see the head of this file for what stands around it)
    int64_t n;               // its bytes
    int64_t base;            // its offset in the piece
    int64_t nsel;            // values a line must hold, lines a piece must hold
    int32_t last;            // the piece ends with this slab
};

// The lane at text[at ..) in the emit pass.  in: the state in front of the lane (in.emits counts from the staging's start).  Every value > 0 that ends in the lane
// goes to sink.entry(place, row, column, value) — row or column beyond nsel, or a value that is an offence, with value 0 — and the lane's least offence is
// returned (MAT_NO_OFFENCE: none).  sum[0], sum[1] grow by value >> 20 and value & 0xfffff of the values handed on.
template <typename Sink>
MP_HD uint64_t mat_lane_emit(const MatSlab& S, int64_t at, const MatLane& L, const MatSum64& in, Sink& sink, uint64_t (&sum)[2]) {
    uint64_t off = MAT_NO_OFFENCE;
    const int64_t place = S.base + at;
#define MAT_HIT(i, kind) do { const uint64_t o__ = mat_offence(place + (i), (kind)); if (o__ < off) off = o__; } while (0)
    if (L.bad) MAT_HIT(__builtin_ctz(L.bad), MAT_BAD_BYTE);
    if (L.empty) MAT_HIT(__builtin_ctz(L.empty), MAT_EMPTY_VALUE);
    if (L.lng) MAT_HIT(__builtin_ctz(L.lng), MAT_LONG_VALUE);
    for (uint32_t m = L.term; m; m &= m - 1) {
        const int i = __builtin_ctz(m);
        if (mat_col_at(L, in.cols, i) + 1 != S.nsel) { MAT_HIT(i, MAT_RAGGED); break; }
    }
    if (in.rows <= S.nsel && in.rows + mat_popc(L.start) > S.nsel)
        for (uint32_t m = L.start; m; m &= m - 1) {
            const int i = __builtin_ctz(m);
            if (in.rows + mat_popc(L.start & mat_below(i)) == S.nsel) { MAT_HIT(i, MAT_ROWS_MANY); break; }
        }
    int64_t out = in.emits;
    for (uint32_t m = L.ends; m; m &= m - 1, out++) {
        const int i = __builtin_ctz(m), e = 32 + i;
        const uint64_t gaps = ~L.dig64 & ((1ULL << e) - 1);
        const int s = gaps ? 64 - __builtin_clzll(gaps) : 0;                 // the run's first digit in the 64 bits
        int64_t row = -1, col = -1;
        uint64_t v = 0;
        if (e - s + 1 <= MAT_MAX_DIGITS) {                                   // (a longer run is the long value found above)
            for (int k = s; k <= e; k++) v = v * 10 + (uint64_t)(S.text[at - 32 + k] - 48u);
            if (v > MAT_MAX_VALUE) { MAT_HIT(s - 32, MAT_BIG_VALUE); v = 0; }
            row = in.rows + mat_popc(L.start & mat_below(i + 1)) - 1;
            col = mat_col_at(L, in.cols, i);
            if (row < 0 || row >= S.nsel || col >= S.nsel) v = 0;
        }
        sum[0] += v >> 20; sum[1] += v & 0xfffffu;
        sink.entry(out, row, col, v);
    }
    const int64_t j = S.n - at;                                              // the piece's end, seen from the lane that holds its last byte
    if (S.last && j >= 1 && j <= 32) {
        if (L.sep >> (j - 1) & 1u) MAT_HIT(j, MAT_EMPTY_VALUE);
        if (!(L.nl >> (j - 1) & 1u) && mat_col_at(L, in.cols, (int)j) + 1 != S.nsel) MAT_HIT(j, MAT_RAGGED);
        if (in.rows + mat_popc(L.start) < S.nsel) MAT_HIT(j, MAT_ROWS_FEW);
    }
#undef MAT_HIT
    return off;
}

// lines ended and separators since the last line end in front of byte p of the slab, from the state in front of byte `from` (the walk of the error path)
MP_HD void mat_where(const uint8_t* text, int64_t from, int64_t p, uint32_t sep, int64_t* nl, int64_t* cols) {
    for (int64_t i = from; i < p; i++) {
        if (text[i] == 10u) { (*nl)++; *cols = 0; }
        else if (text[i] == sep) (*cols)++;
    }
}

// What is carried from slab to slab (device memory in matrix_read.hip): the lines ended, the separators of the open line and the non-empty lines of the piece
// so far, the entries staged in the call so far, the least offence, and the sum of the values in two parts.
struct MatState { int64_t nl, cols, rows, out; uint64_t offence, sum_hi, sum_lo, reserved; };      // 64 bytes

#ifndef __HIP_DEVICE_COMPILE__
// One slab by one host thread: the lanes in text order, each with the same code the kernels run.  first: the slab opens its piece.
template <typename Sink>
static inline void mat_host_slab(const MatSlab& S, int32_t first, uint32_t sep, MatState& st, Sink& sink) {
    MatSum64 run = {first ? 0 : st.nl, first ? 0 : st.cols, first ? 0 : st.rows, st.out};
    MatRaw prev = mat_raw_bytes(S.text - MAT_LEAD, sep);
    uint64_t sum[2] = {0, 0};
    for (int64_t at = 0; at < S.n; at += MAT_LANE) {
        const MatRaw cur = mat_raw_bytes(S.text + at, sep);
        const MatLane L = mat_lane(cur, prev, S.text[at + MAT_LANE], (int)(S.n - at < 32 ? S.n - at : 32));
        const uint64_t off = mat_lane_emit(S, at, L, run, sink, sum);
        if (off < st.offence) st.offence = off;
        run = mat_combine(run, mat_summary(L));
        prev = cur;
    }
    st.nl = run.nl; st.cols = run.cols; st.rows = run.rows; st.out = run.emits;
    st.sum_hi += sum[0]; st.sum_lo += sum[1];
}
#endif
