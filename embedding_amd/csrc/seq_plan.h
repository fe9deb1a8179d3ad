// seq_plan.h — the host-side planning of the .seq ingest (seq_ingest.hip), free of HIP so that tests/native/seq_plan_harness.cpp builds it with g++:
// which bytes are whitespace, how the caller's pieces (prior names, then the files or the text) are laid out in the ONE buffer the kernels read, and how
// the name table grows.  Nothing here touches a device.
#pragma once
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define SEQ_HD __host__ __device__ __forceinline__
#else
#define SEQ_HD static inline
#endif

// C's isspace in the "C" locale: 0x09-0x0D and 0x20.  Every other byte, 0x80-0xFF included, is token material.
SEQ_HD bool seq_is_space(uint32_t c) { return (c - 9u) < 5u || c == 32u; }

// The byte written behind a piece (a file, or the caller's text).  A piece whose last byte is not '\n' ends its last line where it ends: the pad is the
// missing '\n', so its last token never merges with the first token of the next piece.  Behind a piece that ends in '\n' (or is empty) the pad is a blank:
// it starts the next piece's first line with one more whitespace byte, which changes no token, no line and no row.
static inline uint8_t seq_pad_byte(int64_t size, uint8_t last_byte) { return (size > 0 && last_byte != '\n') ? (uint8_t)'\n' : (uint8_t)' '; }

constexpr int64_t SEQ_CHUNK = 8192;   // bytes one workgroup classifies (256 lanes x 32 bytes)
constexpr int64_t SEQ_TAIL = 64;      // blanks behind the last chunk: the kernels' 8-byte reads of a token never leave the buffer

struct seq_layout {
    std::vector<int64_t> offset;   // piece k occupies [offset[k], offset[k] + size[k]); its pad byte is at offset[k] + size[k]
    int64_t prefix_bytes = 0;      // the prior names, one per line, in front of piece 0
    int64_t used = 0;              // prefix + pieces + pads
    int64_t padded = 0;            // used rounded up to whole chunks, plus SEQ_TAIL: the allocation; [used, padded) is blanks
    int64_t text_bytes = 0;        // sum of the piece sizes: dge_seq_info.bytes
};

// false: a negative size, or the sum leaves int64
static inline bool seq_plan_layout(int64_t prefix_bytes, const int64_t* sizes, int64_t n, seq_layout* out) {
    const int64_t LIM = INT64_MAX / 2;
    if (prefix_bytes < 0 || prefix_bytes > LIM || n < 0) return false;
    seq_layout L;
    L.prefix_bytes = prefix_bytes;
    int64_t at = prefix_bytes;
    for (int64_t k = 0; k < n; k++) {
        if (sizes[k] < 0 || sizes[k] > LIM - at - 1) return false;
        L.offset.push_back(at);
        at += sizes[k] + 1;
        L.text_bytes += sizes[k];
    }
    L.used = at;
    L.padded = (at + SEQ_CHUNK - 1) / SEQ_CHUNK * SEQ_CHUNK + SEQ_TAIL;
    *out = L;
    return true;
}

// The name table: a power of two of slots, at most half full.  No text has more names than tokens, so a table of seq_slots_cap(tokens) slots never
// fills; below it a pass that finds the table more than half full (or a probe that comes round) is given up and redone with eight times the slots.
static inline int64_t seq_pow2_at_least(int64_t n) { int64_t s = 1; while (s < n) s <<= 1; return s; }
static inline int64_t seq_slots_cap(int64_t tokens) { return seq_pow2_at_least(2 * (tokens > 0 ? tokens : 1)); }
static inline int64_t seq_slots_first(int64_t tokens, int64_t initial_slots) {
    const int64_t cap = seq_slots_cap(tokens);
    int64_t s = initial_slots > 0 ? seq_pow2_at_least(initial_slots) : (int64_t)1 << 20;
    return s < cap ? s : cap;
}
static inline int64_t seq_slots_next(int64_t slots, int64_t tokens) {
    const int64_t cap = seq_slots_cap(tokens);
    return slots >= cap / 8 ? cap : slots * 8;
}
