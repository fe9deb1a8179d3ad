// seq_out_plan.h — the host-side planning of the .seq writer (seq_write.hip), free of HIP so that tests/native/seq_out_plan_harness.cpp builds it with g++:
// how the text is cut into tiles (the output bytes one workgroup assembles) and slabs (the output bytes one launch produces and one copy takes to the
// host), and how a decimal is sized and spelled without floating point.  Nothing here touches a device.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SEQ_OUT_HD __host__ __device__ __forceinline__
#else
#define SEQ_OUT_HD static inline
#endif

// A tile: 256 lanes x one 16-byte store each — the widest store a lane issues, 64 lanes of it one contiguous KiB.  A tile starts on a 16-byte
// boundary of the text AND of the device buffer: a slab starts on a tile boundary and sits at the start of a 16-byte-aligned allocation.
constexpr int64_t SEQ_OUT_TILE = 4096;
// A slab: what one launch formats and one copy brings to a pinned buffer.  Two of them are all the device ever holds of the text, however long it is.
constexpr int64_t SEQ_OUT_SLAB = (int64_t)16 << 20;
static_assert(SEQ_OUT_SLAB % SEQ_OUT_TILE == 0 && SEQ_OUT_TILE % 16 == 0, "slabs are whole tiles, tiles whole 16-byte stores");

static inline int64_t seq_out_slab_count(int64_t total) { return total <= 0 ? 0 : (total + SEQ_OUT_SLAB - 1) / SEQ_OUT_SLAB; }
static inline int64_t seq_out_slab_begin(int64_t s) { return s * SEQ_OUT_SLAB; }
static inline int64_t seq_out_slab_end(int64_t total, int64_t s) { const int64_t e = (s + 1) * SEQ_OUT_SLAB; return e < total ? e : total; }
static inline int64_t seq_out_tiles(int64_t slab_bytes) { return (slab_bytes + SEQ_OUT_TILE - 1) / SEQ_OUT_TILE; }
// bytes of one of the two device (and pinned) slab buffers: whole tiles, so that a tile's last 16-byte store never leaves the allocation
static inline int64_t seq_out_buffer_bytes(int64_t total) {
    const int64_t b = total < SEQ_OUT_SLAB ? total : SEQ_OUT_SLAB;
    return seq_out_tiles(b > 0 ? b : 1) * SEQ_OUT_TILE;
}

// decimal digits of v >= 0, by comparison
SEQ_OUT_HD int seq_out_digits(uint32_t v) {
    return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 : v < 1000000u ? 6 : v < 10000000u ? 7 : v < 100000000u ? 8 : v < 1000000000u ? 9 : 10;
}
// the q-th character (0 = the leading one) of the decimal form of v, which has nd digits
SEQ_OUT_HD uint8_t seq_out_digit(uint32_t v, int nd, int q) {
    uint32_t p = 1;
    for (int k = nd - 1 - q; k > 0; k--) p *= 10u;
    return (uint8_t)('0' + (v / p) % 10u);
}
