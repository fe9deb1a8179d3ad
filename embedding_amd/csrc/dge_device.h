// dge_device.h — the small device-side habits that the modules around the trainer share: a pair of timing events, the launch grid of a flat kernel, the
// library's "ask for the scratch's size, allocate it, call again" idiom with the sorts and prefix sums built on it, and the move of a double inside a DPP row
// of 16 lanes.  Only translation units outside the build stamp include it (csrc/Makefile): a change here voids no committed counter profile.
#pragma once
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "dge_internal.h"

// the event time between start() and stop() on one stream, as often as wanted; the two events are made by the first start() and go with the object, on every
// exit path (the object is not copied)
struct dge_stopwatch {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipStream_t stream = nullptr;
    ~dge_stopwatch() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    int start(hipStream_t s) {
        stream = s;
        if (!e0) DGE_HIP(hipEventCreate(&e0));
        if (!e1) DGE_HIP(hipEventCreate(&e1));
        DGE_HIP(hipEventRecord(e0, s));
        return DGE_OK;
    }
    // one counted host wait: when this returns, everything queued on the stream before it has run
    int stop(float* ms) { DGE_HIP(hipEventRecord(e1, stream)); DGE_HIP(hipEventSynchronize(e1)); DGE_HIP(hipEventElapsedTime(ms, e0, e1)); return DGE_OK; }
};

static inline unsigned dge_grid(int64_t n, int block = 256) { return (unsigned)((n + block - 1) / block); }
static inline int dge_bits(uint64_t v) { int b = 1; while (b < 64 && (v >> b)) b++; return b; }       // the bits that hold v, one at least

// ------------------------------------------------------------------------------------------ the two passes of a library call
// call(tmp, bytes) -> hipError_t is the library routine: with tmp == nullptr it only sets bytes.  scratch(bytes, &tmp) -> int allocates; it owns the memory, so
// the scratch lives as long as the allocator object does.  What a caller wants between the allocation and the run — the start of its timed bracket, the kernel
// that fills the routine's input — goes at the end of its allocator.  wait: a counted wait for the stream behind the run (a scratch that goes at once needs it).
template <typename Scratch, typename Call>
int dge_two_pass(Scratch&& scratch, Call&& call, hipStream_t stream, bool wait) {
    size_t bytes = 0;
    void* tmp = nullptr;
    DGE_HIP(call(tmp, bytes));
    if (int rc = scratch(bytes, &tmp)) return rc;
    DGE_HIP(call(tmp, bytes));
    if (wait) DGE_HIP(hipStreamSynchronize(stream));
    return DGE_OK;
}

// the plain allocator: a dge_tmp of the asked size
struct dge_scratch {
    dge_tmp<uint8_t> t;
    int operator()(size_t bytes, void** p) { const int rc = t.alloc(bytes); *p = t.p; return rc; }
};

// stable radix sorts over the key bits [0, end_bit), and sums of int64 values: out[i] = in[0] + .. + in[i] (inclusive) or in[0] + .. + in[i - 1] (exclusive).
// The arrays go to the library with the types the caller has them in: a const input and a plain one are two sets of kernels to it.
template <typename Scratch, typename KIn, typename KOut, typename VIn, typename VOut>
int dge_sort_pairs(Scratch&& scratch, KIn k_in, KOut k_out, VIn v_in, VOut v_out, int64_t n, int end_bit, hipStream_t stream, bool wait) {
    return dge_two_pass(scratch, [&](void* tmp, size_t& bytes) { return rocprim::radix_sort_pairs(tmp, bytes, k_in, k_out, v_in, v_out, (size_t)n, 0, end_bit, stream); }, stream, wait);
}
template <typename Scratch, typename KIn, typename KOut>
int dge_sort_keys(Scratch&& scratch, KIn k_in, KOut k_out, int64_t n, int end_bit, hipStream_t stream, bool wait) {
    return dge_two_pass(scratch, [&](void* tmp, size_t& bytes) { return rocprim::radix_sort_keys(tmp, bytes, k_in, k_out, (size_t)n, 0, end_bit, stream); }, stream, wait);
}
template <typename Scratch, typename In>
int dge_inclusive_sum(Scratch&& scratch, In in, int64_t* out, int64_t n, hipStream_t stream, bool wait) {
    return dge_two_pass(scratch, [&](void* tmp, size_t& bytes) { return rocprim::inclusive_scan(tmp, bytes, in, out, (size_t)n, rocprim::plus<int64_t>(), stream); }, stream, wait);
}
template <typename Scratch, typename In>
int dge_exclusive_sum(Scratch&& scratch, In in, int64_t* out, int64_t n, hipStream_t stream, bool wait) {
    return dge_two_pass(scratch, [&](void* tmp, size_t& bytes) { return rocprim::exclusive_scan(tmp, bytes, in, out, (int64_t)0, (size_t)n, rocprim::plus<int64_t>(), stream); }, stream, wait);
}

// ------------------------------------------------------------------------------------------ a double across a DPP row of 16 lanes
template <int CTRL, bool BOUND>
__device__ __forceinline__ double dge_row16_move(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xF, 0xF, BOUND);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xF, 0xF, BOUND);
    return __hiloint2double(hi, lo);
}
// lane l takes the value of lane l + S (lanes past the row's end give 0)
template <int S>
__device__ __forceinline__ double dge_row16_shl(double x) { return dge_row16_move<0x100 + S, true>(x); }
// lane l takes the value of lane (l + S) mod 16 of its row
template <int S>
__device__ __forceinline__ double dge_row16_ror(double x) { return dge_row16_move<0x120 + S, false>(x); }
