// dge_device.h — the small device-side habits that the modules around the trainer share: a pair of timing events, the launch grid of a flat kernel, the
// library's "ask for the scratch's size, allocate it, call again" idiom with the sorts and prefix sums built on it, the device half of the used-rows intake of
// the row-table estimators (used_rows.h), and the move of a double inside a DPP row of 16 lanes.  Only translation units outside the build stamp include it (csrc/Makefile): a change here voids no committed counter profile.
#pragma once
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <vector>

#include "dge_internal.h"
#include "used_rows.h"

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

// ------------------------------------------------------------------------------------------ the used rows of a call, on the device
// a dge_tmp allocation that says who asked: memory that does not fit is the caller's DGE_ERR_CAP, not a device error
template <typename T>
static int dge_alloc_for(dge_tmp<T>& t, size_t n, const char* who) {
    if (t.p) { (void)hipFree(t.p); t.p = nullptr; }
    if (n == 0) n = 1;
    const hipError_t e = hipMalloc((void**)&t.p, n * sizeof(T));
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); t.p = nullptr; DGE_FAIL(DGE_ERR_CAP, "%s: %zu bytes of device memory do not fit", who, n * sizeof(T)); }
    DGE_HIP(e);
    return DGE_OK;
}

static inline int dge_range_check(const char* who, const char* name, int v, int max) {
    char msg[192];
    if (ur_outside(msg, who, name, v, max)) DGE_FAIL(DGE_ERR_ARG, "%s", msg);
    return DGE_OK;
}

// the present bytes of v on the host; p stays nullptr when every row is present
struct dge_present {
    std::vector<uint8_t> bytes;
    const uint8_t* p = nullptr;
    int load(const dge_vectors* v) {
        if (v->n_present == v->rows) return DGE_OK;
        bytes.resize((size_t)v->rows);
        if (v->rows) DGE_HIP(hipMemcpy(bytes.data(), v->d_present, (size_t)v->rows, hipMemcpyDeviceToHost));
        p = bytes.data();
        return DGE_OK;
    }
};

// the used rows' numbers on the device; p stays nullptr when no row is left out.  who: the allocation is dge_alloc_for's; nullptr: the plain one
struct dge_used_rows {
    dge_tmp<int64_t> d;
    const int64_t* p = nullptr;
    int upload(const ur_rows& u, const char* who) {
        if (u.all) return DGE_OK;
        if (int rc = who ? dge_alloc_for(d, (size_t)u.n, who) : d.alloc((size_t)u.n)) return rc;
        DGE_HIP(hipMemcpy(d.p, u.used.data(), (size_t)u.n * sizeof(int64_t), hipMemcpyHostToDevice));
        p = d.p;
        return DGE_OK;
    }
};

// the handle a host-array entry makes for its rows: freed on every exit path
struct dge_vectors_guard {
    dge_vectors* v = nullptr;
    dge_vectors_guard() = default;
    dge_vectors_guard(const dge_vectors_guard&) = delete;
    dge_vectors_guard& operator=(const dge_vectors_guard&) = delete;
    ~dge_vectors_guard() { if (v) dge_vectors_free(v); }
};

// The least element e = i * dim + c, i counting the used rows, that holds a value that is not finite, and with max_bits the greatest |x| of the finite ones as
// float bits (the bits of non-negative floats order as unsigned integers).  A wave reduces before it touches memory.  Templates, so that only the translation
// units that scan carry the kernel.
#define DGE_SCAN_NONE (~0ULL)
#define DGE_SCAN_BLOCKS 4096
template <bool MAX>
__global__ void k_dge_scan(const float* __restrict__ x, const int64_t* __restrict__ used, int64_t n, int dim, unsigned* __restrict__ max_bits,
                           unsigned long long* __restrict__ bad) {
    const size_t total = (size_t)n * (size_t)dim, step = (size_t)gridDim.x * blockDim.x;
    unsigned m = 0;
    unsigned long long b = DGE_SCAN_NONE;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
        const size_t i = e / (size_t)dim, c = e - i * (size_t)dim;
        const size_t row = used ? (size_t)used[i] : i;
        const unsigned bits = __float_as_uint(x[row * (size_t)dim + c]) & 0x7fffffffu;
        if (bits >= 0x7f800000u) { if ((unsigned long long)e < b) b = e; }
        else if (MAX && bits > m) m = bits;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned m2 = __shfl_xor(m, o);
        const unsigned long long b2 = __shfl_xor(b, o);
        if (m2 > m) m = m2;
        if (b2 < b) b = b2;
    }
    if ((threadIdx.x & 63) == 0) {
        if (MAX && m) atomicMax(max_bits, m);
        if (b != DGE_SCAN_NONE) atomicMin(bad, b);
    }
}
// words: device memory the caller owns: word 0 is the scan's, then `more` words of the caller's that start as all ones like it (minima of later kernels: one memset
// arms them all), then with MAX the word of max_bits.  *bad: the element, or -1 where every value is finite.  One blocking read-back.
template <bool MAX>
static int dge_scan_rows(const float* x, const int64_t* used, int64_t n, int dim, unsigned long long* words, int more, unsigned* max_bits, int64_t* bad) {
    std::vector<unsigned long long> w((size_t)(1 + more + (MAX ? 1 : 0)));
    DGE_HIP(hipMemsetAsync(words, 0xff, (size_t)(1 + more) * sizeof w[0], 0));
    if (MAX) DGE_HIP(hipMemsetAsync(words + 1 + more, 0, sizeof w[0], 0));
    const size_t blocks = ((size_t)n * (size_t)dim + 255) / 256;
    hipLaunchKernelGGL(k_dge_scan<MAX>, dim3((unsigned)(blocks < DGE_SCAN_BLOCKS ? blocks : DGE_SCAN_BLOCKS)), dim3(256), 0, 0, x, used, n, dim, MAX ? (unsigned*)(words + 1 + more) : (unsigned*)nullptr, words);
    DGE_HIP(hipGetLastError());
    DGE_HIP(hipMemcpy(w.data(), words, w.size() * sizeof w[0], hipMemcpyDeviceToHost));
    if (MAX) *max_bits = (unsigned)w.back();
    *bad = w[0] == DGE_SCAN_NONE ? -1 : (int64_t)w[0];
    return DGE_OK;
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
