// seq_tokens.h — the tokeniser, the name table and the byte transport that the text readers share: seq_ingest.hip (.seq walks), vec_read.hip (.vec vectors) and
// od_read.hip (.od flows; it interns nothing) all include it, so every kernel and host routine below exists once in source.  Everything is static: each
// translation unit gets its own copy of the code and the library exports nothing from here.  Outside the build stamp, like the readers.  The host half of
// the intake — files and texts as pieces, the read step, the joiner of the one buffer — is plain C++ in seq_pieces.h, which this header includes.
//
// One buffer holds everything the kernels read (seq_plan.h: seq_layout): the names the caller's dge_names already holds, one per line, then every file
// (or the caller's text) with one pad byte behind it, then blanks up to whole chunks.  The prior names are thereby the first tokens of the buffer and take
// ids 0 .. n-1 under the same first-appearance rule as every other name.  All offsets and token indices are 64-bit.
//
//   k_seq_count / k_seq_emit   per byte: "a token starts here", "newline"; two passes around a scan of the per-chunk counts give token t its first byte
//                              and its line
//   rows                       a scan of "t is the first token of its line" numbers the rows; row_first[r] gives a token its position in the row
//   k_seq_hash                 entry e's length and a 64-bit hash of its bytes — an ENTRY is whatever the caller wants interned, given by its first byte:
//                              every token (.seq), or the prior names and the token that opens each row (.vec)
//   k_seq_intern               open addressing, one 8-byte slot per string = the SMALLEST entry index seen with that string (its first appearance)
//   ids                        a scan of "e is its string's first appearance" numbers the names in first-appearance order; id[e] = number of its string
//   seq_tokens_to_host         selected tokens (the new names; the value tokens a reader leaves to the host) NUL-terminated into one blob for the host:
//                              seq_pick or k_seq_name_tok lists them, k_seq_tok_bytes copies them, seq_host_numbers finishes numbers with strtod / strtof
//   k_seq_ragged               the least row that has not the number of tokens its reader wants; seq_row_where turns it into an offset for the message
//
// Why the intern pass is right on eight L2s that are not coherent.  A slot's history is EMPTY -> t1 -> t2 < t1 -> ..., every ti a
// token of ONE string: a slot is claimed once (compare-and-swap from EMPTY) and afterwards only lowered (atomicMin) by tokens that compared equal to
// the token it held.  Both are agent-scope read-modify-writes and execute at memory, on the slot's true value.  The READ in front of them may return any
// earlier value of that history:
//   * EMPTY although the slot is taken: the compare-and-swap fails and returns the true value, and the token goes on with that — one atomic more.
//   * a token index v of the slot's string that has been lowered since: the byte comparison has the same outcome as against the present value (same
//     string); if v > t the token issues an atomicMin that may no longer be needed — one atomic more; if v < t the true value is lower still and
//     skipping the atomic is right.
// A string never sits in two slots: a token that passed a slot saw a token of ANOTHER string there (true or stale, the slot's string is fixed) or failed
// its claim against one.  So after the kernel every slot holds the least token index of its string whatever the timing; which slot a string got does
// depend on timing, and nothing below reads it other than through the token indices.  The bytes, starts, lengths and hashes the pass compares were
// written by earlier kernels and are only read here.
// Contention: a token that reads its string in the slot with a first appearance below its own index issues no atomic at all — on a corpus of few names
// that is nearly every token (atomics on one address complete one after the other).
#pragma once
#include <locale.h>
#include <stdlib.h>

#include <chrono>
#include <hipcub/hipcub.hpp>
#include <memory>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <string_view>

#include "dge_algos.h"
#include "dge_device.h"
#include "seq_pieces.h"

// blob: count strings, string k at blob + off[k], NUL-terminated; takes the blob over
static inline void names_append(dge_names* n, std::unique_ptr<char[]> blob, const int64_t* off, int64_t count) {
    for (int64_t k = 0; k < count; k++) {
        n->ptr.push_back(blob.get() + off[k]);
        n->len.push_back(off[k + 1] - off[k] - 1);
        n->bytes += off[k + 1] - off[k] - 1;
    }
    n->blobs.push_back(std::move(blob));
}

// ------------------------------------------------------------------------------------------ kernels
constexpr int SEQ_BLOCK = 256;
constexpr unsigned long long SEQ_EMPTY = ~0ull;
constexpr int SEQ_SHARDS = 256;          // counters of claimed slots, one 128-byte line each
constexpr int SEQ_SHARD_STRIDE = 16;     // in 8-byte words

// 32 bytes of one lane: bit i of starts = a token starts at base + i (not whitespace, behind whitespace or the buffer's start)
__device__ __forceinline__ void seq_masks(const uint8_t* buf, int64_t base, uint32_t& starts, uint32_t& nls, uint32_t& nuls) {
    const uint4 a = *reinterpret_cast<const uint4*>(buf + base), b = *reinterpret_cast<const uint4*>(buf + base + 16);
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    bool prev_ws = base == 0 ? true : seq_is_space(buf[base - 1]);
    starts = nls = nuls = 0;
#pragma unroll
    for (int i = 0; i < 32; i++) {
        const uint32_t c = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
        const bool ws = seq_is_space(c);
        starts |= (uint32_t)(!ws && prev_ws) << i;
        nls |= (uint32_t)(c == 10u) << i;
        nuls |= (uint32_t)(c == 0u) << i;
        prev_ws = ws;
    }
}

// per chunk: token starts (low word) and newlines (high word); the first NUL byte of the buffer
static __global__ void __launch_bounds__(SEQ_BLOCK) k_seq_count(const uint8_t* buf, int64_t used, int64_t* chunk_tok, int64_t* chunk_nl, unsigned long long* nul_at) {
    typedef hipcub::BlockReduce<unsigned long long, SEQ_BLOCK> Reduce;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t base = (int64_t)blockIdx.x * SEQ_CHUNK + (int64_t)threadIdx.x * 32;
    uint32_t starts, nls, nuls;
    seq_masks(buf, base, starts, nls, nuls);
    if (nuls) {
        const int64_t at = base + (__ffs(nuls) - 1);
        if (at < used) atomicMin(nul_at, (unsigned long long)at);
    }
    const unsigned long long sum = Reduce(tmp).Sum((unsigned long long)__popc(starts) | ((unsigned long long)__popc(nls) << 32));
    if (threadIdx.x == 0) { chunk_tok[blockIdx.x] = (int64_t)(sum & 0xffffffffull); chunk_nl[blockIdx.x] = (int64_t)(sum >> 32); }
}

// token t (numbered in byte order through the scanned chunk counts): its first byte and the number of newlines in front of it
static __global__ void __launch_bounds__(SEQ_BLOCK) k_seq_emit(const uint8_t* buf, const int64_t* chunk_tokx, const int64_t* chunk_nlx, int64_t* tok_start, int64_t* tok_line) {
    typedef hipcub::BlockScan<unsigned long long, SEQ_BLOCK> Scan;
    __shared__ typename Scan::TempStorage tmp;
    const int64_t base = (int64_t)blockIdx.x * SEQ_CHUNK + (int64_t)threadIdx.x * 32;
    uint32_t starts, nls, nuls;
    seq_masks(buf, base, starts, nls, nuls);
    unsigned long long before;
    Scan(tmp).ExclusiveSum((unsigned long long)__popc(starts) | ((unsigned long long)__popc(nls) << 32), before);
    int64_t t = chunk_tokx[blockIdx.x] + (int64_t)(before & 0xffffffffull);
    const int64_t line0 = chunk_nlx[blockIdx.x] + (int64_t)(before >> 32);
    while (starts) {
        const int i = __ffs(starts) - 1;
        starts &= starts - 1;
        tok_start[t] = base + i;
        tok_line[t] = line0 + __popc(nls & ((1u << i) - 1u));
        t++;
    }
}

__device__ __forceinline__ uint64_t seq_ld8(const uint8_t* p) { uint64_t w; __builtin_memcpy(&w, p, 8); return w; }
// how many of the word's 8 bytes (lowest first) are token material before the first whitespace byte
__device__ __forceinline__ int seq_run(uint64_t w) {
    int n = 8;
#pragma unroll
    for (int i = 7; i >= 0; i--) if (seq_is_space((uint32_t)(w >> (8 * i)) & 0xffu)) n = i;
    return n;
}
__device__ __forceinline__ uint64_t seq_keep(uint64_t w, int n) { return n >= 8 ? w : (n == 0 ? 0ull : (w & (~0ull >> (64 - 8 * n)))); }

// bytes of the token that starts at p (the buffer ends in SEQ_TAIL blanks)
__device__ __forceinline__ int64_t seq_tok_len(const uint8_t* p) {
    int64_t len = 0;
    for (;;) {
        const int n = seq_run(seq_ld8(p + len));
        len += n;
        if (n < 8) return len;
    }
}

// the piece a buffer offset lies in: the last k with piece_off[k] <= at (at is never in front of piece 0)
__device__ __forceinline__ int64_t seq_piece_of(const int64_t* piece_off, int64_t n_pieces, int64_t at) {
    int64_t lo = 0, hi = n_pieces;
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (piece_off[mid] <= at) lo = mid; else hi = mid; }
    return lo;
}

// The buffer ends in SEQ_TAIL blanks: the 8-byte reads stop at a whitespace byte inside the allocation.
static __global__ void __launch_bounds__(SEQ_BLOCK) k_seq_hash(const uint8_t* buf, const int64_t* tok_start, int64_t T, int32_t hash_bits, int64_t* tok_len, uint64_t* tok_hash) {
    const int64_t t = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (t >= T) return;
    const uint8_t* p = buf + tok_start[t];
    uint64_t h = 0x9E3779B97F4A7C15ull;
    int64_t len = 0;
    for (;;) {
        const uint64_t w = seq_ld8(p + len);
        const int n = seq_run(w);
        h = (h ^ seq_keep(w, n)) * 0xFF51AFD7ED558CCDull;
        h ^= h >> 32;
        len += n;
        if (n < 8) break;
    }
    h = dge_mix64(h ^ (uint64_t)len);
    if (hash_bits < 64) h &= (1ull << hash_bits) - 1ull;
    tok_len[t] = len;
    tok_hash[t] = h;
}

__device__ __forceinline__ bool seq_same_bytes(const uint8_t* a, const uint8_t* b, int64_t len) {
    for (int64_t k = 0; k < len; k += 8) {
        const int n = len - k >= 8 ? 8 : (int)(len - k);
        if (seq_keep(seq_ld8(a + k), n) != seq_keep(seq_ld8(b + k), n)) return false;
    }
    return true;
}

// the argument for this kernel is at the head of the file
static __global__ void __launch_bounds__(SEQ_BLOCK) k_seq_intern(const uint8_t* buf, const int64_t* tok_start, const int64_t* tok_len, const uint64_t* tok_hash, int64_t T,
                                                          unsigned long long* table, int64_t mask, int64_t* tok_slot, unsigned long long* claims,
                                                          unsigned long long claim_limit, int* give_up) {
    const int64_t t = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (t >= T) return;
    if (__hip_atomic_load(give_up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;       // a stale 0 only costs this token's work
    const uint64_t h = tok_hash[t];
    const int64_t len = tok_len[t];
    const uint8_t* mine = buf + tok_start[t];
    int64_t s = (int64_t)(h & (uint64_t)mask);
    for (int64_t probes = 0; probes <= mask; probes++, s = (s + 1) & mask) {
        unsigned long long cur = __hip_atomic_load(table + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == SEQ_EMPTY) {
            cur = atomicCAS(table + s, SEQ_EMPTY, (unsigned long long)t);
            if (cur == SEQ_EMPTY) {
                tok_slot[t] = s;
                const unsigned long long had = atomicAdd(claims + (blockIdx.x % SEQ_SHARDS) * SEQ_SHARD_STRIDE, 1ull);
                if (had >= claim_limit) __hip_atomic_store(give_up, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // more than half full: redo with more slots
                return;
            }
        }
        if (tok_hash[cur] == h && tok_len[cur] == len && seq_same_bytes(buf + tok_start[cur], mine, len)) {
            if (cur > (unsigned long long)t) atomicMin(table + s, (unsigned long long)t);
            tok_slot[t] = s;
            return;
        }
    }
    __hip_atomic_store(give_up, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);               // came round: the table is full
}

struct SeqRowFlag {      // token t opens a row: the first text token of its line (the prior names in front open none)
    const int64_t* line; int64_t P, T;
    __device__ int64_t operator()(int64_t t) const { return (t >= P && t < T && (t == P || line[t - 1] != line[t])) ? 1 : 0; }
};
struct SeqFirstFlag {    // token t is the first appearance of its string
    const unsigned long long* table; const int64_t* slot; int64_t T;
    __device__ int64_t operator()(int64_t t) const { return (t < T && table[slot[t]] == (unsigned long long)t) ? 1 : 0; }
};
struct SeqByteFlag {     // byte i of an array is set
    const uint8_t* p; int64_t n;
    __device__ int64_t operator()(int64_t i) const { return (i < n && p[i] != 0) ? 1 : 0; }
};
template <typename Start>
struct SeqItemLen {      // bytes of item k in the blob, its NUL included: the token whose first byte is start_of(k)
    const uint8_t* buf; Start start_of; int64_t n;
    __device__ int64_t operator()(int64_t k) const { return k < n ? seq_tok_len(buf + start_of(k)) + 1 : 0; }
};
struct SeqNameStart {    // new name k: entry name_tok[k] of the intern pass
    const int64_t* starts; const int64_t* name_tok;
    __device__ int64_t operator()(int64_t k) const { return starts[name_tok[k]]; }
};

static __global__ void __launch_bounds__(SEQ_BLOCK) k_seq_row_first(const int64_t* rowx, int64_t P, int64_t T, int64_t* row_first) {
    const int64_t t = P + (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (t >= T) return;
    if (rowx[t + 1] != rowx[t]) row_first[rowx[t]] = t;
    if (t == T - 1) row_first[rowx[T]] = T;
}

static __global__ void __launch_bounds__(SEQ_BLOCK) k_seq_max_len(const int64_t* row_first, int64_t rows, unsigned long long* max_len) {
    typedef hipcub::BlockReduce<unsigned long long, SEQ_BLOCK> Reduce;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t r = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    const unsigned long long mine = r < rows ? (unsigned long long)(row_first[r + 1] - row_first[r]) : 0ull;
    const unsigned long long m = Reduce(tmp).Reduce(mine, hipcub::Max());
    if (threadIdx.x == 0) atomicMax(max_len, m);
}

// id of token t = the number of its string among the first appearances; with intern == 0 a string that first appears behind the prior names is unknown
static __global__ void __launch_bounds__(SEQ_BLOCK) k_seq_ids(const unsigned long long* table, const int64_t* tok_slot, const int64_t* namex, int64_t P, int64_t T, int intern,
                                                       int32_t* tok_id, unsigned long long* unknown) {
    typedef hipcub::BlockReduce<unsigned long long, SEQ_BLOCK> Reduce;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t t = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    unsigned long long u = 0;
    if (t < T) {
        const int64_t rep = (int64_t)table[tok_slot[t]];
        const bool unk = !intern && rep >= P;
        tok_id[t] = unk ? -1 : (int32_t)namex[rep];
        u = (unk && t >= P) ? 1ull : 0ull;
    }
    const unsigned long long sum = Reduce(tmp).Sum(u);
    if (threadIdx.x == 0 && sum) atomicAdd(unknown, sum);
}

static __global__ void __launch_bounds__(SEQ_BLOCK) k_seq_name_tok(const int64_t* namex, int64_t P, int64_t T, int64_t* name_tok) {
    const int64_t t = P + (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (t >= T) return;
    if (namex[t + 1] != namex[t]) name_tok[namex[t] - P] = t;
}

// item k's bytes and a NUL to blob + off[k]; off is the scan of SeqItemLen over the same start_of
template <typename Start>
static __global__ void __launch_bounds__(SEQ_BLOCK) k_seq_tok_bytes(const uint8_t* buf, Start start_of, const int64_t* off, int64_t n, uint8_t* blob) {
    const int64_t k = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (k >= n) return;
    const uint8_t* src = buf + start_of(k);
    const int64_t len = off[k + 1] - off[k] - 1;
    uint8_t* dst = blob + off[k];
    for (int64_t i = 0; i < len; i++) dst[i] = src[i];
    dst[len] = 0;
}

// every row that skip (when given) does not mark must have want tokens: the least row that has not
[[maybe_unused]] static __global__ void __launch_bounds__(SEQ_BLOCK) k_seq_ragged(const int64_t* row_first, const uint8_t* skip, int64_t rows, int64_t want, unsigned long long* ragged) {
    const int64_t r = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (r >= rows || (skip && skip[r])) return;
    if (row_first[r + 1] - row_first[r] != want) atomicMin(ragged, (unsigned long long)r);
}

// one lane: where[0] = newlines in [lo, at), where[1] = bytes between the start of at's line (or lo) and at.  The lane walks inside three chunks at the most,
// however long the line is: the chunks of lo and of at for the counts, and the chunk that holds the last newline in front of at, which the scanned
// per-chunk counts give by bisection (the last chunk with fewer newlines in front of it than at has).
[[maybe_unused]] static __global__ void k_seq_locate(const uint8_t* buf, const int64_t* chunk_nlx, int64_t lo, int64_t at, int64_t* where) {
    int64_t nl[2];
    const int64_t pos[2] = {lo, at};
    for (int i = 0; i < 2; i++) {
        const int64_t c = pos[i] / SEQ_CHUNK;
        nl[i] = chunk_nlx[c];
        for (int64_t b = c * SEQ_CHUNK; b < pos[i]; b++) nl[i] += buf[b] == '\n';
    }
    int64_t b = lo;                                      // no newline in [lo, at): the line starts with the piece
    if (nl[1] > nl[0]) {
        int64_t c = 0, hi = at / SEQ_CHUNK + 1;          // chunk_nlx[0] = 0 < nl[1]; the newline sought lies in front of at
        while (hi - c > 1) { const int64_t mid = (c + hi) >> 1; if (chunk_nlx[mid] < nl[1]) c = mid; else hi = mid; }
        b = at < (c + 1) * SEQ_CHUNK ? at : (c + 1) * SEQ_CHUNK;
        while (b > c * SEQ_CHUNK && buf[b - 1] != '\n') b--;
    }
    where[0] = nl[1] - nl[0];
    where[1] = at - b;
}

// ------------------------------------------------------------------------------------------ host side of one ingest
namespace {

struct SeqRun {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t copied[2] = {nullptr, nullptr};
    dge_stopwatch kernels;            // seq_kernels_begin .. seq_kernels_end, summed in kernel_ms
    uint8_t* pin[2] = {nullptr, nullptr};
    std::vector<SeqPiece> pieces;
    seq_layout L;
    int64_t held = 0;                 // device bytes this call holds (for DGE_ERR_CAP's message)
    const char* what = "seq ingest";  // how the messages about memory name the call
    double read_ms = 0, kernel_ms = 0;
    // device results
    dge_tmp<uint8_t> buf;
    dge_tmp<int64_t> tok_start, tok_len, tok_slot, rowx, row_first, namex;      // tok_len .. tok_id: per ENTRY of the intern pass (seq_intern)
    dge_tmp<uint64_t> tok_hash;
    dge_tmp<unsigned long long> table;
    dge_tmp<int32_t> tok_id;
    dge_tmp<int64_t> chunk_nlx;               // newlines in front of every chunk (the .vec reader turns an offset into a line with it)
    dge_tmp<unsigned long long> words;        // [0] first NUL, [1] longest row, [2] unknown entries, [3] give_up (as int); then the claim counters
    int64_t P = 0, T = 0, lines = 0, rows = 0, max_len = 1, n_names = 0, unknown = 0;
    int64_t N = 0;                    // entries interned: T (.seq: every token), or P + the rows (.vec: the token that opens each)
    ~SeqRun() {
        seq_close_pieces(pieces);
        for (int i = 0; i < 2; i++) { if (pin[i]) (void)hipHostFree(pin[i]); if (copied[i]) (void)hipEventDestroy(copied[i]); }
        if (stream) (void)hipStreamDestroy(stream);
    }
};

template <typename T>
int seq_alloc(SeqRun& R, dge_tmp<T>& t, int64_t n, const char* what) {
    if (t.p) { (void)hipFree(t.p); t.p = nullptr; }
    const size_t bytes = (size_t)(n > 0 ? n : 1) * sizeof(T);
    const hipError_t e = hipMalloc((void**)&t.p, bytes);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        t.p = nullptr;
        DGE_FAIL(DGE_ERR_CAP, "%s: the working set does not fit in device memory: %lld bytes for %s on top of the %lld this call holds", R.what, (long long)bytes, what, (long long)R.held);
    }
    if (e != hipSuccess) { t.p = nullptr; DGE_FAIL(DGE_ERR_DEVICE, "%s: hipMalloc of %lld bytes for %s failed: %s", R.what, (long long)bytes, what, hipGetErrorName(e)); }
    R.held += (int64_t)bytes;
    return DGE_OK;
}
template <typename T>
void seq_release(SeqRun& R, dge_tmp<T>& t, int64_t n) { if (t.p) { (void)hipFree(t.p); t.p = nullptr; R.held -= (int64_t)((size_t)(n > 0 ? n : 1) * sizeof(T)); } }

#define SEQ_TRY(expr) do { int rc__ = (expr); if (rc__) return rc__; } while (0)

// what every run starts with: its device, its name in the messages about memory, its stream
[[maybe_unused]] int seq_open(SeqRun& R, int device, const char* what) {
    R.device = device; R.what = what;
    DGE_HIP(hipStreamCreateWithFlags(&R.stream, hipStreamNonBlocking));
    return DGE_OK;
}

int seq_read_back(SeqRun& R, void* dst, const void* src, size_t bytes) {
    DGE_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, R.stream));
    DGE_HIP(hipStreamSynchronize(R.stream));
    return DGE_OK;
}
int seq_kernels_begin(SeqRun& R) { return R.kernels.start(R.stream); }
int seq_kernels_end(SeqRun& R) {
    float ms = 0.f;
    SEQ_TRY(R.kernels.stop(&ms));
    R.kernel_ms += ms;
    return DGE_OK;
}
unsigned seq_grid(int64_t n) { return (unsigned)((n + SEQ_BLOCK - 1) / SEQ_BLOCK); }

// the allocator of a library call's scratch (dge_two_pass) under the run's accounting; begin: the kernels' clock starts once the scratch is there
struct SeqScratch {
    SeqRun& R; const char* what; bool begin;
    dge_tmp<uint8_t> t;
    int64_t n = 0;
    int operator()(size_t bytes, void** p) { n = (int64_t)bytes; SEQ_TRY(seq_alloc(R, t, n, what)); *p = t.p; return begin ? seq_kernels_begin(R) : DGE_OK; }
    void release() { seq_release(R, t, n); }
};

template <typename In>
int seq_scan(SeqRun& R, In in, int64_t* out, int64_t n) {      // out[i] = sum of in[0 .. i), n entries
    SeqScratch tmp{R, "the scan's scratch", false};
    SEQ_TRY(dge_exclusive_sum(tmp, in, out, n, R.stream, true));
    tmp.release();
    return DGE_OK;
}

// buffer offset -> offset in the caller's text (the pieces taken one after the other, pads and prefix not counted) and the piece it lies in
int64_t seq_text_offset(const SeqRun& R, int64_t at, size_t* piece) {
    int64_t before = 0;
    for (size_t k = 0; k < R.pieces.size(); k++) {
        if (at < R.L.offset[k] + R.pieces[k].size + 1) { *piece = k; return before + (at - R.L.offset[k]); }
        before += R.pieces[k].size;
    }
    *piece = 0;
    return at;
}

// "offset O of the text (piece K[, path]), line L, column C" for a buffer offset; line and column count from 1 inside the piece
[[maybe_unused]] std::string seq_where(SeqRun& R, int64_t at) {
    size_t piece = 0;
    const int64_t off = seq_text_offset(R, at, &piece);
    int64_t where[2] = {0, 0};
    dge_tmp<int64_t> d;
    if (seq_alloc(R, d, 2, "a position") == DGE_OK) {
        hipLaunchKernelGGL(k_seq_locate, dim3(1), dim3(1), 0, R.stream, R.buf.p, R.chunk_nlx.p, R.L.offset[piece], at, d.p);
        (void)seq_read_back(R, where, d.p, sizeof(where));
    }
    char msg[512];
    snprintf(msg, sizeof(msg), "offset %lld of the text (piece %lld%s%s), line %lld, column %lld", (long long)off, (long long)piece, R.pieces[piece].path ? ", " : "",
             R.pieces[piece].path ? R.pieces[piece].path : "", (long long)where[0] + 1, (long long)where[1] + 1);
    return msg;
}

struct SeqOptions { int32_t hash_bits = 64; int64_t initial_slots = 0; int intern = 1; };

// bytes to the device, tokens (first byte, line), rows (rowx, row_first, max_len)
[[maybe_unused]] int seq_tokenise(SeqRun& R, const dge_names* names, const char* who) {
    using clock = std::chrono::steady_clock;
    // ---- layout
    std::string prefix;
    if (names) {
        prefix.reserve((size_t)(names->bytes + (int64_t)names->ptr.size()));
        for (size_t i = 0; i < names->ptr.size(); i++) { prefix.append(names->ptr[i], (size_t)names->len[i]); prefix.push_back('\n'); }
        R.P = (int64_t)names->ptr.size();
    }
    std::vector<int64_t> sizes;
    for (const SeqPiece& p : R.pieces) sizes.push_back(p.size);
    if (!seq_plan_layout((int64_t)prefix.size(), sizes.data(), (int64_t)sizes.size(), &R.L)) DGE_FAIL(DGE_ERR_ARG, "%s: the text's size leaves 64 bits", who);
    SEQ_TRY(seq_open(R, R.device, R.what));
    // ---- bytes to the device: chunk c + 1 is read (or copied out of the caller's memory) into one pinned buffer while chunk c leaves the other
    const auto t0 = clock::now();
    SEQ_TRY(seq_alloc(R, R.buf, R.L.padded, "the text"));
    {
        const int64_t PIN = (int64_t)16 << 20;
        const int64_t pin_bytes = std::min<int64_t>(PIN, std::max<int64_t>(R.L.used, 1));
        for (int i = 0; i < 2; i++) {
            DGE_HIP(hipHostMalloc((void**)&R.pin[i], (size_t)pin_bytes, hipHostMallocDefault));
            DGE_HIP(hipEventCreateWithFlags(&R.copied[i], hipEventDisableTiming));
        }
        SeqJoiner join{R.pieces, prefix};
        int64_t done = 0;
        for (int64_t c = 0; done < R.L.used; c++) {
            const int b = (int)(c & 1);
            if (c >= 2) DGE_HIP(hipEventSynchronize(R.copied[b]));
            int64_t got = 0;
            SEQ_TRY(join.fill(R.pin[b], std::min<int64_t>(pin_bytes, R.L.used - done), &got));
            if (got <= 0) DGE_FAIL(DGE_ERR_IO, "%s: the input ended %lld bytes short", who, (long long)(R.L.used - done));
            DGE_HIP(hipMemcpyAsync(R.buf.p + done, R.pin[b], (size_t)got, hipMemcpyHostToDevice, R.stream));
            DGE_HIP(hipEventRecord(R.copied[b], R.stream));
            done += got;
        }
        DGE_HIP(hipMemsetAsync(R.buf.p + R.L.used, ' ', (size_t)(R.L.padded - R.L.used), R.stream));
        DGE_HIP(hipStreamSynchronize(R.stream));
    }
    R.read_ms = std::chrono::duration<double, std::milli>(clock::now() - t0).count();

    // ---- classify: token starts and newlines per chunk, scanned; a NUL byte ends the call
    const int64_t n_chunks = (R.L.padded - SEQ_TAIL) / SEQ_CHUNK;
    dge_tmp<int64_t> chunk_tok, chunk_nl, chunk_tokx, tok_line;
    dge_tmp<int64_t>& chunk_nlx = R.chunk_nlx;
    dge_tmp<unsigned long long>& words = R.words;
    const int64_t n_words = 4 + (int64_t)SEQ_SHARDS * SEQ_SHARD_STRIDE;
    SEQ_TRY(seq_alloc(R, chunk_tok, n_chunks + 1, "the chunk counts"));
    SEQ_TRY(seq_alloc(R, chunk_nl, n_chunks + 1, "the chunk counts"));
    SEQ_TRY(seq_alloc(R, chunk_tokx, n_chunks + 1, "the chunk counts"));
    SEQ_TRY(seq_alloc(R, chunk_nlx, n_chunks + 1, "the chunk counts"));
    SEQ_TRY(seq_alloc(R, words, n_words, "the counters"));
    SEQ_TRY(seq_kernels_begin(R));
    DGE_HIP(hipMemsetAsync(words.p, 0, (size_t)n_words * 8, R.stream));
    DGE_HIP(hipMemsetAsync(words.p, 0xFF, 8, R.stream));
    DGE_HIP(hipMemsetAsync(chunk_tok.p + n_chunks, 0, 8, R.stream));
    DGE_HIP(hipMemsetAsync(chunk_nl.p + n_chunks, 0, 8, R.stream));
    if (n_chunks) hipLaunchKernelGGL(k_seq_count, dim3((unsigned)n_chunks), dim3(SEQ_BLOCK), 0, R.stream, R.buf.p, R.L.used, chunk_tok.p, chunk_nl.p, words.p);
    SEQ_TRY(seq_scan(R, chunk_tok.p, chunk_tokx.p, n_chunks + 1));
    SEQ_TRY(seq_scan(R, chunk_nl.p, chunk_nlx.p, n_chunks + 1));
    SEQ_TRY(seq_kernels_end(R));
    unsigned long long nul_at = 0;
    int64_t total_nl = 0;
    SEQ_TRY(seq_read_back(R, &nul_at, words.p, 8));
    SEQ_TRY(seq_read_back(R, &R.T, chunk_tokx.p + n_chunks, 8));
    SEQ_TRY(seq_read_back(R, &total_nl, chunk_nlx.p + n_chunks, 8));
    if (nul_at != SEQ_EMPTY) {
        size_t piece = 0;
        const int64_t off = seq_text_offset(R, (int64_t)nul_at, &piece);
        if (R.pieces[piece].path) DGE_FAIL(DGE_ERR_IO, "%s: a NUL byte at offset %lld of the text (in %s): names are handed out as C strings", who, (long long)off, R.pieces[piece].path);
        DGE_FAIL(DGE_ERR_IO, "%s: a NUL byte at offset %lld of the text: names are handed out as C strings", who, (long long)off);
    }
    R.lines = total_nl - R.P;
    const int64_t T = R.T, P = R.P;
    if (T < P) DGE_FAIL(DGE_ERR_STATE, "%s: the prior names did not come back as %lld tokens", who, (long long)P);

    // ---- tokens: first byte, line
    SEQ_TRY(seq_alloc(R, R.tok_start, T, "the tokens' offsets"));
    SEQ_TRY(seq_alloc(R, tok_line, T, "the tokens' lines"));
    SEQ_TRY(seq_alloc(R, R.rowx, T + 1, "the tokens' rows"));
    SEQ_TRY(seq_kernels_begin(R));
    if (n_chunks) hipLaunchKernelGGL(k_seq_emit, dim3((unsigned)n_chunks), dim3(SEQ_BLOCK), 0, R.stream, R.buf.p, chunk_tokx.p, chunk_nlx.p, R.tok_start.p, tok_line.p);
    // ---- rows
    SEQ_TRY(seq_scan(R, rocprim::make_transform_iterator(rocprim::counting_iterator<int64_t>(0), SeqRowFlag{tok_line.p, P, T}), R.rowx.p, T + 1));
    SEQ_TRY(seq_kernels_end(R));
    SEQ_TRY(seq_read_back(R, &R.rows, R.rowx.p + T, 8));
    seq_release(R, tok_line, T);
    SEQ_TRY(seq_alloc(R, R.row_first, R.rows + 1, "the rows' first tokens"));
    SEQ_TRY(seq_kernels_begin(R));
    if (T > P) {
        hipLaunchKernelGGL(k_seq_row_first, dim3(seq_grid(T - P)), dim3(SEQ_BLOCK), 0, R.stream, R.rowx.p, P, T, R.row_first.p);
        hipLaunchKernelGGL(k_seq_max_len, dim3(seq_grid(R.rows)), dim3(SEQ_BLOCK), 0, R.stream, R.row_first.p, R.rows, words.p + 1);
    }
    SEQ_TRY(seq_kernels_end(R));
    unsigned long long longest = 0;
    SEQ_TRY(seq_read_back(R, &longest, words.p + 1, 8));
    R.max_len = std::max<int64_t>((int64_t)longest, 1);
    return DGE_OK;
}

// Entries e = 0 .. N-1, entry e the token whose first byte is starts[e] (device), the first P of them the prior names: length, hash, name table, ids in
// first-appearance order.  The kernels are the same whatever the entries are; the .seq reader interns every token (starts = tok_start, N = T).
[[maybe_unused]] int seq_intern(SeqRun& R, const int64_t* starts, int64_t N, const SeqOptions& opt, const char* who) {
    const int64_t T = N, P = R.P;
    dge_tmp<unsigned long long>& words = R.words;
    const int64_t n_words = 4 + (int64_t)SEQ_SHARDS * SEQ_SHARD_STRIDE;
    R.N = N;
    SEQ_TRY(seq_alloc(R, R.tok_len, T, "the tokens' lengths"));
    SEQ_TRY(seq_alloc(R, R.tok_hash, T, "the tokens' hashes"));
    SEQ_TRY(seq_kernels_begin(R));
    if (T) hipLaunchKernelGGL(k_seq_hash, dim3(seq_grid(T)), dim3(SEQ_BLOCK), 0, R.stream, R.buf.p, starts, T, opt.hash_bits, R.tok_len.p, R.tok_hash.p);
    SEQ_TRY(seq_kernels_end(R));

    // ---- intern: redone with eight times the slots while a pass gives up (seq_plan.h)
    SEQ_TRY(seq_alloc(R, R.tok_slot, T, "the tokens' slots"));
    int64_t slots = seq_slots_first(T, opt.initial_slots);
    for (;;) {
        SEQ_TRY(seq_alloc(R, R.table, slots, "the name table"));
        const bool last = slots >= seq_slots_cap(T);
        const unsigned long long limit = last ? ~0ull : (unsigned long long)std::max<int64_t>(slots / 2 / SEQ_SHARDS, 1);
        SEQ_TRY(seq_kernels_begin(R));
        DGE_HIP(hipMemsetAsync(R.table.p, 0xFF, (size_t)slots * 8, R.stream));
        DGE_HIP(hipMemsetAsync(words.p + 3, 0, (size_t)(n_words - 3) * 8, R.stream));
        if (T) hipLaunchKernelGGL(k_seq_intern, dim3(seq_grid(T)), dim3(SEQ_BLOCK), 0, R.stream, R.buf.p, starts, R.tok_len.p, R.tok_hash.p, T, R.table.p, slots - 1,
                                  R.tok_slot.p, words.p + 4, limit, reinterpret_cast<int*>(words.p + 3));
        SEQ_TRY(seq_kernels_end(R));
        int give_up = 0;
        SEQ_TRY(seq_read_back(R, &give_up, words.p + 3, 4));
        if (!give_up) break;
        if (last) DGE_FAIL(DGE_ERR_STATE, "%s: a name table of %lld slots filled on %lld tokens", who, (long long)slots, (long long)T);
        R.held -= slots * 8;
        (void)hipFree(R.table.p); R.table.p = nullptr;
        slots = seq_slots_next(slots, T);
    }

    // ---- ids in first-appearance order
    SEQ_TRY(seq_alloc(R, R.namex, T + 1, "the names' numbers"));
    SEQ_TRY(seq_alloc(R, R.tok_id, T, "the tokens' ids"));
    SEQ_TRY(seq_kernels_begin(R));
    SEQ_TRY(seq_scan(R, rocprim::make_transform_iterator(rocprim::counting_iterator<int64_t>(0), SeqFirstFlag{R.table.p, R.tok_slot.p, T}), R.namex.p, T + 1));
    SEQ_TRY(seq_kernels_end(R));
    SEQ_TRY(seq_read_back(R, &R.n_names, R.namex.p + T, 8));
    if (R.n_names > 0x7fffffffLL) DGE_FAIL(DGE_ERR_RANGE, "%s: %lld names do not fit int32 ids", who, (long long)R.n_names);
    SEQ_TRY(seq_kernels_begin(R));
    if (T) hipLaunchKernelGGL(k_seq_ids, dim3(seq_grid(T)), dim3(SEQ_BLOCK), 0, R.stream, R.table.p, R.tok_slot.p, R.namex.p, P, T, opt.intern, R.tok_id.p, words.p + 2);
    SEQ_TRY(seq_kernels_end(R));
    unsigned long long unknown = 0;
    SEQ_TRY(seq_read_back(R, &unknown, words.p + 2, 8));
    R.unknown = (int64_t)unknown;
    return DGE_OK;
}

// the indices of the set bytes of flags[0 .. n), ascending, in picked; count: how many are set (the caller has counted them).  what: "the host tokens"
[[maybe_unused]] int seq_pick(SeqRun& R, const uint8_t* flags, int64_t n, int64_t count, dge_tmp<int64_t>& picked, const char* what) {
    dge_tmp<int64_t> numx;
    SEQ_TRY(seq_alloc(R, numx, n + 1, (std::string(what) + "' numbers").c_str()));
    SEQ_TRY(seq_alloc(R, picked, count, what));
    SEQ_TRY(seq_scan(R, rocprim::make_transform_iterator(rocprim::counting_iterator<int64_t>(0), SeqByteFlag{flags, n}), numx.p, n + 1));
    hipLaunchKernelGGL(k_seq_name_tok, dim3(seq_grid(n)), dim3(SEQ_BLOCK), 0, R.stream, numx.p, (int64_t)0, n, picked.p);
    seq_release(R, numx, n + 1);
    return DGE_OK;
}

// The n tokens whose first bytes are at start_of(k) (a device functor), NUL-terminated, in ONE blob for the host: string k at off[k].  Called with the kernels'
// clock running (seq_kernels_begin; the caller's own index kernels stand in front) and stops it before the blob comes back.  what: "the new names"
template <typename Start>
int seq_tokens_to_host(SeqRun& R, Start start_of, int64_t n, std::vector<int64_t>& off, std::unique_ptr<char[]>& host_blob, const char* what) {
    dge_tmp<int64_t> d_off;
    dge_tmp<uint8_t> blob;
    off.assign((size_t)n + 1, 0);
    SEQ_TRY(seq_alloc(R, d_off, n + 1, (std::string(what) + "' offsets").c_str()));
    SEQ_TRY(seq_scan(R, rocprim::make_transform_iterator(rocprim::counting_iterator<int64_t>(0), SeqItemLen<Start>{R.buf.p, start_of, n}), d_off.p, n + 1));
    SEQ_TRY(seq_read_back(R, off.data(), d_off.p, (size_t)(n + 1) * 8));
    SEQ_TRY(seq_alloc(R, blob, off[(size_t)n], (std::string(what) + "' bytes").c_str()));
    hipLaunchKernelGGL(k_seq_tok_bytes<Start>, dim3(seq_grid(n)), dim3(SEQ_BLOCK), 0, R.stream, R.buf.p, start_of, d_off.p, n, blob.p);
    SEQ_TRY(seq_kernels_end(R));
    host_blob.reset(new char[(size_t)off[(size_t)n]]);
    return seq_read_back(R, host_blob.get(), blob.p, (size_t)off[(size_t)n]);
}

// the bytes of the n_new names behind the prior ones (entries as in seq_intern).  A name's length comes from seq_tok_len here, not from the stored tok_len[]:
// the same number by construction, k_seq_hash runs the same seq_run loop over the same bytes.
[[maybe_unused]] int seq_new_names(SeqRun& R, const int64_t* starts, int64_t n_new, std::vector<int64_t>& off, std::unique_ptr<char[]>& host_blob) {
    off.assign((size_t)std::max<int64_t>(n_new, 0) + 1, 0);
    if (n_new <= 0) return DGE_OK;
    dge_tmp<int64_t> name_tok;
    SEQ_TRY(seq_alloc(R, name_tok, n_new, "the new names' tokens"));
    SEQ_TRY(seq_kernels_begin(R));
    hipLaunchKernelGGL(k_seq_name_tok, dim3(seq_grid(R.N - R.P)), dim3(SEQ_BLOCK), 0, R.stream, R.namex.p, R.P, R.N, name_tok.p);
    return seq_tokens_to_host(R, SeqNameStart{starts, name_tok.p}, n_new, off, host_blob, "the new names");
}

// the "C" locale for the numbers the host finishes, whatever the process has set
struct SeqCLocale {
    locale_t c = (locale_t)0;
    ~SeqCLocale() { if (c) freelocale(c); }
    int open(const char* who) {
        c = newlocale(LC_ALL_MASK, "C", (locale_t)0);
        if (!c) DGE_FAIL(DGE_ERR_STATE, "%s: the \"C\" locale is not available", who);
        return DGE_OK;
    }
};

// the n strings of seq_tokens_to_host as numbers: the bits of strtod (T = uint64_t) or of strtof (T = uint32_t)
template <typename T>
int seq_host_numbers(const char* text, const int64_t* off, int64_t n, std::vector<T>& bits, const char* who) {
    SeqCLocale loc;
    SEQ_TRY(loc.open(who));
    bits.resize((size_t)n);
    for (int64_t k = 0; k < n; k++) {
        if constexpr (sizeof(T) == 8) { const double d = strtod_l(text + off[k], nullptr, loc.c); memcpy(&bits[(size_t)k], &d, 8); }
        else { const float f = strtof_l(text + off[k], nullptr, loc.c); memcpy(&bits[(size_t)k], &f, 4); }
    }
    return DGE_OK;
}

// row r for a message: the buffer offset of its first token and how many tokens it has
[[maybe_unused]] int seq_row_where(SeqRun& R, int64_t r, int64_t* at, int64_t* count) {
    int64_t f[2];
    SEQ_TRY(seq_read_back(R, f, R.row_first.p + r, 16));
    *count = f[1] - f[0];
    return seq_read_back(R, at, R.tok_start.p + f[0], 8);
}

}  // namespace
