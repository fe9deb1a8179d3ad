// seq_write.hip — a resident walk corpus out as .seq text (include/dge.h: dge_walks_to_seq_text / dge_walks_write_seq): the mirror image of seq_ingest.hip.
//
// The reference's walk stage writes text (J/CrossTimeGraph.java:127-148, J/SpatialGraph.java:91-121): one line per walk, the names joined by blanks.  The
// lines are sized and spelled here on the device; the host only moves bytes.  This translation unit is outside the build stamp: nothing in it is read or
// written by a training launch.  No floating point anywhere in the text path; all offsets are 64-bit.
//
//   names          one blob of the names' bytes and an int64 offset array, built from dge_names' ptr / len; without names the kernels spell decimals
//   k_sqw_size     per row: the bytes of its line, the column of its last id >= 0, ids >= 0, bare newlines, and the least (row, column) of an id that has
//                  no name — found before a byte is written
//   row_off        an exclusive scan of the line lengths: row r's line is bytes [row_off[r], row_off[r + 1]) of the text
//   k_sqw_emit     OUTPUT-centric: a workgroup owns SEQ_OUT_TILE bytes of the text (seq_out_plan.h), finds the row its first byte lies in by binary search
//                  in row_off, walks the entries from there — a block scan of their byte counts gives every token its place — assembles the tile in LDS and
//                  stores it with one aligned 16-byte store per lane.  Where a tile begins and ends (inside a name, inside a prefix, on a newline) is the
//                  normal case: a token is clipped to the tile, whoever writes it.  Tokens of up to SQW_SHORT bytes are written by the lane that owns the
//                  entry; longer ones go on a list and are copied by the whole workgroup, one byte per lane and trip, so a name longer than a tile costs
//                  a tile's worth of coalesced reads and not one lane's patience.
//
// Every byte of the text is written by exactly one lane of exactly one workgroup, and what it writes depends on the corpus, the names and the flag alone:
// which lane of which launch does it (tile and slab size, the order of the long-token list) changes nothing in the output.
//
// Host side: the text leaves in slabs of SEQ_OUT_SLAB output bytes.  The device holds two slab buffers, the host two pinned ones; slab s + 1 is formatted while
// slab s is copied out and slab s - 1 goes to write() or to the caller's memory.  Nothing is staged through pageable memory.  That loop and the sink are
// text_out_pump.h, shared with flow_text.hip.
#include <algorithm>
#include <chrono>
#include <hipcub/hipcub.hpp>

#include "text_out_pump.h"

// ------------------------------------------------------------------------------------------ kernels
constexpr int SQW_BLOCK = 256;
constexpr int64_t SQW_SHORT = 64;       // tokens (prefix and trailing byte included) up to this many bytes are written by their entry's lane
static_assert(SEQ_OUT_TILE == (int64_t)SQW_BLOCK * 16, "a tile is one 16-byte store per lane");
constexpr unsigned long long SQW_NONE = ~0ull;

struct SqwNames {
    const uint8_t* blob;      // null: a token is the decimal form of its id
    const int64_t* off;       // name v is blob[off[v] .. off[v + 1])
    int64_t count;            // ids at or above it have no name (without names: 2^31)
};

__device__ __forceinline__ int64_t sqw_name_len(const SqwNames& N, int32_t v) { return N.blob ? N.off[v + 1] - N.off[v] : (int64_t)seq_out_digits((uint32_t)v); }

// counters: [0] ids >= 0, [1] rows without one, [2] least row * L + column of an id without a name
__global__ void __launch_bounds__(SQW_BLOCK) k_sqw_size(const int32_t* walks, int32_t L, int64_t n_rows, SqwNames N, int prefix, int64_t* row_len, int32_t* row_last,
                                                        unsigned long long* counters) {
    typedef hipcub::BlockReduce<unsigned long long, SQW_BLOCK> Reduce;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t r = (int64_t)blockIdx.x * SQW_BLOCK + threadIdx.x;
    unsigned long long tokens = 0, empty = 0;
    if (r < n_rows) {
        const int32_t* row = walks + r * L;
        int64_t len = 0, bad = -1;
        int32_t last = -1;
        for (int32_t j = 0; j < L; j++) {
            const int32_t v = row[j];
            if (v < 0) continue;
            if ((int64_t)v >= N.count) { if (bad < 0) bad = r * L + j; continue; }
            len += sqw_name_len(N, v) + (prefix ? seq_out_digits((uint32_t)j) + 1 : 0) + 1;      // + the blank or the newline behind it
            last = j;
            tokens++;
        }
        if (last < 0) { len = 1; empty = 1; }
        row_len[r] = len;
        row_last[r] = last;
        if (bad >= 0) atomicMin(counters + 2, (unsigned long long)bad);
    }
    const unsigned long long t = Reduce(tmp).Sum(tokens);
    __syncthreads();
    const unsigned long long e = Reduce(tmp).Sum(empty);
    if (threadIdx.x == 0) { if (t) atomicAdd(counters, t); if (e) atomicAdd(counters + 1, e); }
}

struct SqwTok { int64_t dst, c; int32_t id, j, trail; };      // c bytes at text offset dst: ["j-"] name, then the byte `trail`; c == 1: the bare newline of a row without ids

__device__ __forceinline__ uint8_t sqw_byte(const SqwNames& N, int prefix, const SqwTok& t, int64_t q) {
    if (q == t.c - 1) return (uint8_t)t.trail;
    if (prefix) {
        const int nd = seq_out_digits((uint32_t)t.j);
        if (q < nd) return seq_out_digit((uint32_t)t.j, nd, (int)q);
        if (q == nd) return (uint8_t)'-';
        q -= nd + 1;
    }
    if (N.blob) return N.blob[N.off[t.id] + q];
    return seq_out_digit((uint32_t)t.id, seq_out_digits((uint32_t)t.id), (int)q);
}

// bytes [slab0, slab1) of the text into out (out[0] is byte slab0; slab0 is a multiple of the tile); block b owns the tile that starts at slab0 + b * SEQ_OUT_TILE
__global__ void __launch_bounds__(SQW_BLOCK) k_sqw_emit(const int32_t* walks, int32_t L, int64_t n_rows, SqwNames N, int prefix, const int64_t* row_off, const int32_t* row_last,
                                                        int64_t slab0, int64_t slab1, uint8_t* out) {
    typedef hipcub::BlockScan<unsigned long long, SQW_BLOCK> Scan;
    __shared__ typename Scan::TempStorage tmp;
    __shared__ __attribute__((aligned(16))) uint8_t tile[SEQ_OUT_TILE];
    __shared__ SqwTok longs[SQW_BLOCK];
    __shared__ int n_long;
    __shared__ int64_t first_row;
    const int tid = threadIdx.x;
    const int64_t t0 = slab0 + (int64_t)blockIdx.x * SEQ_OUT_TILE;
    const int64_t t1 = t0 + SEQ_OUT_TILE < slab1 ? t0 + SEQ_OUT_TILE : slab1;
    if (tid == 0) {      // the row byte t0 lies in: the largest r with row_off[r] <= t0 (every row has at least its newline, so row_off rises strictly)
        int64_t lo = 0, hi = n_rows;
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (row_off[mid] <= t0) lo = mid; else hi = mid;
        }
        first_row = lo;
        n_long = 0;
    }
    __syncthreads();
    const int64_t Lc = L > 0 ? L : 1;      // a corpus of width 0 still has a bare newline per row: entry 0 of the row carries it
    const int64_t e1 = n_rows * Lc;
    int64_t carry = row_off[first_row];
    for (int64_t base = first_row * Lc; base < e1 && carry < t1; base += SQW_BLOCK) {
        const int64_t e = base + tid;
        SqwTok t;
        t.c = 0; t.id = -1; t.j = 0; t.trail = '\n';
        if (e < e1) {
            const int64_t r = e / Lc;
            t.j = (int32_t)(e - r * Lc);
            const int32_t last = row_last[r];
            t.id = t.j < L ? walks[r * L + t.j] : -1;
            if (t.id >= 0) {
                t.c = sqw_name_len(N, t.id) + (prefix ? seq_out_digits((uint32_t)t.j) + 1 : 0) + 1;
                t.trail = t.j == last ? '\n' : ' ';
            } else if (t.j == 0 && last < 0) {
                t.c = 1;
            }
        }
        unsigned long long before, total;
        Scan(tmp).ExclusiveSum((unsigned long long)t.c, before, total);
        t.dst = carry + (int64_t)before;
        if (t.c > 0 && t.dst < t1 && t.dst + t.c > t0) {
            if (t.c <= SQW_SHORT) {
                const int64_t k1 = t.dst + t.c < t1 ? t.dst + t.c : t1;
                for (int64_t k = t.dst > t0 ? t.dst : t0; k < k1; k++) tile[k - t0] = sqw_byte(N, prefix, t, k - t.dst);
            } else {
                longs[atomicAdd(&n_long, 1)] = t;
            }
        }
        __syncthreads();
        const int nl = n_long;
        for (int i = 0; i < nl; i++) {
            const SqwTok g = longs[i];
            const int64_t k1 = g.dst + g.c < t1 ? g.dst + g.c : t1;
            for (int64_t k = (g.dst > t0 ? g.dst : t0) + tid; k < k1; k += SQW_BLOCK) tile[k - t0] = sqw_byte(N, prefix, g, k - g.dst);
        }
        __syncthreads();
        if (tid == 0) n_long = 0;
        __syncthreads();
        carry += (int64_t)total;
    }
    __syncthreads();
    // one aligned 16-byte store per lane.  The store that holds the slab's last byte is whole too: the buffer is whole tiles, and what lies behind slab1 in it
    // is never copied out.
    if (t0 + (int64_t)tid * 16 < t1) *reinterpret_cast<uint4*>(out + (t0 - slab0) + (int64_t)tid * 16) = *reinterpret_cast<const uint4*>(tile + tid * 16);
}

// ------------------------------------------------------------------------------------------ host side
namespace {

#define SQW_TRY(expr) do { int rc__ = (expr); if (rc__) return rc__; } while (0)

struct SqwRun : TextPump {                                          // the streams, the events and the slab buffers: text_out_pump.h
    dge_tmp<uint8_t> blob, scratch;
    dge_tmp<int64_t> name_off, row_len, row_off;
    dge_tmp<int32_t> row_last;
    dge_tmp<unsigned long long> counters;
    ~SqwRun() { drain(); }                                          // the streams rest before the arrays above go
};

using SqwSink = TextSink;

// what both entries check before a device is looked for
int sqw_check(const char* who, const dge_walks* w, int64_t row0, int64_t n_rows, bool null_or_negative) {
    if (!w || null_or_negative || row0 < 0 || n_rows < 0) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    if (row0 > w->n || n_rows > w->n - row0) DGE_FAIL(DGE_ERR_ARG, "%s: rows [%lld, %lld) leave the corpus of %lld rows", who, (long long)row0, (long long)(row0 + n_rows), (long long)w->n);
    return DGE_OK;
}

int sqw_run(const dge_walks* w, int64_t row0, int64_t n_rows, const dge_names* names, int prefix, SqwSink& sink, int64_t* n_bytes, dge_seq_out_info* info) {
    using clock = std::chrono::steady_clock;
    const char* who = sink.who;
    SQW_TRY(dge_require_device(w->device));
    SqwRun R;
    SQW_TRY(R.open());
    SQW_TRY(dge_walks_order(w, R.ks));                              // every kernel that reads the rows runs on ks: behind a model's launch that still writes them
    const int32_t L = w->L;
    const int32_t* walks = w->d + row0 * L;
    prefix = prefix ? 1 : 0;

    // ---- names: one blob, one offset array
    SqwNames N{nullptr, nullptr, (int64_t)1 << 31};
    std::vector<int64_t> off;
    std::vector<uint8_t> bytes;
    if (names) {
        const size_t n = names->ptr.size();
        off.assign(n + 1, 0);
        bytes.resize((size_t)std::max<int64_t>(names->bytes, 1));
        for (size_t v = 0; v < n; v++) {
            memcpy(bytes.data() + off[v], names->ptr[v], (size_t)names->len[v]);
            off[v + 1] = off[v] + names->len[v];
        }
        SQW_TRY(R.blob.alloc(bytes.size()));
        SQW_TRY(R.name_off.alloc(n + 1));
        DGE_HIP(hipMemcpyAsync(R.blob.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice, R.ks));
        DGE_HIP(hipMemcpyAsync(R.name_off.p, off.data(), (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, R.ks));
        DGE_HIP(hipStreamSynchronize(R.ks));
        N.blob = R.blob.p; N.off = R.name_off.p; N.count = (int64_t)n;
    }

    // ---- sizing: line lengths, their scan, the counts, the first id without a name
    int64_t total = 0;
    unsigned long long counters[3] = {0, 0, SQW_NONE};
    if (n_rows > 0) {
        SQW_TRY(R.row_len.alloc((size_t)n_rows + 1));
        SQW_TRY(R.row_off.alloc((size_t)n_rows + 1));
        SQW_TRY(R.row_last.alloc((size_t)n_rows));
        SQW_TRY(R.counters.alloc(3));
        auto scratch_then_sizes = [&](size_t scan_bytes, void** p) -> int {         // the scan's input is made once its scratch is there and the clock runs
            SQW_TRY(R.scratch.alloc(scan_bytes));
            *p = R.scratch.p;
            DGE_HIP(hipEventRecord(R.ka[0], R.ks));
            DGE_HIP(hipMemsetAsync(R.counters.p, 0, 16, R.ks));
            DGE_HIP(hipMemsetAsync(R.counters.p + 2, 0xFF, 8, R.ks));
            DGE_HIP(hipMemsetAsync(R.row_len.p + n_rows, 0, 8, R.ks));
            hipLaunchKernelGGL(k_sqw_size, dim3(dge_grid(n_rows, SQW_BLOCK)), dim3(SQW_BLOCK), 0, R.ks, walks, L, n_rows, N, prefix, R.row_len.p, R.row_last.p, R.counters.p);
            DGE_HIP(hipGetLastError());
            return DGE_OK;
        };
        SQW_TRY(dge_exclusive_sum(scratch_then_sizes, R.row_len.p, R.row_off.p, n_rows + 1, R.ks, false));
        DGE_HIP(hipEventRecord(R.kb[0], R.ks));
        DGE_HIP(hipMemcpyAsync(counters, R.counters.p, sizeof counters, hipMemcpyDeviceToHost, R.ks));
        DGE_HIP(hipMemcpyAsync(&total, R.row_off.p + n_rows, 8, hipMemcpyDeviceToHost, R.ks));
        DGE_HIP(hipStreamSynchronize(R.ks));
        SQW_TRY(R.add_kernel_ms(0));
        if (counters[2] != SQW_NONE) {
            const int64_t key = (int64_t)counters[2];
            int32_t id = 0;
            DGE_HIP(hipMemcpyAsync(&id, walks + key, 4, hipMemcpyDeviceToHost, R.ks));
            DGE_HIP(hipStreamSynchronize(R.ks));
            DGE_FAIL(DGE_ERR_RANGE, "%s: id %d in row %lld, column %lld has no name: the names hold %lld", who, id, (long long)(row0 + key / L), (long long)(key % L), (long long)N.count);
        }
    }

    // ---- the sink: nothing has been written, created or truncated up to here
    int done = 0;
    SQW_TRY(sink.begin(total, n_bytes, &done));
    const auto t0 = clock::now();
    if (!done)
        SQW_TRY(R.run(total, sink, nullptr, [&](int64_t s0, int64_t s1, uint8_t* out) -> int {
            hipLaunchKernelGGL(k_sqw_emit, dim3((unsigned)seq_out_tiles(s1 - s0)), dim3(SQW_BLOCK), 0, R.ks, walks, L, n_rows, N, prefix, R.row_off.p, R.row_last.p, s0, s1, out);
            return DGE_OK;
        }));
    SQW_TRY(sink.end());
    if (info) {
        info->bytes = total; info->lines = n_rows; info->tokens = (int64_t)counters[0]; info->empty_lines = (int64_t)counters[1];
        info->kernel_ms = R.kernel_ms;
        info->write_ms = std::chrono::duration<double, std::milli>(clock::now() - t0).count();
    }
    return DGE_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------ entries
extern "C" int dge_walks_to_seq_text(const dge_walks* w, int64_t row0, int64_t n_rows, const dge_names* names, int position_prefix, char* text, int64_t cap, int64_t* n_bytes,
                                     dge_seq_out_info* info) {
    SQW_TRY(sqw_check("dge_walks_to_seq_text", w, row0, n_rows, !n_bytes || cap < 0 || (cap > 0 && !text)));
    SqwSink sink{"dge_walks_to_seq_text"};
    sink.text = text; sink.cap = cap;
    return sqw_run(w, row0, n_rows, names, position_prefix, sink, n_bytes, info);
}

extern "C" int dge_walks_write_seq(const dge_walks* w, int64_t row0, int64_t n_rows, const dge_names* names, int position_prefix, const char* path, int append,
                                   dge_seq_out_info* info) {
    SQW_TRY(sqw_check("dge_walks_write_seq", w, row0, n_rows, !path));
    SqwSink sink{"dge_walks_write_seq"};
    sink.path = path; sink.append = append;
    return sqw_run(w, row0, n_rows, names, position_prefix, sink, nullptr, info);
}
