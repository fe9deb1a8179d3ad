// flow_text.hip — the resident flow table out as text (include/dge.h: dge_flows_to_text / dge_flows_write_text, dge_flows_time_series / _text /
// dge_flows_write_time_series): the .od edge files, the layered edge text, the .matrix adjacency files and the in / out traffic time series that the
// reference writes from taxiFlows (J/Tracts.java:187-330, J/CommunityAreas.java:127-166).  seq_write.hip's design applied to a sparse table: the text is sized
// and spelled on the device, the host only moves bytes.  This translation unit is outside the build stamp: nothing in it is read or written by a training
// launch.  No floating point anywhere in the text path; all offsets are 64-bit.
//
//   edges          both sources end as sorted device keys (slice R + rank of src id) R + rank of dst id with int64 weights (dge_flows_slot_keys, trip_map.hip;
//                  dge_flows_window_keys, flow_windows.hip); k_ft_bounds finds the slices' boundaries in them by bisection
//   .od, layered   k_ft_od_len: a lane per edge gives the bytes of its line from digit counts; an exclusive scan gives every line its place; slice k's text is
//                  the bytes between the offsets of its first edge and of the next slice's
//   .matrix        WITHOUT n^2 (flow_text_plan.h): the edges with both ends selected are compacted in key order (k_ft_mat_compact; `select` re-ranks rows and
//                  columns through map[rank]), P is the scan of (digits(w) - 1) over them, rowb the first kept edge of every row (k_ft_rowb, bisection).  Row
//                  i starts at 2 n i + P[rowb[i]]; the zeros exist only as arithmetic
//   time series    out: a reduce-by-key of the table over (hour, src), contiguous in key order, scattered to the selected rows (k_ft_series_out); in: an
//                  integer atomic add from a lane per entry whose two ends are selected (k_ft_series_in) — integers, so the order of the adds does not
//                  matter.  k_ft_series_len sizes the two lines of every region; the text goes through the same emitter, 25 decimals per line
//   k_ft_emit      ONE emitter, OUTPUT-centric: a workgroup owns SEQ_OUT_TILE bytes of the text.  Lines (.od, layered, series): it finds the line its first
//                  byte lies in by binary search in the offsets; lane t takes the t-th line from there (a tile holds a few hundred at most) and spells it
//                  into LDS, clipped to the tile.  Matrix: lane t owns bytes [16 t, 16 t + 16) of the tile, finds row and entry of its first byte by
//                  bisection (ftp_seek) and walks on a byte at a time (ftp_next).  Then one aligned 16-byte store per lane.  Where a tile begins and ends
//                  (inside a number, on a separator) is the normal case.
//
// Every byte of a text is written by exactly one lane of exactly one workgroup, and what it writes depends on the table and the arguments alone.  Plain C++
// and vector stores only.  Host side: the slab pump of text_out_pump.h, shared with seq_write.hip; device memory is bounded by the edges and two slabs
// whatever n is.
//
// Coherence: no protocol.  Every array is written by one kernel and read by later ones on the same stream, or after a host wait on another.
#include <chrono>
#include <numeric>

#include "flow_text_plan.h"
#include "text_out_pump.h"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"      // trip_flows.h and od_commit.h hold static passes for their other users: the join, the decode, the commit
#include "trip_flows.h"
#pragma clang diagnostic pop

// ------------------------------------------------------------------------------------------ kernels
constexpr int FT_BLOCK = 256;
static_assert(SEQ_OUT_TILE == (int64_t)FT_BLOCK * 16, "a tile is one 16-byte store per lane");
enum { FT_OD = DGE_FLOW_TEXT_OD, FT_LAYERED = DGE_FLOW_TEXT_OD_LAYERED, FT_MATRIX = DGE_FLOW_TEXT_MATRIX, FT_SERIES = 3 };

// first[k] = the first of the sorted edges that belongs to slice k or a later one, k = 0 .. S
__global__ void __launch_bounds__(FT_BLOCK) k_ft_bounds(const uint64_t* key, int64_t E, uint64_t R, int64_t S, int64_t* first) {
    const int64_t k = (int64_t)blockIdx.x * FT_BLOCK + threadIdx.x;
    if (k <= S) first[k] = coo_lower_bound(key, E, (uint64_t)k * R * R);
}

// out[i] = val[idx[i * stride]] and at[i] = idx[i * stride]: the few numbers the host needs of two long arrays
__global__ void __launch_bounds__(FT_BLOCK) k_ft_gather(const int64_t* val, const int64_t* idx, int64_t stride, int64_t count, int64_t* out, int64_t* at) {
    const int64_t i = (int64_t)blockIdx.x * FT_BLOCK + threadIdx.x;
    if (i < count) { const int64_t j = idx[i * stride]; at[i] = j; out[i] = val[j]; }
}

// the bytes of edge e's line; S > 0: the layered form with its two slice numbers.  len[E] = 0 for the scan
__global__ void __launch_bounds__(FT_BLOCK) k_ft_od_len(const uint64_t* key, const int64_t* w, int64_t E, uint64_t R, const int64_t* id_by_rank, int32_t S, int64_t* len) {
    const int64_t e = (int64_t)blockIdx.x * FT_BLOCK + threadIdx.x;
    if (e > E) return;
    int64_t n = 0;
    if (e < E) {
        const uint64_t k = key[e];
        n = ftp_len(id_by_rank[(k / R) % R]) + ftp_len(id_by_rank[k % R]) + ftp_len(w[e]) + 3;
        if (S > 0) { const int64_t s = (int64_t)(k / R / R); n += ftp_len(s) + ftp_len((s + 1) % S) + 2; }
    }
    len[e] = n;
}

// edge e0 + i is kept when both its ends are selected: map[rank] is the region's number among the selected ones, or -1
struct FtKeep {
    const uint64_t* key; const int32_t* map; uint64_t R; int64_t e0, m;
    __device__ int64_t operator()(int64_t i) const { if (i >= m) return 0; const uint64_t k = key[e0 + i]; return map[(k / R) % R] >= 0 && map[k % R] >= 0 ? 1 : 0; }
};
// the kept edges in key order: row (slice - k0) n + the source's number, the destination's number as column, the weight
__global__ void __launch_bounds__(FT_BLOCK) k_ft_mat_compact(const uint64_t* key, const int64_t* w, int64_t e0, int64_t m, uint64_t R, const int32_t* map, const int64_t* pos, int64_t k0,
                                                             int64_t n, int64_t* crow, int32_t* ccol, int64_t* cw) {
    const int64_t i = (int64_t)blockIdx.x * FT_BLOCK + threadIdx.x;
    if (i >= m) return;
    const uint64_t k = key[e0 + i];
    const int32_t a = map[(k / R) % R], b = map[k % R];
    if (a < 0 || b < 0) return;
    const int64_t at = pos[i];
    crow[at] = ((int64_t)(k / R / R) - k0) * n + a;
    ccol[at] = b;
    cw[at] = w[e0 + i];
}
struct FtExtra {
    const int64_t* cw; int64_t M;
    __device__ int64_t operator()(int64_t i) const { return i < M ? ftp_digits_u((uint64_t)cw[i]) - 1 : 0; }
};
// rowb[i] = the first kept edge of row i or a later one, i = 0 .. rows
__global__ void __launch_bounds__(FT_BLOCK) k_ft_rowb(const int64_t* crow, int64_t M, int64_t rows, int64_t* rowb) {
    const int64_t i = (int64_t)blockIdx.x * FT_BLOCK + threadIdx.x;
    if (i <= rows) rowb[i] = coo_lower_bound(crow, M, i);
}

// in[r][h] += c(h, s, r) for the entries whose two ends are selected; map[region index] is the region's number among the selected ones, or -1
__global__ void __launch_bounds__(FT_BLOCK) k_ft_series_in(const uint64_t* key, const int64_t* cnt, int64_t N, uint64_t R, const int32_t* map, int64_t* in) {
    const int64_t i = (int64_t)blockIdx.x * FT_BLOCK + threadIdx.x;
    if (i >= N) return;
    const uint64_t k = key[i];
    const int32_t s = map[(k / R) % R], e = map[k % R];
    if (s < 0 || e < 0) return;
    atomicAdd(reinterpret_cast<unsigned long long*>(in + (int64_t)e * 24 + (int64_t)(k / R / R)), (unsigned long long)cnt[i]);
}
struct FtHourSrc {
    const uint64_t* key; uint64_t R;
    __device__ uint64_t operator()(int64_t i) const { return key[i] / R; }
};
// the sums over all destinations by (hour, src), to the selected rows
__global__ void __launch_bounds__(FT_BLOCK) k_ft_series_out(const uint64_t* ukey, const int64_t* usum, int64_t U, uint64_t R, const int32_t* map, int64_t* out) {
    const int64_t i = (int64_t)blockIdx.x * FT_BLOCK + threadIdx.x;
    if (i >= U) return;
    const uint64_t k = ukey[i];
    const int32_t s = map[k % R];
    if (s >= 0) out[(int64_t)s * 24 + (int64_t)(k / R)] = usum[i];
}
// line 2 r: the id and the 24 sums into region r; line 2 r + 1: the negated id and the 24 sums out of it.  len[2 n] = 0 for the scan
__global__ void __launch_bounds__(FT_BLOCK) k_ft_series_len(const int64_t* ids, const int64_t* in, const int64_t* out, int64_t n, int64_t* len) {
    const int64_t l = (int64_t)blockIdx.x * FT_BLOCK + threadIdx.x;
    if (l > 2 * n) return;
    int64_t c = 0;
    if (l < 2 * n) {
        const int64_t r = l >> 1;
        const int64_t* v = ((l & 1) ? out : in) + r * 24;
        c = ftp_len((l & 1) ? -ids[r] : ids[r]) + 1;
        for (int h = 0; h < 24; h++) c += 1 + ftp_len(v[h]);
    }
    len[l] = c;
}

struct FtJob {
    int32_t kind, S;                   // FT_*; the slices of the layered form
    uint32_t sep;
    // lines (.od, layered, series): item i of [e0, e1) is bytes [off[i] - base, off[i + 1] - base) of the text
    const int64_t* off; int64_t e0, e1, base;
    const uint64_t* key; const int64_t* w; const int64_t* id_by_rank; uint64_t R;      // .od, layered: the edges
    const int64_t* ids; const int64_t* in; const int64_t* out;                         // series: the selected ids and the two [n x 24] sums
    // matrix (flow_text_plan.h): rowb points at the slice's first row; pbase = P[rowb[0]], what the rows in front of the slice hold
    const int32_t* ccol; const int64_t* cw; const int64_t* P; const int64_t* rowb; int64_t n, pbase;
};

// the bytes of "%lld" of v at text offset pos, clipped to the tile [t0, t1); -> the offset behind them
__device__ __forceinline__ int64_t ft_put(uint8_t* tile, int64_t t0, int64_t t1, int64_t pos, int64_t v) {
    const int len = ftp_len(v);
    if (pos + len > t0 && pos < t1) {
        uint64_t m = ftp_mag(v);
        const int lead = v < 0 ? 1 : 0;
        for (int q = len - 1; q >= lead; q--) {                      // from the last digit forward: a division by ten each
            const int64_t at = pos + q;
            if (at >= t0 && at < t1) tile[at - t0] = (uint8_t)('0' + m % 10u);
            m /= 10u;
        }
        if (lead && pos >= t0) tile[pos - t0] = (uint8_t)'-';
    }
    return pos + len;
}
__device__ __forceinline__ int64_t ft_putc(uint8_t* tile, int64_t t0, int64_t t1, int64_t pos, uint8_t c) {
    if (pos >= t0 && pos < t1) tile[pos - t0] = c;
    return pos + 1;
}

// bytes [slab0, slab1) of the text into out (out[0] is byte slab0; slab0 is a multiple of the tile); block b owns the tile that starts at slab0 + b * SEQ_OUT_TILE
__global__ void __launch_bounds__(FT_BLOCK) k_ft_emit(FtJob J, int64_t slab0, int64_t slab1, uint8_t* out) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[SEQ_OUT_TILE];
    __shared__ int64_t first_item;
    const int tid = threadIdx.x;
    const int64_t t0 = slab0 + (int64_t)blockIdx.x * SEQ_OUT_TILE;
    const int64_t t1 = t0 + SEQ_OUT_TILE < slab1 ? t0 + SEQ_OUT_TILE : slab1;
    if (J.kind == FT_MATRIX) {
        const int64_t q0 = t0 + (int64_t)tid * 16;
        if (q0 < t1) {
            const int64_t q1 = q0 + 16 < t1 ? q0 + 16 : t1;
            ftp_cursor c;
            ftp_seek(c, J.n, J.n, J.ccol, J.P, J.rowb, q0 + J.pbase);          // (the slice's rows start at pbase in P's count: the shift cancels in c.q)
            unsigned long long lo = 0, hi = 0;
            for (int k = 0; k < (int)(q1 - q0); k++) {
                const unsigned long long ch = ftp_next(c, J.n, J.n, J.ccol, J.P, J.cw, J.rowb, (uint8_t)J.sep);
                if (k < 8) lo |= ch << (8 * k); else hi |= ch << (8 * (k - 8));
            }
            *reinterpret_cast<ulonglong2*>(tile + tid * 16) = make_ulonglong2(lo, hi);
        }
    } else {
        if (tid == 0) {      // the line byte t0 lies in: the largest i with off[i] - base <= t0 (every line has at least its newline, so the offsets rise strictly)
            int64_t lo = J.e0, hi = J.e1;
            while (hi - lo > 1) {
                const int64_t mid = lo + (hi - lo) / 2;
                if (J.off[mid] - J.base <= t0) lo = mid; else hi = mid;
            }
            first_item = lo;
        }
        __syncthreads();
        for (int64_t i = first_item + tid; i < J.e1; i += FT_BLOCK) {
            int64_t pos = J.off[i] - J.base;
            if (pos >= t1) break;
            if (J.kind == FT_SERIES) {
                const int64_t r = i >> 1;
                const int64_t* v = ((i & 1) ? J.out : J.in) + r * 24;
                pos = ft_put(tile, t0, t1, pos, (i & 1) ? -J.ids[r] : J.ids[r]);
                for (int h = 0; h < 24; h++) { pos = ft_putc(tile, t0, t1, pos, (uint8_t)','); pos = ft_put(tile, t0, t1, pos, v[h]); }
            } else {
                const uint64_t k = J.key[i];
                const int64_t s = (int64_t)(k / J.R / J.R);
                if (J.kind == FT_LAYERED) { pos = ft_put(tile, t0, t1, pos, s); pos = ft_putc(tile, t0, t1, pos, (uint8_t)'-'); }
                pos = ft_put(tile, t0, t1, pos, J.id_by_rank[(k / J.R) % J.R]);
                pos = ft_putc(tile, t0, t1, pos, (uint8_t)' ');
                if (J.kind == FT_LAYERED) { pos = ft_put(tile, t0, t1, pos, (s + 1) % J.S); pos = ft_putc(tile, t0, t1, pos, (uint8_t)'-'); }
                pos = ft_put(tile, t0, t1, pos, J.id_by_rank[k % J.R]);
                pos = ft_putc(tile, t0, t1, pos, (uint8_t)' ');
                pos = ft_put(tile, t0, t1, pos, J.w[i]);
            }
            ft_putc(tile, t0, t1, pos, (uint8_t)'\n');
        }
    }
    __syncthreads();
    // one aligned 16-byte store per lane.  The store that holds the slab's last byte is whole too: the buffer is whole tiles, and what lies behind slab1 in it
    // is never copied out.
    if (t0 + (int64_t)tid * 16 < t1) *reinterpret_cast<uint4*>(out + (t0 - slab0) + (int64_t)tid * 16) = *reinterpret_cast<const uint4*>(tile + tid * 16);
}

// ------------------------------------------------------------------------------------------ host side
namespace {

using ft_clock = std::chrono::steady_clock;

struct FtCall {                        // one entry's run: the sizing passes' stream and clock, the pump, the report
    const char* who;
    SeqRun R;
    TextPump pump;
    dge_flow_text_info I = {};
    explicit FtCall(const char* w) : who(w) {}
    int open(int device) { SEQ_TRY(dge_require_device(device)); SEQ_TRY(seq_open(R, device, who)); return pump.open(); }
    void report(dge_flow_text_info* info) { if (info) { *info = I; info->kernel_ms += R.kernel_ms + pump.kernel_ms; } }
};

struct FtEdges {
    dge_tmp<uint64_t> key;
    dge_tmp<int64_t> w, first;
    int64_t E = 0;
    int32_t S = 0;
    uint64_t Ru = 1;
};

// the slices struct by itself: no handle is read
int ft_slices_check(const dge_flow_slices* s, const char* who, int32_t* S) {
    if (s->K < 0 || s->reserved != 0) DGE_FAIL(DGE_ERR_ARG, "%s: the slices hold K = %d and reserved = %d: K >= 0 and reserved = 0 are needed", who, s->K, s->reserved);
    if (s->K == 0) { SEQ_TRY(dge_flows_slot_check(s->T, s->mode, who)); *S = s->T; return DGE_OK; }
    if (s->T != 0 || s->mode != 0) DGE_FAIL(DGE_ERR_ARG, "%s: the slices hold K = %d windows and T = %d, mode = %d: with windows T and mode are 0", who, s->K, s->T, s->mode);
    SEQ_TRY(dge_flows_windows_check(s->win, s->K, who));
    *S = s->K;
    return DGE_OK;
}

// what the two text entries check before a device is looked for: plain values first, the table last.  slice < 0: every slice (the file entry)
int ft_check(const char* who, const dge_flows* f, const dge_flow_slices* s, int32_t kind, int32_t slice, const uint8_t* select, int32_t sep, bool null_or_negative, int32_t* S) {
    if (!s || null_or_negative) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    if (kind != DGE_FLOW_TEXT_OD && kind != DGE_FLOW_TEXT_OD_LAYERED && kind != DGE_FLOW_TEXT_MATRIX)
        DGE_FAIL(DGE_ERR_ARG, "%s: kind %d is none of DGE_FLOW_TEXT_OD, DGE_FLOW_TEXT_OD_LAYERED, DGE_FLOW_TEXT_MATRIX", who, kind);
    if (kind == DGE_FLOW_TEXT_MATRIX) { if (sep != ',' && sep != ' ' && sep != '\t') DGE_FAIL(DGE_ERR_ARG, "%s: sep %d is none of ',', ' ', '\\t'", who, sep); }
    else if (sep != 0 || select) DGE_FAIL(DGE_ERR_ARG, "%s: the .od kinds take sep = 0 and select = NULL, not sep %d and a %s select", who, sep, select ? "given" : "null");
    SEQ_TRY(ft_slices_check(s, who, S));
    if (slice >= 0 && slice >= (kind == DGE_FLOW_TEXT_OD_LAYERED ? 1 : *S))
        DGE_FAIL(DGE_ERR_ARG, "%s: slice = %d is outside 0 .. %d%s", who, slice, kind == DGE_FLOW_TEXT_OD_LAYERED ? 0 : *S - 1, kind == DGE_FLOW_TEXT_OD_LAYERED ? " (the layered text is one)" : "");
    if (!f) DGE_FAIL(DGE_ERR_ARG, "%s: null table", who);
    return DGE_OK;
}

// the regions' indices in ascending id (ids are distinct: dge_regions_create)
std::vector<int64_t> ft_by_rank(const dge_regions* rg) {
    std::vector<int64_t> order((size_t)rg->R);
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return rg->ids[(size_t)a] < rg->ids[(size_t)b]; });
    return order;
}

int ft_edges(FtCall& C, const dge_flows* f, const dge_flow_slices* s, int32_t S, FtEdges& X) {
    X.S = S;
    X.Ru = (uint64_t)std::max<int64_t>(f->regions->R, 1);
    SEQ_TRY(s->K == 0 ? dge_flows_slot_keys(f, s->T, s->mode, C.who, X.key, X.w, &X.E, &C.I.kernel_ms) : dge_flows_window_keys(f, s->win, s->K, C.who, X.key, X.w, &X.E, &C.I.kernel_ms));
    if (X.E == 0) return DGE_OK;
    SEQ_TRY(seq_alloc(C.R, X.first, (int64_t)S + 1, "the slices' first edges"));
    SEQ_TRY(seq_kernels_begin(C.R));
    hipLaunchKernelGGL(k_ft_bounds, dim3(seq_grid((int64_t)S + 1)), dim3(FT_BLOCK), 0, C.R.stream, X.key.p, X.E, X.Ru, (int64_t)S, X.first.p);
    DGE_HIP(hipGetLastError());
    return seq_kernels_end(C.R);
}

// val[idx[i * stride]] and idx[i * stride], i = 0 .. count - 1, on the host
int ft_gather(FtCall& C, const int64_t* val, const int64_t* idx, int64_t stride, int64_t count, std::vector<int64_t>& out, std::vector<int64_t>& at) {
    dge_tmp<int64_t> d_out, d_at;
    out.assign((size_t)count, 0); at.assign((size_t)count, 0);
    SEQ_TRY(seq_alloc(C.R, d_out, count, "the slices' offsets"));
    SEQ_TRY(seq_alloc(C.R, d_at, count, "the slices' offsets"));
    hipLaunchKernelGGL(k_ft_gather, dim3(seq_grid(count)), dim3(FT_BLOCK), 0, C.R.stream, val, idx, stride, count, d_out.p, d_at.p);
    DGE_HIP(hipGetLastError());
    SEQ_TRY(seq_read_back(C.R, out.data(), d_out.p, (size_t)count * 8));
    return seq_read_back(C.R, at.data(), d_at.p, (size_t)count * 8);
}

// a text of `total` bytes to its sink through the pump: the sink is opened here, after everything the sizing could find
int ft_deliver(FtCall& C, const FtJob& J, int64_t total, TextSink& sink, int64_t* n_bytes) {
    int done = 0;
    SEQ_TRY(sink.begin(total, n_bytes, &done));
    const auto t0 = ft_clock::now();
    if (!done)
        SEQ_TRY(C.pump.run(total, sink, C.who, [&](int64_t s0, int64_t s1, uint8_t* out) -> int {
            hipLaunchKernelGGL(k_ft_emit, dim3((unsigned)seq_out_tiles(s1 - s0)), dim3(FT_BLOCK), 0, C.pump.ks, J, s0, s1, out);
            return DGE_OK;
        }));
    SEQ_TRY(sink.end());
    C.I.write_ms += std::chrono::duration<double, std::milli>(ft_clock::now() - t0).count();
    C.I.bytes += total;
    C.I.slices++;
    return DGE_OK;
}

// a matrix over a table without edges: zero arrays of the shapes the emitter reads
struct FtZeros {
    dge_tmp<int64_t> P, rowb, cw;
    dge_tmp<int32_t> ccol;
    int make(FtCall& C, int64_t n, FtJob& J) {
        SEQ_TRY(seq_alloc(C.R, P, 1, "the kept edges' extra digits"));
        SEQ_TRY(seq_alloc(C.R, cw, 1, "the kept edges' weights"));
        SEQ_TRY(seq_alloc(C.R, ccol, 1, "the kept edges' columns"));
        SEQ_TRY(seq_alloc(C.R, rowb, n + 1, "the rows' first edges"));
        DGE_HIP(hipMemsetAsync(P.p, 0, 8, C.R.stream));
        DGE_HIP(hipMemsetAsync(cw.p, 0, 8, C.R.stream));
        DGE_HIP(hipMemsetAsync(ccol.p, 0, 4, C.R.stream));
        DGE_HIP(hipMemsetAsync(rowb.p, 0, (size_t)(n + 1) * 8, C.R.stream));
        DGE_HIP(hipStreamSynchronize(C.R.stream));
        J.ccol = ccol.p; J.cw = cw.p; J.P = P.p; J.rowb = rowb.p; J.n = n; J.pbase = 0;
        return DGE_OK;
    }
};

// what a kind needs beside the edges, for the slices [k0, k1), and the job of each of them
struct FtTexts {
    int32_t kind = 0, k0 = 0, k1 = 0;
    dge_tmp<int64_t> off;                              // .od, layered: the lines' offsets
    dge_tmp<int32_t> map, ccol;                        // matrix
    dge_tmp<int64_t> crow, cw, P, rowb;
    int64_t n = 0;
    std::vector<int64_t> at, val;                      // per slice boundary: .od — first edge and its offset; matrix — first kept edge and P there
    FtZeros zeros;                                     // matrix over a table without edges
};

int ft_prepare(FtCall& C, const dge_flows* f, const FtEdges& X, int32_t kind, int32_t k0, int32_t k1, const uint8_t* select, FtTexts& Tx) {
    Tx.kind = kind; Tx.k0 = k0; Tx.k1 = k1;
    const dge_regions* rg = f->regions;
    const int64_t E = X.E;
    if (kind == DGE_FLOW_TEXT_MATRIX) {
        const std::vector<int64_t> order = ft_by_rank(rg);
        std::vector<int32_t> map((size_t)std::max<int64_t>(rg->R, 1), -1);
        int64_t n = 0;
        for (int64_t r = 0; r < rg->R; r++) if (!select || select[(size_t)order[(size_t)r]]) map[(size_t)r] = (int32_t)n++;
        Tx.n = n;
        if (n == 0 || E == 0) return DGE_OK;
        const int64_t slices = k1 - k0, rows = slices * n;
        std::vector<int64_t> first((size_t)X.S + 1);
        SEQ_TRY(seq_read_back(C.R, first.data(), X.first.p, first.size() * 8));
        const int64_t e0 = first[(size_t)k0], m = first[(size_t)k1] - e0;
        dge_tmp<int64_t> pos;
        int64_t M = 0;
        SEQ_TRY(seq_alloc(C.R, Tx.map, (int64_t)map.size(), "the regions' numbers"));
        SEQ_TRY(seq_alloc(C.R, pos, m + 1, "the kept edges' places"));
        DGE_HIP(hipMemcpyAsync(Tx.map.p, map.data(), map.size() * 4, hipMemcpyHostToDevice, C.R.stream));
        DGE_HIP(hipStreamSynchronize(C.R.stream));
        SEQ_TRY(seq_kernels_begin(C.R));
        SEQ_TRY(seq_scan(C.R, rocprim::make_transform_iterator(rocprim::counting_iterator<int64_t>(0), FtKeep{X.key.p, Tx.map.p, X.Ru, e0, m}), pos.p, m + 1));
        SEQ_TRY(seq_kernels_end(C.R));
        SEQ_TRY(seq_read_back(C.R, &M, pos.p + m, 8));
        SEQ_TRY(seq_alloc(C.R, Tx.crow, M, "the kept edges' rows"));
        SEQ_TRY(seq_alloc(C.R, Tx.ccol, M, "the kept edges' columns"));
        SEQ_TRY(seq_alloc(C.R, Tx.cw, M, "the kept edges' weights"));
        SEQ_TRY(seq_alloc(C.R, Tx.P, M + 1, "the kept edges' extra digits"));
        SEQ_TRY(seq_alloc(C.R, Tx.rowb, rows + 1, "the rows' first edges"));
        SEQ_TRY(seq_kernels_begin(C.R));
        if (m) hipLaunchKernelGGL(k_ft_mat_compact, dim3(seq_grid(m)), dim3(FT_BLOCK), 0, C.R.stream, X.key.p, X.w.p, e0, m, X.Ru, Tx.map.p, pos.p, (int64_t)k0, n, Tx.crow.p, Tx.ccol.p, Tx.cw.p);
        SEQ_TRY(seq_scan(C.R, rocprim::make_transform_iterator(rocprim::counting_iterator<int64_t>(0), FtExtra{Tx.cw.p, M}), Tx.P.p, M + 1));
        hipLaunchKernelGGL(k_ft_rowb, dim3(seq_grid(rows + 1)), dim3(FT_BLOCK), 0, C.R.stream, Tx.crow.p, M, rows, Tx.rowb.p);
        DGE_HIP(hipGetLastError());
        SEQ_TRY(seq_kernels_end(C.R));
        return ft_gather(C, Tx.P.p, Tx.rowb.p, n, slices + 1, Tx.val, Tx.at);
    }
    if (E == 0) return DGE_OK;
    dge_tmp<int64_t> len;
    SEQ_TRY(seq_alloc(C.R, len, E + 1, "the lines' lengths"));
    SEQ_TRY(seq_alloc(C.R, Tx.off, E + 1, "the lines' offsets"));
    SEQ_TRY(seq_kernels_begin(C.R));
    hipLaunchKernelGGL(k_ft_od_len, dim3(seq_grid(E + 1)), dim3(FT_BLOCK), 0, C.R.stream, X.key.p, X.w.p, E, X.Ru, rg->d_id_by_rank, kind == DGE_FLOW_TEXT_OD_LAYERED ? X.S : 0, len.p);
    DGE_HIP(hipGetLastError());
    SEQ_TRY(seq_scan(C.R, len.p, Tx.off.p, E + 1));
    SEQ_TRY(seq_kernels_end(C.R));
    return ft_gather(C, Tx.off.p, X.first.p, 1, (int64_t)X.S + 1, Tx.val, Tx.at);
}

// slice k of the prepared texts (k0 <= k < k1; the layered text: k = 0 stands for all): its job and its size; the counts go into the report
int64_t ft_job(FtCall& C, const dge_flows* f, const FtEdges& X, const FtTexts& Tx, int32_t k, int32_t sep, FtJob& J) {
    J = FtJob{};
    J.kind = Tx.kind; J.S = X.S; J.sep = (uint32_t)sep; J.R = X.Ru;
    if (Tx.kind == DGE_FLOW_TEXT_MATRIX) {
        const int64_t n = Tx.n;
        C.I.lines += n;
        if (n == 0) return 0;
        if (X.E == 0) {                                  // no edge at all: still n lines of zeros, through the same arithmetic on arrays of nothing
            C.I.zeros += n * n;
            return -1;
        }
        const size_t i = (size_t)(k - Tx.k0);
        const int64_t M = Tx.at[i + 1] - Tx.at[i];
        C.I.edges += M; C.I.zeros += n * n - M;
        J.ccol = Tx.ccol.p; J.cw = Tx.cw.p; J.P = Tx.P.p; J.rowb = Tx.rowb.p + (int64_t)i * n; J.n = n; J.pbase = Tx.val[i];
        return 2 * n * n + (Tx.val[i + 1] - Tx.val[i]);
    }
    if (X.E == 0) return 0;
    const size_t a = Tx.kind == DGE_FLOW_TEXT_OD_LAYERED ? 0 : (size_t)k, b = Tx.kind == DGE_FLOW_TEXT_OD_LAYERED ? (size_t)X.S : (size_t)k + 1;
    J.off = Tx.off.p; J.e0 = Tx.at[a]; J.e1 = Tx.at[b]; J.base = Tx.val[a];
    J.key = X.key.p; J.w = X.w.p; J.id_by_rank = f->regions->d_id_by_rank;
    C.I.lines += J.e1 - J.e0; C.I.edges += J.e1 - J.e0;
    return Tx.val[b] - Tx.val[a];
}

// ---- the time series
struct FtSeries {
    std::vector<int64_t> regions, ids;                 // the selected regions' indices and ids, ascending by id
    dge_tmp<int64_t> d_in, d_out, d_ids;
    int64_t n = 0;
};

// the selection by itself: host work on the regions' ids.  negated: the text spells -id
int ft_series_select(const dge_flows* f, const uint8_t* select, const char* who, bool negated, FtSeries& Z) {
    const dge_regions* rg = f->regions;
    for (int64_t r : ft_by_rank(rg)) {
        if (select && !select[(size_t)r]) continue;
        const int64_t id = rg->ids[(size_t)r];
        if (negated && id == INT64_MIN) DGE_FAIL(DGE_ERR_RANGE, "%s: region %lld has the id -2^63, which cannot be negated for its second line", who, (long long)r);
        Z.regions.push_back(r); Z.ids.push_back(id);
    }
    Z.n = (int64_t)Z.ids.size();
    return DGE_OK;
}

int ft_series(FtCall& C, const dge_flows* f, FtSeries& Z) {
    const dge_regions* rg = f->regions;
    const int64_t n = Z.n, N = f->n;
    const uint64_t Ru = (uint64_t)std::max<int64_t>(rg->R, 1);
    SEQ_TRY(seq_alloc(C.R, Z.d_in, n * 24, "the sums into the regions"));
    SEQ_TRY(seq_alloc(C.R, Z.d_out, n * 24, "the sums out of the regions"));
    SEQ_TRY(seq_alloc(C.R, Z.d_ids, n, "the regions' ids"));
    if (n == 0) return DGE_OK;
    DGE_HIP(hipMemsetAsync(Z.d_in.p, 0, (size_t)n * 24 * 8, C.R.stream));
    DGE_HIP(hipMemsetAsync(Z.d_out.p, 0, (size_t)n * 24 * 8, C.R.stream));
    DGE_HIP(hipMemcpyAsync(Z.d_ids.p, Z.ids.data(), (size_t)n * 8, hipMemcpyHostToDevice, C.R.stream));
    DGE_HIP(hipStreamSynchronize(C.R.stream));
    if (N == 0) return DGE_OK;
    std::vector<int32_t> map((size_t)Ru, -1);
    for (int64_t c = 0; c < n; c++) map[(size_t)Z.regions[(size_t)c]] = (int32_t)c;
    dge_tmp<int32_t> d_map;
    dge_tmp<uint64_t> ukey;
    dge_tmp<int64_t> usum, count;
    SEQ_TRY(seq_alloc(C.R, d_map, (int64_t)map.size(), "the regions' numbers"));
    SEQ_TRY(seq_alloc(C.R, ukey, N, "the (hour, source) keys"));
    SEQ_TRY(seq_alloc(C.R, usum, N, "the (hour, source) sums"));
    SEQ_TRY(seq_alloc(C.R, count, 1, "the number of keys"));
    DGE_HIP(hipMemcpyAsync(d_map.p, map.data(), map.size() * 4, hipMemcpyHostToDevice, C.R.stream));
    DGE_HIP(hipStreamSynchronize(C.R.stream));
    SeqScratch tmp{C.R, "the reduction's scratch", true};
    auto keys = rocprim::make_transform_iterator(rocprim::counting_iterator<int64_t>(0), FtHourSrc{f->d_key, Ru});
    SEQ_TRY(dge_two_pass(tmp, [&](void* t, size_t& bytes) {
        return rocprim::reduce_by_key(t, bytes, keys, f->d_cnt, (size_t)N, ukey.p, usum.p, count.p, rocprim::plus<int64_t>(), rocprim::equal_to<uint64_t>(), C.R.stream);
    }, C.R.stream, false));
    hipLaunchKernelGGL(k_ft_series_in, dim3(seq_grid(N)), dim3(FT_BLOCK), 0, C.R.stream, f->d_key, f->d_cnt, N, Ru, d_map.p, Z.d_in.p);
    SEQ_TRY(seq_kernels_end(C.R));
    int64_t U = 0;
    SEQ_TRY(seq_read_back(C.R, &U, count.p, 8));
    SEQ_TRY(seq_kernels_begin(C.R));
    if (U) hipLaunchKernelGGL(k_ft_series_out, dim3(seq_grid(U)), dim3(FT_BLOCK), 0, C.R.stream, ukey.p, usum.p, U, Ru, d_map.p, Z.d_out.p);
    DGE_HIP(hipGetLastError());
    return seq_kernels_end(C.R);
}

int ft_series_text(const char* who, const dge_flows* f, const uint8_t* select, TextSink& sink, int64_t* n_bytes, dge_flow_text_info* info) {
    FtSeries Z;
    SEQ_TRY(ft_series_select(f, select, who, true, Z));
    dge_tmp<int64_t> len, off;
    FtCall C(who);
    SEQ_TRY(C.open(f->regions->device));
    SEQ_TRY(ft_series(C, f, Z));
    const int64_t lines = 2 * Z.n;
    int64_t total = 0;
    FtJob J = {};
    if (lines > 0) {
        SEQ_TRY(seq_alloc(C.R, len, lines + 1, "the lines' lengths"));
        SEQ_TRY(seq_alloc(C.R, off, lines + 1, "the lines' offsets"));
        SEQ_TRY(seq_kernels_begin(C.R));
        hipLaunchKernelGGL(k_ft_series_len, dim3(seq_grid(lines + 1)), dim3(FT_BLOCK), 0, C.R.stream, Z.d_ids.p, Z.d_in.p, Z.d_out.p, Z.n, len.p);
        DGE_HIP(hipGetLastError());
        SEQ_TRY(seq_scan(C.R, len.p, off.p, lines + 1));
        SEQ_TRY(seq_kernels_end(C.R));
        SEQ_TRY(seq_read_back(C.R, &total, off.p + lines, 8));
        J.kind = FT_SERIES; J.off = off.p; J.e0 = 0; J.e1 = lines; J.base = 0; J.ids = Z.d_ids.p; J.in = Z.d_in.p; J.out = Z.d_out.p;
    }
    C.I.lines = lines; C.I.edges = 24 * lines;
    SEQ_TRY(ft_deliver(C, J, total, sink, n_bytes));
    C.report(info);
    return DGE_OK;
}

// one slice's text to its sink
int ft_slice(FtCall& C, const dge_flows* f, const FtEdges& X, FtTexts& Tx, int32_t k, int32_t sep, TextSink& sink, int64_t* n_bytes) {
    FtJob J;
    int64_t total = ft_job(C, f, X, Tx, k, sep, J);
    if (total < 0) { SEQ_TRY(Tx.zeros.make(C, Tx.n, J)); total = 2 * Tx.n * Tx.n; }
    return ft_deliver(C, J, total, sink, n_bytes);
}

}  // namespace

// ------------------------------------------------------------------------------------------ entries
extern "C" int dge_flows_to_text(const dge_flows* f, const dge_flow_slices* s, int32_t kind, int32_t slice, const uint8_t* select, int32_t sep, char* text, int64_t cap, int64_t* n_bytes,
                                 dge_flow_text_info* info) {
    const char* who = "dge_flows_to_text";
    int32_t S = 0;
    SEQ_TRY(ft_check(who, f, s, kind, slice, select, sep, !n_bytes || cap < 0 || (cap > 0 && !text) || slice < 0, &S));
    FtEdges X;                                          // (the arrays outlive the call: its streams drain before they go)
    FtTexts Tx;
    FtCall C(who);
    SEQ_TRY(C.open(f->regions->device));
    SEQ_TRY(ft_edges(C, f, s, S, X));
    SEQ_TRY(ft_prepare(C, f, X, kind, kind == DGE_FLOW_TEXT_MATRIX ? slice : 0, kind == DGE_FLOW_TEXT_MATRIX ? slice + 1 : S, select, Tx));
    TextSink sink{who};
    sink.text = text; sink.cap = cap;
    SEQ_TRY(ft_slice(C, f, X, Tx, slice, sep, sink, n_bytes));
    C.report(info);
    return DGE_OK;
}

extern "C" int dge_flows_write_text(const dge_flows* f, const dge_flow_slices* s, int32_t kind, const uint8_t* select, int32_t sep, const char* const* paths, int32_t n_paths,
                                    dge_flow_text_info* info) {
    const char* who = "dge_flows_write_text";
    int32_t S = 0;
    bool bad = !paths || n_paths < 0;
    for (int32_t i = 0; !bad && i < n_paths; i++) bad = !paths[i];
    SEQ_TRY(ft_check(who, f, s, kind, -1, select, sep, bad, &S));
    const int32_t texts = kind == DGE_FLOW_TEXT_OD_LAYERED ? 1 : S;
    if (n_paths != texts) DGE_FAIL(DGE_ERR_ARG, "%s: n_paths = %d, the slices give %d text%s", who, n_paths, texts, texts == 1 ? "" : "s");
    FtEdges X;                                          // (the arrays outlive the call: its streams drain before they go)
    FtTexts Tx;
    FtCall C(who);
    SEQ_TRY(C.open(f->regions->device));
    SEQ_TRY(ft_edges(C, f, s, S, X));
    SEQ_TRY(ft_prepare(C, f, X, kind, 0, S, select, Tx));
    // nothing has been written, created or truncated up to here
    for (int32_t k = 0; k < texts; k++) {
        TextSink sink{who};
        sink.path = paths[k];
        SEQ_TRY(ft_slice(C, f, X, Tx, k, sep, sink, nullptr));
    }
    C.report(info);
    return DGE_OK;
}

extern "C" int dge_flows_time_series(const dge_flows* f, const uint8_t* select, int64_t* in_flow, int64_t* out_flow, int64_t* region_index, int64_t cap, int64_t* n) {
    const char* who = "dge_flows_time_series";
    if (!f || !n || cap < 0 || (cap > 0 && (!in_flow || !out_flow || !region_index))) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    FtSeries Z;
    SEQ_TRY(ft_series_select(f, select, who, false, Z));
    *n = Z.n;
    if (cap < Z.n) DGE_FAIL(DGE_ERR_CAP, "%s: %lld selected regions exceed cap %lld", who, (long long)Z.n, (long long)cap);
    if (Z.n == 0) return DGE_OK;
    FtCall C(who);
    SEQ_TRY(C.open(f->regions->device));
    SEQ_TRY(ft_series(C, f, Z));
    SEQ_TRY(seq_read_back(C.R, in_flow, Z.d_in.p, (size_t)Z.n * 24 * 8));
    SEQ_TRY(seq_read_back(C.R, out_flow, Z.d_out.p, (size_t)Z.n * 24 * 8));
    memcpy(region_index, Z.regions.data(), (size_t)Z.n * 8);
    return DGE_OK;
}

extern "C" int dge_flows_time_series_text(const dge_flows* f, const uint8_t* select, char* text, int64_t cap, int64_t* n_bytes, dge_flow_text_info* info) {
    const char* who = "dge_flows_time_series_text";
    if (!f || !n_bytes || cap < 0 || (cap > 0 && !text)) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    TextSink sink{who};
    sink.text = text; sink.cap = cap;
    return ft_series_text(who, f, select, sink, n_bytes, info);
}

extern "C" int dge_flows_write_time_series(const dge_flows* f, const uint8_t* select, const char* path, dge_flow_text_info* info) {
    const char* who = "dge_flows_write_time_series";
    if (!f || !path) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    TextSink sink{who};
    sink.path = path;
    return ft_series_text(who, f, select, sink, nullptr, info);
}
