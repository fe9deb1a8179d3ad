// trip_text.hip — taxi trip text in, records or flows out (include/dge.h: dge_trips_parse_texts, dge_flows_add_trip_texts / _files).
//
// The front of the pipeline: the reference reads every trip line in TaxiTrip(String line) and ShortDate (J/TaxiTrip.java:39-78,199-223), driven by
// J/TaxiTrip.java:123-143 and J/TaxiTripIterator.java:32-62.  Here the text streams through the device in slabs, every line is parsed in a lane by trip_parse.h
// (integer arithmetic only), and the status-0 records of a slab go straight to dge_flows_add_trips_device.  Outside the build stamp: nothing here is read or
// written by a training launch.
//
// Transport (this reader's own; seq_tokens.h's loads a whole text, and the trip files are the one text of the pipeline that must not be resident).  The host
// (TripFeeder of seq_pieces.h, plain C++ that tests/test_seq_pieces_host.py runs without a device) cuts each piece into SLABS of whole lines: it fills a
// pinned buffer with the tail the last slab left and fresh bytes up to slab_bytes, looks backwards for the last terminator, sends everything up to it and keeps the rest as the next tail.  That search touches the end of the buffer only; no per-line work is done on
// the host.  What the cut guarantees the kernels:
//   - a slab holds whole lines of ONE piece; only a piece's last slab may end without a terminator;
//   - a "\r" that ends a slab is a whole terminator: when the piece goes on with "\n" that byte is dropped on the way in (it is half of the "\r\n" already
//     sent), so it can never count as a line of its own;
//   - slab_bytes >= 131072 bytes without a terminator are a line beyond TRIP_MAX_LINE: its first 65 536 bytes go out as a line of their own (status 3 whatever
//     they hold) and the rest up to the next terminator is skipped and counted, not carried.  So the tail is bounded by slab_bytes and device memory by the slab.
// Two pinned buffers alternate: slab k+1 is filled while slab k is in its kernels.
//
// Kernels of a slab, on its bytes in one device buffer (zeros behind them up to whole chunks and 32 bytes more):
//   k_trip_count / k_trip_emit   a lane takes 32 bytes as two 16-byte loads; bit i = "a line ends at byte i": "\n", or "\r" not followed by "\n".  Per-chunk
//                                counts, a rocPRIM scan and the second pass give line l the offset of its terminator; line l starts behind terminator l-1.
//   k_trip_parse                 a workgroup takes 256 consecutive lines, copies their contiguous bytes into LDS with 16-byte loads (a tile of TRIP_TILE bytes;
//                                a range that does not fit is read from global memory by the same code) and every lane parses its own line out of it.
//   host path                    lines with a coordinate od_parse_f64 hands back come back by index (seq_pick, k_trip_host_list); the host parses them again out of the pinned slab with the
//                                same trip_parse.h, finishes the coordinates with strtod, and k_trip_patch writes the records in place — before anything reads them.
//   k_trip_compact around a scan the status-0 records in text order, for dge_flows_add_trips_device.
// Offsets inside a slab are 32-bit; line numbers and byte totals are 64-bit.  Counters are integers added with atomicAdd after a block reduction.
// Coherence: no protocol.  Every array is written by one kernel and read by later ones on the same stream.
//
// The shape (slab transport, LDS tile, one lane per line) is the one the design proposed; none of it has been measured against an alternative.
#include <algorithm>

#include "seq_tokens.h"
#include "trip_parse.h"

constexpr int64_t TRIP_SLAB_DEFAULT = (int64_t)16 << 20, TRIP_SLAB_MIN = 131072, TRIP_SLAB_MAX = (int64_t)1 << 30;
constexpr int TRIP_TILE = 60 * 1024;             // bytes of LDS a workgroup's 256 lines may take (of the CU's 160 KiB: two workgroups a CU)
enum { TT_OK = 0, TT_BAD_FIELDS, TT_BAD_PARSE, TT_TOO_LONG, TT_HOST_LINES, TT_N };

// ------------------------------------------------------------------------------------------ kernels
// 32 bytes of one lane: bit i = a line ends at base + i.  The byte behind the 32 decides for a "\r" in the last place (the buffer goes on for 32 zero bytes).
__device__ __forceinline__ uint32_t trip_end_mask(const uint8_t* buf, int64_t base) {
    const uint4 a = *reinterpret_cast<const uint4*>(buf + base), b = *reinterpret_cast<const uint4*>(buf + base + 16);
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const uint32_t after = buf[base + 32];
    uint32_t nl = 0, cr = 0;
#pragma unroll
    for (int i = 0; i < 32; i++) {
        const uint32_t c = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
        nl |= (uint32_t)(c == 10u) << i;
        cr |= (uint32_t)(c == 13u) << i;
    }
    const uint32_t nl_next = (nl >> 1) | ((uint32_t)(after == 10u) << 31);
    return nl | (cr & ~nl_next);
}

__global__ void __launch_bounds__(SEQ_BLOCK) k_trip_count(const uint8_t* buf, int64_t* chunk_ends) {
    typedef hipcub::BlockReduce<int, SEQ_BLOCK> Reduce;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t base = (int64_t)blockIdx.x * SEQ_CHUNK + (int64_t)threadIdx.x * 32;
    const int sum = Reduce(tmp).Sum(__popc(trip_end_mask(buf, base)));
    if (threadIdx.x == 0) chunk_ends[blockIdx.x] = sum;
}

// line_end[l] = offset of the byte that ends line l (of "\r\n" the "\n"); a last line without a terminator ends at n, written by the first lane
__global__ void __launch_bounds__(SEQ_BLOCK) k_trip_emit(const uint8_t* buf, const int64_t* chunk_endx, int32_t n, int64_t L, int open_end, int32_t* line_end) {
    typedef hipcub::BlockScan<int, SEQ_BLOCK> Scan;
    __shared__ typename Scan::TempStorage tmp;
    const int64_t base = (int64_t)blockIdx.x * SEQ_CHUNK + (int64_t)threadIdx.x * 32;
    uint32_t ends = trip_end_mask(buf, base);
    int before;
    Scan(tmp).ExclusiveSum(__popc(ends), before);
    int64_t l = chunk_endx[blockIdx.x] + before;
    while (ends) {
        const int i = __ffs(ends) - 1;
        ends &= ends - 1;
        line_end[l++] = (int32_t)(base + i);
    }
    if (open_end && blockIdx.x == 0 && threadIdx.x == 0) line_end[L - 1] = n;
}

// record i = line skip + i of the slab (skip = 1: the slab opens a piece and its first line is the header)
__global__ void __launch_bounds__(SEQ_BLOCK) k_trip_parse(const uint8_t* buf, int32_t n, const int32_t* line_end, int64_t L, int32_t skip, int32_t format, uint8_t* status,
                                                          int32_t* hour, double* sxy, double* exy, uint8_t* host_mask, int32_t* line_at, int32_t* line_len,
                                                          unsigned long long* counters) {
    typedef hipcub::BlockReduce<unsigned long long, SEQ_BLOCK> Reduce;
    __shared__ typename Reduce::TempStorage tmp;
    __shared__ __attribute__((aligned(16))) uint8_t tile[TRIP_TILE];
    const int64_t l0 = (int64_t)skip + (int64_t)blockIdx.x * SEQ_BLOCK, l1 = l0 + SEQ_BLOCK <= L ? l0 + SEQ_BLOCK : L;      // l0 < L: the grid covers L - skip records
    const int32_t lo = l0 == 0 ? 0 : line_end[l0 - 1] + 1, hi = line_end[l1 - 1];                                        // hi <= n; byte hi is the last terminator, or a zero
    const int32_t abase = lo & ~15, bytes = hi + 1 - abase;
    const bool staged = bytes <= TRIP_TILE;
    if (staged) {
        const uint4* src = reinterpret_cast<const uint4*>(buf + abase);
        uint4* dst = reinterpret_cast<uint4*>(tile);
        for (int32_t q = threadIdx.x; q * 16 < bytes; q += SEQ_BLOCK) dst[q] = src[q];      // at most 15 bytes past byte hi: inside the zeros behind the slab
    }
    __syncthreads();
    const int64_t l = l0 + threadIdx.x;
    unsigned long long v[TT_N] = {0, 0, 0, 0, 0};
    if (l < l1) {
        const int32_t start = l == 0 ? 0 : line_end[l - 1] + 1, end = line_end[l];
        const uint8_t* p = staged ? tile + (start - abase) : buf + start;
        int32_t len = end - start;
        if (len > 0 && end < n && p[len] == '\n' && p[len - 1] == '\r') len--;
        trip_rec r;
        trip_parse_line(p, len, format, &r);
        const int64_t i = l - skip;
        status[i] = (uint8_t)r.status; hour[i] = r.hour; host_mask[i] = (uint8_t)r.host_mask; line_at[i] = start; line_len[i] = len;
        unsigned long long* s = reinterpret_cast<unsigned long long*>(sxy) + 2 * i;
        unsigned long long* e = reinterpret_cast<unsigned long long*>(exy) + 2 * i;
        s[0] = r.xy[0]; s[1] = r.xy[1]; e[0] = r.xy[2]; e[1] = r.xy[3];
        if (r.host_mask) v[TT_HOST_LINES] = 1; else v[r.status] = 1;
    }
    for (int k = 0; k < TT_N; k++) {
        const unsigned long long sum = Reduce(tmp).Sum(v[k]);
        if (threadIdx.x == 0 && sum) atomicAdd(counters + k, sum);
        __syncthreads();
    }
}

struct TripOkFlag { const uint8_t* status; int64_t n; __device__ int64_t operator()(int64_t i) const { return i < n && status[i] == 0 ? 1 : 0; } };

// host line k = record picked[k]: (record, offset, length)
__global__ void __launch_bounds__(SEQ_BLOCK) k_trip_host_list(const int64_t* picked, const int32_t* line_at, const int32_t* line_len, int64_t n, int64_t* list) {
    const int64_t k = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (k >= n) return;
    const int64_t i = picked[k];
    list[3 * k] = i; list[3 * k + 1] = line_at[i]; list[3 * k + 2] = line_len[i];
}

__global__ void __launch_bounds__(SEQ_BLOCK) k_trip_patch(const int64_t* list, const int32_t* p_status_hour, const uint64_t* p_xy, int64_t n, uint8_t* status, int32_t* hour,
                                                          double* sxy, double* exy) {
    const int64_t k = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (k >= n) return;
    const int64_t i = list[3 * k];
    status[i] = (uint8_t)p_status_hour[2 * k]; hour[i] = p_status_hour[2 * k + 1];
    unsigned long long* s = reinterpret_cast<unsigned long long*>(sxy) + 2 * i;
    unsigned long long* e = reinterpret_cast<unsigned long long*>(exy) + 2 * i;
    s[0] = p_xy[4 * k]; s[1] = p_xy[4 * k + 1]; e[0] = p_xy[4 * k + 2]; e[1] = p_xy[4 * k + 3];
}

__global__ void __launch_bounds__(SEQ_BLOCK) k_trip_compact(const int64_t* okx, const int32_t* hour, const double* sxy, const double* exy, int64_t n, int32_t* c_hour, double* c_sxy,
                                                            double* c_exy) {
    const int64_t i = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (i >= n || okx[i + 1] == okx[i]) return;
    const int64_t k = okx[i];
    c_hour[k] = hour[i];
    c_sxy[2 * k] = sxy[2 * i]; c_sxy[2 * k + 1] = sxy[2 * i + 1];
    c_exy[2 * k] = exy[2 * i]; c_exy[2 * k + 1] = exy[2 * i + 1];
}

// ------------------------------------------------------------------------------------------ host side
namespace {

struct TripSink {                     // where the records go: the caller's arrays (dge_trips_parse_texts) or a flow table
    uint8_t* status = nullptr; int32_t* hour = nullptr; double* sxy = nullptr; double* exy = nullptr;
    int64_t cap = 0;
    dge_flows* flows = nullptr;
    int64_t records = 0;
};

struct TripSlab { int b = 0; int64_t n = 0, L = 0, m = 0; bool live = false; };      // pinned buffer, bytes, lines, records

struct TripReader {
    SeqRun R;
    int32_t format = 0, header = 0;
    int64_t S = 0, cap_lines = 0;
    dge_tmp<uint8_t> buf, status, host_mask;
    dge_tmp<int64_t> chunk_ends, chunk_endx;
    dge_tmp<int32_t> line_end, hour, line_at, line_len;
    dge_tmp<double> sxy, exy;
    dge_tmp<unsigned long long> counters;
    hipEvent_t ea = nullptr, eb = nullptr;
    SeqCLocale locale;
    dge_trip_text_info info = {};
    ~TripReader() {
        if (ea) (void)hipEventDestroy(ea);
        if (eb) (void)hipEventDestroy(eb);
    }

    int open(const char* who) {
        SEQ_TRY(locale.open(who));
        SEQ_TRY(seq_open(R, R.device, who));
        DGE_HIP(hipEventCreate(&ea));
        DGE_HIP(hipEventCreate(&eb));
        int64_t total = 0, largest = 0;
        for (const SeqPiece& p : R.pieces) { total += p.size; largest = std::max(largest, p.size); }
        info.bytes = total;
        S = std::min(S, std::max(TRIP_SLAB_MIN, largest));          // no buffer beyond the largest piece
        for (int i = 0; i < 2; i++) {
            const hipError_t e = hipHostMalloc((void**)&R.pin[i], (size_t)S, hipHostMallocDefault);
            if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); R.pin[i] = nullptr; DGE_FAIL(DGE_ERR_CAP, "%s: two pinned buffers of %lld bytes do not fit", who, (long long)S); }
            DGE_HIP(e);
        }
        SEQ_TRY(seq_alloc(R, buf, (S + SEQ_CHUNK - 1) / SEQ_CHUNK * SEQ_CHUNK + SEQ_CHUNK, "the slab"));
        SEQ_TRY(seq_alloc(R, chunk_ends, S / SEQ_CHUNK + 2, "the chunk counts"));
        SEQ_TRY(seq_alloc(R, chunk_endx, S / SEQ_CHUNK + 2, "the chunk counts"));
        SEQ_TRY(seq_alloc(R, counters, TT_N, "the counters"));
        DGE_HIP(hipMemsetAsync(counters.p, 0, TT_N * 8, R.stream));
        return DGE_OK;
    }

    int reserve(int64_t lines) {
        if (lines <= cap_lines) return DGE_OK;
        const int64_t c = std::max(lines, cap_lines * 2);
        SEQ_TRY(seq_alloc(R, line_end, c, "the lines' ends"));
        SEQ_TRY(seq_alloc(R, status, c, "the records' states"));
        SEQ_TRY(seq_alloc(R, host_mask, c, "the records' host flags"));
        SEQ_TRY(seq_alloc(R, hour, c, "the records' hours"));
        SEQ_TRY(seq_alloc(R, line_at, c, "the lines' offsets"));
        SEQ_TRY(seq_alloc(R, line_len, c, "the lines' lengths"));
        SEQ_TRY(seq_alloc(R, sxy, 2 * c, "the start points"));
        SEQ_TRY(seq_alloc(R, exy, 2 * c, "the end points"));
        cap_lines = c;
        return DGE_OK;
    }

    // bytes to the device, lines found, the parse kernel launched; returns without waiting for it
    int submit(TripSlab& s, bool first, bool open_end) {
        const int64_t n = s.n, n_chunks = (n + SEQ_CHUNK - 1) / SEQ_CHUNK;
        DGE_HIP(hipMemcpyAsync(buf.p, R.pin[s.b], (size_t)n, hipMemcpyHostToDevice, R.stream));
        DGE_HIP(hipMemsetAsync(buf.p + n, 0, (size_t)(n_chunks * SEQ_CHUNK + 32 - n), R.stream));
        DGE_HIP(hipEventRecord(ea, R.stream));
        DGE_HIP(hipMemsetAsync(chunk_ends.p + n_chunks, 0, 8, R.stream));
        hipLaunchKernelGGL(k_trip_count, dim3((unsigned)n_chunks), dim3(SEQ_BLOCK), 0, R.stream, buf.p, chunk_ends.p);
        SEQ_TRY(seq_scan(R, chunk_ends.p, chunk_endx.p, n_chunks + 1));
        int64_t ends = 0;
        SEQ_TRY(seq_read_back(R, &ends, chunk_endx.p + n_chunks, 8));
        s.L = ends + (open_end ? 1 : 0);
        const int32_t skip = header && first ? 1 : 0;              // (a slab holds a line at least: L >= 1)
        s.m = s.L - skip;
        info.lines += s.L; info.header_lines += skip; info.slabs++;
        SEQ_TRY(reserve(s.L));
        hipLaunchKernelGGL(k_trip_emit, dim3((unsigned)n_chunks), dim3(SEQ_BLOCK), 0, R.stream, buf.p, chunk_endx.p, (int32_t)n, s.L, open_end ? 1 : 0, line_end.p);
        if (s.m > 0)
            hipLaunchKernelGGL(k_trip_parse, dim3(seq_grid(s.m)), dim3(SEQ_BLOCK), 0, R.stream, buf.p, (int32_t)n, line_end.p, s.L, skip, format, status.p, hour.p, sxy.p, exy.p,
                               host_mask.p, line_at.p, line_len.p, counters.p);
        DGE_HIP(hipEventRecord(eb, R.stream));
        DGE_HIP(hipGetLastError());
        s.live = true;
        return DGE_OK;
    }

    // waits for the slab's kernels, finishes what they left to the host, hands the records on
    int finish(TripSlab& s, TripSink& sink) {
        if (!s.live) return DGE_OK;
        s.live = false;
        DGE_HIP(hipEventSynchronize(eb));
        float ms = 0.f;
        DGE_HIP(hipEventElapsedTime(&ms, ea, eb));
        R.kernel_ms += ms;
        const int64_t m = s.m;
        if (m == 0) return DGE_OK;
        unsigned long long c[TT_N];
        SEQ_TRY(seq_read_back(R, c, counters.p, sizeof(c)));
        DGE_HIP(hipMemsetAsync(counters.p, 0, TT_N * 8, R.stream));
        info.ok += (int64_t)c[TT_OK]; info.bad_fields += (int64_t)c[TT_BAD_FIELDS]; info.bad_parse += (int64_t)c[TT_BAD_PARSE]; info.too_long += (int64_t)c[TT_TOO_LONG];
        const int64_t n_host = (int64_t)c[TT_HOST_LINES];
        if (n_host > 0) {
            dge_tmp<int64_t> picked, list;
            dge_tmp<int32_t> p_sh;
            dge_tmp<uint64_t> p_xy;
            SEQ_TRY(seq_alloc(R, list, 3 * n_host, "the host lines"));
            SEQ_TRY(seq_alloc(R, p_sh, 2 * n_host, "the host lines' records"));
            SEQ_TRY(seq_alloc(R, p_xy, 4 * n_host, "the host lines' points"));
            SEQ_TRY(seq_kernels_begin(R));
            SEQ_TRY(seq_pick(R, host_mask.p, m, n_host, picked, "the host lines"));
            hipLaunchKernelGGL(k_trip_host_list, dim3(seq_grid(n_host)), dim3(SEQ_BLOCK), 0, R.stream, picked.p, line_at.p, line_len.p, n_host, list.p);
            SEQ_TRY(seq_kernels_end(R));
            std::vector<int64_t> l((size_t)n_host * 3);
            std::vector<int32_t> sh((size_t)n_host * 2);
            std::vector<uint64_t> xy((size_t)n_host * 4);
            SEQ_TRY(seq_read_back(R, l.data(), list.p, l.size() * 8));
            for (int64_t k = 0; k < n_host; k++) {
                const uint8_t* line = R.pin[s.b] + l[(size_t)k * 3 + 1];
                trip_rec r;
                trip_parse_line(line, l[(size_t)k * 3 + 2], format, &r);
                info.host_values += trip_finish_host(line, &r, locale.c);
                sh[(size_t)k * 2] = r.status; sh[(size_t)k * 2 + 1] = r.hour;
                memcpy(&xy[(size_t)k * 4], r.xy, 32);
                if (r.status == TRIP_OK) info.ok++; else info.bad_parse++;
            }
            DGE_HIP(hipMemcpyAsync(p_sh.p, sh.data(), sh.size() * 4, hipMemcpyHostToDevice, R.stream));
            DGE_HIP(hipMemcpyAsync(p_xy.p, xy.data(), xy.size() * 8, hipMemcpyHostToDevice, R.stream));
            SEQ_TRY(seq_kernels_begin(R));
            hipLaunchKernelGGL(k_trip_patch, dim3(seq_grid(n_host)), dim3(SEQ_BLOCK), 0, R.stream, list.p, p_sh.p, p_xy.p, n_host, status.p, hour.p, sxy.p, exy.p);
            SEQ_TRY(seq_kernels_end(R));
        }
        if (sink.flows) {
            dge_tmp<int64_t> okx;
            dge_tmp<int32_t> c_hour;
            dge_tmp<double> c_sxy, c_exy;
            int64_t K = 0;
            SEQ_TRY(seq_alloc(R, okx, m + 1, "the kept records' numbers"));
            SEQ_TRY(seq_kernels_begin(R));
            SEQ_TRY(seq_scan(R, rocprim::make_transform_iterator(rocprim::counting_iterator<int64_t>(0), TripOkFlag{status.p, m}), okx.p, m + 1));
            SEQ_TRY(seq_kernels_end(R));
            SEQ_TRY(seq_read_back(R, &K, okx.p + m, 8));
            if (K > 0) {
                SEQ_TRY(seq_alloc(R, c_hour, K, "the kept hours"));
                SEQ_TRY(seq_alloc(R, c_sxy, 2 * K, "the kept start points"));
                SEQ_TRY(seq_alloc(R, c_exy, 2 * K, "the kept end points"));
                SEQ_TRY(seq_kernels_begin(R));
                hipLaunchKernelGGL(k_trip_compact, dim3(seq_grid(m)), dim3(SEQ_BLOCK), 0, R.stream, okx.p, hour.p, sxy.p, exy.p, m, c_hour.p, c_sxy.p, c_exy.p);
                SEQ_TRY(seq_kernels_end(R));
                SEQ_TRY(dge_flows_add_trips_device(sink.flows, c_sxy.p, c_exy.p, c_hour.p, K));
            }
        } else if (sink.records + m <= sink.cap) {
            SEQ_TRY(seq_read_back(R, sink.status + sink.records, status.p, (size_t)m));
            SEQ_TRY(seq_read_back(R, sink.hour + sink.records, hour.p, (size_t)m * 4));
            SEQ_TRY(seq_read_back(R, sink.sxy + 2 * sink.records, sxy.p, (size_t)m * 16));
            SEQ_TRY(seq_read_back(R, sink.exy + 2 * sink.records, exy.p, (size_t)m * 16));
        }
        sink.records += m;
        return DGE_OK;
    }

    int run(TripSink& sink) {
        using clock = std::chrono::steady_clock;
        TripFeeder feed{R.pieces, S};
        TripSlab slab[2];
        for (int64_t k = 0;; k++) {
            TripSlab& s = slab[k & 1];
            bool first = false, open_end = false;
            const auto t0 = clock::now();
            s.b = (int)(k & 1);
            SEQ_TRY(feed.next(R.pin[s.b], &s.n, &first, &open_end));       // (slab k - 1 is in its kernels meanwhile; slab k - 2, which had this buffer, is done)
            info.read_ms += std::chrono::duration<double, std::milli>(clock::now() - t0).count();
            SEQ_TRY(finish(slab[(k + 1) & 1], sink));
            if (s.n == 0) break;
            SEQ_TRY(submit(s, first, open_end));
        }
        info.kernel_ms = R.kernel_ms;
        return DGE_OK;
    }
};

int trip_check_options(const struct dge_trip_text_options* opt, const char* who) {
    if (!opt) DGE_FAIL(DGE_ERR_ARG, "%s: null argument: the options", who);
    if (opt->format < DGE_TRIPS_TYPE1 || opt->format > DGE_TRIPS_TYPE3) DGE_FAIL(DGE_ERR_ARG, "%s: format %d is none of DGE_TRIPS_TYPE1 .. DGE_TRIPS_TYPE3", who, opt->format);
    if (opt->slab_bytes < 0 || (opt->slab_bytes > 0 && opt->slab_bytes < TRIP_SLAB_MIN))
        DGE_FAIL(DGE_ERR_ARG, "%s: slab_bytes %lld is neither 0 nor at least %lld", who, (long long)opt->slab_bytes, (long long)TRIP_SLAB_MIN);
    return DGE_OK;
}

int trip_check_texts(const char* const* texts, const int64_t* n_bytes, int32_t n, const char* who) {
    if (n < 0 || (n > 0 && (!texts || !n_bytes))) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    return seq_check_texts(texts, n_bytes, n, who);
}

void trip_configure(TripReader& T, int device, const struct dge_trip_text_options* opt) {
    T.R.device = device;
    T.format = opt->format; T.header = opt->header != 0;
    T.S = opt->slab_bytes == 0 ? TRIP_SLAB_DEFAULT : std::min(opt->slab_bytes, TRIP_SLAB_MAX);
}

// the text's trips into a table of their own, that table into f: on any error f is as it was
int trip_into_flows(TripReader& T, dge_flows* f, dge_trip_text_info* info, const char* who) {
    dge_flows* part = nullptr;
    SEQ_TRY(dge_flows_like(f, &part));
    struct Free { dge_flows* p; ~Free() { dge_flows_free(p); } } guard{part};
    SEQ_TRY(T.open(who));
    TripSink sink;
    sink.flows = part;
    SEQ_TRY(T.run(sink));
    SEQ_TRY(dge_flows_merge(f, part));
    if (info) *info = T.info;
    return DGE_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------ entries
extern "C" int dge_trips_parse_texts(int device, const char* const* texts, const int64_t* n_bytes, int32_t n, const struct dge_trip_text_options* opt, uint8_t* status, int32_t* hour,
                                     double* start_xy, double* end_xy, int64_t cap, int64_t* n_lines, dge_trip_text_info* info) {
    const char* who = "dge_trips_parse_texts";
    if (!n_lines || cap < 0 || (cap > 0 && (!status || !hour || !start_xy || !end_xy))) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    SEQ_TRY(trip_check_texts(texts, n_bytes, n, who));
    SEQ_TRY(trip_check_options(opt, who));
    SEQ_TRY(dge_require_device(device));
    TripReader T;
    trip_configure(T, device, opt);
    SEQ_TRY(seq_add_texts(T.R.pieces, texts, n_bytes, n, who));
    SEQ_TRY(T.open(who));
    TripSink sink;
    sink.status = status; sink.hour = hour; sink.sxy = start_xy; sink.exy = end_xy; sink.cap = cap;
    SEQ_TRY(T.run(sink));
    *n_lines = sink.records;
    if (info) *info = T.info;
    if (sink.records > cap) DGE_FAIL(DGE_ERR_CAP, "%s: %lld lines exceed cap %lld", who, (long long)sink.records, (long long)cap);
    return DGE_OK;
}

extern "C" int dge_flows_add_trip_texts(dge_flows* f, const char* const* texts, const int64_t* n_bytes, int32_t n, const struct dge_trip_text_options* opt, dge_trip_text_info* info) {
    const char* who = "dge_flows_add_trip_texts";
    if (!f) DGE_FAIL(DGE_ERR_ARG, "%s: null argument: the flows", who);
    SEQ_TRY(trip_check_texts(texts, n_bytes, n, who));
    SEQ_TRY(trip_check_options(opt, who));
    SEQ_TRY(dge_require_device(dge_flows_device(f)));
    TripReader T;
    trip_configure(T, dge_flows_device(f), opt);
    SEQ_TRY(seq_add_texts(T.R.pieces, texts, n_bytes, n, who));
    return trip_into_flows(T, f, info, who);
}

extern "C" int dge_flows_add_trip_files(dge_flows* f, const char* const* paths, int32_t n, const struct dge_trip_text_options* opt, dge_trip_text_info* info) {
    const char* who = "dge_flows_add_trip_files";
    if (!f || n < 0 || (n > 0 && !paths)) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    SEQ_TRY(seq_check_paths(paths, n, who));
    SEQ_TRY(trip_check_options(opt, who));
    SEQ_TRY(dge_require_device(dge_flows_device(f)));
    TripReader T;
    trip_configure(T, dge_flows_device(f), opt);
    SEQ_TRY(seq_add_files(T.R.pieces, paths, n, who));
    return trip_into_flows(T, f, info, who);
}
