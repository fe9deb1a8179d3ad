// matrix_read.hip — .matrix adjacency text in, flow-table entries out (include/dge.h: dge_flows_add_matrix_texts / _files; the rule's per-element pieces:
// matrix_parse.h; the transport's host side: matrix_feed.h).  The reference reads these files with np.loadtxt and indexes the dense result
// (P/matrixFactorization_tract.py:35, P/flowFeatureGeneration_tract.py:29-40); here the text streams through the device in slabs, only the values > 0 leave it,
// and nothing of size n^2 or one record per value is formed.  Outside the build stamp: nothing here is read or written by a training launch.
//
// Transport.  MatrixFeeder cuts every piece into slabs of at most slab_bytes behind a separator or '\n' (it looks at a slab's last 32 bytes only) and frames
// each with the byte before and the byte behind it.  Two pinned buffers alternate: while slab k is copied, counted and scanned, the host reads slab k + 1.
// Between slabs a MatState of 64 bytes lives in device memory (lines ended, separators of the open line, non-empty lines, entries staged, the least offence,
// the values' sum); the byte in front of a slab tells whether the open line has a byte.  Per slab the host reads that state back twice — after the scan, to
// size the entry staging, and after the emit, to see an offence — and does nothing per line or per value.  After an offence nothing more is launched.
//
// Kernels of a slab (a workgroup of 256 lanes takes a tile of 8 192 bytes, a lane 32 bytes as two 16-byte loads; the masks and all that follows from them are
// matrix_parse.h's, the lane before hands its raw masks on through LDS):
//   k_mat_count   the lane's summary (lines ended, separators since, non-empty lines opened, values > 0 ended), a block scan under the segmented operator, the
//                 tile's aggregate to global memory.
//   k_mat_tiles   ONE workgroup scans the at most 2 048 aggregates, eight a lane, seeded with the carried state, and leaves every tile's state in front of it
//                 and the new carry.  A launch of its own: no look-back, no spin, no wait between workgroups.
//   k_mat_emit    forms the masks again (the slab is 16 MiB at most and was just read), gives every lane its exclusive (line, column, row, place), parses the
//                 values > 0 that end in the lane by integer arithmetic out of global memory and writes key = (hour R + idx[row]) R + idx[col] and the count
//                 at the value's place: text order, no atomics for data.  Line ends and line starts are checked against n here; a lane's least offence goes
//                 through one 64-bit atomicMin of (offset << 3 | kind), the values' sum through two integer atomicAdd after a block reduction.
//   k_mat_where   the error path: one thread walks from the offending tile's first byte to the offence and counts its line and column.
// All pieces are staged; trip_commit_entries (trip_flows.h) is the one commit at the end.
// Coherence: no protocol.  Every array is written by one kernel and read by later ones on the same stream; the state is read back between launches.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), VGPR / SGPR / scratch / LDS bytes:
//   k_mat_count 76 / 17 / 0 / 7 332, k_mat_tiles 48 / 42 / 0 / 8 448, k_mat_emit 78 / 46 / 0 / 7 332, k_mat_where 8 / 22 / 0 / 0.
// The shape is the one the design proposed; it has not been measured against an alternative.
#include "trip_flows.h"
#include "flow_rule.h"
#include "matrix_feed.h"

// ------------------------------------------------------------------------------------------ kernels
__device__ __forceinline__ MatRaw mat_load(const uint8_t* p, uint32_t sep) {
    const uint4 a = *reinterpret_cast<const uint4*>(p), b = *reinterpret_cast<const uint4*>(p + 16);
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    return mat_raw(w, sep);
}

// the lane at text[at ..) with what the lane before it hands on (for a tile's first lane: the 32 bytes in front of the tile, read by itself)
__device__ __forceinline__ MatLane mat_tile_lane(const uint8_t* text, int64_t n, uint32_t sep, int64_t at) {
    __shared__ uint32_t s_dig[MAT_BLOCK + 1], s_nz[MAT_BLOCK + 1], s_top[MAT_BLOCK + 1];
    const int t = threadIdx.x;
    const MatRaw cur = mat_load(text + at, sep);
    s_dig[t + 1] = cur.dig; s_nz[t + 1] = cur.nz; s_top[t + 1] = (cur.sep >> 31) | (cur.nl >> 31) << 1 | (cur.cr >> 31) << 2;
    if (t == 0) {
        const MatRaw q = mat_load(text + at - MAT_LANE, sep);
        s_dig[0] = q.dig; s_nz[0] = q.nz; s_top[0] = (q.sep >> 31) | (q.nl >> 31) << 1 | (q.cr >> 31) << 2;
    }
    __syncthreads();
    const uint32_t top = s_top[t];
    const MatRaw p = {s_dig[t], s_nz[t], (top & 1u) << 31, (top >> 1 & 1u) << 31, (top >> 2 & 1u) << 31};
    const int64_t left = n - at;
    return mat_lane(cur, p, text[at + MAT_LANE], left < 0 ? 0 : left > MAT_LANE ? MAT_LANE : (int)left);
}

__global__ void __launch_bounds__(MAT_BLOCK) k_mat_count(const uint8_t* text, int64_t n, uint32_t sep, MatSum* tile_agg) {
    typedef hipcub::BlockScan<MatSum, MAT_BLOCK> Scan;
    __shared__ typename Scan::TempStorage tmp;
    const int64_t at = (int64_t)blockIdx.x * MAT_TILE + (int64_t)threadIdx.x * MAT_LANE;
    const MatLane L = mat_tile_lane(text, n, sep, at);
    MatSum ex, agg;
    Scan(tmp).ExclusiveScan(mat_summary(L), ex, MatSum{0, 0, 0, 0}, MatCombine(), agg);
    if (threadIdx.x == 0) tile_agg[blockIdx.x] = agg;
}

// tile_excl[t] = the state in front of tile t; st: the carry in (first: the slab opens a piece, whose lines, separators and rows start at 0) and out
__global__ void __launch_bounds__(MAT_BLOCK) k_mat_tiles(const MatSum* tile_agg, int32_t tiles, int32_t first, MatState* st, MatSum64* tile_excl) {
    typedef hipcub::BlockScan<MatSum64, MAT_BLOCK> Scan;
    __shared__ typename Scan::TempStorage tmp;
    constexpr int PER = MAT_MAX_TILES / MAT_BLOCK;
    const MatSum64 seed = {first ? 0 : st->nl, first ? 0 : st->cols, first ? 0 : st->rows, st->out};
    const int t0 = threadIdx.x * PER;
    MatSum64 mine = {0, 0, 0, 0};
    for (int j = 0; j < PER; j++) if (t0 + j < tiles) mine = mat_combine(mine, tile_agg[t0 + j]);
    MatSum64 ex, agg;
    Scan(tmp).ExclusiveScan(mine, ex, MatSum64{0, 0, 0, 0}, MatCombine(), agg);
    MatSum64 run = mat_combine(seed, ex);
    for (int j = 0; j < PER; j++)
        if (t0 + j < tiles) { tile_excl[t0 + j] = run; run = mat_combine(run, tile_agg[t0 + j]); }
    __syncthreads();                               // every lane has read the carry
    if (threadIdx.x == 0) {
        const MatSum64 all = mat_combine(seed, agg);
        st->nl = all.nl; st->cols = all.cols; st->rows = all.rows; st->out = all.emits;
    }
}

struct MatDevSink {
    uint64_t* key; int64_t* cnt; const int32_t* idx; uint64_t hour_base, R;
    __device__ void entry(int64_t out, int64_t row, int64_t col, uint64_t v) {
        key[out] = v ? hour_base + (uint64_t)idx[row] * R + (uint64_t)idx[col] : 0;           // v == 0: an offence stands somewhere and nothing is committed
        cnt[out] = (int64_t)v;
    }
};

__global__ void __launch_bounds__(MAT_BLOCK) k_mat_emit(const uint8_t* text, int64_t n, int64_t base, int32_t last, uint32_t sep, int64_t nsel, const MatSum64* tile_excl,
                                                        const int32_t* idx, uint64_t hour_base, uint64_t R, uint64_t* key, int64_t* cnt, MatState* st) {
    typedef hipcub::BlockScan<MatSum, MAT_BLOCK> Scan;
    typedef hipcub::BlockReduce<unsigned long long, MAT_BLOCK> Reduce;
    __shared__ union { typename Scan::TempStorage scan; typename Reduce::TempStorage reduce; } tmp;
    const int64_t at = (int64_t)blockIdx.x * MAT_TILE + (int64_t)threadIdx.x * MAT_LANE;
    const MatLane L = mat_tile_lane(text, n, sep, at);
    MatSum ex;
    Scan(tmp.scan).ExclusiveScan(mat_summary(L), ex, MatSum{0, 0, 0, 0}, MatCombine());
    const MatSum64 in = mat_combine(tile_excl[blockIdx.x], ex);
    const MatSlab S = {text, n, base, nsel, last};
    MatDevSink sink = {key, cnt, idx, hour_base, R};
    uint64_t sum[2] = {0, 0};
    const uint64_t off = mat_lane_emit(S, at, L, in, sink, sum);
    if (off != MAT_NO_OFFENCE) atomicMin(reinterpret_cast<unsigned long long*>(&st->offence), (unsigned long long)off);
    __syncthreads();
    const unsigned long long hi = Reduce(tmp.reduce).Sum((unsigned long long)sum[0]);
    __syncthreads();
    const unsigned long long lo = Reduce(tmp.reduce).Sum((unsigned long long)sum[1]);
    if (threadIdx.x == 0 && (hi | lo)) {
        atomicAdd(reinterpret_cast<unsigned long long*>(&st->sum_hi), hi);
        atomicAdd(reinterpret_cast<unsigned long long*>(&st->sum_lo), lo);
    }
}

// where[0], where[1] = lines ended and separators since the last line end in front of byte p of the slab (0 <= p <= n)
__global__ void k_mat_where(const uint8_t* text, const MatSum64* tile_excl, int32_t tiles, int64_t p, uint32_t sep, int64_t* where) {
    const int64_t tile = p / MAT_TILE < tiles ? p / MAT_TILE : tiles - 1;
    int64_t nl = tile_excl[tile].nl, cols = tile_excl[tile].cols;
    mat_where(text, tile * MAT_TILE, p, sep, &nl, &cols);
    where[0] = nl; where[1] = cols;
}

// ------------------------------------------------------------------------------------------ host side
namespace {

const char* const MAT_KIND_NAME[8] = {"", "bad byte", "empty value", "long value", "value above 2^40", "ragged line", "too many rows", "too few rows"};

struct MatCut { int b = 0; int64_t n = 0, base = 0; int32_t piece = 0; bool first = false, last = false; };

struct MatReader {
    SeqRun R;
    const char* who = "";
    const int32_t* hour = nullptr;
    int64_t S = 0, nsel = 0, cap = 0;
    uint32_t sep = ',';
    uint64_t Ru = 1;
    dge_tmp<uint8_t> buf;
    dge_tmp<MatSum> tile_agg;
    dge_tmp<MatSum64> tile_excl;
    dge_tmp<MatState> state;
    dge_tmp<int32_t> idx;
    dge_tmp<uint64_t> key;
    dge_tmp<int64_t> cnt;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    dge_matrix_read_info info = {};
    uint64_t sums[2] = {0, 0};        // the staged values' sum: value >> 20 and value & 0xfffff, each added up
    ~MatReader() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }

    int open(const dge_flows* f, const uint8_t* select) {
        const dge_regions* rg = f->regions;
        std::vector<int64_t> order((size_t)rg->R);
        for (int64_t r = 0; r < rg->R; r++) order[(size_t)r] = r;
        std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return rg->ids[(size_t)a] < rg->ids[(size_t)b]; });
        std::vector<int32_t> sel;                                   // row and column i of the text -> region index: the selected regions, ascending by id
        for (int64_t r = 0; r < rg->R; r++) if (!select || select[(size_t)order[(size_t)r]]) sel.push_back((int32_t)order[(size_t)r]);
        nsel = (int64_t)sel.size();
        Ru = (uint64_t)std::max<int64_t>(rg->R, 1);
        SEQ_TRY(seq_open(R, rg->device, who));
        for (hipEvent_t& e : ev) DGE_HIP(hipEventCreate(&e));
        int64_t total = 0, largest = 0;
        for (const SeqPiece& p : R.pieces) { total += p.size; largest = std::max(largest, p.size); }
        info.bytes = total; info.pieces = (int32_t)R.pieces.size(); info.n = (int32_t)nsel; info.tile_bytes = MAT_TILE;
        S = std::min(S, std::max<int64_t>(MAT_SLAB_MIN, largest));              // no buffer beyond the largest piece
        for (int i = 0; i < 2; i++) {
            const hipError_t e = hipHostMalloc((void**)&R.pin[i], (size_t)mat_frame_bytes(S), hipHostMallocDefault);
            if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); R.pin[i] = nullptr; DGE_FAIL(DGE_ERR_CAP, "%s: two pinned buffers of %lld bytes do not fit", who, (long long)mat_frame_bytes(S)); }
            DGE_HIP(e);
        }
        const int64_t tiles = (S + MAT_TILE - 1) / MAT_TILE;
        SEQ_TRY(seq_alloc(R, buf, MAT_LEAD + tiles * MAT_TILE + 2 * MAT_LANE, "the slab"));
        SEQ_TRY(seq_alloc(R, tile_agg, tiles, "the tiles' sums"));
        SEQ_TRY(seq_alloc(R, tile_excl, tiles, "the tiles' states"));
        SEQ_TRY(seq_alloc(R, state, 1, "the carried state"));
        SEQ_TRY(seq_alloc(R, idx, nsel, "the selected regions"));
        MatState zero = {};
        zero.offence = MAT_NO_OFFENCE;
        DGE_HIP(hipMemcpyAsync(state.p, &zero, sizeof(zero), hipMemcpyHostToDevice, R.stream));
        if (nsel) DGE_HIP(hipMemcpyAsync(idx.p, sel.data(), (size_t)nsel * 4, hipMemcpyHostToDevice, R.stream));
        DGE_HIP(hipStreamSynchronize(R.stream));
        return DGE_OK;
    }

    int reserve(int64_t need, int64_t have) {
        if (need <= cap) return DGE_OK;
        const int64_t c = std::max<int64_t>(std::max(need, cap * 2), 1024);
        dge_tmp<uint64_t> k2;
        dge_tmp<int64_t> c2;
        SEQ_TRY(seq_alloc(R, k2, c, "the entries' keys"));
        SEQ_TRY(seq_alloc(R, c2, c, "the entries' counts"));
        if (have) {
            DGE_HIP(hipMemcpyAsync(k2.p, key.p, (size_t)have * 8, hipMemcpyDeviceToDevice, R.stream));
            DGE_HIP(hipMemcpyAsync(c2.p, cnt.p, (size_t)have * 8, hipMemcpyDeviceToDevice, R.stream));
            DGE_HIP(hipStreamSynchronize(R.stream));
        }
        seq_release(R, key, cap); seq_release(R, cnt, cap);
        key = std::move(k2); cnt = std::move(c2); cap = c;
        return DGE_OK;
    }

    int refuse(int kind, int32_t piece, int64_t offset, int64_t nl, int64_t cols) {
        char path[320] = "";
        if (R.pieces[(size_t)piece].path) snprintf(path, sizeof(path), " (%s)", R.pieces[(size_t)piece].path);
        char more[96] = "";
        if (kind == MAT_RAGGED) snprintf(more, sizeof(more), ": %lld values found, %lld expected", (long long)cols + 1, (long long)nsel);
        if (kind == MAT_ROWS_MANY || kind == MAT_ROWS_FEW) snprintf(more, sizeof(more), ": %lld non-empty lines expected", (long long)nsel);
        DGE_FAIL(kind == MAT_BIG_VALUE ? DGE_ERR_RANGE : DGE_ERR_IO, "%s: %s at piece %d%s, offset %lld, line %lld, column %lld%s", who, MAT_KIND_NAME[kind], piece, path,
                 (long long)offset, (long long)nl + 1, (long long)cols, more);
    }

    // pieces [from, to) hold no byte: fine when no line is expected
    int empty_pieces(int32_t from, int32_t to) {
        if (from < to && nsel > 0) return refuse(MAT_ROWS_FEW, from, 0, 0, 0);
        return DGE_OK;
    }

    int fill(MatrixFeeder& feed, MatCut& c) {
        using clock = std::chrono::steady_clock;
        const auto t0 = clock::now();
        SEQ_TRY(feed.next(R.pin[c.b], &c.n, &c.piece, &c.base, &c.first, &c.last));
        info.read_ms += std::chrono::duration<double, std::milli>(clock::now() - t0).count();
        return DGE_OK;
    }

    int run() {
        MatrixFeeder feed{R.pieces, S, sep};
        MatCut cut[2];
        cut[0].b = 0; cut[1].b = 1;
        int32_t next_piece = 0;
        SEQ_TRY(fill(feed, cut[0]));
        for (int64_t k = 0; cut[k & 1].n > 0; k++) {
            const MatCut& c = cut[k & 1];
            SEQ_TRY(empty_pieces(next_piece, c.piece));
            const int32_t tiles = (int32_t)((c.n + MAT_TILE - 1) / MAT_TILE);
            uint8_t* text = buf.p + MAT_LEAD;
            DGE_HIP(hipMemcpyAsync(buf.p, R.pin[c.b], (size_t)(MAT_LEAD + (c.n + MAT_LANE - 1) / MAT_LANE * MAT_LANE + MAT_LANE + 1), hipMemcpyHostToDevice, R.stream));
            DGE_HIP(hipEventRecord(ev[0], R.stream));
            hipLaunchKernelGGL(k_mat_count, dim3((unsigned)tiles), dim3(MAT_BLOCK), 0, R.stream, text, c.n, sep, tile_agg.p);
            hipLaunchKernelGGL(k_mat_tiles, dim3(1), dim3(MAT_BLOCK), 0, R.stream, tile_agg.p, tiles, c.first ? 1 : 0, state.p, tile_excl.p);
            DGE_HIP(hipEventRecord(ev[1], R.stream));
            DGE_HIP(hipGetLastError());
            SEQ_TRY(fill(feed, cut[(k + 1) & 1]));                   // (the host reads slab k + 1 while slab k is copied, counted and scanned)
            MatState st;
            const int64_t have = info.entries;
            SEQ_TRY(seq_read_back(R, &st, state.p, sizeof(st)));
            SEQ_TRY(reserve(st.out, have));
            DGE_HIP(hipEventRecord(ev[2], R.stream));
            hipLaunchKernelGGL(k_mat_emit, dim3((unsigned)tiles), dim3(MAT_BLOCK), 0, R.stream, text, c.n, c.base, c.last ? 1 : 0, sep, nsel, tile_excl.p, idx.p,
                               (uint64_t)hour[c.piece] * Ru * Ru, Ru, key.p, cnt.p, state.p);
            DGE_HIP(hipEventRecord(ev[3], R.stream));
            DGE_HIP(hipGetLastError());
            SEQ_TRY(seq_read_back(R, &st, state.p, sizeof(st)));
            float a = 0.f, b = 0.f;
            DGE_HIP(hipEventElapsedTime(&a, ev[0], ev[1]));
            DGE_HIP(hipEventElapsedTime(&b, ev[2], ev[3]));
            R.kernel_ms += a + b;
            info.slabs++;
            if (st.offence != MAT_NO_OFFENCE) {
                const int kind = (int)(st.offence & 7);
                const int64_t offset = (int64_t)(st.offence >> 3);
                dge_tmp<int64_t> d_where;
                int64_t where[2] = {0, 0};
                SEQ_TRY(seq_alloc(R, d_where, 2, "a position"));
                hipLaunchKernelGGL(k_mat_where, dim3(1), dim3(1), 0, R.stream, text, tile_excl.p, tiles, std::min(std::max<int64_t>(offset - c.base, 0), c.n), sep, d_where.p);
                SEQ_TRY(seq_read_back(R, where, d_where.p, sizeof(where)));
                return refuse(kind, c.piece, offset, where[0], where[1]);
            }
            info.entries = st.out;
            if (c.last) {
                info.lines += st.nl + (R.pin[c.b][MAT_LEAD + c.n - 1] != '\n' ? 1 : 0);
                info.rows += st.rows;
                next_piece = c.piece + 1;
            }
            sums[0] = st.sum_hi; sums[1] = st.sum_lo;
        }
        SEQ_TRY(empty_pieces(next_piece, (int32_t)R.pieces.size()));
        return DGE_OK;
    }
};

int mat_check(const char* who, const dge_flows* f, const void* pieces, const int64_t* n_bytes, bool texts, const int32_t* hour, int32_t n_pieces, const dge_matrix_read_options* opt) {
    if (!f || !pieces || (texts && !n_bytes) || !hour || !opt || n_pieces < 0) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    if (n_pieces < 1) DGE_FAIL(DGE_ERR_ARG, "%s: n_pieces %d: one piece at least is needed", who, n_pieces);
    if (opt->sep != ',' && opt->sep != ' ' && opt->sep != '\t') DGE_FAIL(DGE_ERR_ARG, "%s: sep %d is none of ',', ' ' and a tab", who, opt->sep);
    if (opt->reserved != 0) DGE_FAIL(DGE_ERR_ARG, "%s: the options' reserved field is %d, not 0", who, opt->reserved);
    if (opt->slab_bytes < 0 || (opt->slab_bytes > 0 && (opt->slab_bytes < MAT_SLAB_MIN || opt->slab_bytes > MAT_SLAB_MAX)))
        DGE_FAIL(DGE_ERR_ARG, "%s: slab_bytes %lld is neither 0 nor in %d .. %lld", who, (long long)opt->slab_bytes, MAT_SLAB_MIN, (long long)MAT_SLAB_MAX);
    for (int32_t k = 0; k < n_pieces; k++)
        if (hour[k] < 0 || hour[k] > 23) DGE_FAIL(DGE_ERR_ARG, "%s: piece %d has hour %d: 0 .. 23 is needed", who, k, hour[k]);
    return DGE_OK;
}

// the handle's part of the checks, the device, and what both entries do once their pieces stand in T.R.pieces
int mat_into_flows(MatReader& T, dge_flows* f, const uint8_t* select, dge_matrix_read_info* info) {
    SEQ_TRY(T.open(f, select));
    SEQ_TRY(T.run());
    const int64_t u = T.info.entries;
    const unsigned __int128 total = ((unsigned __int128)T.sums[0] << 20) + T.sums[1];
    if (total > (unsigned __int128)1 << 62) DGE_FAIL(DGE_ERR_RANGE, "%s: the values add up to more than 2^62", T.who);
    if (u > 0) SEQ_TRY(trip_commit_entries(T.R, f, T.key.p, T.cnt.p, u, (int64_t)total, (int64_t)FR_MAX_COUNT, T.who));
    T.info.total = (int64_t)total;
    T.info.values = T.info.rows * T.nsel;
    T.info.zeros = T.info.values - u;
    T.info.kernel_ms = T.R.kernel_ms;
    if (info) *info = T.info;
    return DGE_OK;
}

int mat_select_check(const char* who, const dge_flows* f, const uint8_t* select) {
    if (select && f->regions->R == 0) DGE_FAIL(DGE_ERR_ARG, "%s: a select array over no regions", who);
    return DGE_OK;
}

void mat_configure(MatReader& T, const char* who, const int32_t* hour, const dge_matrix_read_options* opt) {
    T.who = who; T.hour = hour; T.sep = (uint32_t)opt->sep;
    T.S = opt->slab_bytes == 0 ? MAT_SLAB_MAX : opt->slab_bytes;
}

}  // namespace

// ------------------------------------------------------------------------------------------ entries
extern "C" int dge_flows_add_matrix_texts(dge_flows* f, const char* const* texts, const int64_t* n_bytes, const int32_t* hour, int32_t n_pieces, const uint8_t* select,
                                          const dge_matrix_read_options* opt, dge_matrix_read_info* info) {
    const char* who = "dge_flows_add_matrix_texts";
    SEQ_TRY(mat_check(who, f, texts, n_bytes, true, hour, n_pieces, opt));
    SEQ_TRY(seq_check_texts(texts, n_bytes, n_pieces, who));
    SEQ_TRY(mat_select_check(who, f, select));
    SEQ_TRY(dge_require_device(dge_flows_device(f)));
    MatReader T;
    mat_configure(T, who, hour, opt);
    SEQ_TRY(seq_add_texts(T.R.pieces, texts, n_bytes, n_pieces, who));
    return mat_into_flows(T, f, select, info);
}

extern "C" int dge_flows_add_matrix_files(dge_flows* f, const char* const* paths, const int32_t* hour, int32_t n_pieces, const uint8_t* select, const dge_matrix_read_options* opt,
                                          dge_matrix_read_info* info) {
    const char* who = "dge_flows_add_matrix_files";
    SEQ_TRY(mat_check(who, f, paths, nullptr, false, hour, n_pieces, opt));
    SEQ_TRY(seq_check_paths(paths, n_pieces, who));
    SEQ_TRY(mat_select_check(who, f, select));
    SEQ_TRY(dge_require_device(dge_flows_device(f)));
    MatReader T;
    mat_configure(T, who, hour, opt);
    SEQ_TRY(seq_add_files(T.R.pieces, paths, n_pieces, who));
    return mat_into_flows(T, f, select, info);
}
