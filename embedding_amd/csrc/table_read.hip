// table_read.hip — count tables: a resident int64 table c[R][C] over a dge_regions handle, filled from delimited text, from points and from entries, merged
// along a region map and handed on as dge_vectors (include/dge.h: dge_counts_*; the per-line rule: table_parse.h).  The reference builds these tables line by
// line on the host (getLEHDfeatures_helper, P/embeddingEvaluation_tract.py:512-536, and its siblings; Tweets.mapTweetsIntoTracts, J/Tweets.java:43-88).
// Outside the build stamp: nothing here is read or written by a training launch.
//
// Transport and line finding are the trip reader's (trip_text.hip): TripFeeder of seq_pieces.h, unchanged, cuts every piece into slabs of whole lines; two
// pinned buffers alternate, the host reads slab k + 1 while slab k is in its kernels.  The feeder does not say where in its piece a slab starts; the reader
// works that out from the feeder's counters after the call (fill()).  A line the feeder had to cut (no terminator in a whole buffer) is the offence "long
// line" at the slab's first byte and is decided on the host — unless it is one of its piece's skip_lines headers, which are never looked at: its stub then
// goes through the kernels as the one skipped line it is, so the verdict is the same whether or not a slab holds the line.
//
// Kernels of a slab:
//   k_tab_count / k_tab_emit   a lane takes 32 bytes as two 16-byte loads and gives the line-end mask; per-chunk counts, a scan and the second pass give line l
//                              the offset of its terminator (as k_trip_count / k_trip_emit).
//   k_tab_parse                a workgroup takes 256 consecutive lines, stages their bytes in LDS with 16-byte loads (TAB_TILE bytes; a range that does not fit
//                              is read from global memory by the same code), every lane parses its own line with table_parse.h and looks its key up among
//                              the regions' ids by bisection.  Then, column by column, every lane takes its next value and the workgroup combines the 256
//                              values by cell: a segmented inclusive scan whose runs are the maximal runs of lanes with one cell (neighbour inequality), and
//                              only the lane that CLOSES a run adds the run's sum to the staging table with one 64-bit integer atomicAdd (cnt_block_add).
//                              Census files are sorted by block code, so a tract's hundred-odd lines become two or three atomics per column, not a chain of
//                              a hundred on one address.  A lane's least offence goes through one 64-bit atomicMin of (offset << 4 | kind); counters are
//                              integers added after a block reduction.
//   k_tab_where                the error path: one thread finds the offence's line by bisection and counts the separators in front of it.
// Everything that reaches the staging table is an integer sum, so its bits depend on neither the slab size nor the order of the atomics.  The other entries
// (add_entries, add_points) hand (cell, value) items to the same cnt_block_add; merge and vectors are a lane per output cell.  One commit (cnt_commit) ends
// every call that fills a table: a check of every cell against 2^62, then the addition.
// Coherence: no protocol.  Every array is written by one kernel and read by later ones on the same stream; counters are read back between launches.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), VGPR / SGPR / scratch / LDS bytes:
//   k_tab_count 58 / 14 / 0 / 16, k_tab_emit 57 / 20 / 0 / 1 056, k_tab_parse 64 / 66 / 0 / 55 472 (two workgroups a compute unit), k_tab_where 6 / 23 / 0 / 0,
//   k_cnt_entries 22 / 18 / 0 / 6 280, k_cnt_points 21 / 18 / 0 / 6 280, k_cnt_merge 14 / 33 / 0 / 0, k_cnt_row_sums 10 / 20 / 0 / 32, k_cnt_vectors 22 / 29 / 0 / 0.
// The shape is the one the design proposed; none of it has been measured against an alternative.
#include <algorithm>

#include "seq_tokens.h"
#include "table_parse.h"

constexpr int64_t TAB_SLAB_DEFAULT = (int64_t)16 << 20, TAB_SLAB_MIN = 131072, TAB_SLAB_MAX = (int64_t)1 << 30;      // the trip reader's range
constexpr int TAB_TILE = 48 * 1024;              // bytes of LDS a workgroup's 256 lines may take
constexpr int64_t CNT_MAX_CELL = (int64_t)1 << 62;
enum { TC_OFFENCE = 0, TC_ROWS, TC_EMPTY, TC_FOREIGN, TC_SUM_HI, TC_SUM_LO, TC_N };

struct dge_counts {
    int device = 0;
    dge_regions* regions = nullptr;              // a reference is held
    int64_t R = 0;
    int32_t C = 0;
    dge_tmp<int64_t> d = nullptr;                // [R x C], row = rank of the region's id
    ~dge_counts() { if (regions) dge_regions_free(regions); }
};

// ------------------------------------------------------------------------------------------ kernels
// 32 bytes of one lane: bit i = a line ends at base + i ("\n", or "\r" not followed by "\n"); the buffer goes on for 32 zero bytes
__device__ __forceinline__ uint32_t tab_end_mask(const uint8_t* buf, int64_t base) {
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

__global__ void __launch_bounds__(SEQ_BLOCK) k_tab_count(const uint8_t* buf, int64_t* chunk_ends) {
    typedef hipcub::BlockReduce<int, SEQ_BLOCK> Reduce;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t base = (int64_t)blockIdx.x * SEQ_CHUNK + (int64_t)threadIdx.x * 32;
    const int sum = Reduce(tmp).Sum(__popc(tab_end_mask(buf, base)));
    if (threadIdx.x == 0) chunk_ends[blockIdx.x] = sum;
}

// line_end[l] = offset of the byte that ends line l (of "\r\n" the "\n"); a last line without a terminator ends at n
__global__ void __launch_bounds__(SEQ_BLOCK) k_tab_emit(const uint8_t* buf, const int64_t* chunk_endx, int32_t n, int64_t L, int open_end, int32_t* line_end) {
    typedef hipcub::BlockScan<int, SEQ_BLOCK> Scan;
    __shared__ typename Scan::TempStorage tmp;
    const int64_t base = (int64_t)blockIdx.x * SEQ_CHUNK + (int64_t)threadIdx.x * 32;
    uint32_t ends = tab_end_mask(buf, base);
    int before;
    Scan(tmp).ExclusiveSum(__popc(ends), before);
    int64_t l = chunk_endx[blockIdx.x] + before;
    while (ends) {
        const int i = __ffs(ends) - 1;
        ends &= ends - 1;
        if (l < L) line_end[l] = (int32_t)(base + i);
        l++;
    }
    if (open_end && blockIdx.x == 0 && threadIdx.x == 0) line_end[L - 1] = n;
}

struct CntSeg { unsigned long long v; int head; };
struct CntSegOp { __device__ CntSeg operator()(const CntSeg& a, const CntSeg& b) const { return b.head ? b : CntSeg{a.v + b.v, a.head}; } };

// All SEQ_BLOCK lanes call it.  The lanes' values are combined by cell over maximal runs of neighbouring lanes with one cell; the lane that closes a run adds
// the run's sum to stage[cell].  cell < 0: the lane has nothing (such lanes form runs of their own and add nothing).
__device__ __forceinline__ void cnt_block_add(unsigned long long* stage, int64_t cell, unsigned long long v) {
    typedef hipcub::BlockScan<CntSeg, SEQ_BLOCK> Scan;
    __shared__ typename Scan::TempStorage tmp;
    __shared__ int64_t s_cell[SEQ_BLOCK + 1];
    const int t = threadIdx.x;
    s_cell[t + 1] = cell;
    __syncthreads();
    const bool head = t == 0 || s_cell[t] != cell, closes = t == SEQ_BLOCK - 1 || s_cell[t + 2] != cell;
    CntSeg x = {v, head ? 1 : 0};
    Scan(tmp).InclusiveScan(x, x, CntSegOp());
    if (closes && cell >= 0 && x.v) atomicAdd(stage + cell, x.v);
    __syncthreads();
}

struct TabDev {
    tab_rule rule;
    const int64_t* ids;          // the regions' ids, ascending: row = place
    int64_t R;
    int32_t C, col_offset, neg_col_offset;
};

// line skip + i of the slab is lane i's (skip: header lines the slab opens with)
__global__ void __launch_bounds__(SEQ_BLOCK) k_tab_parse(const uint8_t* buf, int32_t n, const int32_t* line_end, int64_t L, int32_t skip, TabDev D, unsigned long long* stage,
                                                         unsigned long long* counters) {
    typedef hipcub::BlockReduce<unsigned long long, SEQ_BLOCK> Reduce;
    __shared__ typename Reduce::TempStorage tmp;
    __shared__ __attribute__((aligned(16))) uint8_t tile[TAB_TILE];
    const int64_t l0 = (int64_t)skip + (int64_t)blockIdx.x * SEQ_BLOCK, l1 = l0 + SEQ_BLOCK <= L ? l0 + SEQ_BLOCK : L;      // l0 < L: the grid covers L - skip lines
    const int32_t lo = l0 == 0 ? 0 : line_end[l0 - 1] + 1, hi = line_end[l1 - 1];                                        // hi <= n; byte hi is the last terminator, or a zero
    const int32_t abase = lo & ~15, bytes = hi + 1 - abase;
    const bool staged = bytes <= TAB_TILE;
    if (staged) {
        const uint4* src = reinterpret_cast<const uint4*>(buf + abase);
        uint4* dst = reinterpret_cast<uint4*>(tile);
        for (int32_t q = threadIdx.x; q * 16 < bytes; q += SEQ_BLOCK) dst[q] = src[q];      // at most 15 bytes past byte hi: inside the zeros behind the slab
    }
    __syncthreads();
    const int64_t l = l0 + threadIdx.x;
    unsigned long long v[TC_N] = {0, 0, 0, 0, 0, 0};
    const uint8_t* p = buf;
    int32_t len = 0, at = 0;
    int64_t cell0 = -1;                          // the cell of the line's first value; -1: the line adds nothing
    if (l < l1) {
        const int32_t start = l == 0 ? 0 : line_end[l - 1] + 1, end = line_end[l];
        p = staged ? tile + (start - abase) : buf + start;
        len = end - start;
        if (len > 0 && end < n && p[len] == '\n' && p[len - 1] == '\r') len--;
        if (len == 0) v[TC_EMPTY] = 1;
        else {
            tab_line T;
            tab_parse_line(p, len, D.rule, &T);
            if (T.offence != TAB_NO_OFFENCE) atomicMin(counters + TC_OFFENCE, (unsigned long long)(((uint64_t)(uint32_t)start << 4) + T.offence));
            else {
                int64_t a = 0, b = D.R;          // the first place whose id is not below the key
                while (a < b) { const int64_t m = (a + b) >> 1; if (D.ids[m] < T.key) a = m + 1; else b = m; }
                if (a < D.R && D.ids[a] == T.key) { cell0 = a * D.C + (T.neg ? D.neg_col_offset : D.col_offset); at = T.val_at; v[TC_ROWS] = 1; }
                else v[TC_FOREIGN] = 1;
            }
        }
    }
    unsigned long long sum = 0;
    const int32_t cols = __syncthreads_or(cell0 >= 0) ? D.rule.n_cols : 0;      // a tile of foreign and empty lines has nothing to combine
    for (int32_t j = 0; j < cols; j++) {
        unsigned long long x = 0;
        if (cell0 >= 0) { x = tab_next_value(p, len, D.rule.sep, &at); sum += x; }
        cnt_block_add(stage, cell0 >= 0 ? cell0 + j : -1, x);
    }
    v[TC_SUM_HI] = sum >> 20; v[TC_SUM_LO] = sum & 0xfffffu;
    for (int k = TC_ROWS; k < TC_N; k++) {
        const unsigned long long s = Reduce(tmp).Sum(v[k]);
        if (threadIdx.x == 0 && s) atomicAdd(counters + k, s);
        __syncthreads();
    }
}

// where[0] = the line of the slab that holds byte p (0 <= p <= n), where[1] = the sep bytes between that line's start and p
__global__ void k_tab_where(const uint8_t* buf, const int32_t* line_end, int64_t L, int32_t p, int32_t sep, int64_t* where) {
    int64_t a = 0, b = L - 1;                    // the first line whose end is not in front of p
    while (a < b) { const int64_t m = (a + b) >> 1; if (line_end[m] < p) a = m + 1; else b = m; }
    int64_t seps = 0;
    for (int32_t q = a == 0 ? 0 : line_end[a - 1] + 1; q < p; q++) seps += buf[q] == (uint8_t)sep;
    where[0] = a; where[1] = seps;
}

// items (cell or -1, value) into the staging table
__global__ void __launch_bounds__(SEQ_BLOCK) k_cnt_entries(const int32_t* row, const int32_t* col, const int64_t* val, int64_t n, int32_t C, unsigned long long* stage) {
    const int64_t i = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    cnt_block_add(stage, i < n ? (int64_t)row[i] * C + col[i] : -1, i < n ? (unsigned long long)val[i] : 0);
}
__global__ void __launch_bounds__(SEQ_BLOCK) k_cnt_points(const int32_t* region, const int32_t* idrank, const int32_t* col, int64_t n, int32_t C, unsigned long long* stage) {
    const int64_t i = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    const bool in = i < n && region[i] >= 0;
    cnt_block_add(stage, in ? (int64_t)idrank[region[i]] * C + col[i] : -1, in ? 1 : 0);
}

__global__ void __launch_bounds__(SEQ_BLOCK) k_cnt_check(const int64_t* table, const unsigned long long* stage, int64_t n, int32_t* over) {
    const int64_t i = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (i < n && stage[i] && (stage[i] > (unsigned long long)CNT_MAX_CELL || (unsigned long long)table[i] + stage[i] > (unsigned long long)CNT_MAX_CELL)) *over = 1;
}
__global__ void __launch_bounds__(SEQ_BLOCK) k_cnt_commit(int64_t* table, const unsigned long long* stage, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (i < n) table[i] += (int64_t)stage[i];
}

// out[0] = cells != 0, out[1], out[2] = the cells' sum as sums of cell >> 20 and cell & 0xfffff
__global__ void __launch_bounds__(SEQ_BLOCK) k_cnt_info(const int64_t* table, int64_t n, unsigned long long* out) {
    typedef hipcub::BlockReduce<unsigned long long, SEQ_BLOCK> Reduce;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t i = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    const unsigned long long c = i < n ? (unsigned long long)table[i] : 0;
    const unsigned long long v[3] = {c ? 1ull : 0ull, c >> 20, c & 0xfffffu};
    for (int k = 0; k < 3; k++) {
        const unsigned long long s = Reduce(tmp).Sum(v[k]);
        if (threadIdx.x == 0 && s) atomicAdd(out + k, s);
        __syncthreads();
    }
}

// a lane per cell of the new table: the rows member[first[g] .. first[g + 1]) of the old one, added up
__global__ void __launch_bounds__(SEQ_BLOCK) k_cnt_merge(const int64_t* table, int32_t C, const int64_t* first, const int32_t* member, int64_t G, int64_t* out, int32_t* over) {
    const int64_t i = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (i >= G * C) return;
    const int64_t g = i / C, j = i % C;
    unsigned long long s = 0;                    // every addend is at most 2^62: no wrap before the check
    for (int64_t k = first[g]; k < first[g + 1] && s <= (unsigned long long)CNT_MAX_CELL; k++) s += (unsigned long long)table[(int64_t)member[k] * C + j];
    if (s > (unsigned long long)CNT_MAX_CELL) { *over = 1; s = 0; }
    out[i] = (int64_t)s;
}

// a + b, held at 2^63 once it gets there (a, b <= 2^63: no wrap); 2^63 is what dge_counts_vectors refuses
struct CntSatAdd {
    __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const {
        const unsigned long long top = (unsigned long long)1 << 63;
        return a + b >= top ? top : a + b;
    }
};

// sum[i] = the sum of row i's columns [col_lo, col_lo + n_cols); a workgroup per row
__global__ void __launch_bounds__(SEQ_BLOCK) k_cnt_row_sums(const int64_t* table, int32_t C, int32_t col_lo, int32_t n_cols, unsigned long long* sum) {
    typedef hipcub::BlockReduce<unsigned long long, SEQ_BLOCK> Reduce;
    __shared__ typename Reduce::TempStorage tmp;
    unsigned long long s = 0;
    for (int32_t j = threadIdx.x; j < n_cols; j += SEQ_BLOCK) s = CntSatAdd()(s, (unsigned long long)table[(int64_t)blockIdx.x * C + col_lo + j]);      // a cell is 2^62 at most
    const unsigned long long all = Reduce(tmp).Reduce(s, CntSatAdd());
    if (threadIdx.x == 0) sum[blockIdx.x] = all;
}

// a lane per cell of the rows
__global__ void __launch_bounds__(SEQ_BLOCK) k_cnt_vectors(const int64_t* table, int32_t C, int32_t col_lo, int32_t n_cols, int64_t R, const unsigned long long* sum, int normalise,
                                                           int present_mode, float* out, uint8_t* present) {
    const int64_t i = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (i >= R * n_cols) return;
    const int64_t r = i / n_cols, j = i % n_cols;
    const int64_t c = table[r * C + col_lo + j];
    const unsigned long long s = sum[r];
    out[i] = !normalise ? (float)c : s == 0 ? 0.0f : (float)((double)c / (double)(int64_t)s);
    if (j == 0) present[r] = present_mode == DGE_COUNTS_PRESENT_ALL || s != 0 ? 1 : 0;
}

// ------------------------------------------------------------------------------------------ host side
namespace {

const char* const TAB_KIND_NAME[TAB_KINDS] = {"", "short line", "short key", "bad key", "key sign", "empty value", "bad value byte", "long value", "value above 2^40", "long line"};

int cnt_stage(SeqRun& R, const dge_counts* c, dge_tmp<unsigned long long>& stage) {
    SEQ_TRY(seq_alloc(R, stage, c->R * c->C, "the staging table"));
    DGE_HIP(hipMemsetAsync(stage.p, 0, (size_t)std::max<int64_t>(c->R * c->C, 1) * 8, R.stream));
    return DGE_OK;
}

// the one commit: every cell of table + stage against 2^62, then the addition
int cnt_commit(SeqRun& R, dge_counts* c, const unsigned long long* stage, const char* who) {
    const int64_t n = c->R * c->C;
    if (n == 0) return DGE_OK;
    dge_tmp<int32_t> over;
    int32_t flag = 0;
    SEQ_TRY(seq_alloc(R, over, 1, "a flag"));
    DGE_HIP(hipMemsetAsync(over.p, 0, 4, R.stream));
    hipLaunchKernelGGL(k_cnt_check, dim3(seq_grid(n)), dim3(SEQ_BLOCK), 0, R.stream, c->d.p, stage, n, over.p);
    SEQ_TRY(seq_read_back(R, &flag, over.p, 4));
    if (flag) DGE_FAIL(DGE_ERR_RANGE, "%s: a cell would stand above 2^62", who);
    hipLaunchKernelGGL(k_cnt_commit, dim3(seq_grid(n)), dim3(SEQ_BLOCK), 0, R.stream, c->d.p, stage, n);
    DGE_HIP(hipGetLastError());
    DGE_HIP(hipStreamSynchronize(R.stream));
    return DGE_OK;
}

template <typename T>
int cnt_upload(SeqRun& R, dge_tmp<T>& d, const T* src, int64_t n, const char* what) {
    SEQ_TRY(seq_alloc(R, d, n, what));
    if (n) DGE_HIP(hipMemcpyAsync(d.p, src, (size_t)n * sizeof(T), hipMemcpyHostToDevice, R.stream));
    return DGE_OK;
}

struct TabCut { int b = 0; int64_t n = 0, L = 0, base = 0, lines_before = 0; int32_t piece = 0, skip = 0; bool first = false, open_end = false, long_cut = false, live = false; };

struct TabReader {
    SeqRun R;
    const char* who = "";
    dge_table_read_options opt = {};
    TabDev D = {};
    int64_t S = 0, cap_lines = 0;
    dge_tmp<uint8_t> buf;
    dge_tmp<int64_t> chunk_ends, chunk_endx;
    dge_tmp<int32_t> line_end;
    dge_tmp<unsigned long long> counters, stage;
    hipEvent_t ea = nullptr, eb = nullptr;
    dge_table_read_info info = {};
    int64_t cursor = 0, lines_in_piece = 0;      // of the piece being fed: how far it was taken when the last slab came (fill() checks the next one against it); of the piece being submitted: its lines so far
    unsigned __int128 total = 0;
    ~TabReader() {
        if (ea) (void)hipEventDestroy(ea);
        if (eb) (void)hipEventDestroy(eb);
    }

    int open(dge_counts* c) {
        SEQ_TRY(seq_open(R, c->device, who));
        DGE_HIP(hipEventCreate(&ea));
        DGE_HIP(hipEventCreate(&eb));
        int64_t total_bytes = 0, largest = 0;
        for (const SeqPiece& p : R.pieces) { total_bytes += p.size; largest = std::max(largest, p.size); }
        info.bytes = total_bytes; info.pieces = (int32_t)R.pieces.size();
        S = std::min(S, std::max(TAB_SLAB_MIN, largest));           // no buffer beyond the largest piece
        for (int i = 0; i < 2; i++) {
            const hipError_t e = hipHostMalloc((void**)&R.pin[i], (size_t)S, hipHostMallocDefault);
            if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); R.pin[i] = nullptr; DGE_FAIL(DGE_ERR_CAP, "%s: two pinned buffers of %lld bytes do not fit", who, (long long)S); }
            DGE_HIP(e);
        }
        SEQ_TRY(seq_alloc(R, buf, (S + SEQ_CHUNK - 1) / SEQ_CHUNK * SEQ_CHUNK + SEQ_CHUNK, "the slab"));
        SEQ_TRY(seq_alloc(R, chunk_ends, S / SEQ_CHUNK + 2, "the chunk counts"));
        SEQ_TRY(seq_alloc(R, chunk_endx, S / SEQ_CHUNK + 2, "the chunk counts"));
        SEQ_TRY(seq_alloc(R, counters, TC_N, "the counters"));
        SEQ_TRY(cnt_stage(R, c, stage));
        D.rule = tab_rule{opt.sep, opt.key_field, opt.key_lo, opt.key_hi, opt.col_lo, opt.n_cols, opt.neg_col_offset >= 0 ? 1 : 0};
        D.ids = c->regions->d_id_by_rank; D.R = c->R; D.C = c->C; D.col_offset = opt.col_offset; D.neg_col_offset = opt.neg_col_offset;
        return DGE_OK;
    }

    int refuse(int kind, int32_t piece, int64_t offset, int64_t line, int64_t field) {
        char path[320] = "";
        if (R.pieces[(size_t)piece].path) snprintf(path, sizeof(path), " (%s)", R.pieces[(size_t)piece].path);
        DGE_FAIL(kind == TAB_BIG_VALUE ? DGE_ERR_RANGE : DGE_ERR_IO, "%s: %s at piece %d%s, offset %lld, line %lld, field %lld", who, TAB_KIND_NAME[kind], piece, path,
                 (long long)offset, (long long)line, (long long)field);
    }

    // The next slab and where it lies.  TripFeeder says neither; its counters do (seq_pieces.h names this reader above the struct).  `end` is where the bytes
    // taken from the piece, less the tail kept, end: the piece's size behind its last slab.  Of the bytes the call took — the tail it found and what it
    // read — all but at most one (the "\n" of a "\r\n" that the slab before halved) are in the slab or in the new tail, unless the feeder cut a line that
    // no buffer holds and dropped its rest: then far more than one byte is gone, the slab is that line's 65 536-byte stub, and it starts where the slab
    // before ended, or one byte on when the halved "\r\n"'s "\n" comes first — that byte is looked at.  Every other slab ends at `end`.
    int fill(TripFeeder& feed, TabCut& c) {
        using clock = std::chrono::steady_clock;
        const bool pending = feed.pending_cr;
        const int64_t at0 = feed.at, tail0 = feed.n_tail;
        const auto t0 = clock::now();
        SEQ_TRY(feed.next(R.pin[c.b], &c.n, &c.first, &c.open_end));
        info.read_ms += std::chrono::duration<double, std::milli>(clock::now() - t0).count();
        if (c.n == 0) return DGE_OK;
        c.piece = (int32_t)(feed.opens ? feed.k - 1 : feed.k);
        const SeqPiece& p = R.pieces[(size_t)c.piece];
        const int64_t end = feed.opens ? p.size : feed.at - feed.n_tail;
        const int64_t start = c.first ? 0 : at0 - tail0;              // where the bytes this call had to place begin
        const int64_t gone = end - start - c.n;
        if (gone < 0 || (!c.first && start != cursor))                // the feeder's counters no longer mean what this reader takes them to mean
            DGE_FAIL(DGE_ERR_STATE, "%s: a slab of piece %d does not lie behind the one before it (%lld bytes from %lld, the piece taken up to %lld)", who, c.piece, (long long)c.n,
                     (long long)start, (long long)end);
        c.long_cut = gone > 1;
        if (!c.long_cut) c.base = end - c.n;
        else {
            c.base = start;
            if (pending && !c.first) {
                uint8_t next = 0;
                if (p.mem) next = p.mem[c.base];
                else if (pread(p.fd, &next, 1, (off_t)c.base) != 1) DGE_FAIL(DGE_ERR_IO, "cannot read %s: %s", p.path, strerror(errno));
                if (next == '\n') c.base++;
            }
        }
        cursor = end;
        return DGE_OK;
    }

    int reserve(int64_t lines) {
        if (lines <= cap_lines) return DGE_OK;
        const int64_t c = std::max(lines, cap_lines * 2);
        SEQ_TRY(seq_alloc(R, line_end, c, "the lines' ends"));
        cap_lines = c;
        return DGE_OK;
    }

    // bytes to the device, lines found, the parse kernel launched; returns without waiting for it
    int submit(TabCut& s) {
        const int64_t n = s.n, n_chunks = (n + SEQ_CHUNK - 1) / SEQ_CHUNK;
        if (s.first) lines_in_piece = 0;
        s.lines_before = lines_in_piece;
        DGE_HIP(hipMemcpyAsync(buf.p, R.pin[s.b], (size_t)n, hipMemcpyHostToDevice, R.stream));
        DGE_HIP(hipMemsetAsync(buf.p + n, 0, (size_t)(n_chunks * SEQ_CHUNK + 32 - n), R.stream));
        unsigned long long zero[TC_N] = {TAB_NO_OFFENCE, 0, 0, 0, 0, 0};
        DGE_HIP(hipMemcpyAsync(counters.p, zero, sizeof(zero), hipMemcpyHostToDevice, R.stream));
        DGE_HIP(hipEventRecord(ea, R.stream));
        DGE_HIP(hipMemsetAsync(chunk_ends.p + n_chunks, 0, 8, R.stream));
        hipLaunchKernelGGL(k_tab_count, dim3((unsigned)n_chunks), dim3(SEQ_BLOCK), 0, R.stream, buf.p, chunk_ends.p);
        SEQ_TRY(seq_scan(R, chunk_ends.p, chunk_endx.p, n_chunks + 1));
        int64_t ends = 0;
        SEQ_TRY(seq_read_back(R, &ends, chunk_endx.p + n_chunks, 8));
        s.L = ends + (s.open_end ? 1 : 0);                           // (a slab holds a line at least: L >= 1)
        s.skip = (int32_t)std::min<int64_t>(std::max<int64_t>((int64_t)opt.skip_lines - s.lines_before, 0), s.L);
        lines_in_piece += s.L;
        SEQ_TRY(reserve(s.L));
        hipLaunchKernelGGL(k_tab_emit, dim3((unsigned)n_chunks), dim3(SEQ_BLOCK), 0, R.stream, buf.p, chunk_endx.p, (int32_t)n, s.L, s.open_end ? 1 : 0, line_end.p);
        if (s.L > s.skip)
            hipLaunchKernelGGL(k_tab_parse, dim3(seq_grid(s.L - s.skip)), dim3(SEQ_BLOCK), 0, R.stream, buf.p, (int32_t)n, line_end.p, s.L, s.skip, D, stage.p, counters.p);
        DGE_HIP(hipEventRecord(eb, R.stream));
        DGE_HIP(hipGetLastError());
        s.live = true;
        return DGE_OK;
    }

    // waits for the slab's kernels and reads what they counted
    int finish(TabCut& s) {
        if (!s.live) return DGE_OK;
        s.live = false;
        unsigned long long c[TC_N];
        SEQ_TRY(seq_read_back(R, c, counters.p, sizeof(c)));
        float ms = 0.f;
        DGE_HIP(hipEventElapsedTime(&ms, ea, eb));
        R.kernel_ms += ms;
        if (c[TC_OFFENCE] != TAB_NO_OFFENCE) {
            const int kind = (int)(c[TC_OFFENCE] & 15);
            const int64_t at = (int64_t)(c[TC_OFFENCE] >> 4);
            dge_tmp<int64_t> d_where;
            int64_t where[2] = {0, 0};
            SEQ_TRY(seq_alloc(R, d_where, 2, "a position"));
            hipLaunchKernelGGL(k_tab_where, dim3(1), dim3(1), 0, R.stream, buf.p, line_end.p, s.L, (int32_t)at, opt.sep, d_where.p);
            SEQ_TRY(seq_read_back(R, where, d_where.p, sizeof(where)));
            return refuse(kind, s.piece, s.base + at, s.lines_before + where[0] + 1, where[1]);
        }
        info.lines += s.L; info.skipped += s.skip; info.slabs++;
        info.rows += (int64_t)c[TC_ROWS]; info.empty += (int64_t)c[TC_EMPTY]; info.foreign += (int64_t)c[TC_FOREIGN];
        total += ((unsigned __int128)c[TC_SUM_HI] << 20) + c[TC_SUM_LO];
        if (total > (unsigned __int128)CNT_MAX_CELL) DGE_FAIL(DGE_ERR_RANGE, "%s: the values add up to more than 2^62", who);
        return DGE_OK;
    }

    int run() {
        TripFeeder feed{R.pieces, S};
        TabCut cut[2];
        cut[0].b = 0; cut[1].b = 1;
        SEQ_TRY(fill(feed, cut[0]));
        for (int64_t k = 0; cut[k & 1].n > 0; k++) {
            TabCut& c = cut[k & 1];
            // a line the feeder cut is a long line at the slab's first byte, unless it is one of the piece's headers: those are not looked at, and its stub goes the slab's way
            if (c.long_cut && (c.first ? 0 : lines_in_piece) >= opt.skip_lines) return refuse(TAB_LONG_LINE, c.piece, c.base, (c.first ? 0 : lines_in_piece) + 1, 0);
            SEQ_TRY(submit(c));
            SEQ_TRY(fill(feed, cut[(k + 1) & 1]));                   // (the host reads slab k + 1 while slab k is in its kernels)
            SEQ_TRY(finish(c));
        }
        info.values = info.rows * opt.n_cols;
        info.total = (int64_t)total;
        info.kernel_ms = R.kernel_ms;
        return DGE_OK;
    }
};

int tab_check(const char* who, const dge_counts* c, const void* pieces, const int64_t* n_bytes, bool texts, int32_t n_pieces, const dge_table_read_options* opt) {
    if (!c || !pieces || (texts && !n_bytes) || !opt || n_pieces < 0) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    if (n_pieces < 1) DGE_FAIL(DGE_ERR_ARG, "%s: n_pieces %d: one piece at least is needed", who, n_pieces);
    if (opt->sep != ',' && opt->sep != ' ' && opt->sep != '\t') DGE_FAIL(DGE_ERR_ARG, "%s: sep %d is none of ',', ' ' and a tab", who, opt->sep);
    if (opt->reserved != 0 || opt->reserved2 != 0) DGE_FAIL(DGE_ERR_ARG, "%s: a reserved field of the options is not 0", who);
    if (opt->skip_lines < 0) DGE_FAIL(DGE_ERR_ARG, "%s: skip_lines %d is negative", who, opt->skip_lines);
    if (opt->key_field < 0 || opt->key_lo < 0 || opt->key_hi < 0 || (opt->key_hi != 0 && opt->key_hi <= opt->key_lo) || opt->key_lo > TAB_MAX_LINE || opt->key_hi > TAB_MAX_LINE)
        DGE_FAIL(DGE_ERR_ARG, "%s: key_field %d, key_lo %d, key_hi %d: none may be negative, key_hi is 0 or above key_lo, and neither goes beyond a line's %d bytes", who,
                 opt->key_field, opt->key_lo, opt->key_hi, TAB_MAX_LINE);
    if (opt->col_lo < 0 || opt->n_cols < 1 || opt->n_cols > TAB_MAX_COLS || opt->col_lo > 0x7fffffff - opt->n_cols)
        DGE_FAIL(DGE_ERR_ARG, "%s: col_lo %d, n_cols %d: col_lo >= 0 and 1 <= n_cols <= %d are needed", who, opt->col_lo, opt->n_cols, TAB_MAX_COLS);
    if (opt->key_field >= opt->col_lo && opt->key_field < opt->col_lo + opt->n_cols) DGE_FAIL(DGE_ERR_ARG, "%s: key_field %d lies among the value fields", who, opt->key_field);
    if (opt->col_offset < 0 || opt->neg_col_offset < -1) DGE_FAIL(DGE_ERR_ARG, "%s: col_offset %d, neg_col_offset %d: a column, or -1 for the second", who, opt->col_offset, opt->neg_col_offset);
    if (opt->slab_bytes < 0 || (opt->slab_bytes > 0 && opt->slab_bytes < TAB_SLAB_MIN))
        DGE_FAIL(DGE_ERR_ARG, "%s: slab_bytes %lld is neither 0 nor at least %lld", who, (long long)opt->slab_bytes, (long long)TAB_SLAB_MIN);
    return DGE_OK;
}

// the handle's part of the checks
int tab_check_handle(const char* who, const dge_counts* c, const dge_table_read_options* opt) {
    if (opt->col_offset > c->C - opt->n_cols || (opt->neg_col_offset >= 0 && opt->neg_col_offset > c->C - opt->n_cols))
        DGE_FAIL(DGE_ERR_ARG, "%s: %d columns from col_offset %d or neg_col_offset %d leave the table's %d columns", who, opt->n_cols, opt->col_offset, opt->neg_col_offset, c->C);
    return DGE_OK;
}

int tab_into_counts(TabReader& T, dge_counts* c, dge_table_read_info* info) {
    SEQ_TRY(T.open(c));
    SEQ_TRY(T.run());
    SEQ_TRY(cnt_commit(T.R, c, T.stage.p, T.who));
    if (info) *info = T.info;
    return DGE_OK;
}

void tab_configure(TabReader& T, const char* who, const dge_table_read_options* opt) {
    T.who = who; T.opt = *opt;
    T.S = opt->slab_bytes == 0 ? TAB_SLAB_DEFAULT : std::min(opt->slab_bytes, TAB_SLAB_MAX);
}

}  // namespace

// ------------------------------------------------------------------------------------------ entries
extern "C" int dge_counts_create(const dge_regions* rg, int32_t n_cols, dge_counts** out) {
    const char* who = "dge_counts_create";
    if (!out || !rg) DGE_FAIL(DGE_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    if (n_cols < 1 || n_cols > TAB_MAX_COLS) DGE_FAIL(DGE_ERR_ARG, "%s: n_cols %d: 1 .. %d is needed", who, n_cols, TAB_MAX_COLS);
    SEQ_TRY(dge_require_device(rg->device));
    std::unique_ptr<dge_counts> c(new dge_counts());
    c->device = rg->device; c->R = rg->R; c->C = n_cols;
    const hipError_t e = hipMalloc((void**)&c->d.p, (size_t)std::max<int64_t>(c->R * c->C, 1) * 8);
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); c->d.p = nullptr; DGE_FAIL(DGE_ERR_CAP, "%s: a table of %lld x %d cells does not fit in device memory", who, (long long)c->R, n_cols); }
    DGE_HIP(e);
    DGE_HIP(hipMemset(c->d.p, 0, (size_t)std::max<int64_t>(c->R * c->C, 1) * 8));
    DGE_HIP(hipDeviceSynchronize());
    c->regions = const_cast<dge_regions*>(rg);
    c->regions->refs.fetch_add(1);
    *out = c.release();
    return DGE_OK;
}

extern "C" void dge_counts_destroy(dge_counts* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

extern "C" int dge_counts_info(const dge_counts* c, struct dge_counts_info* out) {
    const char* who = "dge_counts_info";
    if (!c || !out) DGE_FAIL(DGE_ERR_ARG, "%s: null argument", who);
    SEQ_TRY(dge_require_device(c->device));
    SeqRun R;
    SEQ_TRY(seq_open(R, c->device, who));
    dge_tmp<unsigned long long> d;
    unsigned long long h[3] = {0, 0, 0};
    SEQ_TRY(seq_alloc(R, d, 3, "the counters"));
    DGE_HIP(hipMemsetAsync(d.p, 0, sizeof(h), R.stream));
    const int64_t n = c->R * c->C;
    if (n) hipLaunchKernelGGL(k_cnt_info, dim3(seq_grid(n)), dim3(SEQ_BLOCK), 0, R.stream, c->d.p, n, d.p);
    SEQ_TRY(seq_read_back(R, h, d.p, sizeof(h)));
    const unsigned __int128 total = ((unsigned __int128)h[1] << 20) + h[2];
    out->regions = c->R; out->cols = c->C; out->nonzero = (int64_t)h[0];
    out->total = total > (unsigned __int128)INT64_MAX ? INT64_MAX : (int64_t)total;
    return DGE_OK;
}

extern "C" int dge_counts_to_host(const dge_counts* c, int64_t* out) {
    if (!c || (c->R * c->C > 0 && !out)) DGE_FAIL(DGE_ERR_ARG, "dge_counts_to_host: null argument");
    SEQ_TRY(dge_require_device(c->device));
    if (c->R * c->C) DGE_HIP(hipMemcpy(out, c->d.p, (size_t)(c->R * c->C) * 8, hipMemcpyDeviceToHost));
    return DGE_OK;
}

extern "C" int dge_counts_add_entries(dge_counts* c, const int32_t* row, const int32_t* col, const int64_t* value, int64_t n) {
    const char* who = "dge_counts_add_entries";
    if (!c || n < 0 || (n > 0 && (!row || !col || !value))) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    unsigned __int128 total = 0;
    for (int64_t i = 0; i < n; i++) {
        if (row[i] < 0 || row[i] >= c->R || col[i] < 0 || col[i] >= c->C || value[i] < 0 || value[i] > (int64_t)TAB_MAX_VALUE)
            DGE_FAIL(DGE_ERR_ARG, "%s: entry %lld is (row %d, col %d, value %lld): rows 0 .. %lld, columns 0 .. %d, values 0 .. 2^40", who, (long long)i, row[i], col[i],
                     (long long)value[i], (long long)c->R - 1, c->C - 1);
        total += (unsigned __int128)value[i];
    }
    if (total > (unsigned __int128)CNT_MAX_CELL) DGE_FAIL(DGE_ERR_RANGE, "%s: the values add up to more than 2^62", who);
    if (n == 0) return DGE_OK;
    SEQ_TRY(dge_require_device(c->device));
    SeqRun R;
    SEQ_TRY(seq_open(R, c->device, who));
    dge_tmp<int32_t> d_row, d_col;
    dge_tmp<int64_t> d_val;
    dge_tmp<unsigned long long> stage;
    SEQ_TRY(cnt_stage(R, c, stage));
    SEQ_TRY(cnt_upload(R, d_row, row, n, "the entries' rows"));
    SEQ_TRY(cnt_upload(R, d_col, col, n, "the entries' columns"));
    SEQ_TRY(cnt_upload(R, d_val, value, n, "the entries' values"));
    hipLaunchKernelGGL(k_cnt_entries, dim3(seq_grid(n)), dim3(SEQ_BLOCK), 0, R.stream, d_row.p, d_col.p, d_val.p, n, c->C, stage.p);
    DGE_HIP(hipGetLastError());
    return cnt_commit(R, c, stage.p, who);
}

extern "C" int dge_counts_add_table_texts(dge_counts* c, const char* const* texts, const int64_t* n_bytes, int32_t n_pieces, const dge_table_read_options* opt, dge_table_read_info* info) {
    const char* who = "dge_counts_add_table_texts";
    SEQ_TRY(tab_check(who, c, texts, n_bytes, true, n_pieces, opt));
    SEQ_TRY(seq_check_texts(texts, n_bytes, n_pieces, who));
    SEQ_TRY(tab_check_handle(who, c, opt));
    SEQ_TRY(dge_require_device(c->device));
    TabReader T;
    tab_configure(T, who, opt);
    SEQ_TRY(seq_add_texts(T.R.pieces, texts, n_bytes, n_pieces, who));
    return tab_into_counts(T, c, info);
}

extern "C" int dge_counts_add_table_files(dge_counts* c, const char* const* paths, int32_t n_pieces, const dge_table_read_options* opt, dge_table_read_info* info) {
    const char* who = "dge_counts_add_table_files";
    SEQ_TRY(tab_check(who, c, paths, nullptr, false, n_pieces, opt));
    SEQ_TRY(seq_check_paths(paths, n_pieces, who));
    SEQ_TRY(tab_check_handle(who, c, opt));
    SEQ_TRY(dge_require_device(c->device));
    TabReader T;
    tab_configure(T, who, opt);
    SEQ_TRY(seq_add_files(T.R.pieces, paths, n_pieces, who));
    return tab_into_counts(T, c, info);
}

extern "C" int dge_counts_add_points(dge_counts* c, const double* xy, const int32_t* col, int64_t n, int64_t* dropped) {
    const char* who = "dge_counts_add_points";
    if (!c || n < 0 || (n > 0 && (!xy || !col))) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    for (int64_t i = 0; i < n; i++)
        if (col[i] < 0 || col[i] >= c->C) DGE_FAIL(DGE_ERR_ARG, "%s: point %lld has column %d: 0 .. %d is needed", who, (long long)i, col[i], c->C - 1);
    if (dropped) *dropped = 0;
    if (n == 0) return DGE_OK;
    SEQ_TRY(dge_require_device(c->device));
    SeqRun R;
    SEQ_TRY(seq_open(R, c->device, who));
    dge_tmp<double> d_xy;
    dge_tmp<int32_t> d_col, d_region;
    dge_tmp<unsigned long long> stage;
    dge_locate_info li = {};
    SEQ_TRY(cnt_stage(R, c, stage));
    SEQ_TRY(cnt_upload(R, d_xy, xy, 2 * n, "the points"));
    SEQ_TRY(cnt_upload(R, d_col, col, n, "the points' columns"));
    SEQ_TRY(seq_alloc(R, d_region, n, "the points' regions"));
    DGE_HIP(hipStreamSynchronize(R.stream));
    SEQ_TRY(dge_regions_locate_device(c->regions, d_xy.p, n, d_region.p, &li));
    hipLaunchKernelGGL(k_cnt_points, dim3(seq_grid(n)), dim3(SEQ_BLOCK), 0, R.stream, d_region.p, c->regions->d_idrank, d_col.p, n, c->C, stage.p);
    DGE_HIP(hipGetLastError());
    SEQ_TRY(cnt_commit(R, c, stage.p, who));
    if (dropped) *dropped = n - li.located;
    return DGE_OK;
}

extern "C" int dge_counts_merge(const dge_counts* c, const dge_regions* groups, const int32_t* group_of, dge_counts** out) {
    const char* who = "dge_counts_merge";
    if (!out) DGE_FAIL(DGE_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    if (!c || !groups || (c->R > 0 && !group_of)) DGE_FAIL(DGE_ERR_ARG, "%s: null argument", who);
    if (groups->device != c->device) DGE_FAIL(DGE_ERR_ARG, "%s: the table lies on device %d, the groups on device %d", who, c->device, groups->device);
    const int64_t G = groups->R;
    std::vector<int64_t> first((size_t)G + 1, 0);
    for (int64_t i = 0; i < c->R; i++) {
        if (group_of[i] < -1 || group_of[i] >= G) DGE_FAIL(DGE_ERR_ARG, "%s: group_of[%lld] is %d: -1 .. %lld is needed", who, (long long)i, group_of[i], (long long)G - 1);
        if (group_of[i] >= 0) first[(size_t)group_of[i] + 1]++;
    }
    for (int64_t g = 0; g < G; g++) first[(size_t)g + 1] += first[(size_t)g];
    std::vector<int32_t> member((size_t)first[(size_t)G]);
    std::vector<int64_t> next(first.begin(), first.end() - 1);
    for (int64_t i = 0; i < c->R; i++) if (group_of[i] >= 0) member[(size_t)next[(size_t)group_of[i]]++] = (int32_t)i;
    dge_counts* m = nullptr;
    SEQ_TRY(dge_counts_create(groups, c->C, &m));
    std::unique_ptr<dge_counts, void (*)(dge_counts*)> guard(m, dge_counts_destroy);
    if (G == 0) { *out = guard.release(); return DGE_OK; }
    SeqRun R;
    SEQ_TRY(seq_open(R, c->device, who));
    dge_tmp<int64_t> d_first;
    dge_tmp<int32_t> d_member, over;
    int32_t flag = 0;
    SEQ_TRY(cnt_upload(R, d_first, first.data(), G + 1, "the groups' rows"));
    SEQ_TRY(cnt_upload(R, d_member, member.data(), (int64_t)member.size(), "the groups' rows"));
    SEQ_TRY(seq_alloc(R, over, 1, "a flag"));
    DGE_HIP(hipMemsetAsync(over.p, 0, 4, R.stream));
    hipLaunchKernelGGL(k_cnt_merge, dim3(seq_grid(G * c->C)), dim3(SEQ_BLOCK), 0, R.stream, c->d.p, c->C, d_first.p, d_member.p, G, m->d.p, over.p);
    DGE_HIP(hipGetLastError());
    SEQ_TRY(seq_read_back(R, &flag, over.p, 4));
    if (flag) DGE_FAIL(DGE_ERR_RANGE, "%s: a cell would stand above 2^62", who);
    *out = guard.release();
    return DGE_OK;
}

extern "C" int dge_counts_vectors(const dge_counts* c, int32_t col_lo, int32_t n_cols, int32_t normalise, int32_t present_mode, dge_vectors** out) {
    const char* who = "dge_counts_vectors";
    if (!out) DGE_FAIL(DGE_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    if (!c) DGE_FAIL(DGE_ERR_ARG, "%s: null argument", who);
    if (present_mode != DGE_COUNTS_PRESENT_ALL && present_mode != DGE_COUNTS_PRESENT_NONZERO) DGE_FAIL(DGE_ERR_ARG, "%s: present_mode %d is none of ALL and NONZERO", who, present_mode);
    if (col_lo < 0 || n_cols < 1 || col_lo > c->C - n_cols) DGE_FAIL(DGE_ERR_ARG, "%s: columns %d .. %d + %d leave the table's %d columns", who, col_lo, col_lo, n_cols, c->C);
    SEQ_TRY(dge_require_device(c->device));
    std::unique_ptr<dge_vectors> v(new dge_vectors());
    v->device = c->device; v->rows = c->R; v->dim = n_cols;
    SEQ_TRY(v->d.alloc((size_t)c->R * (size_t)n_cols));
    SEQ_TRY(v->d_present.alloc((size_t)c->R));
    if (c->R > 0) {
        SeqRun R;
        SEQ_TRY(seq_open(R, c->device, who));
        dge_tmp<unsigned long long> sum;
        SEQ_TRY(seq_alloc(R, sum, c->R, "the rows' sums"));
        hipLaunchKernelGGL(k_cnt_row_sums, dim3((unsigned)c->R), dim3(SEQ_BLOCK), 0, R.stream, c->d.p, c->C, col_lo, n_cols, sum.p);
        hipLaunchKernelGGL(k_cnt_vectors, dim3(seq_grid(c->R * n_cols)), dim3(SEQ_BLOCK), 0, R.stream, c->d.p, c->C, col_lo, n_cols, c->R, sum.p, normalise, present_mode, v->d.p,
                           v->d_present.p);
        DGE_HIP(hipGetLastError());
        std::vector<unsigned long long> h((size_t)c->R);
        SEQ_TRY(seq_read_back(R, h.data(), sum.p, (size_t)c->R * 8));
        for (int64_t r = 0; r < c->R; r++) {
            if (h[(size_t)r] > (unsigned long long)INT64_MAX) DGE_FAIL(DGE_ERR_RANGE, "%s: the selected columns of row %lld add up to more than 2^63 - 1", who, (long long)r);
            v->n_present += present_mode == DGE_COUNTS_PRESENT_ALL || h[(size_t)r] != 0 ? 1 : 0;
        }
    }
    *out = v.release();
    return DGE_OK;
}
