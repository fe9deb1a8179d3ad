// od_read.hip — .od flow text in, a layered graph out (include/dge.h: dge_graph_add_od_files / _texts, dge_graph_regions).
//
// One "src dst w" line per flow, one piece (a file or a text) per time slice; the rule of the graph is that of embedding_amd/io.py: read_od_slices
// (J/CrossTimeGraph.java:25-52,68-95).  The host only moves bytes, finishes the few weight tokens the device routine hands back, formats the vertex names
// and hands the layer-0 vertices to dge_graph_set_sources; the edges never visit it.  Outside the build stamp: nothing here is read or written by a
// training launch.
//
// The passes, on the one buffer of seq_tokens.h (every piece with its pad byte):
//   seq_tokenise               token t's first byte and line, the rows (rowx, row_first) — the .seq reader's kernels and chunk transport, unchanged
//   k_seq_ragged               every row must have 3 tokens
//   k_od_parse                 a lane per row: its piece (= slice), od_parse.h's integer routines -> src id, dst id, the weight's bits; "not mine" weights flagged
//   host path                  seq_pick / seq_tokens_to_host / seq_host_numbers (seq_tokens.h): the flagged tokens' bytes in one blob, strtod in the "C"
//                              locale; k_od_scatter puts the bits in place
//   k_od_keep                  a weight that is not finite is a bad token; keep[r] = w > 0
//   scan of keep               a stable compaction: kept flow r is edge keepx[r], edges stand in text order
//   od_commit.h, which dge_graph_add_flows (trip_map.hip) runs too:
//   k_od_endpoints, radix sort, k_od_unique around a scan
//                              the kept endpoints' ids sorted as signed 64-bit integers, each distinct one once: the R regions, ascending
//   k_od_edges                 rank by binary search -> the COO staging the graph takes over (dge_graph_adopt_coo), edge h*R + rank(src) -> ((h+1) % T)*R + rank(dst);
//                              marks the layer-0 endpoints
//   k_od_sources around a scan the marked layer-0 vertices, ascending
// Every error is the LEAST position of its kind, found with atomicMin on a row or a byte offset: which lane gets there first does not matter.
//
// Coherence: no protocol.  Every array is written by one kernel and read by later ones on the same stream; the only words several lanes write are the error
// minima (atomicMin), the host-token counter (atomicAdd) and mark[] (every writer stores 1).
//
// What bounds the per-row kernel: a row is three tokens, known from the ragged pass, so a lane touches exactly its own three tokens' bytes.  A token ends at a
// whitespace byte and the buffer ends in SEQ_TAIL blanks, so the byte loops stop inside the allocation; their length is the token's.  Lanes of a wave hold
// adjacent lines (~20 bytes each), so their reads fall into the same few cache lines; divergence is over the digits of a token (ids 5-6, weights 1-4 in
// the reference's files), and the division loop of od_parse_f64 has a fixed trip count.
#include "od_commit.h"
#include "od_parse.h"
#include "seq_tokens.h"

// ------------------------------------------------------------------------------------------ kernels
// row r = tokens row_first[r] .. + 2 (the ragged pass has run).  status[r]: 1 = the host finishes the weight.  bad_at: least offset of a malformed token
__global__ void __launch_bounds__(SEQ_BLOCK) k_od_parse(const uint8_t* buf, const int64_t* tok_start, const int64_t* row_first, int64_t rows, const int64_t* piece_off,
                                                        int64_t n_pieces, int64_t* src_id, int64_t* dst_id, uint64_t* w_bits, int32_t* slice, uint8_t* status,
                                                        unsigned long long* bad_at, unsigned long long* n_host) {
    typedef hipcub::BlockReduce<unsigned long long, SEQ_BLOCK> Reduce;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t r = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    unsigned long long for_host = 0;
    if (r < rows) {
        const int64_t t = row_first[r];
        const int64_t at[3] = {tok_start[t], tok_start[t + 1], tok_start[t + 2]};
        int64_t id[2] = {0, 0};
        for (int i = 0; i < 2; i++) {
            const uint8_t* p = buf + at[i];
            if (!od_parse_id(p, seq_tok_len(p), &id[i])) atomicMin(bad_at, (unsigned long long)at[i]);
        }
        const uint8_t* p = buf + at[2];
        uint64_t bits = 0;
        const int rc = od_parse_f64(p, seq_tok_len(p), &bits);
        if (rc == VEC_PARSE_BAD) atomicMin(bad_at, (unsigned long long)at[2]);
        for_host = rc == VEC_PARSE_HOST ? 1 : 0;
        src_id[r] = id[0]; dst_id[r] = id[1]; w_bits[r] = bits;
        slice[r] = (int32_t)seq_piece_of(piece_off, n_pieces, at[0]);
        status[r] = (uint8_t)for_host;
    }
    const unsigned long long sum = Reduce(tmp).Sum(for_host);
    if (threadIdx.x == 0 && sum) atomicAdd(n_host, sum);
}

struct OdHostStart {     // host token k: the weight, the third token, of row host_row[k]
    const int64_t* tok_start; const int64_t* row_first; const int64_t* host_row;
    __device__ int64_t operator()(int64_t k) const { return tok_start[row_first[host_row[k]] + 2]; }
};

__global__ void __launch_bounds__(SEQ_BLOCK) k_od_scatter(const int64_t* host_row, const uint64_t* host_bits, int64_t n, uint64_t* w_bits) {
    const int64_t k = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (k < n) w_bits[host_row[k]] = host_bits[k];
}

// a weight that is not finite (inf, nan, overflow — decided here or by strtod) is a bad token; a flow is kept when its weight is > 0
__global__ void __launch_bounds__(SEQ_BLOCK) k_od_keep(const uint64_t* w_bits, const int64_t* tok_start, const int64_t* row_first, int64_t rows, uint8_t* keep,
                                                       unsigned long long* bad_at) {
    const int64_t r = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (r >= rows) return;
    const uint64_t b = w_bits[r], mag = b & 0x7FFFFFFFFFFFFFFFull;
    if (mag >= 0x7FF0000000000000ull) atomicMin(bad_at, (unsigned long long)tok_start[row_first[r] + 2]);
    keep[r] = (b >> 63) == 0 && mag != 0 ? 1 : 0;
}

// ------------------------------------------------------------------------------------------ host side of one read
namespace {

int od_read(SeqRun& R, dge_graph* g, dge_names* names, dge_od_info* info, const char* who) {
    R.what = "od read";
    SEQ_TRY(seq_tokenise(R, nullptr, who));
    const int64_t rows = R.rows, T = (int64_t)R.pieces.size();
    // words: [0] ragged row, [1] malformed token (offset), [2] host tokens
    dge_tmp<unsigned long long> words;
    unsigned long long w[3] = {~0ull, ~0ull, 0ull};
    SEQ_TRY(seq_alloc(R, words, 3, "the counters"));
    DGE_HIP(hipMemcpyAsync(words.p, w, sizeof(w), hipMemcpyHostToDevice, R.stream));
    SEQ_TRY(seq_kernels_begin(R));
    if (rows) hipLaunchKernelGGL(k_seq_ragged, dim3(seq_grid(rows)), dim3(SEQ_BLOCK), 0, R.stream, R.row_first.p, (const uint8_t*)nullptr, rows, (int64_t)3, words.p);
    SEQ_TRY(seq_kernels_end(R));
    SEQ_TRY(seq_read_back(R, w, words.p, 8));
    if (w[0] != ~0ull) {
        int64_t at = 0, count = 0;
        SEQ_TRY(seq_row_where(R, (int64_t)w[0], &at, &count));
        DGE_FAIL(DGE_ERR_IO, "%s: the line at %s has %lld token%s where 3 are expected: src dst w", who, seq_where(R, at).c_str(), (long long)count, count == 1 ? "" : "s");
    }

    // ---- the flows: two ids, a weight, the slice
    dge_tmp<int64_t> piece_off, src_id, dst_id, keepx;
    dge_tmp<uint64_t> w_bits;
    dge_tmp<int32_t> slice;
    dge_tmp<uint8_t> status, keep;
    SEQ_TRY(seq_alloc(R, piece_off, T, "the pieces"));
    SEQ_TRY(seq_alloc(R, src_id, rows, "the flows' sources"));
    SEQ_TRY(seq_alloc(R, dst_id, rows, "the flows' destinations"));
    SEQ_TRY(seq_alloc(R, w_bits, rows, "the flows' weights"));
    SEQ_TRY(seq_alloc(R, slice, rows, "the flows' slices"));
    SEQ_TRY(seq_alloc(R, status, rows, "the weights' states"));
    SEQ_TRY(seq_alloc(R, keep, rows, "the kept flows"));
    SEQ_TRY(seq_alloc(R, keepx, rows + 1, "the kept flows' numbers"));
    DGE_HIP(hipMemcpyAsync(piece_off.p, R.L.offset.data(), (size_t)T * 8, hipMemcpyHostToDevice, R.stream));
    SEQ_TRY(seq_kernels_begin(R));
    if (rows) hipLaunchKernelGGL(k_od_parse, dim3(seq_grid(rows)), dim3(SEQ_BLOCK), 0, R.stream, R.buf.p, R.tok_start.p, R.row_first.p, rows, piece_off.p, T, src_id.p, dst_id.p,
                                 w_bits.p, slice.p, status.p, words.p + 1, words.p + 2);
    SEQ_TRY(seq_kernels_end(R));
    SEQ_TRY(seq_read_back(R, w + 2, words.p + 2, 8));

    // ---- the host path: the flagged weights' bytes in one blob, strtod, the bits back into place
    const int64_t n_host = (int64_t)w[2];
    if (n_host > 0) {
        dge_tmp<int64_t> host_row;
        dge_tmp<uint64_t> host_bits;
        std::vector<int64_t> off;
        std::unique_ptr<char[]> text;
        std::vector<uint64_t> bits;
        SEQ_TRY(seq_alloc(R, host_bits, n_host, "the host tokens' values"));
        SEQ_TRY(seq_kernels_begin(R));
        SEQ_TRY(seq_pick(R, status.p, rows, n_host, host_row, "the host tokens"));
        SEQ_TRY(seq_tokens_to_host(R, OdHostStart{R.tok_start.p, R.row_first.p, host_row.p}, n_host, off, text, "the host tokens"));
        SEQ_TRY(seq_host_numbers(text.get(), off.data(), n_host, bits, who));
        DGE_HIP(hipMemcpyAsync(host_bits.p, bits.data(), (size_t)n_host * 8, hipMemcpyHostToDevice, R.stream));
        SEQ_TRY(seq_kernels_begin(R));
        hipLaunchKernelGGL(k_od_scatter, dim3(seq_grid(n_host)), dim3(SEQ_BLOCK), 0, R.stream, host_row.p, host_bits.p, n_host, w_bits.p);
        SEQ_TRY(seq_kernels_end(R));
    }

    // ---- the kept flows, numbered in text order
    SEQ_TRY(seq_kernels_begin(R));
    if (rows) hipLaunchKernelGGL(k_od_keep, dim3(seq_grid(rows)), dim3(SEQ_BLOCK), 0, R.stream, w_bits.p, R.tok_start.p, R.row_first.p, rows, keep.p, words.p + 1);
    SEQ_TRY(seq_scan(R, rocprim::make_transform_iterator(rocprim::counting_iterator<int64_t>(0), SeqByteFlag{keep.p, rows}), keepx.p, rows + 1));
    SEQ_TRY(seq_kernels_end(R));
    SEQ_TRY(seq_read_back(R, w + 1, words.p + 1, 8));
    if (w[1] != ~0ull)
        DGE_FAIL(DGE_ERR_IO, "%s: the token at %s is not a region id ([+-] digits, an int64) or not a weight (a finite decimal number)", who, seq_where(R, (int64_t)w[1]).c_str());
    int64_t E = 0;
    SEQ_TRY(seq_read_back(R, &E, keepx.p + rows, 8));
    seq_release(R, status, rows);
    seq_release(R, keep, rows);

    int64_t Rn = 0, S = 0;
    SEQ_TRY(od_commit(R, g, names, rows, E, T, src_id.p, dst_id.p, w_bits.p, slice.p, keepx.p, who, &Rn, &S));
    if (info) {
        info->bytes = R.L.text_bytes; info->lines = R.lines; info->flows = rows; info->edges = E; info->dropped = rows - E; info->regions = Rn; info->sources = S;
        info->host_values = n_host; info->slices = (int32_t)T; info->reserved = 0; info->read_ms = R.read_ms; info->kernel_ms = R.kernel_ms;
    }
    return DGE_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------ entries
extern "C" int dge_graph_add_od_texts(dge_graph* g, const char* const* texts, const int64_t* n_bytes, int32_t n_slices, dge_names* names, dge_od_info* info) {
    if (!g || !texts || !n_bytes || n_slices < 1) DGE_FAIL(DGE_ERR_ARG, "dge_graph_add_od_texts: null or negative argument, or fewer than 1 slice");
    SEQ_TRY(seq_check_texts(texts, n_bytes, n_slices, "dge_graph_add_od_texts"));
    SEQ_TRY(od_check(g, names, "dge_graph_add_od_texts"));
    SEQ_TRY(dge_require_device(g->device));
    SeqRun R;
    R.device = g->device;
    SEQ_TRY(seq_add_texts(R.pieces, texts, n_bytes, n_slices, "dge_graph_add_od_texts"));
    return od_read(R, g, names, info, "dge_graph_add_od_texts");
}

extern "C" int dge_graph_add_od_files(dge_graph* g, const char* const* paths, int32_t n_slices, dge_names* names, dge_od_info* info) {
    if (!g || !paths || n_slices < 1) DGE_FAIL(DGE_ERR_ARG, "dge_graph_add_od_files: null or negative argument, or fewer than 1 slice");
    SEQ_TRY(seq_check_paths(paths, n_slices, "dge_graph_add_od_files"));
    SEQ_TRY(od_check(g, names, "dge_graph_add_od_files"));
    SEQ_TRY(dge_require_device(g->device));
    SeqRun R;
    R.device = g->device;
    SEQ_TRY(seq_add_files(R.pieces, paths, n_slices, "dge_graph_add_od_files"));
    return od_read(R, g, names, info, "dge_graph_add_od_files");
}

extern "C" int dge_graph_regions(const dge_graph* g, int64_t* regions, int64_t cap, int64_t* n) {
    if (!g || !n || cap < 0 || (cap > 0 && !regions)) DGE_FAIL(DGE_ERR_ARG, "dge_graph_regions: null or negative argument");
    *n = (int64_t)g->od_regions.size();
    if (cap < *n) DGE_FAIL(DGE_ERR_CAP, "dge_graph_regions: %lld regions exceed cap %lld", (long long)*n, (long long)cap);
    if (*n) memcpy(regions, g->od_regions.data(), (size_t)*n * 8);
    return DGE_OK;
}
