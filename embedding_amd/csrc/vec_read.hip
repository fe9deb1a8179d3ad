// vec_read.hip — .vec text in, resident float32 rows aligned by name out (include/dge.h: dge_vectors_from_vec_text / _files and the dge_vectors_* entries).
//
// The mirror image of dge_write_vec (sgns_io.hip): "name v1 .. vD" per line, optionally a "V D" line in front of every file.  The host only moves bytes and
// finishes the few value tokens the device routine hands back.  Outside the build stamp: nothing here is read or written by a training launch.
//
// The passes, on the one buffer of seq_tokens.h (prior names as its leading lines, then every piece with its pad byte):
//   seq_tokenise               token t's first byte and line, the rows (rowx, row_first) — the .seq reader's kernels and chunk transport, unchanged
//   k_vec_mark                 per row: its piece; with header != 0 the first row of a piece is its "V D" line, checked and read here
//   k_seq_ragged               every other row must have dim + 1 tokens (dim: the first such row's); the header lines are its skip mask
//   k_vec_entries + seq_intern only the token that OPENS a row is a name: the prior names and those tokens — 1 token in dim + 1 — are the entries the
//                              .seq reader's k_seq_hash / k_seq_intern / ids passes run on.  Entry order is text order, so ids are first-appearance ids.
//   k_vec_parse                a lane per value token: vec_parse.h's integer routine -> out[id(row) * dim + column]; "not mine" tokens are flagged
//   k_vec_first_row / _dups    a row is a duplicate when its name opened an earlier ROW: when the string's first appearance is an earlier row, or, for a
//                              name the caller already held (first appearance among the prior names), when it is not the least row with that name
//   host path                  seq_pick / seq_tokens_to_host / seq_host_numbers (seq_tokens.h): the flagged tokens' bytes in one blob, as the new names',
//                              strtof in the "C" locale; k_vec_scatter puts the bits in place
// Every error is the LEAST position of its kind, found with atomicMin on a row, an entry or a byte offset: which lane gets there first does not matter.
// Absent rows are the zero fill of the result; present[] is written by the lane of the row's name.
//
// Coherence: the intern pass is the .seq reader's, on entries instead of tokens, and the argument at the head of seq_tokens.h carries
// over unchanged — slots are claimed once and only lowered, by agent-scope read-modify-writes, and everything else the pass reads was written by earlier
// kernels.  No second protocol: every other array here is written by one kernel and read by later ones on the same stream; out[] and present[] are
// written at most once per element unless a name opens two rows (a new name or a prior one), in which case k_vec_dups finds the second row, the call
// fails and the result is discarded.
#include "seq_tokens.h"
#include "vec_parse.h"

// ------------------------------------------------------------------------------------------ kernels
// an unsigned decimal integer of up to 18 digits (more: INT64_MAX, which equals no count); -1: not one
__device__ __forceinline__ int64_t vec_uint(const uint8_t* p) {
    const int64_t len = seq_tok_len(p);
    int64_t v = 0;
    for (int64_t i = 0; i < len; i++) {
        const uint32_t d = (uint32_t)p[i] - '0';
        if (d > 9u) return -1;
        v = i < 18 ? v * 10 + d : INT64_MAX;
    }
    return v;
}

__global__ void __launch_bounds__(SEQ_BLOCK) k_vec_mark(const uint8_t* buf, const int64_t* tok_start, const int64_t* row_first, int64_t rows, const int64_t* piece_off,
                                                        int64_t n_pieces, int header, uint8_t* is_hdr, int64_t* piece_first, int64_t* hdr_v, int64_t* hdr_d,
                                                        unsigned long long* bad_hdr, unsigned long long* first_data) {
    const int64_t r = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (r >= rows) return;
    const int64_t t = row_first[r];
    const int64_t k = seq_piece_of(piece_off, n_pieces, tok_start[t]);
    const bool hdr = header && (r == 0 || seq_piece_of(piece_off, n_pieces, tok_start[row_first[r - 1]]) != k);
    is_hdr[r] = hdr ? 1 : 0;
    if (!hdr) { atomicMin(first_data, (unsigned long long)r); return; }
    piece_first[k] = r;
    int64_t v = -1, d = -1;
    if (row_first[r + 1] - t == 2) { v = vec_uint(buf + tok_start[t]); d = vec_uint(buf + tok_start[t + 1]); }
    hdr_v[k] = v; hdr_d[k] = d;
    if (v < 0 || d < 0) atomicMin(bad_hdr, (unsigned long long)r);
}

// entry e: the prior names, then the token that opens each row that is no header line, in text order
__global__ void __launch_bounds__(SEQ_BLOCK) k_vec_entries(const int64_t* tok_start, const int64_t* row_first, const uint8_t* is_hdr, const int64_t* hdrx, int64_t P, int64_t rows,
                                                           int64_t* ent_tok, int64_t* ent_start) {
    const int64_t i = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (i < P) { ent_tok[i] = i; ent_start[i] = tok_start[i]; return; }
    const int64_t r = i - P;
    if (r >= rows || is_hdr[r]) return;
    const int64_t e = P + r - hdrx[r], t = row_first[r];
    ent_tok[e] = t; ent_start[e] = tok_start[t];
}

// status[t - P]: 1 = the host finishes this value token.  bad_at: least offset of a malformed value; n_host: tokens for the host
__global__ void __launch_bounds__(SEQ_BLOCK) k_vec_parse(const uint8_t* buf, const int64_t* tok_start, const int64_t* rowx, const int64_t* row_first, const uint8_t* is_hdr,
                                                         const int64_t* hdrx, const int32_t* ent_id, int64_t P, int64_t T, int64_t dim, uint32_t* out, uint8_t* present,
                                                         uint8_t* status, unsigned long long* bad_at, unsigned long long* n_host) {
    typedef hipcub::BlockReduce<unsigned long long, SEQ_BLOCK> Reduce;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t t = P + (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    unsigned long long for_host = 0;
    if (t < T) {
        uint8_t st = 0;
        const int64_t r = rowx[t + 1] - 1;
        if (!is_hdr[r]) {
            const int64_t id = ent_id[P + r - hdrx[r]], col = t - row_first[r] - 1;
            if (col < 0) { if (id >= 0) present[id] = 1; }
            else if (col < dim) {
                const uint8_t* p = buf + tok_start[t];
                uint32_t bits = 0;
                const int rc = vec_parse_f32(p, seq_tok_len(p), &bits);
                if (rc == VEC_PARSE_BAD) atomicMin(bad_at, (unsigned long long)tok_start[t]);
                else if (id >= 0) {
                    if (rc == VEC_PARSE_OK) out[id * dim + col] = bits;
                    else { st = 1; for_host = 1; }
                }
            }
        }
        status[t - P] = st;
    }
    const unsigned long long sum = Reduce(tmp).Sum(for_host);
    if (threadIdx.x == 0 && sum) atomicAdd(n_host, sum);
}

// first_row[i] (preset to all ones): the least row entry whose name is prior name i.  The table is the finished one of seq_intern, only read here.
__global__ void __launch_bounds__(SEQ_BLOCK) k_vec_first_row(const unsigned long long* table, const int64_t* slot, int64_t P, int64_t N, unsigned long long* first_row) {
    const int64_t e = P + (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (e >= N) return;
    const unsigned long long rep = table[slot[e]];
    if (rep < (unsigned long long)P) atomicMin(first_row + rep, (unsigned long long)e);
}

// dup: the least row entry whose name opened an earlier row.  The first row of a string is its first appearance (a new name) or first_row[] of the
// prior name it equals; every other row of the string is a second occurrence.
__global__ void __launch_bounds__(SEQ_BLOCK) k_vec_dups(const unsigned long long* table, const int64_t* slot, const unsigned long long* first_row, int64_t P, int64_t N,
                                                        unsigned long long* dup) {
    const int64_t e = P + (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (e >= N) return;
    const unsigned long long rep = table[slot[e]];
    const unsigned long long first = rep < (unsigned long long)P ? first_row[rep] : rep;
    if (first != (unsigned long long)e) atomicMin(dup, (unsigned long long)e);
}

struct VecHostStart {    // host token k: value token host_tok[k], counted from the first token behind the prior names
    const int64_t* tok_start; const int64_t* host_tok; int64_t P;
    __device__ int64_t operator()(int64_t k) const { return tok_start[P + host_tok[k]]; }
};

__global__ void __launch_bounds__(SEQ_BLOCK) k_vec_scatter(const int64_t* host_tok, const uint32_t* host_bits, int64_t n, const int64_t* rowx, const int64_t* row_first,
                                                           const int64_t* hdrx, const int32_t* ent_id, int64_t P, int64_t dim, uint32_t* out) {
    const int64_t k = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (k >= n) return;
    const int64_t t = P + host_tok[k], r = rowx[t + 1] - 1;
    out[(int64_t)ent_id[P + r - hdrx[r]] * dim + (t - row_first[r] - 1)] = host_bits[k];
}

// ------------------------------------------------------------------------------------------ host side of one read
namespace {

int vec_token_offset(SeqRun& R, int64_t t, int64_t* at) { return seq_read_back(R, at, R.tok_start.p + t, 8); }

int vec_read(SeqRun& R, int header, dge_names* names, int intern, dge_vectors** out, dge_vec_info* info, const char* who) {
    R.what = "vec read";
    SEQ_TRY(seq_tokenise(R, names, who));
    const int64_t T = R.T, P = R.P, rows = R.rows, n_pieces = (int64_t)R.pieces.size();
    // words: [0] header line that is not two integers (row), [1] first row that is none, [2] ragged row, [3] malformed value (offset), [4] duplicate (entry), [5] host tokens
    dge_tmp<unsigned long long> words;
    dge_tmp<uint8_t> is_hdr;
    dge_tmp<int64_t> piece_off, piece_first, hdr_v, hdr_d, hdrx;
    unsigned long long w[6] = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull, 0ull};
    SEQ_TRY(seq_alloc(R, words, 6, "the counters"));
    SEQ_TRY(seq_alloc(R, is_hdr, rows, "the rows' kinds"));
    SEQ_TRY(seq_alloc(R, hdrx, rows + 1, "the rows' numbers"));
    SEQ_TRY(seq_alloc(R, piece_off, n_pieces, "the pieces"));
    SEQ_TRY(seq_alloc(R, piece_first, n_pieces, "the pieces"));
    SEQ_TRY(seq_alloc(R, hdr_v, n_pieces, "the pieces"));
    SEQ_TRY(seq_alloc(R, hdr_d, n_pieces, "the pieces"));
    DGE_HIP(hipMemcpyAsync(words.p, w, sizeof(w), hipMemcpyHostToDevice, R.stream));
    if (n_pieces) DGE_HIP(hipMemcpyAsync(piece_off.p, R.L.offset.data(), (size_t)n_pieces * 8, hipMemcpyHostToDevice, R.stream));
    SEQ_TRY(seq_kernels_begin(R));
    DGE_HIP(hipMemsetAsync(piece_first.p, 0xFF, (size_t)std::max<int64_t>(n_pieces, 1) * 8, R.stream));
    if (rows) hipLaunchKernelGGL(k_vec_mark, dim3(seq_grid(rows)), dim3(SEQ_BLOCK), 0, R.stream, R.buf.p, R.tok_start.p, R.row_first.p, rows, piece_off.p, n_pieces, header ? 1 : 0,
                                 is_hdr.p, piece_first.p, hdr_v.p, hdr_d.p, words.p, words.p + 1);
    SEQ_TRY(seq_scan(R, rocprim::make_transform_iterator(rocprim::counting_iterator<int64_t>(0), SeqByteFlag{is_hdr.p, rows}), hdrx.p, rows + 1));
    SEQ_TRY(seq_kernels_end(R));
    SEQ_TRY(seq_read_back(R, w, words.p, sizeof(w)));
    int64_t n_hdr = 0;
    SEQ_TRY(seq_read_back(R, &n_hdr, hdrx.p + rows, 8));
    std::vector<int64_t> first((size_t)n_pieces, -1), hv((size_t)n_pieces, 0), hd((size_t)n_pieces, 0);
    if (header && n_pieces) {
        SEQ_TRY(seq_read_back(R, first.data(), piece_first.p, (size_t)n_pieces * 8));
        SEQ_TRY(seq_read_back(R, hv.data(), hdr_v.p, (size_t)n_pieces * 8));
        SEQ_TRY(seq_read_back(R, hd.data(), hdr_d.p, (size_t)n_pieces * 8));
    }
    if (w[0] != ~0ull) {
        int64_t at = 0, count = 0;
        SEQ_TRY(seq_row_where(R, (int64_t)w[0], &at, &count));
        DGE_FAIL(DGE_ERR_IO, "%s: the header line at %s is not two unsigned decimal integers \"V D\" (it has %lld tokens)", who, seq_where(R, at).c_str(), (long long)count);
    }
    // ---- dim: the first row's token count less the name
    const int64_t n_data = rows - n_hdr;
    int64_t dim = 0;
    if (n_data > 0) {
        int64_t at = 0, count = 0;
        SEQ_TRY(seq_row_where(R, (int64_t)w[1], &at, &count));
        dim = count - 1;
        if (dim < 1) DGE_FAIL(DGE_ERR_IO, "%s: the row at %s has 1 token where at least 2 are expected: a name and its values", who, seq_where(R, at).c_str());
        if (dim > 0x7fffffffLL) DGE_FAIL(DGE_ERR_RANGE, "%s: %lld values a row do not fit an int32 dim", who, (long long)dim);
        SEQ_TRY(seq_kernels_begin(R));
        hipLaunchKernelGGL(k_seq_ragged, dim3(seq_grid(rows)), dim3(SEQ_BLOCK), 0, R.stream, R.row_first.p, is_hdr.p, rows, dim + 1, words.p + 2);
        SEQ_TRY(seq_kernels_end(R));
        SEQ_TRY(seq_read_back(R, w + 2, words.p + 2, 8));
        if (w[2] != ~0ull) {
            SEQ_TRY(seq_row_where(R, (int64_t)w[2], &at, &count));
            DGE_FAIL(DGE_ERR_IO, "%s: the row at %s has %lld tokens where %lld are expected (a name and %lld values, as on the first row)", who, seq_where(R, at).c_str(),
                     (long long)count, (long long)(dim + 1), (long long)dim);
        }
    } else if (header) {
        for (int64_t k = 0; k < n_pieces && dim == 0; k++) if (first[(size_t)k] >= 0) dim = std::min<int64_t>(hd[(size_t)k], 0x7fffffffLL);      // no row anywhere: the first header's D
    }

    // ---- names: the prior names and the token that opens each row
    const int64_t N = P + n_data;
    dge_tmp<int64_t> ent_tok, ent_start;
    SEQ_TRY(seq_alloc(R, ent_tok, N, "the names' tokens"));
    SEQ_TRY(seq_alloc(R, ent_start, N, "the names' offsets"));
    SEQ_TRY(seq_kernels_begin(R));
    if (P + rows) hipLaunchKernelGGL(k_vec_entries, dim3(seq_grid(P + rows)), dim3(SEQ_BLOCK), 0, R.stream, R.tok_start.p, R.row_first.p, is_hdr.p, hdrx.p, P, rows, ent_tok.p, ent_start.p);
    SEQ_TRY(seq_kernels_end(R));
    SeqOptions opt; opt.intern = intern;
    SEQ_TRY(seq_intern(R, ent_start.p, N, opt, who));
    const int64_t rows_out = intern ? R.n_names : P, dropped = R.unknown;

    // ---- values
    dge_tmp<uint32_t> vals;
    dge_tmp<uint8_t> present, status;
    dge_tmp<unsigned long long> first_row;
    SEQ_TRY(seq_alloc(R, vals, rows_out * dim, "the vectors"));
    SEQ_TRY(seq_alloc(R, present, rows_out, "the present bytes"));
    SEQ_TRY(seq_alloc(R, status, T - P, "the value tokens' states"));
    SEQ_TRY(seq_alloc(R, first_row, P, "the prior names' rows"));
    SEQ_TRY(seq_kernels_begin(R));
    DGE_HIP(hipMemsetAsync(vals.p, 0, (size_t)std::max<int64_t>(rows_out * dim, 1) * 4, R.stream));
    DGE_HIP(hipMemsetAsync(present.p, 0, (size_t)std::max<int64_t>(rows_out, 1), R.stream));
    if (T > P) hipLaunchKernelGGL(k_vec_parse, dim3(seq_grid(T - P)), dim3(SEQ_BLOCK), 0, R.stream, R.buf.p, R.tok_start.p, R.rowx.p, R.row_first.p, is_hdr.p, hdrx.p, R.tok_id.p, P, T,
                                  dim, vals.p, present.p, status.p, words.p + 3, words.p + 5);
    DGE_HIP(hipMemsetAsync(first_row.p, 0xFF, (size_t)std::max<int64_t>(P, 1) * 8, R.stream));
    if (N > P) {
        hipLaunchKernelGGL(k_vec_first_row, dim3(seq_grid(N - P)), dim3(SEQ_BLOCK), 0, R.stream, R.table.p, R.tok_slot.p, P, N, first_row.p);
        hipLaunchKernelGGL(k_vec_dups, dim3(seq_grid(N - P)), dim3(SEQ_BLOCK), 0, R.stream, R.table.p, R.tok_slot.p, first_row.p, P, N, words.p + 4);
    }
    SEQ_TRY(seq_kernels_end(R));
    SEQ_TRY(seq_read_back(R, w + 3, words.p + 3, 24));
    if (w[3] != ~0ull) DGE_FAIL(DGE_ERR_IO, "%s: the value token at %s is not a decimal number, inf or nan", who, seq_where(R, (int64_t)w[3]).c_str());
    if (w[4] != ~0ull) {
        int64_t t = 0, at = 0;
        SEQ_TRY(seq_read_back(R, &t, ent_tok.p + (int64_t)w[4], 8));
        SEQ_TRY(vec_token_offset(R, t, &at));
        DGE_FAIL(DGE_ERR_IO, "%s: the name of the row at %s occurred on an earlier row: a name may have one vector", who, seq_where(R, at).c_str());
    }
    if (header) {
        int64_t next = rows;
        for (int64_t k = n_pieces - 1; k >= 0; k--) {
            if (first[(size_t)k] < 0) continue;                              // a piece without a token has no header line to check
            const int64_t held = next - first[(size_t)k] - 1;
            next = first[(size_t)k];
            if (hv[(size_t)k] != held || hd[(size_t)k] != dim)
                DGE_FAIL(DGE_ERR_IO, "%s: the header of piece %lld%s%s says %lld rows of %lld values, the text holds %lld rows of %lld", who, (long long)k, R.pieces[(size_t)k].path ? ", " : "",
                         R.pieces[(size_t)k].path ? R.pieces[(size_t)k].path : "", (long long)hv[(size_t)k], (long long)hd[(size_t)k], (long long)held, (long long)dim);
        }
    }

    // ---- the host path: the flagged tokens' bytes in one blob, strtof, the bits back into place
    const int64_t n_host = (int64_t)w[5];
    if (n_host > 0) {
        dge_tmp<int64_t> host_tok;
        dge_tmp<uint32_t> host_bits;
        std::vector<int64_t> off;
        std::unique_ptr<char[]> text;
        std::vector<uint32_t> bits;
        SEQ_TRY(seq_alloc(R, host_bits, n_host, "the host tokens' values"));
        SEQ_TRY(seq_kernels_begin(R));
        SEQ_TRY(seq_pick(R, status.p, T - P, n_host, host_tok, "the host tokens"));
        SEQ_TRY(seq_tokens_to_host(R, VecHostStart{R.tok_start.p, host_tok.p, P}, n_host, off, text, "the host tokens"));
        SEQ_TRY(seq_host_numbers(text.get(), off.data(), n_host, bits, who));
        DGE_HIP(hipMemcpyAsync(host_bits.p, bits.data(), (size_t)n_host * 4, hipMemcpyHostToDevice, R.stream));
        SEQ_TRY(seq_kernels_begin(R));
        hipLaunchKernelGGL(k_vec_scatter, dim3(seq_grid(n_host)), dim3(SEQ_BLOCK), 0, R.stream, host_tok.p, host_bits.p, n_host, R.rowx.p, R.row_first.p, hdrx.p, R.tok_id.p, P, dim, vals.p);
        SEQ_TRY(seq_kernels_end(R));
    }

    // ---- the new names' bytes
    const int64_t n_new = intern ? R.n_names - P : 0;
    std::vector<int64_t> off;
    std::unique_ptr<char[]> host_blob;
    SEQ_TRY(seq_new_names(R, ent_start.p, n_new, off, host_blob));
    std::unique_ptr<dge_vectors> v(new dge_vectors());
    DGE_HIP(hipStreamSynchronize(R.stream));
    // nothing can fail from here on: the names and the vectors change hands together
    if (n_new > 0) names_append(names, std::move(host_blob), off.data(), n_new);
    v->device = R.device; v->rows = rows_out; v->dim = (int32_t)dim; v->d.adopt(std::move(vals)); v->d_present = std::move(present);
    v->n_present = n_data - dropped;
    if (info) {
        info->bytes = R.L.text_bytes; info->lines = R.lines; info->rows = n_data; info->values = n_data * dim; info->dropped = dropped; info->missing = rows_out - v->n_present;
        info->names_added = n_new; info->host_values = n_host; info->dim = (int32_t)dim; info->reserved = 0; info->read_ms = R.read_ms; info->kernel_ms = R.kernel_ms;
    }
    *out = v.release();
    return DGE_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------ entries
extern "C" int dge_vectors_from_vec_text(int device, const char* text, int64_t n_bytes, int header, dge_names* names, int intern, dge_vectors** out, dge_vec_info* info) {
    if (!out || !names || n_bytes < 0 || (n_bytes > 0 && !text)) DGE_FAIL(DGE_ERR_ARG, "dge_vectors_from_vec_text: null or negative argument");
    *out = nullptr;
    SEQ_TRY(dge_require_device(device));
    SeqRun R;
    R.device = device;
    SEQ_TRY(seq_add_texts(R.pieces, &text, &n_bytes, 1, "dge_vectors_from_vec_text"));
    return vec_read(R, header, names, intern ? 1 : 0, out, info, "dge_vectors_from_vec_text");
}

extern "C" int dge_vectors_from_vec_files(int device, const char* const* paths, int32_t n_paths, int header, dge_names* names, int intern, dge_vectors** out, dge_vec_info* info) {
    if (!out || !names || n_paths < 0 || (n_paths > 0 && !paths)) DGE_FAIL(DGE_ERR_ARG, "dge_vectors_from_vec_files: null or negative argument");
    SEQ_TRY(seq_check_paths(paths, n_paths, "dge_vectors_from_vec_files"));
    *out = nullptr;
    SEQ_TRY(dge_require_device(device));
    SeqRun R;
    R.device = device;
    SEQ_TRY(seq_add_files(R.pieces, paths, n_paths, "dge_vectors_from_vec_files"));
    return vec_read(R, header, names, intern ? 1 : 0, out, info, "dge_vectors_from_vec_files");
}

extern "C" int dge_vectors_from_host(int device, const float* rows, int64_t n_rows, int32_t dim, const uint8_t* present, dge_vectors** out) {
    if (!out || n_rows < 0 || dim < 0 || (n_rows > 0 && dim > 0 && !rows)) DGE_FAIL(DGE_ERR_ARG, "dge_vectors_from_host: null or negative argument");
    *out = nullptr;
    SEQ_TRY(dge_require_device(device));
    std::unique_ptr<dge_vectors> v(new dge_vectors());
    v->device = device; v->rows = n_rows; v->dim = dim; v->n_present = n_rows;
    SEQ_TRY(v->d.alloc((size_t)n_rows * (size_t)dim));
    SEQ_TRY(v->d_present.alloc((size_t)n_rows));
    if (n_rows * dim) DGE_HIP(hipMemcpy(v->d.p, rows, (size_t)n_rows * (size_t)dim * sizeof(float), hipMemcpyHostToDevice));
    if (n_rows) {
        if (present) {
            std::vector<uint8_t> norm((size_t)n_rows);
            v->n_present = 0;
            for (int64_t i = 0; i < n_rows; i++) { norm[(size_t)i] = present[i] ? 1 : 0; v->n_present += norm[(size_t)i]; }
            DGE_HIP(hipMemcpy(v->d_present.p, norm.data(), (size_t)n_rows, hipMemcpyHostToDevice));
        } else {
            DGE_HIP(hipMemset(v->d_present.p, 1, (size_t)n_rows));
            DGE_HIP(hipDeviceSynchronize());
        }
    }
    *out = v.release();
    return DGE_OK;
}

extern "C" int dge_vectors_info(const dge_vectors* v, int64_t* rows, int32_t* dim, const float** d_ptr, const uint8_t** d_present) {
    if (!v) DGE_FAIL(DGE_ERR_ARG, "dge_vectors_info: null vectors");
    if (rows) *rows = v->rows;
    if (dim) *dim = v->dim;
    if (d_ptr) *d_ptr = v->d;
    if (d_present) *d_present = v->d_present;
    return DGE_OK;
}

extern "C" int dge_vectors_to_host(const dge_vectors* v, float* out, uint8_t* present, int64_t cap_elems) {
    if (!v || cap_elems < 0) DGE_FAIL(DGE_ERR_ARG, "dge_vectors_to_host: null or negative argument");
    if (out && cap_elems < v->rows * v->dim) DGE_FAIL(DGE_ERR_CAP, "dge_vectors_to_host: out holds %lld of %lld elements", (long long)cap_elems, (long long)(v->rows * v->dim));
    DGE_HIP(hipSetDevice(v->device));
    if (out && v->rows * v->dim) DGE_HIP(hipMemcpy(out, v->d, (size_t)(v->rows * v->dim) * sizeof(float), hipMemcpyDeviceToHost));
    if (present && v->rows) DGE_HIP(hipMemcpy(present, v->d_present, (size_t)v->rows, hipMemcpyDeviceToHost));
    return DGE_OK;
}

extern "C" void dge_vectors_free(dge_vectors* v) {
    if (!v) return;
    (void)hipSetDevice(v->device);
    delete v;
}
