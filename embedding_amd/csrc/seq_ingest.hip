// seq_ingest.hip — .seq text in, a resident walk corpus and the interned names out (include/dge.h: dge_names_*, dge_walks_from_seq_text / _files).
//
// The mirror image of the .vec writer (sgns_io.hip): the reference hands its walks to the trainer as text (J/DeepWalk.java:49-56), one walk per line,
// names joined by blanks.  Tokenising, interning and packing run here on the device; the host only moves bytes.  This translation unit is outside the
// build stamp: nothing in it is read or written by a training launch.
//
// The tokeniser, the name table (with the argument for it on eight L2s that are not coherent) and the byte transport are in seq_tokens.h, which the .vec
// reader (vec_read.hip) includes too; what is here is the names object, the packing of ids into corpus rows and the entries.
#include <unordered_set>

#include "seq_tokens.h"

// ------------------------------------------------------------------------------------------ dge_names: a host object, no device involved (the struct: dge_internal.h)
static void names_index(dge_names* n) {
    for (; n->indexed < n->ptr.size(); n->indexed++) n->index.emplace(n->ptr[n->indexed], (size_t)n->len[n->indexed]);
}

extern "C" int dge_names_create(dge_names** out) {
    if (!out) DGE_FAIL(DGE_ERR_ARG, "dge_names_create: null output");
    *out = new dge_names();
    return DGE_OK;
}

extern "C" void dge_names_free(dge_names* n) { delete n; }

extern "C" int dge_names_add(dge_names* n, const char* const* strs, int64_t count) {
    if (!n || count < 0 || (count > 0 && !strs)) DGE_FAIL(DGE_ERR_ARG, "dge_names_add: null or negative argument");
    names_index(n);
    std::unordered_set<std::string_view> fresh;
    std::vector<int64_t> off((size_t)count + 1, 0);
    for (int64_t k = 0; k < count; k++) {
        if (!strs[k] || !strs[k][0]) DGE_FAIL(DGE_ERR_ARG, "dge_names_add: name %lld is null or empty", (long long)k);
        const size_t l = strlen(strs[k]);
        for (size_t i = 0; i < l; i++)
            if (seq_is_space((uint8_t)strs[k][i])) DGE_FAIL(DGE_ERR_ARG, "dge_names_add: name %lld holds a whitespace byte: it can never be a token", (long long)k);
        std::string_view sv(strs[k], l);
        if (n->index.count(sv) || !fresh.insert(sv).second) DGE_FAIL(DGE_ERR_ARG, "dge_names_add: duplicate name \"%s\"", strs[k]);
        off[(size_t)k + 1] = off[(size_t)k] + (int64_t)l + 1;
    }
    if (count == 0) return DGE_OK;
    std::unique_ptr<char[]> blob(new char[(size_t)off[(size_t)count]]);
    for (int64_t k = 0; k < count; k++) memcpy(blob.get() + off[(size_t)k], strs[k], (size_t)(off[(size_t)k + 1] - off[(size_t)k]));
    names_append(n, std::move(blob), off.data(), count);
    names_index(n);
    return DGE_OK;
}

extern "C" int dge_names_count(const dge_names* n, int64_t* count) {
    if (!n || !count) DGE_FAIL(DGE_ERR_ARG, "dge_names_count: null argument");
    *count = (int64_t)n->ptr.size();
    return DGE_OK;
}

extern "C" int dge_names_cstrs(const dge_names* n, const char* const** strs) {
    if (!n || !strs) DGE_FAIL(DGE_ERR_ARG, "dge_names_cstrs: null argument");
    *strs = n->ptr.data();
    return DGE_OK;
}

__global__ void __launch_bounds__(SEQ_BLOCK) k_seq_pack(const int32_t* tok_id, const int64_t* rowx, const int64_t* row_first, int64_t P, int64_t T, int64_t max_len, int32_t* out) {
    const int64_t t = P + (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (t >= T) return;
    const int64_t r = rowx[t + 1] - 1;
    out[r * max_len + (t - row_first[r])] = tok_id[t];
}

namespace {

// everything up to the per-token ids of a .seq text; what leaves the device is up to the caller
int seq_ingest(SeqRun& R, const dge_names* names, const SeqOptions& opt, const char* who) {
    SEQ_TRY(seq_tokenise(R, names, who));
    return seq_intern(R, R.tok_start.p, R.T, opt, who);
}

// corpus + new names + info out of a finished seq_ingest
int seq_finish(SeqRun& R, dge_names* names, int intern, dge_walks** out, dge_seq_info* info, const char* who) {
    const int64_t T = R.T, P = R.P;
    if (R.max_len > 0x7fffffffLL) DGE_FAIL(DGE_ERR_RANGE, "%s: a line of %lld tokens does not fit a corpus row", who, (long long)R.max_len);
    std::unique_ptr<dge_walks> w(new dge_walks());
    w->device = R.device; w->n = R.rows; w->L = (int32_t)R.max_len;
    SEQ_TRY(seq_alloc(R, w->d, R.rows * R.max_len, "the corpus"));
    SEQ_TRY(seq_kernels_begin(R));
    DGE_HIP(hipMemsetAsync(w->d.p, 0xFF, (size_t)std::max<int64_t>(R.rows * R.max_len, 1) * sizeof(int32_t), R.stream));
    if (T > P) hipLaunchKernelGGL(k_seq_pack, dim3(seq_grid(T - P)), dim3(SEQ_BLOCK), 0, R.stream, R.tok_id.p, R.rowx.p, R.row_first.p, P, T, R.max_len, w->d.p);
    SEQ_TRY(seq_kernels_end(R));
    // ---- the new names' bytes
    const int64_t n_new = intern ? R.n_names - P : 0;
    std::vector<int64_t> off;
    std::unique_ptr<char[]> host_blob;
    SEQ_TRY(seq_new_names(R, R.tok_start.p, n_new, off, host_blob));
    // nothing can fail from here on: the names and the corpus change hands together
    if (n_new > 0) names_append(names, std::move(host_blob), off.data(), n_new);
    w->gen = dge_next_generation();
    if (info) {
        info->bytes = R.L.text_bytes; info->lines = R.lines; info->rows = R.rows; info->tokens = T - P; info->unknown = R.unknown; info->names_added = n_new;
        info->max_len = (int32_t)R.max_len; info->reserved = 0; info->read_ms = R.read_ms; info->kernel_ms = R.kernel_ms;
    }
    *out = w.release();
    return DGE_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------ entries
extern "C" int dge_walks_from_seq_text(int device, const char* text, int64_t n_bytes, dge_names* names, int intern, dge_walks** out, dge_seq_info* info) {
    if (!out || !names || n_bytes < 0 || (n_bytes > 0 && !text)) DGE_FAIL(DGE_ERR_ARG, "dge_walks_from_seq_text: null or negative argument");
    *out = nullptr;
    SEQ_TRY(dge_require_device(device));
    SeqRun R;
    R.device = device;
    SEQ_TRY(seq_add_texts(R.pieces, &text, &n_bytes, 1, "dge_walks_from_seq_text"));
    SeqOptions opt; opt.intern = intern ? 1 : 0;
    SEQ_TRY(seq_ingest(R, names, opt, "dge_walks_from_seq_text"));
    return seq_finish(R, names, opt.intern, out, info, "dge_walks_from_seq_text");
}

extern "C" int dge_walks_from_seq_files(int device, const char* const* paths, int32_t n_paths, dge_names* names, int intern, dge_walks** out, dge_seq_info* info) {
    if (!out || !names || n_paths < 0 || (n_paths > 0 && !paths)) DGE_FAIL(DGE_ERR_ARG, "dge_walks_from_seq_files: null or negative argument");
    SEQ_TRY(seq_check_paths(paths, n_paths, "dge_walks_from_seq_files"));
    *out = nullptr;
    SEQ_TRY(dge_require_device(device));
    SeqRun R;
    R.device = device;
    SEQ_TRY(seq_add_files(R.pieces, paths, n_paths, "dge_walks_from_seq_files"));
    SeqOptions opt; opt.intern = intern ? 1 : 0;
    SEQ_TRY(seq_ingest(R, names, opt, "dge_walks_from_seq_files"));
    return seq_finish(R, names, opt.intern, out, info, "dge_walks_from_seq_files");
}

extern "C" int dge_selftest_seq_intern(int device, const char* text, int64_t n_bytes, int32_t hash_bits, int64_t initial_slots, int32_t* ids, int64_t cap, int64_t* n_tokens,
                                       int64_t* n_names) {
    if (!n_tokens || !n_names || n_bytes < 0 || (n_bytes > 0 && !text) || cap < 0 || (cap > 0 && !ids) || hash_bits < 1 || hash_bits > 64 || initial_slots < 1)
        DGE_FAIL(DGE_ERR_ARG, "dge_selftest_seq_intern: null, negative or out-of-range argument");
    SEQ_TRY(dge_require_device(device));
    SeqRun R;
    R.device = device;
    SEQ_TRY(seq_add_texts(R.pieces, &text, &n_bytes, 1, "dge_selftest_seq_intern"));
    SeqOptions opt; opt.hash_bits = hash_bits; opt.initial_slots = initial_slots;
    SEQ_TRY(seq_ingest(R, nullptr, opt, "dge_selftest_seq_intern"));
    *n_tokens = R.T;
    *n_names = R.n_names;
    if (R.T > cap) DGE_FAIL(DGE_ERR_CAP, "dge_selftest_seq_intern: ids holds %lld of %lld tokens", (long long)cap, (long long)R.T);
    if (R.T) SEQ_TRY(seq_read_back(R, ids, R.tok_id.p, (size_t)R.T * sizeof(int32_t)));
    return DGE_OK;
}
