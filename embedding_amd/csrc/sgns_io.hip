// sgns_io.hip — what a host reads back from a trained model (libdge.so, gfx950): the tables' host mirrors (dge_model_vectors and its family), the
// vocabulary's counts, Huffman paths and unigram table, and the `.vec` text file — and the way back in, dge_model_load_vectors.  Runs between launches: outside the build stamp (dge_build_stamp, include/dge.h).
#include <string.h>

#include <algorithm>
#include <charconv>
#include <string>
#include <thread>
#include <vector>

#include "dge_internal.h"
#include "sgns_kernels.h"      // neg_table_row
#include "sgns_model.h"
#include "fmt_g9.h"

static int sync_tables_to_host(dge_model* m, bool want_syn0, bool want_syn1, bool want_hs = false) {
    DGE_HIP(hipSetDevice(m->device));
    DGE_HIP(hipStreamSynchronize(m->stream));
    size_t tab = (size_t)m->V * (size_t)m->stride;
    std::vector<float> tmp(tab ? tab : 1);
    for (int which = 0; which < 3; which++) {
        if ((which == 0 && !want_syn0) || (which == 1 && !want_syn1) || (which == 2 && !want_hs)) continue;
        const float* src = which == 0 ? m->d_syn0 : (which == 1 ? m->d_syn1neg : m->d_syn1);
        if (tab) DGE_HIP(hipMemcpy(tmp.data(), src, tab * sizeof(float), hipMemcpyDeviceToHost));
        std::vector<float>& dst = which == 0 ? m->h_syn0 : (which == 1 ? m->h_syn1neg : m->h_syn1);
        const int64_t rows = which == 2 ? std::max<int64_t>(m->V - 1, 0) : m->V;
        dst.resize((size_t)rows * (size_t)m->D + 1);
        for (int64_t r = 0; r < rows; r++) memcpy(dst.data() + r * m->D, tmp.data() + r * m->stride, (size_t)m->D * sizeof(float));
    }
    return DGE_OK;
}

extern "C" int dge_model_vectors(dge_model* m, const float** syn0, const int32_t** vocab_ids, int64_t* V, int32_t* dim) {
    if (!m) DGE_FAIL(DGE_ERR_ARG, "dge_model_vectors: null model");
    int rc = sync_tables_to_host(m, true, false);
    if (rc) return rc;
    if (syn0) *syn0 = m->h_syn0.data();
    if (vocab_ids) *vocab_ids = m->h_vocab_ids.data();
    if (V) *V = m->V;
    if (dim) *dim = m->D;
    return DGE_OK;
}
extern "C" int dge_model_syn1neg(dge_model* m, const float** syn1neg) {
    if (!m || !syn1neg) DGE_FAIL(DGE_ERR_ARG, "dge_model_syn1neg: null argument");
    int rc = sync_tables_to_host(m, false, true);
    if (rc) return rc;
    *syn1neg = m->h_syn1neg.data();
    return DGE_OK;
}
extern "C" int dge_model_syn1(dge_model* m, const float** syn1, int64_t* rows) {
    if (!m || !syn1) DGE_FAIL(DGE_ERR_ARG, "dge_model_syn1: null argument");
    if (!m->d_syn1) DGE_FAIL(DGE_ERR_STATE, "dge_model_syn1: the model was created without use_hs");
    int rc = sync_tables_to_host(m, false, false, true);
    if (rc) return rc;
    *syn1 = m->h_syn1.data();
    if (rows) *rows = std::max<int64_t>(m->V - 1, 0);
    return DGE_OK;
}
extern "C" int dge_model_huffman(dge_model* m, const int64_t** offsets, const int32_t** points, const uint64_t** codes) {
    if (!m) DGE_FAIL(DGE_ERR_ARG, "dge_model_huffman: null model");
    if (!m->d_syn1) DGE_FAIL(DGE_ERR_STATE, "dge_model_huffman: the model was created without use_hs");
    if (offsets) *offsets = m->h_hs_off.data();
    if (points) *points = m->h_hs_points.data();
    if (codes) *codes = m->h_hs_codes.data();
    return DGE_OK;
}
extern "C" int dge_model_counts(dge_model* m, const int64_t** counts) {
    if (!m || !counts) DGE_FAIL(DGE_ERR_ARG, "dge_model_counts: null argument");
    *counts = m->h_counts.data();
    return DGE_OK;
}
// the unigram table's rank-block form (k_table_pack, sgns.hip) back into word2vec's one row per slot: one thread per slot
__global__ void k_table_unpack(const uint4* __restrict__ ctab, int64_t T, int32_t* __restrict__ table) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a < T) table[a] = neg_table_row(ctab, (uint64_t)a);
}
extern "C" int dge_model_table(dge_model* m, const int32_t** table, int64_t* table_size) {
    if (!m || !table) DGE_FAIL(DGE_ERR_ARG, "dge_model_table: null argument");
    DGE_HIP(hipSetDevice(m->device));
    m->h_table.resize((size_t)m->T);
    dge_tmp<int32_t> flat;                                   // word2vec's one-row-per-slot form, expanded from the rank blocks
    int rc = flat.alloc((size_t)m->T);
    if (rc) return rc;
    DGE_HIP(hipStreamSynchronize(m->stream));
    hipLaunchKernelGGL(k_table_unpack, dim3(dge_grid_for(m->T, 256)), dim3(256), 0, m->stream, m->d_ctab, m->T, flat.p);
    DGE_HIP(hipStreamSynchronize(m->stream));
    DGE_HIP(hipMemcpy(m->h_table.data(), flat.p, (size_t)m->T * sizeof(int32_t), hipMemcpyDeviceToHost));
    *table = m->h_table.data();
    if (table_size) *table_size = m->T;
    return DGE_OK;
}

// WordVectorSerializer.writeWordVectors: V lines of D decimal numbers.  At the reference's sizes (6 408 x 20) that is nothing; at cfg3's (10^6 x 128 =
// 1.3e8 conversions, 1.5 GB of text) one thread formats for ~25 s — longer than the epoch trained.  Rows are formatted in slabs by up to 16 host threads
// (each row into its own string, the slab written in row order): same bytes as the serial loop.
extern "C" int dge_write_vec(dge_model* m, const char* const* names, const char* path, int header) {
    if (!m || !path) DGE_FAIL(DGE_ERR_ARG, "dge_write_vec: null argument");
    int rc = sync_tables_to_host(m, true, false);
    if (rc) return rc;
    FILE* f = fopen(path, "w");
    if (!f) DGE_FAIL(DGE_ERR_IO, "dge_write_vec: cannot open %s", path);
    if (header) fprintf(f, "%lld %d\n", (long long)m->V, m->D);
    const int64_t V = m->V; const int D = m->D;
    const unsigned hw = std::thread::hardware_concurrency();
    const int n_thr = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<unsigned>(hw ? hw : 1, 16u), V * (int64_t)D / 65536));
    const int64_t slab = 4096 * (int64_t)n_thr;                                  // rows formatted before they are written
    // two sets of slab buffers: while slab k is being written (one thread, in row order), slab k + 1 is being formatted — the text file of cfg3 is 1.67 GB,
    // and writing it takes as long as formatting it
    std::vector<std::string> out[2] = {std::vector<std::string>((size_t)n_thr), std::vector<std::string>((size_t)n_thr)};
    bool ok = true;
    std::thread writer;
    int cur = 0;
    for (int64_t r0 = 0; r0 < V; r0 += slab, cur ^= 1) {
        const int64_t r1 = std::min(V, r0 + slab);
        std::vector<std::string>& ob = out[cur];
        auto work = [&, r0, r1](int t) {
            std::string& sbuf = ob[(size_t)t];
            const int64_t a = r0 + (r1 - r0) * t / n_thr, b = r0 + (r1 - r0) * (t + 1) / n_thr;
            // the rows' text goes straight into the buffer: at most 17 characters an element (sign, nine digits, point, e-XX, the blank in front)
            size_t cap = 0;
            for (int64_t r = a; r < b; r++) { const int32_t id = m->h_vocab_ids[(size_t)r]; cap += (names && names[id] ? strlen(names[id]) : 12) + (size_t)D * 26 + 2; }
            sbuf.resize(cap);
            char* o = sbuf.data();
            for (int64_t r = a; r < b; r++) {
                const int32_t id = m->h_vocab_ids[(size_t)r];
                if (names && names[id]) { const size_t n = strlen(names[id]); memcpy(o, names[id], n); o += n; } else o = std::to_chars(o, o + 12, id).ptr;
                const float* v = m->h_syn0.data() + r * D;
                // "%.9g" of every element: dge_fmt_g9 (integer arithmetic, the same bytes: fmt_g9.h) for the values an embedding holds, and for the rest
                // std::to_chars(double, general, 9), which is specified to give printf's "%.9g"
                for (int j = 0; j < D; j++) {
                    *o++ = ' ';
                    char* e = dge_fmt_g9(v[j], o);
                    o = e ? e : std::to_chars(o, o + 25, (double)v[j], std::chars_format::general, 9).ptr;
                }
                *o++ = '\n';
            }
            sbuf.resize((size_t)(o - sbuf.data()));
        };
        if (n_thr == 1) work(0);
        else {
            std::vector<std::thread> th;
            for (int t = 0; t < n_thr; t++) th.emplace_back(work, t);
            for (auto& x : th) x.join();
        }
        if (writer.joinable()) writer.join();                                   // the previous slab is on its way to the file: now this one
        if (!ok) break;
        writer = std::thread([&ok, &ob, f, n_thr]() {
            for (int t = 0; t < n_thr && ok; t++) ok = ob[(size_t)t].empty() || fwrite(ob[(size_t)t].data(), 1, ob[(size_t)t].size(), f) == ob[(size_t)t].size();
        });
    }
    if (writer.joinable()) writer.join();
    if (fclose(f) != 0 || !ok) DGE_FAIL(DGE_ERR_IO, "dge_write_vec: write to %s failed", path);
    return DGE_OK;
}

// syn0 row r := row vocab_ids[r] of v where v holds that row; a lane per element, the padded row stride honoured
__global__ void k_load_vectors(const int32_t* __restrict__ vocab_ids, int64_t V, int32_t D, int32_t stride, const float* __restrict__ rows, const uint8_t* __restrict__ present,
                               int64_t n_rows, float* __restrict__ syn0, unsigned long long* __restrict__ rows_set) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V * D) return;
    const int64_t r = i / D; const int32_t j = (int32_t)(i - r * D);
    const int64_t id = vocab_ids[r];
    if (id < 0 || id >= n_rows || !present[id]) return;
    syn0[r * stride + j] = rows[id * D + j];
    if (j == 0) atomicAdd(rows_set, 1ull);
}

extern "C" int dge_model_load_vectors(dge_model* m, const dge_vectors* v, int64_t* rows_set) {
    if (!m || !v) DGE_FAIL(DGE_ERR_ARG, "dge_model_load_vectors: null argument");
    if (v->dim != m->D) DGE_FAIL(DGE_ERR_ARG, "dge_model_load_vectors: the vectors have dim %d, the model %d", v->dim, m->D);
    if (v->device != m->device) DGE_FAIL(DGE_ERR_ARG, "dge_model_load_vectors: the vectors are on device %d, the model on %d", v->device, m->device);
    if (m->part_n > 1) DGE_FAIL(DGE_ERR_STATE, "dge_model_load_vectors: a partition is set (n_parts = %d): the tables are in pieces — call dge_model_set_partition(m, 1, 0, 0) first", m->part_n);
    DGE_HIP(hipSetDevice(m->device));
    dge_tmp<unsigned long long> count;
    int rc = count.alloc(1);
    if (rc) return rc;
    DGE_HIP(hipMemsetAsync(count.p, 0, 8, m->stream));
    const int64_t n = m->V * (int64_t)m->D;
    if (n && v->rows) hipLaunchKernelGGL(k_load_vectors, dim3(dge_grid_for(n, 256)), dim3(256), 0, m->stream, m->d_vocab_ids, m->V, m->D, m->stride, v->d, v->d_present, v->rows, m->d_syn0,
                                         count.p);
    DGE_HIP(hipGetLastError());
    unsigned long long set = 0;
    DGE_HIP(hipMemcpyAsync(&set, count.p, 8, hipMemcpyDeviceToHost, m->stream));
    DGE_HIP(hipStreamSynchronize(m->stream));
    if (rows_set) *rows_set = (int64_t)set;
    return DGE_OK;
}
