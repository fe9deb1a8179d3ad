// sgns.hip — the stamped host side of the skip-gram negative-sampling trainer of libdge.so (gfx950): what a training launch reads is built here and
// launched from here.
//
// Replaces `new Word2Vec.Builder()...build(); w2v.fit()` (J/DeepWalk.java:73-79).  The arithmetic of that call
// lives in DL4J-NLP 0.7.2 / ND4J-native 0.7.2 (not among the reference's sources); what is implemented is the word2vec
// skip-gram negative-sampling update with DL4J's pair enumeration, as restated in oracle/dge_oracle.c
// (SURVEY.md §3.3, row a9).
//
// In this file: the tuning knobs and the build stamp; dge_model_create — vocabulary order, the unigram table in its rank-block and run forms, Huffman
// paths, ScheduleStats, syn0's initial values; train_rows — compacts the walks, fills TrainParams, asks sgns_plan.h for the schedule and launches the
// kernel form it names (sgns_kernels.h through sgns_train_dch.hip, or sgns_sorted.hip); the launch statistics.
// HBM layout: syn0, syn1neg (and syn1 with use_hs)  float32 [V x stride], stride = round_up(dim, 64) floats (zero padded)
// so that a row is 1..8 chunks of 256 B.  The kernels, their work decomposition and update policies: sgns_kernels.h, DESIGN.md §5.
//
// This file is hashed into dge_build_stamp together with the kernels and the schedule: a change here can change what a launch reads or writes per pair.
// What cannot lives elsewhere — where the tables lie (sgns_place.hip), read-back and the `.vec` file (sgns_io.hip), the exchange between ranks
// (sgns_exchange.hip), the self-tests (sgns_selftest.hip) — and shares dge_model with this file through sgns_model.h.
#include <hipcub/hipcub.hpp>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <string>

#include "dge_algos.h"
#include "dge_internal.h"
#include "sgns_kernels.h"
#include "sgns_model.h"

std::atomic<int64_t> g_dge_tuning[DGE_TUNE_COUNT];
namespace { struct TuningInit { TuningInit() { for (auto& k : g_dge_tuning) k.store(-1); } } g_tuning_init; }
std::atomic<int64_t> g_dge_host_syncs{0};
extern "C" int dge_host_sync_count(int64_t* n) {
    if (!n) DGE_FAIL(DGE_ERR_ARG, "dge_host_sync_count: null output");
    *n = g_dge_host_syncs.load(std::memory_order_relaxed);
    return DGE_OK;
}
extern "C" int dge_set_tuning(int32_t knob, int64_t value) {
    if (knob < 0 || knob >= DGE_TUNE_COUNT) DGE_FAIL(DGE_ERR_ARG, "dge_set_tuning: unknown knob %d", knob);
    g_dge_tuning[knob] = value < 0 ? -1 : value;
    return DGE_OK;
}
extern "C" int dge_get_tuning(int32_t knob, int64_t* value) {
    if (knob < 0 || knob >= DGE_TUNE_COUNT || !value) DGE_FAIL(DGE_ERR_ARG, "dge_get_tuning: unknown knob %d", knob);
    *value = g_dge_tuning[knob];
    return DGE_OK;
}

#ifndef DGE_KERNELS_HASH
#define DGE_KERNELS_HASH "unknown"
#endif
#ifndef DGE_SORTED_HASH
#define DGE_SORTED_HASH "unknown"
#endif
extern "C" const char* dge_build_stamp(void) { return "kernels=" DGE_KERNELS_HASH " sorted=" DGE_SORTED_HASH; }

// ------------------------------------------------------------------------------------------ vocabulary
__global__ void k_count_tokens(const int32_t* __restrict__ walks, int64_t n, int32_t NV, unsigned long long* counts) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int32_t t = walks[i];
        if (t >= 0 && t < NV) atomicAdd(&counts[t], 1ULL);
    }
}

__global__ void k_iota_i32(int32_t* p, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = (int32_t)i;
}

__global__ void k_count_kept(const int64_t* sorted_counts, int64_t n, int64_t min_count, unsigned long long* out) {
    unsigned long long c = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        c += (sorted_counts[i] >= min_count && sorted_counts[i] > 0) ? 1ULL : 0ULL;
    for (int o = 32; o > 0; o >>= 1) c += (unsigned long long)__shfl_xor((long long)c, o);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

__global__ void k_scatter_remap(const int32_t* vocab_ids, int64_t V, int32_t* remap) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < V) remap[vocab_ids[r]] = (int32_t)r;
}

// word2vec.c InitUnigramTable without the serial loop.  The loop advances the word index i by at most one per
// slot a, whenever a/T > cum[i]; with j(a) = #{i : cum[i] < a/T} this is i(a+1) = min(i(a)+1, j(a)), whose
// closed form is i(a) = a + min(0, min_{b<a}(j(b) - b - 1)): a binary search, an exclusive prefix-min, a clamp.
__global__ void k_table_chase(const double* __restrict__ cum, int64_t V, int64_t T, int32_t* g) {
    int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= T) return;
    double x = (double)a / (double)T;
    int64_t lo = 0, hi = V;
    while (lo < hi) { int64_t mid = (lo + hi) >> 1; if (cum[mid] < x) lo = mid + 1; else hi = mid; }
    g[a] = (int32_t)(lo - a - 1);
}
__global__ void k_table_fill(const int32_t* __restrict__ m, int64_t V, int64_t T, int32_t* table) {
    int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= T) return;
    int64_t i = a + (int64_t)min(0, m[a]);
    table[a] = (int32_t)min(i, V - 1);
}

// the run form of the table (neg_row_by_runs) against the table itself, slot by slot: the slots at which they differ
__global__ void k_runs_verify(const int32_t* __restrict__ table, int64_t T, const double* base, const uint32_t* row, const uint32_t* exc_slot,
                              const int32_t* exc_row, int n_exc, double T_inv, int64_t V, unsigned* n_bad, uint32_t* bad_slot, int32_t* bad_row, unsigned cap) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= T) return;
    const int32_t r = neg_row_by_runs((uint32_t)a, base, row, exc_slot, exc_row, n_exc, T_inv, V);
    if (r != -2 && r != table[a]) {
        const unsigned idx = atomicAdd(n_bad, 1u);
        if (idx < cap) { bad_slot[idx] = (uint32_t)a; bad_row[idx] = table[a]; }
    }
}

// the table in rank-block form (neg_table_row, sgns_kernels.h): thread (block b, word k) collects the step bits of slots 96b + 32k .. + 31
__global__ void k_table_pack(const int32_t* __restrict__ table, int64_t T, int64_t n_blocks, uint32_t* __restrict__ ctab) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_blocks * 3) return;
    const int64_t b = i / 3; const int k = (int)(i - b * 3);
    const int64_t a0 = b * DGE_CTAB_SLOTS + 32 * k;
    uint32_t bits = 0;
    int32_t prev = a0 > 0 && a0 - 1 < T ? table[a0 - 1] : 0;
    for (int j = 0; j < 32; j++) {
        const int64_t a = a0 + j;
        if (a >= T) break;
        const int32_t cur = table[a];
        if (a > b * DGE_CTAB_SLOTS && cur != prev) bits |= 1u << j;
        prev = cur;
    }
    ctab[b * 4 + 1 + k] = bits;
    if (k == 0) ctab[b * 4] = (uint32_t)(b * DGE_CTAB_SLOTS < T ? table[b * DGE_CTAB_SLOTS] : 0);
}

// word2vec.c InitNet: syn0[a][b] = ((lcg & 0xFFFF)/65536 - 0.5)/dim, one LCG stream over the whole table
__global__ void k_init_syn0(float* syn0, int64_t V, int32_t D, int32_t stride, uint64_t seed) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= V) return;
    uint64_t s = dge_w2v_jump(seed, (uint64_t)r * (uint64_t)D);
    float* row = syn0 + r * stride;
    for (int b = 0; b < D; b++) {
        s = s * DGE_W2V_MULT + 11;
        row[b] = (((float)(s & 0xFFFF) / (float)65536) - 0.5f) / (float)D;
    }
    for (int b = D; b < stride; b++) row[b] = 0.0f;
}

// vertex ids -> vocabulary rows, out-of-vocabulary tokens dropped and the walk left-packed (word2vec / DL4J
// filter the sentence before windowing); len = tokens kept.  One 16-lane group per walk: lane j takes tokens j, j + 16, ... (coalesced
// 64-byte reads and writes; one thread per walk, every thread striding through its own row, ran 6.3 ms per 8 M walks of 24 tokens)
__global__ void __launch_bounds__(256) k_remap_compact(const int32_t* __restrict__ walks, int64_t n_rows, int32_t L, const int32_t* __restrict__ remap,
                                                        int32_t NV, int32_t* __restrict__ sen, int64_t* __restrict__ len_out) {
    const int lane = threadIdx.x & 15, sh = threadIdx.x & 48;
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    if (r >= n_rows) return;
    const int32_t* in = walks + r * L;
    int32_t* out = sen + r * L;
    int len = 0;
    for (int j0 = 0; j0 < L; j0 += 16) {
        const int j = j0 + lane;
        int32_t v = -1;
        if (j < L) { const int32_t t = in[j]; if (t >= 0 && t < NV) v = remap[t]; }
        const unsigned keep = (unsigned)(__ballot(v >= 0) >> sh) & 0xFFFFu;
        if (v >= 0) out[len + __popc(keep & ((1u << lane) - 1u))] = v;
        len += __popc(keep);
    }
    for (int j = len + lane; j < L; j += 16) out[j] = -1;
    if (lane == 0) len_out[r] = len;
}

// ------------------------------------------------------------------------------------------ host side
extern "C" int dge_count_tokens(const dge_walks* w, int64_t row0, int64_t n_rows, int32_t n_vertices, int64_t* d_counts) {
    if (!w || !d_counts || row0 < 0 || n_rows < 0 || row0 + n_rows > w->n || n_vertices <= 0) DGE_FAIL(DGE_ERR_ARG, "dge_count_tokens: bad argument");
    DGE_HIP(hipSetDevice(w->device));
    int64_t n = n_rows * w->L;
    if (n == 0) return DGE_OK;
    // d_counts is accumulated into: whatever the caller's streams still do to it comes first, and so does a model's launch that still writes the corpus
    // (dge_model_walk_and_train) — the one wait for the device covers both; stream 0 is then ordered behind everything this call can depend on
    DGE_HIP(hipDeviceSynchronize());
    dge_walks_settled(w);
    unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_count_tokens, dim3(blocks), dim3(256), 0, 0, w->d + row0 * w->L, n, n_vertices, (unsigned long long*)d_counts);
    DGE_HIP(hipGetLastError());
    DGE_HIP(hipStreamSynchronize(0));
    return DGE_OK;
}

static void model_release(dge_model* m) {
    dge_table_free(m->d_syn0); dge_table_free(m->d_syn1neg); dge_dev_free(m->d_locks); dge_dev_free(m->d_ctab);
    dge_dev_free(m->d_run_base); dge_dev_free(m->d_run_row); dge_dev_free(m->d_exc_slot); dge_dev_free(m->d_exc_row);
    dge_dev_free(m->d_snap); dge_dev_free(m->d_vocab_ids);
    dge_table_free(m->d_syn1); dge_dev_free(m->d_hs_off); dge_dev_free(m->d_hs_points); dge_dev_free(m->d_hs_codes);
    dge_dev_free(m->d_counts); dge_dev_free(m->d_remap); dge_dev_free(m->d_exp);
    dge_dev_free(m->d_sen); dge_dev_free(m->d_len); dge_dev_free(m->d_wb); dge_dev_free(m->d_scan_tmp); dge_dev_free(m->d_counters);
    dge_sorted_release(m);
    if (m->ev_peer) (void)hipEventDestroy(m->ev_peer);
    for (auto& e : m->pending) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    if (m->own_stream && m->stream) (void)hipStreamDestroy(m->stream);
}

extern "C" void dge_model_free(dge_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    model_release(m);
    delete m;
}

extern "C" int dge_model_set_stream(dge_model* m, void* hip_stream) {
    if (!m) DGE_FAIL(DGE_ERR_ARG, "dge_model_set_stream: null model");
    DGE_HIP(hipSetDevice(m->device));
    DGE_HIP(hipStreamSynchronize(m->stream));
    if (m->own_stream && m->stream) (void)hipStreamDestroy(m->stream);
    m->stream = (hipStream_t)hip_stream;
    m->own_stream = false;
    return DGE_OK;
}

static bool dim_supported(int dch) { return dch == 1 || dch == 2 || dch == 3 || dch == 4 || dch == 6 || dch == 8; }

extern "C" int dge_model_create(int device, const dge_train_config* cfg, const int64_t* d_counts, dge_model** out) {
    if (!out || !cfg || !d_counts) DGE_FAIL(DGE_ERR_ARG, "dge_model_create: null argument");
    *out = nullptr;
    if (cfg->dim <= 0 || cfg->window <= 0 || cfg->negative < 0 || cfg->n_vertices <= 0 || cfg->epochs < 0 || cfg->workers < 0)
        DGE_FAIL(DGE_ERR_ARG, "dge_model_create: dim/window/n_vertices must be positive, negative/epochs/workers non-negative");
    int dch = (cfg->dim + 63) / 64;
    if (!dim_supported(dch)) dch = dch <= 6 ? 6 : 8;
    if (cfg->dim > 512) DGE_FAIL(DGE_ERR_ARG, "dge_model_create: dim %d > 512 is not supported", cfg->dim);
    if (cfg->update_policy < 0 || cfg->update_policy == 4 || cfg->update_policy > 8) DGE_FAIL(DGE_ERR_ARG, "dge_model_create: unknown update_policy %d", cfg->update_policy);
    if (cfg->use_hs && cfg->update_policy != 0 && cfg->update_policy != 2 && cfg->update_policy != 3)
        DGE_FAIL(DGE_ERR_ARG, "dge_model_create: use_hs runs under update_policy 0 (auto), 2 or 3, not %d", cfg->update_policy);
    int rc = dge_require_device(device);
    if (rc) return rc;
    DGE_HIP(hipDeviceSynchronize());      // d_counts may have been produced on the caller's streams (count kernel, all-reduce)
    dge_model* m = new dge_model();
    m->device = device;
    m->cfg = *cfg;
    if (m->cfg.table_size <= 0) m->cfg.table_size = 100000000LL;
    if (m->cfg.table_size >= 0x7fffffffLL) { delete m; DGE_FAIL(DGE_ERR_ARG, "dge_model_create: table_size must be < 2^31"); }
    m->D = cfg->dim; m->stride = dch * 64; m->NV = cfg->n_vertices; m->T = m->cfg.table_size;
    hipError_t he = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
    if (he != hipSuccess) { delete m; DGE_FAIL(DGE_ERR_DEVICE, "hipStreamCreate failed"); }
    m->own_stream = true;
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, device) == hipSuccess) m->n_cus = prop.multiProcessorCount; }
    hipStream_t st = m->stream;
    const int32_t NV = m->NV;

#define MC(expr) do { int rc__ = (expr); if (rc__) { model_release(m); delete m; return rc__; } } while (0)
#define MH(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) { dge_set_error("HIP error %s at %s:%d", hipGetErrorName(e__), __FILE__, __LINE__); model_release(m); delete m; return DGE_ERR_DEVICE; } } while (0)

    // --- vocabulary: stable descending sort on count (ids ascending inside a tie), keep count >= min_count
    dge_tmp<int32_t> d_ids, d_ids_sorted; dge_tmp<int64_t> d_cnt_sorted; dge_tmp<unsigned long long> d_kept; dge_tmp<char> d_tmp;
    MC(d_ids.alloc((size_t)NV)); MC(d_ids_sorted.alloc((size_t)NV)); MC(d_cnt_sorted.alloc((size_t)NV));
    MC(d_kept.alloc(2));
    hipLaunchKernelGGL(k_iota_i32, dim3(dge_grid_for(NV, 256)), dim3(256), 0, st, d_ids.p, (int64_t)NV);
    size_t tmp_bytes = 0;
    MH(hipcub::DeviceRadixSort::SortPairsDescending(nullptr, tmp_bytes, d_counts, d_cnt_sorted.p, d_ids.p, d_ids_sorted.p, NV, 0, 64, st));
    MC(d_tmp.alloc(tmp_bytes));
    MH(hipcub::DeviceRadixSort::SortPairsDescending((void*)d_tmp.p, tmp_bytes, d_counts, d_cnt_sorted.p, d_ids.p, d_ids_sorted.p, NV, 0, 64, st));
    MH(hipMemsetAsync(d_kept.p, 0, 2 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_count_kept, dim3(std::min<unsigned>(dge_grid_for(NV, 256), 2048u)), dim3(256), 0, st, d_cnt_sorted.p, (int64_t)NV,
                       (int64_t)cfg->min_count, d_kept.p);
    unsigned long long kept = 0;
    MH(hipMemcpyAsync(&kept, d_kept.p, sizeof(kept), hipMemcpyDeviceToHost, st));
    MH(hipStreamSynchronize(st));
    const int64_t V = (int64_t)kept;
    m->V = V;
    // the two tables and their lock words first: before the unigram table and the 0.8 GB of temporaries its construction takes
    const size_t tab = (size_t)V * (size_t)m->stride;
    m->ctab_blocks = (m->T + DGE_CTAB_SLOTS - 1) / DGE_CTAB_SLOTS;
    // syn1neg first: fast memory is scarce on some boxes, and a pair touches K + 1 rows of syn1neg for one of syn0 (syn1neg in fast memory and syn0 in slow:
    // 415 ms per launch; the other way round 423-456).  The lock words and the negative-sampling table are too small for the probe to classify (cache resident
    // when probed alone) and do NOT share a table's allocation: a table with them appended (511 MiB instead of 487) never landed in fast memory in 32 tries,
    // on any of three boxes — allocations of 511 ... 520 MiB never do (scripts/micro/size_class.hip) — so their placement is left to dge_model_tune_placement (sgns_place.hip).
    MC(dge_table_alloc(&m->d_syn1neg, tab + 64, device, st, &m->placed_seen[1], &m->placed_best[1], &m->placed_worst[1]));
    MC(dge_table_alloc(&m->d_syn0, tab + 64, device, st, &m->placed_seen[0], &m->placed_best[0], &m->placed_worst[0]));
    MC(dge_dev_alloc(&m->d_locks, 2 * ((size_t)V + 1)));      // [0,V]: syn1neg rows, [V+1,2V+1]: syn0 rows
    MC(dge_dev_alloc(&m->d_ctab, (size_t)m->ctab_blocks + 1));
    MC(dge_dev_alloc(&m->d_vocab_ids, (size_t)V)); MC(dge_dev_alloc(&m->d_counts, (size_t)V)); MC(dge_dev_alloc(&m->d_remap, (size_t)NV));
    if (V) {
        MH(hipMemcpyAsync(m->d_vocab_ids, d_ids_sorted.p, V * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        MH(hipMemcpyAsync(m->d_counts, d_cnt_sorted.p, V * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    }
    MH(hipMemsetAsync(m->d_remap, 0xFF, (size_t)NV * sizeof(int32_t), st));
    if (V) hipLaunchKernelGGL(k_scatter_remap, dim3(dge_grid_for(V, 256)), dim3(256), 0, st, m->d_vocab_ids, V, m->d_remap);
    m->h_counts.resize((size_t)V); m->h_vocab_ids.resize((size_t)V);
    if (V) {
        MH(hipMemcpyAsync(m->h_counts.data(), m->d_counts, V * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        MH(hipMemcpyAsync(m->h_vocab_ids.data(), m->d_vocab_ids, V * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    MH(hipStreamSynchronize(st));
    m->stats = schedule_stats(m->h_counts.data(), V, m->D, m->stride, m->n_cus);

    // --- unigram^0.75 cumulative (word2vec.c InitUnigramTable's running d1; a serial double sum by definition)
    dge_tmp<int32_t> d_flat;                                 // word2vec's one-row-per-slot table: a temporary, the trainers read its rank-block form
    MC(d_flat.alloc((size_t)m->T));
    if (V > 0) {
        std::vector<double> cum((size_t)V);
        const double twp = m->stats.neg_norm, power = 0.75;
        double d1 = 0.0;
        for (int64_t i = 0; i < V; i++) { d1 = (i == 0) ? pow((double)m->h_counts[0], power) / twp : d1 + pow((double)m->h_counts[(size_t)i], power) / twp; cum[(size_t)i] = d1; }
        dge_tmp<double> d_cum; dge_tmp<int32_t> d_g, d_m; dge_tmp<char> d_tmp2;
        MC(d_cum.alloc((size_t)V)); MC(d_g.alloc((size_t)m->T)); MC(d_m.alloc((size_t)m->T));
        MH(hipMemcpyAsync(d_cum.p, cum.data(), V * sizeof(double), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_table_chase, dim3(dge_grid_for(m->T, 256)), dim3(256), 0, st, d_cum.p, V, m->T, d_g.p);
        tmp_bytes = 0;
        MH(hipcub::DeviceScan::ExclusiveScan(nullptr, tmp_bytes, d_g.p, d_m.p, hipcub::Min(), (int32_t)0, m->T, st));
        MC(d_tmp2.alloc(tmp_bytes));
        MH(hipcub::DeviceScan::ExclusiveScan((void*)d_tmp2.p, tmp_bytes, d_g.p, d_m.p, hipcub::Min(), (int32_t)0, m->T, st));
        hipLaunchKernelGGL(k_table_fill, dim3(dge_grid_for(m->T, 256)), dim3(256), 0, st, d_m.p, V, m->T, d_flat.p);
        MH(hipStreamSynchronize(st));
        // --- the run form of the table, if this vocabulary has one (neg_row_by_runs): runs of adjacent rows of equal count, checked against the table
        if (m->T < 0xFFFFFFFFll && g_dge_tuning[DGE_TUNE_TABLE_RUNS] != 0) {
            std::vector<double> rb(DGE_RUN_MAX, std::numeric_limits<double>::infinity());
            std::vector<uint32_t> rr(DGE_RUN_MAX + 1, (uint32_t)V);
            // the runs are collected from the vocabulary's END — the tail is where equal counts abound — until the arrays are full; head rows in front of the
            // first run keep the table look-up (cfg3: 1 716 runs cover its whole vocabulary of a million rows, counts 2 .. 6 905, and match the table in
            // every one of its 1e8 slots; a vocabulary of several thousand distinct counts keeps its most frequent rows on the table)
            int runs = 0; int64_t i = V;
            std::vector<int64_t> starts;
            const int max_runs = g_dge_tuning[DGE_TUNE_TABLE_RUNS] > 0 ? (int)std::min<int64_t>(g_dge_tuning[DGE_TUNE_TABLE_RUNS], DGE_RUN_MAX - 2) : DGE_RUN_MAX - 2;
            while (i > 0 && runs < max_runs) {
                int64_t j = i - 1;
                while (j > 0 && m->h_counts[(size_t)j - 1] == m->h_counts[(size_t)i - 1]) j--;
                starts.push_back(j); runs++; i = j;
            }
            std::reverse(starts.begin(), starts.end());
            for (int r = 0; r < runs; r++) {
                const int64_t r0 = starts[(size_t)r];
                rb[(size_t)r] = r0 == 0 ? 0.0 : cum[(size_t)r0 - 1];
                rr[(size_t)r] = (uint32_t)r0;
            }
            rb[(size_t)runs] = cum[(size_t)V - 1];       // the boundary behind the last run (behind it: +inf, row V)
            {   // whether the run form is kept is decided by comparing it with the table
                dge_tmp<unsigned> d_nbad; dge_tmp<uint32_t> d_bs; dge_tmp<int32_t> d_br;
                const unsigned cap = 4096;
                MC(d_nbad.alloc(1)); MC(d_bs.alloc(cap)); MC(d_br.alloc(cap));
                MC(dge_dev_alloc(&m->d_run_base, DGE_RUN_MAX)); MC(dge_dev_alloc(&m->d_run_row, DGE_RUN_MAX + 1));
                MC(dge_dev_alloc(&m->d_exc_slot, DGE_RUN_EXC)); MC(dge_dev_alloc(&m->d_exc_row, DGE_RUN_EXC));
                MH(hipMemcpyAsync(m->d_run_base, rb.data(), DGE_RUN_MAX * sizeof(double), hipMemcpyHostToDevice, st));
                MH(hipMemcpyAsync(m->d_run_row, rr.data(), (DGE_RUN_MAX + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
                std::vector<uint32_t> es(DGE_RUN_EXC, 0xFFFFFFFFu); std::vector<int32_t> er(DGE_RUN_EXC, 0);
                unsigned n_bad = 0; int n_exc = 0; bool good = false;
                for (int round = 0; round < 2; round++) {      // first without exceptions (collects them), then with them (must leave nothing)
                    MH(hipMemsetAsync(d_nbad.p, 0, sizeof(unsigned), st));
                    MH(hipMemcpyAsync(m->d_exc_slot, es.data(), DGE_RUN_EXC * sizeof(uint32_t), hipMemcpyHostToDevice, st));
                    MH(hipMemcpyAsync(m->d_exc_row, er.data(), DGE_RUN_EXC * sizeof(int32_t), hipMemcpyHostToDevice, st));
                    hipLaunchKernelGGL(k_runs_verify, dim3(dge_grid_for(m->T, 256)), dim3(256), 0, st, d_flat.p, m->T, m->d_run_base, m->d_run_row, m->d_exc_slot, m->d_exc_row,
                                       n_exc, 1.0 / (double)m->T, V, d_nbad.p, d_bs.p, d_br.p, cap);
                    MH(hipMemcpyAsync(&n_bad, d_nbad.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
                    MH(hipStreamSynchronize(st));
                    if (round == 1) { good = n_bad == 0; break; }
                    if (n_bad > DGE_RUN_EXC) break;
                    if (n_bad > 0) {
                        std::vector<uint32_t> bs(n_bad); std::vector<int32_t> br(n_bad);
                        MH(hipMemcpy(bs.data(), d_bs.p, n_bad * sizeof(uint32_t), hipMemcpyDeviceToHost));
                        MH(hipMemcpy(br.data(), d_br.p, n_bad * sizeof(int32_t), hipMemcpyDeviceToHost));
                        std::vector<size_t> order(n_bad);
                        for (size_t q = 0; q < n_bad; q++) order[q] = q;
                        std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return bs[x] < bs[y]; });
                        for (size_t q = 0; q < n_bad; q++) { es[q] = bs[order[q]]; er[q] = br[order[q]]; }
                    }
                    n_exc = (int)n_bad;
                }
                if (good) { m->n_runs = runs; m->n_exc = n_exc; }
            }
        }
    } else {
        MH(hipMemsetAsync(d_flat.p, 0, (size_t)m->T * sizeof(int32_t), st));
    }
    hipLaunchKernelGGL(k_table_pack, dim3(dge_grid_for(m->ctab_blocks * 3, 256)), dim3(256), 0, st, d_flat.p, m->T, m->ctab_blocks, (uint32_t*)m->d_ctab);
    MH(hipStreamSynchronize(st));

    // --- sigmoid LUT (word2vec.c expTable) and weights
    {
        float e[EXP_TABLE_SIZE];
        for (int i = 0; i < EXP_TABLE_SIZE; i++) {
            // C semantics of word2vec.c: the argument is a float expression, exp() itself is the DOUBLE function
            float x = (float)exp((double)((i / (float)EXP_TABLE_SIZE * 2 - 1) * MAX_EXP));
            e[i] = x / (x + 1);
        }
        MC(dge_dev_alloc(&m->d_exp, EXP_TABLE_SIZE));
        MH(hipMemcpyAsync(m->d_exp, e, sizeof(e), hipMemcpyHostToDevice, st));
        MH(hipStreamSynchronize(st));
    }
    MH(hipMemsetAsync(m->d_syn1neg, 0, (tab + 64) * sizeof(float), st));
    if (V) hipLaunchKernelGGL(k_init_syn0, dim3(dge_grid_for(V, 256)), dim3(256), 0, st, m->d_syn0, V, m->D, m->stride, cfg->seed);
    if (cfg->use_hs) {
        // inner-node table (V rows allocated, V-1 used: the tables stay the same size for the delta exchange) and paths
        std::vector<int64_t> node_w;
        const int longest = dge_huffman_paths(m->h_counts.data(), V, m->h_hs_off, m->h_hs_points, m->h_hs_codes, &node_w);
        schedule_stats_hs(m->stats, node_w);
        // (behind the table: HS_REP_ROWS spare rows for k_sgns_train_hsw's copies of the busiest inner nodes — zero between launches)
        MC(dge_table_alloc(&m->d_syn1, tab + 64 + (size_t)HS_REP_ROWS * m->stride, device, st, &m->placed_seen[2], &m->placed_best[2], &m->placed_worst[2]));
        MH(hipMemsetAsync(m->d_syn1, 0, (tab + 64 + (size_t)HS_REP_ROWS * m->stride) * sizeof(float), st));
        if (longest > 40) { model_release(m); delete m; DGE_FAIL(DGE_ERR_ARG, "dge_model_create: a Huffman code of %d bits exceeds word2vec's MAX_CODE_LENGTH 40", longest); }
        MC(dge_dev_alloc(&m->d_hs_off, (size_t)V + 1)); MC(dge_dev_alloc(&m->d_hs_points, m->h_hs_points.size())); MC(dge_dev_alloc(&m->d_hs_codes, (size_t)V));
        MH(hipMemcpyAsync(m->d_hs_off, m->h_hs_off.data(), ((size_t)V + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        if (!m->h_hs_points.empty()) MH(hipMemcpyAsync(m->d_hs_points, m->h_hs_points.data(), m->h_hs_points.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        if (V) MH(hipMemcpyAsync(m->d_hs_codes, m->h_hs_codes.data(), (size_t)V * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    }
    MH(hipMemsetAsync(m->d_locks, 0, 2 * ((size_t)V + 1) * sizeof(int), st));
    MC(dge_dev_alloc(&m->d_counters, 8));       // pairs, words, the lock kernels' walk counter, their watchdog flag; the block kernels' lock statistics: pairs put back, rounds that left rows unwon, rounds
    MH(hipMemsetAsync(m->d_counters, 0, 8 * sizeof(unsigned long long), st));
    MH(hipStreamSynchronize(st));
    MH(hipGetLastError());
#undef MC
#undef MH
    *out = m;
    return DGE_OK;
}

static int ensure_work(dge_model* m, int64_t n_rows, int32_t L) {
    if (n_rows <= m->cap_rows && L <= m->cap_L) return DGE_OK;
    DGE_HIP(hipStreamSynchronize(m->stream));
    dge_dev_free(m->d_sen); dge_dev_free(m->d_len); dge_dev_free(m->d_wb); dge_dev_free(m->d_scan_tmp);
    m->d_sen = nullptr; m->d_len = nullptr; m->d_wb = nullptr; m->d_scan_tmp = nullptr;
    int64_t nr = std::max(n_rows, m->cap_rows); int32_t nl = std::max(L, m->cap_L);
    int rc;
    if ((rc = dge_dev_alloc(&m->d_sen, (size_t)(nr * nl)))) return rc;
    if ((rc = dge_dev_alloc(&m->d_len, (size_t)nr))) return rc;
    if ((rc = dge_dev_alloc(&m->d_wb, (size_t)nr))) return rc;
    size_t bytes = 0;
    DGE_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, m->d_len, m->d_wb, nr, m->stream));
    DGE_HIP(hipMalloc(&m->d_scan_tmp, bytes ? bytes : 1));
    m->scan_tmp_bytes = bytes;
    m->cap_rows = nr; m->cap_L = nl; m->seen_gen = 0;
    return DGE_OK;
}

// the trainer kernels are compiled per row width in sgns_train_dch.hip (one object per DCH)
void dge_launch_train_dch1(const TrainParams& p, const TrainPlan& plan, hipStream_t st);
void dge_launch_train_dch2(const TrainParams& p, const TrainPlan& plan, hipStream_t st);
void dge_launch_train_dch3(const TrainParams& p, const TrainPlan& plan, hipStream_t st);
void dge_launch_train_dch4(const TrainParams& p, const TrainPlan& plan, hipStream_t st);
void dge_launch_train_dch6(const TrainParams& p, const TrainPlan& plan, hipStream_t st);
void dge_launch_train_dch8(const TrainParams& p, const TrainPlan& plan, hipStream_t st);

// Launch timing: a pair of events per kernel launch, read by dge_model_stats.  A host that trains in a long loop without asking for
// stats must not pile up event handles: launches of one model complete in stream order, so once 64 pairs are pending the finished
// ones at the front are folded into the totals and destroyed.
static void reap_finished_events(dge_model* m) {
    size_t n = 0;
    while (n < m->pending.size() && hipEventQuery(m->pending[n].b) == hipSuccess) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, m->pending[n].a, m->pending[n].b) == hipSuccess) { if (m->pending[n].kind == 0) m->kernel_ms += ms; else m->walk_ms += ms; }
        (void)hipEventDestroy(m->pending[n].a); (void)hipEventDestroy(m->pending[n].b);
        n++;
    }
    m->pending.erase(m->pending.begin(), m->pending.begin() + (ptrdiff_t)n);
}
static int timing_begin(dge_model* m, EventPair& ev, int kind) {
    if (m->pending.size() >= 64) reap_finished_events(m);
    ev.kind = kind; ev.a = nullptr; ev.b = nullptr;
    DGE_HIP(hipEventCreate(&ev.a));
    if (hipEventCreate(&ev.b) != hipSuccess) { (void)hipEventDestroy(ev.a); DGE_FAIL(DGE_ERR_DEVICE, "hipEventCreate failed"); }
    if (hipEventRecord(ev.a, m->stream) != hipSuccess) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); DGE_FAIL(DGE_ERR_DEVICE, "hipEventRecord failed"); }
    return DGE_OK;
}
static int timing_end(dge_model* m, EventPair& ev, int rc_so_far) {
    if (rc_so_far != DGE_OK || hipEventRecord(ev.b, m->stream) != hipSuccess) {
        (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b);
        if (rc_so_far != DGE_OK) return rc_so_far;
        DGE_FAIL(DGE_ERR_DEVICE, "hipEventRecord failed");
    }
    m->pending.push_back(ev);
    return DGE_OK;
}

// k_sgns_train_hsw's copies of the busiest inner nodes: row j of `rows` += its HS_REP - 1 copies, which are cleared (one workgroup a node; runs behind the trainer)
__global__ void k_hs_rep_fold(float* rows, float* rep, int32_t n_rep, int32_t stride) {
    const int j = blockIdx.x;
    for (int e = threadIdx.x; e < stride; e += blockDim.x) {
        float v = rows[(size_t)j * stride + e];
        for (int c = 0; c < HS_REP - 1; c++) { float* q = rep + ((size_t)c * n_rep + j) * stride + e; v += *q; *q = 0.f; }
        rows[(size_t)j * stride + e] = v;
    }
}

static int train_rows(dge_model* m, const int32_t* d_rows, int64_t n_rows, int32_t L, int64_t walk_index_base, int32_t epoch,
                      int64_t words_before, double words_scale, int64_t total_walks, uint64_t corpus_gen) {
    if (n_rows == 0 || m->V == 0) return DGE_OK;
    int rc = ensure_work(m, n_rows, L);
    if (rc) return rc;
    hipStream_t st = m->stream;
    // vocabulary rows of the walks, left-packed, and the words that precede each walk: kept while the same unchanged rows come again
    // (the N episodes of a block-schedule batch train the same walks N times)
    if (!(m->seen_rows == d_rows && m->seen_n == n_rows && m->seen_L == L && m->seen_gen == corpus_gen && corpus_gen != 0)) {
        hipLaunchKernelGGL(k_remap_compact, dim3(dge_grid_for(n_rows * 16, 256)), dim3(256), 0, st, d_rows, n_rows, L, m->d_remap, m->NV, m->d_sen, m->d_len);
        size_t bytes = m->scan_tmp_bytes;
        DGE_HIP(hipcub::DeviceScan::ExclusiveSum(m->d_scan_tmp, bytes, m->d_len, m->d_wb, n_rows, st));
        m->seen_rows = d_rows; m->seen_n = n_rows; m->seen_L = L; m->seen_gen = corpus_gen;
    }

    int64_t knob[DGE_TUNE_COUNT];      // one snapshot of the tuning knobs for the whole launch
    for (int k = 0; k < DGE_TUNE_COUNT; k++) knob[k] = g_dge_tuning[k];

    TrainParams p;
    p.sen = m->d_sen; p.len = m->d_len; p.wb = m->d_wb;
    p.syn0 = m->d_syn0; p.syn1neg = m->d_syn1neg; p.exp_table = m->d_exp;
    p.ctab = m->d_ctab;
    p.run_base = m->d_run_base; p.run_row = m->d_run_row; p.exc_slot = m->d_exc_slot; p.exc_row = m->d_exc_row;
    p.n_runs = knob[DGE_TUNE_TABLE_RUNS] == 0 ? 0 : m->n_runs; p.n_exc = m->n_exc; p.T_inv = 1.0 / (double)std::max<int64_t>(m->T, 1);
    p.n_rows = n_rows; p.L = L; p.W = m->cfg.window; p.K = m->cfg.negative; p.stride = m->stride;
    p.V = m->V; p.T = m->T; p.seed = m->cfg.seed;
    p.T_magic = ~0ull / (uint64_t)std::max<int64_t>(m->T, 1); p.W_magic = ~0ull / (uint64_t)std::max(m->cfg.window, 1);
    p.gidx_base = (int64_t)epoch * total_walks + walk_index_base;
    p.words_done_base = (int64_t)epoch * m->stats.total_words + words_before;
    p.all_words = (int64_t)std::max(m->cfg.epochs, 1) * m->stats.total_words;
    p.words_scale = words_scale;
    p.alpha0 = m->cfg.alpha; p.min_alpha = m->cfg.min_alpha;
    p.D = m->D;
    p.counters = m->d_counters;
    p.locks = m->d_locks;
    p.syn1 = m->d_syn1; p.hs_off = m->d_hs_off; p.hs_points = m->d_hs_points; p.hs_codes = m->d_hs_codes;
    p.part_n = m->part_n; p.part_ctx = m->part_ctx; p.part_tgt = m->part_tgt;
    p.N_magic = 0xFFFFFFFFu / (uint32_t)std::max(m->part_n, 1);
    p.big_seg_shift = 0;
    p.filler_row = (int32_t)(0xFFFFFFF0u / ((uint32_t)m->stride * 4u)) - 1;      // offset + the largest in-row displacement stays below 2^32
    if (knob[DGE_TUNE_SEGMENT_SHIFT] >= 0) p.big_seg_shift = (int32_t)knob[DGE_TUNE_SEGMENT_SHIFT];   // tests: several segments on a small table

    // the schedule (sgns_plan.h) and what it sets
    TrainPlan plan;
    if ((rc = plan_train(m->cfg, m->stats, m->h_counts.data(), m->part_n, n_rows, L, knob, m->block_head_memo, &plan))) DGE_FAIL(rc, "%s", plan.error);
    p.n_workers = plan.workers;
    p.hot_rows = plan.hot_rows; p.acc_rows = plan.acc_rows; p.acc_drain = plan.acc_drain; p.syn0_free = plan.syn0_free;
    p.hs_hot0 = plan.hs_hot0; p.hs_n_hot = plan.hs_n_hot; p.hs_drain = plan.hs_drain; p.hs_cold = plan.hs_cold; p.hs_wave = plan.hs_wave;
    p.hs_rep0 = plan.hs_rep0; p.hs_rep_n = plan.hs_rep_n; for (int k = 0; k < HS_REP; k++) p.hs_rep_thr[k] = plan.hs_rep_thr[k];
    p.wd_ticks = plan.wd_ticks;
    if (plan.runs_off) p.n_runs = 0;
    p.next_walk = plan.walk_counter ? m->d_counters + 2 : nullptr;
    if (plan.walk_counter) DGE_HIP(hipMemsetAsync(p.next_walk, 0, sizeof(unsigned long long), st));
    // k_sgns_train_hsw's copies of the busiest inner nodes must be zero when the launch starts.  k_hs_rep_fold leaves them so behind every launch; an abandoned launch
    // (an error between the two) would not — so they are cleared here as well (hs_rep_n x 15 rows, < 1 MB)
    if (p.hs_rep_n > 0) DGE_HIP(hipMemsetAsync(m->d_syn1 + (size_t)m->V * m->stride, 0, (size_t)(HS_REP - 1) * (size_t)p.hs_rep_n * (size_t)m->stride * sizeof(float), st));

    EventPair ev;
    if ((rc = timing_begin(m, ev, 0))) return rc;
    if (plan.form == TrainForm::Sorted) rc = dge_sorted_train(m, p);
    else if (plan.form == TrainForm::SmallRows) hipLaunchKernelGGL((k_sgns_train_small<32>), dim3(plan.blocks), dim3(plan.threads), 0, st, p);
    else
    switch (m->stride / 64) {
        case 1: dge_launch_train_dch1(p, plan, st); break;
        case 2: dge_launch_train_dch2(p, plan, st); break;
        case 3: dge_launch_train_dch3(p, plan, st); break;
        case 4: dge_launch_train_dch4(p, plan, st); break;
        case 6: dge_launch_train_dch6(p, plan, st); break;
        default: dge_launch_train_dch8(p, plan, st); break;
    }
    if (p.hs_rep_n > 0)      // the copies of the busiest inner nodes go back into their rows (and are zero again for the next launch's memset to find nothing)
        hipLaunchKernelGGL(k_hs_rep_fold, dim3((unsigned)p.hs_rep_n), dim3(128), 0, st, m->d_syn1 + (size_t)p.hs_rep0 * m->stride, m->d_syn1 + (size_t)m->V * m->stride, p.hs_rep_n, m->stride);
    if ((rc = timing_end(m, ev, rc))) return rc;
    m->launches++;
    m->last_plan = plan; m->has_plan = true;
    if (plan.form != TrainForm::Sorted) DGE_HIP(hipGetLastError());
    return DGE_OK;
}

extern "C" int dge_model_train(dge_model* m, const dge_walks* w, int64_t row0, int64_t n_rows, int64_t walk_index_base, int32_t epoch,
                               int64_t words_before, double words_scale, int64_t total_walks) {
    if (!m || !w || row0 < 0 || n_rows < 0 || row0 + n_rows > w->n || epoch < 0 || words_before < 0 || !(words_scale > 0))
        DGE_FAIL(DGE_ERR_ARG, "dge_model_train: bad argument");
    if (w->device != m->device) DGE_FAIL(DGE_ERR_ARG, "dge_model_train: corpus and model live on different devices");
    DGE_HIP(hipSetDevice(m->device));
    if (total_walks <= 0) total_walks = w->n;
    // the launch is left queued: it goes behind a launch of another model that still writes the corpus, and the corpus remembers it (dge_internal.h)
    int rc = dge_walks_order(w, m->stream);
    if (!rc) rc = train_rows(m, w->d + row0 * w->L, n_rows, w->L, walk_index_base, epoch, words_before, words_scale, total_walks, w->gen);
    if (!rc) rc = dge_walks_mark(w, m->stream);
    return rc;
}

extern "C" int dge_model_walk_and_train(dge_model* m, const dge_graph* g, dge_walks* w, int64_t row0, int64_t n_rows, int64_t walk_seed,
                                        int64_t walk_index_base, int32_t epoch, int64_t words_before, double words_scale, int64_t total_walks) {
    if (!m || !g || !w || row0 < 0 || n_rows < 0 || row0 + n_rows > w->n) DGE_FAIL(DGE_ERR_ARG, "dge_model_walk_and_train: bad argument");
    if (!g->alias_built) DGE_FAIL(DGE_ERR_STATE, "dge_model_walk_and_train: alias tables not built");
    if (w->device != m->device || g->device != m->device) DGE_FAIL(DGE_ERR_ARG, "dge_model_walk_and_train: handles live on different devices");
    DGE_HIP(hipSetDevice(m->device));
    w->gen = dge_next_generation();
    int rc = dge_walks_order(w, m->stream);      // the rows are written: behind every launch of another model that still reads them
    if (rc) return rc;
    EventPair ev;
    rc = timing_begin(m, ev, 1);
    if (rc) return rc;
    rc = timing_end(m, ev, dge_launch_walks_strided(g, m->stream, w->d + row0 * w->L, n_rows, w->L, walk_seed, walk_index_base, nullptr));
    if (!rc) rc = dge_walks_mark(w, m->stream);  // (the walk kernel is queued whatever becomes of the training launch)
    if (rc) return rc;
    if (total_walks <= 0) total_walks = w->n;
    rc = train_rows(m, w->d + row0 * w->L, n_rows, w->L, walk_index_base, epoch, words_before, words_scale, total_walks, w->gen);
    if (!rc) rc = dge_walks_mark(w, m->stream);
    return rc;
}

extern "C" int dge_train_sgns_device(const dge_walks* w, const dge_train_config* cfg, dge_model** out) {
    if (!w || !cfg || !out) DGE_FAIL(DGE_ERR_ARG, "dge_train_sgns_device: null argument");
    *out = nullptr;
    if (cfg->n_vertices <= 0) DGE_FAIL(DGE_ERR_ARG, "dge_train_sgns_device: n_vertices must be positive");
    DGE_HIP(hipSetDevice(w->device));
    int64_t* d_counts = nullptr;
    int rc = dge_dev_alloc(&d_counts, (size_t)cfg->n_vertices);
    if (rc) return rc;
    DGE_HIP(hipMemset(d_counts, 0, (size_t)cfg->n_vertices * sizeof(int64_t)));
    rc = dge_count_tokens(w, 0, w->n, cfg->n_vertices, d_counts);
    dge_model* m = nullptr;
    if (!rc) rc = dge_model_create(w->device, cfg, d_counts, &m);
    dge_dev_free(d_counts);
    if (rc) return rc;
    // The placement search first — where it can pay (results are unaffected: dge_model_tune_placement).  A pass of the search is 2 + 4 (candidates - 1)
    // probe launches of n_probe walks (a model that started well needs one pass), and what it can win is ~10 % of the training launches' time
    // (profiles/r03_placement.txt): it runs when a tenth of the projected training — epochs x walks — is more than one pass.  The reference's own
    // iterations(1) fit of cfg3 (10 M walks, 3.9 s) is below that: 1.3 - 8 s of probes would be a net loss there (round-3 verdict); 4 epochs are above.
    if (!rc && cfg->epochs > 0 && cfg->workers != 1 && m->V >= 262144 && w->n >= 262144) {
        const int candidates = 4;
        const int64_t n_probe = std::min<int64_t>(w->n / 8, 262144);
        if (0.10 * (double)cfg->epochs * (double)w->n > (double)(2 + 4 * (candidates - 1)) * (double)n_probe) {
            double before = 0, after = 0; int32_t moved = 0;
            rc = dge_model_tune_placement(m, w, 0, n_probe, candidates, &before, &after, &moved);
        }
    }
    for (int ep = 0; ep < cfg->epochs && !rc; ep++) rc = dge_model_train(m, w, 0, w->n, 0, ep, 0, 1.0, w->n);
    if (!rc) { hipError_t e = hipStreamSynchronize(m->stream); if (e != hipSuccess) { dge_set_error("training failed: %s", hipGetErrorName(e)); rc = DGE_ERR_DEVICE; } }
    if (!rc) { dge_train_stats st; rc = dge_model_stats(m, &st); }      // (a launch ended by the lock kernels' watchdog is an error of the fit, not a model)
    if (rc) { dge_model_free(m); return rc; }
    *out = m;
    return DGE_OK;
}

extern "C" int dge_train_sgns(int device, const int32_t* walks, int64_t n_walks, int32_t max_len, const dge_train_config* cfg, dge_model** out) {
    dge_walks* w = nullptr;
    int rc = dge_walks_from_host(device, walks, n_walks, max_len, &w);
    if (rc) return rc;
    rc = dge_train_sgns_device(w, cfg, out);
    dge_walks_free(w);
    return rc;
}

int dge_drain_events(dge_model* m) {
    if (m->pending.empty()) return DGE_OK;
    DGE_HIP(hipSetDevice(m->device));
    DGE_HIP(hipStreamSynchronize(m->stream));
    for (auto& e : m->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) { if (e.kind == 0) m->kernel_ms += ms; else m->walk_ms += ms; }
        (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b);
    }
    m->pending.clear();
    return DGE_OK;
}

extern "C" int dge_model_stats(const dge_model* mc, dge_train_stats* out) {
    dge_model* m = const_cast<dge_model*>(mc);
    if (!m || !out) DGE_FAIL(DGE_ERR_ARG, "dge_model_stats: null argument");
    int rc = dge_drain_events(m);
    if (rc) return rc;
    unsigned long long c[4] = {0, 0, 0, 0};
    DGE_HIP(hipMemcpy(c, m->d_counters, sizeof(c), hipMemcpyDeviceToHost));
    out->pairs = (int64_t)c[0]; out->words = (int64_t)c[1];
    out->kernel_ms = m->kernel_ms; out->walk_kernel_ms = m->walk_ms; out->launches = m->launches;
    if (c[3]) {     // a lock kernel's watchdog ended a launch (plan_train: wd_ticks): reported once, here — the first call that looks at the device after the launch
        DGE_HIP(hipMemsetAsync(m->d_counters + 3, 0, sizeof(unsigned long long), m->stream));
        DGE_HIP(hipStreamSynchronize(m->stream));
        DGE_FAIL(DGE_ERR_STATE, "a training launch was ended by its watchdog: %llu workers waited for row locks beyond the launch's time budget and left their walks untrained "
                 "(update_policy %d on this vocabulary: use 0 (auto) or 7)", c[3], m->cfg.update_policy);
    }
    return DGE_OK;
}

extern "C" int dge_model_table_runs(const dge_model* m, int32_t* n_runs, int32_t* n_exceptions) {
    if (!m) DGE_FAIL(DGE_ERR_ARG, "dge_model_table_runs: null model");
    if (n_runs) *n_runs = m->n_runs;
    if (n_exceptions) *n_exceptions = m->n_exc;
    return DGE_OK;
}

extern "C" int dge_model_schedule(const dge_model* m, int32_t* update_policy, int64_t* workers, int32_t* hot_rows) {
    if (!m) DGE_FAIL(DGE_ERR_ARG, "dge_model_schedule: null model");
    if (!m->has_plan) DGE_FAIL(DGE_ERR_STATE, "dge_model_schedule: nothing has been trained yet");
    if (update_policy) *update_policy = m->last_plan.reported_policy();
    if (workers) *workers = m->last_plan.workers;
    if (hot_rows) *hot_rows = m->last_plan.hot_rows;
    return DGE_OK;
}

extern "C" int dge_model_lock_stats(const dge_model* mc, int64_t* pairs_put_back, int64_t* rounds_short, int64_t* rounds) {
    dge_model* m = const_cast<dge_model*>(mc);
    if (!m) DGE_FAIL(DGE_ERR_ARG, "dge_model_lock_stats: null model");
    DGE_HIP(hipSetDevice(m->device));
    DGE_HIP(hipStreamSynchronize(m->stream));
    unsigned long long c[3] = {0, 0, 0};
    DGE_HIP(hipMemcpy(c, m->d_counters + 4, sizeof(c), hipMemcpyDeviceToHost));
    if (pairs_put_back) *pairs_put_back = (int64_t)c[0];
    if (rounds_short) *rounds_short = (int64_t)c[1];
    if (rounds) *rounds = (int64_t)c[2];
    return DGE_OK;
}

extern "C" int dge_model_kernel(const dge_model* m, char* buf, int32_t cap) {
    if (!m || !buf || cap <= 0) DGE_FAIL(DGE_ERR_ARG, "dge_model_kernel: bad argument");
    if (!m->has_plan) DGE_FAIL(DGE_ERR_STATE, "dge_model_kernel: nothing has been trained yet");
    snprintf(buf, (size_t)cap, "%s", m->last_plan.kernel_name().c_str());
    return DGE_OK;
}

extern "C" int dge_model_pair_loop(const dge_model* m, int32_t* loop, int32_t* slots) {
    if (!m) DGE_FAIL(DGE_ERR_ARG, "dge_model_pair_loop: null model");
    if (!m->has_plan) DGE_FAIL(DGE_ERR_STATE, "dge_model_pair_loop: nothing has been trained yet");
    if (loop) *loop = m->last_plan.window ? 1 : 0;
    if (slots) *slots = m->last_plan.window ? m->last_plan.win_slots : 0;
    return DGE_OK;
}

extern "C" int dge_model_reset_stats(dge_model* m) {
    if (!m) DGE_FAIL(DGE_ERR_ARG, "dge_model_reset_stats: null model");
    int rc = dge_drain_events(m);
    if (rc) return rc;
    // on the model's own stream (a non-blocking one: a null-stream memset is not ordered against it — a short launch right behind reset_stats lost a tenth of
    // its pair count to the memset landing late: tests/test_gpu_quality.py, round 4)
    DGE_HIP(hipMemsetAsync(m->d_counters, 0, 2 * sizeof(unsigned long long), m->stream));
    DGE_HIP(hipMemsetAsync(m->d_counters + 4, 0, 3 * sizeof(unsigned long long), m->stream));
    DGE_HIP(hipStreamSynchronize(m->stream));
    m->kernel_ms = 0; m->walk_ms = 0; m->launches = 0;
    return DGE_OK;
}

// which block of the multi-GPU schedule the coming launches train (the plan and the kernels read it; the partitions' copies: sgns_exchange.hip)
extern "C" int dge_model_set_partition(dge_model* m, int32_t n_parts, int32_t ctx_part, int32_t tgt_part) {
    if (!m) DGE_FAIL(DGE_ERR_ARG, "dge_model_set_partition: null model");
    if (n_parts <= 1) { m->part_n = 1; m->part_ctx = 0; m->part_tgt = 0; return DGE_OK; }
    if (ctx_part < 0 || ctx_part >= n_parts || tgt_part < 0 || tgt_part >= n_parts) DGE_FAIL(DGE_ERR_ARG, "dge_model_set_partition: partition out of range");
    if (m->V < n_parts) DGE_FAIL(DGE_ERR_ARG, "dge_model_set_partition: %d partitions for %lld vocabulary rows", n_parts, (long long)m->V);
    m->part_n = n_parts; m->part_ctx = ctx_part; m->part_tgt = tgt_part;
    return DGE_OK;
}
