// sgns_model.h — the trainer's handle (vocabulary + tables + per-call work buffers) and the few internals its translation units call across files:
// sgns.hip (creation and the launch path), sgns_sorted.hip (the owner-computes schedule), sgns_place.hip (table placement), sgns_io.hip (read-back,
// `.vec`), sgns_exchange.hip (partitions, deltas, RCCL).  Not in the build stamp: a change of layout that matters to a launch shows in the files that are.
#pragma once
#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "dge_internal.h"
#include "sgns_plan.h"

struct EventPair { hipEvent_t a, b; int kind; };

// ablation / test knobs (dge_set_tuning, include/dge.h): -1 = the library's own rule
extern std::atomic<int64_t> g_dge_tuning[DGE_TUNE_COUNT];      // (set from the host's thread, read by whichever thread launches: relaxed atomics, no ordering implied)

struct dge_sorted_work;       // buffers of the owner-computes schedule (sgns_sorted.hip)

struct dge_model {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    dge_train_config cfg{};
    int64_t V = 0;
    int32_t D = 0, stride = 0, NV = 0;
    int64_t T = 0;
    ScheduleStats stats;                        // what the launch rules read (sgns_plan.h: schedule_stats)
    BlockHeadMemo block_head_memo;              // block_head's latest answer (sgns_plan.h)
    int n_cus = 256;
    float *d_syn0 = nullptr, *d_syn1neg = nullptr, *d_snap = nullptr;
    int placed_seen[3] = {0, 0, 0}; double placed_best[3] = {0, 0, 0}, placed_worst[3] = {0, 0, 0};   // dge_table_alloc's report for syn0, syn1neg, syn1: candidates probed, their best and worst rate (GB/s)
    // hierarchical softmax (cfg.use_hs): inner-node table and the Huffman paths in CSR form
    float* d_syn1 = nullptr;
    int64_t* d_hs_off = nullptr; int32_t* d_hs_points = nullptr; uint64_t* d_hs_codes = nullptr;
    std::vector<int64_t> h_hs_off; std::vector<int32_t> h_hs_points; std::vector<uint64_t> h_hs_codes;
    std::vector<float> h_syn1;

    int32_t* d_vocab_ids = nullptr;
    int64_t* d_counts = nullptr;
    int32_t* d_remap = nullptr;
    uint4* d_ctab = nullptr; int64_t ctab_blocks = 0;   // word2vec's unigram table in rank-block form (neg_table_row)
    // ... and in run form (neg_row_by_runs) when the vocabulary has at most DGE_RUN_MAX distinct adjacent counts and the closed form matches the table
    // everywhere but in at most DGE_RUN_EXC slots; n_runs == 0: not available
    double* d_run_base = nullptr; uint32_t* d_run_row = nullptr; uint32_t* d_exc_slot = nullptr; int32_t* d_exc_row = nullptr;
    int32_t n_runs = 0, n_exc = 0;
    float* d_exp = nullptr;
    // per-call work buffers
    int64_t cap_rows = 0; int32_t cap_L = 0;
    int32_t* d_sen = nullptr; int64_t* d_len = nullptr; int64_t* d_wb = nullptr;
    void* d_scan_tmp = nullptr; size_t scan_tmp_bytes = 0;
    unsigned long long* d_counters = nullptr;   // [0]=pairs [1]=words
    int* d_locks = nullptr;                     // commit-lock word per syn1neg row
    // host mirrors for the read-back API
    std::vector<float> h_syn0, h_syn1neg;
    std::vector<int32_t> h_vocab_ids, h_table;
    std::vector<int64_t> h_counts;
    // stats
    std::vector<EventPair> pending;
    double kernel_ms = 0, walk_ms = 0;
    int64_t launches = 0;
    TrainPlan last_plan; bool has_plan = false;                                  // what the latest launch ran with (dge_model_schedule, dge_model_kernel)
    int32_t search_runs = 0, search_moved = 0; double search_ms_before = 0, search_ms_after = 0;      // dge_model_tune_placement's latest report
    int32_t part_n = 1, part_ctx = 0, part_tgt = 0;                              // block schedule (dge_model_set_partition)
    const int32_t* seen_rows = nullptr; int64_t seen_n = 0; int32_t seen_L = 0; uint64_t seen_gen = 0;   // what d_sen/d_len/d_wb were derived from
    hipEvent_t ev_peer = nullptr;                                                // stream-ordered partition copies: the handshake with the caller's stream
    dge_sorted_work* sorted = nullptr;                                           // update_policy 8 (allocated on first use)
};

// update_policy 8 (sgns_sorted.hip): one pass of the owner-computes schedule over compacted walks [0, n_rows) of m->d_sen
struct TrainParams;
int dge_sorted_train(dge_model* m, const TrainParams& p);
void dge_sorted_release(dge_model* m);

// Internals the translation units above call across files; hidden, so that the library's exported names stay those of include/dge.h.
#define DGE_LOCAL __attribute__((visibility("hidden")))
// table placement (sgns_place.hip): a table of `floats` floats in the best of several candidate allocations under a 2 ms probe (small and very large
// tables: plain hipMalloc); dge_table_free frees what dge_table_alloc or hipMalloc returned
DGE_LOCAL int dge_table_alloc(float** out, size_t floats, int device, hipStream_t st, int* seen, double* rate_best, double* rate_worst);
DGE_LOCAL void dge_table_free(void* p);
// launch timing (sgns.hip): waits for the model's stream and folds every pending event pair into kernel_ms / walk_ms
DGE_LOCAL int dge_drain_events(dge_model* m);
static inline unsigned dge_grid_for(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }
