// sgns_plan.h — how one trainer launch is scheduled: which kernel form runs with which template flags, how many workers in what grid and LDS, and
// which TrainParams knobs apply.  Pure host arithmetic over the vocabulary's statistics, the config and the tuning knobs — no HIP — so that it builds
// with a plain C++17 compiler: tests/native/plan_harness.cpp runs it on the CPU (tests/test_train_plan.py).  sgns.hip (train_rows) applies the plan and
// launches; sgns_kernels.h (launch_train_b) turns the plan's form and flags into the kernel instantiation.
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/dge.h"

#define HS_REP 16            /* most copies an inner node has during a launch of k_sgns_train_hsw (the root's) */
#define HS_REP_NODES 64      /* at most this many inner nodes have copies */
#define HS_REP_ROWS ((HS_REP - 1) * HS_REP_NODES)      /* spare rows behind syn1 for them */
#ifndef DGE_LOCKED_WAVES
#define DGE_LOCKED_WAVES 3
#endif
#ifndef DGE_HOTMIX_WAVES
#define DGE_HOTMIX_WAVES 3
#endif
#ifndef DGE_HS_WAVES
#define DGE_HS_WAVES 3
#endif

// pairs of a full-length walk under DL4J's window (radius uniform in 1 .. W): what a launch's size is estimated from without reading anything back
static inline double dge_expected_pairs_per_walk(int L, int W) {
    double e = 0.0;
    for (int i = 0; i < L; i++)
        for (int r = 1; r <= W; r++) e += (double)(std::min(L - 1, i + r) - std::max(0, i - r)) / (double)W;
    return e;
}

// ------------------------------------------------------------------------------------------ what the rules read
struct ScheduleStats {
    int64_t V = 0;
    int32_t D = 0, stride = 0;
    int64_t total_words = 0;
    double neg_norm = 1.0;                      // sum of count^0.75 over the vocabulary (the unigram table's normaliser)
    double neg_collision = 1.0;                 // sum of squared negative-sampling probabilities: P(two draws hit one row)
    double row_share_max = 1.0;                 // largest share one row has of the tokens / of the negative draws
    int64_t hot_rows_auto = 0;                  // head rows that policy 7 keeps out of the lock protocol
    int64_t hot_rows_serial = 0;                // head rows whose own pairs, serialised by the row's lock, would outlast a launch
    int32_t hs_rep_auto = 0;                    // hierarchical softmax: the inner nodes [V-1 - hs_rep_auto, V-1) are each on a tenth of all paths and more (copies in k_sgns_train_hsw)
    int32_t hs_rep_thr32[32] = {0};             // node >= hs_rep_thr32[k]: on more than k/32 of all paths
    int32_t hs_cold_auto = 0;                   // hierarchical softmax: inner nodes [0, hs_cold_auto) are each on fewer than 2e-5 of the paths
    int n_cus = 256;
};

// the statistics of a vocabulary whose counts descend (dge_model_create's sort); the hierarchical softmax's fields come from schedule_stats_hs
static inline ScheduleStats schedule_stats(const int64_t* counts, int64_t V, int32_t D, int32_t stride, int n_cus) {
    ScheduleStats s;
    s.V = V; s.D = D; s.stride = stride; s.n_cus = n_cus;
    int64_t tw = 0;
    for (int64_t i = 0; i < V; i++) tw += counts[i];
    s.total_words = tw;
    if (V == 0) return s;
    double twp = 0.0; const double power = 0.75;
    for (int64_t i = 0; i < V; i++) twp += pow((double)counts[i], power);
    double s2 = 0.0;
    for (int64_t i = 0; i < V; i++) { double q = pow((double)counts[i], power) / twp; s2 += q * q; }
    s.neg_collision = s2; s.neg_norm = twp;
    s.row_share_max = std::max((double)counts[0] / (double)std::max<int64_t>(tw, 1), pow((double)counts[0], power) / twp);
    // Head of the vocabulary for the mixed policy (7).  A try-lock fails when another worker holds the row: per pair
    // ~5 syn1neg rows drawn with q_i (unigram^0.75) and one syn0 row that occurs with p_i (unigram), held for the whole
    // pair.  Expected failures per attempt with W workers ~ W * 5 * (sum q_i^2 + sum p_i^2) over the LOCKED rows; the
    // head [0, H) is taken out until that is below 0.1.  (cfg3: 0.14 with H = 0 — left alone, see plan_train; cfg5: 3.3 M
    // rows, H ~ 1e4.)
    const double W0 = (double)((int64_t)n_cus * 3 * 16);
    double tail = 0.0; int64_t H = V;
    while (H > 0) {
        const double c = (double)counts[H - 1];
        const double q = pow(c, power) / twp, pp = c / (double)tw;
        if (W0 * 5.0 * (tail + q * q + pp * pp) >= 0.1) break;
        tail += q * q + pp * pp; H--;
    }
    s.hot_rows_auto = H;
    // A second, sharper reason to keep a row out of the lock protocol: the pair holds its syn0 row's lock for its whole
    // duration, so the pairs whose context is row i run one after the other — p_i * pairs of them, while the launch as a
    // whole lasts pairs / W pair-times.  A row with W * p_i near 1 therefore becomes the critical path of the launch
    // (measured: ONE vertex with 1e-4 of all tokens in an otherwise flat 1 M-row vocabulary — W * p = 1.2 — slows the lock
    // kernel by 20-25 %; the bench graph's busiest row has 0.36).  Rows beyond 0.5 go to the atomics side.
    int64_t Hs = 0;
    while (Hs < V && W0 * (double)counts[Hs] / (double)tw > 0.5) Hs++;
    s.hot_rows_serial = Hs;
    return s;
}

// the hierarchical softmax's fields, from the Huffman tree's inner-node weights (dge_huffman_paths: they ascend with the node number)
static inline void schedule_stats_hs(ScheduleStats& s, const std::vector<int64_t>& node_w) {
    const int64_t tot = s.total_words;
    // cold inner nodes: on fewer than 2e-5 of all paths (their weights ascend with the node number: a prefix)
    const int64_t limit = (int64_t)((double)tot * 2e-5);
    s.hs_cold_auto = (int32_t)(std::upper_bound(node_w.begin(), node_w.end(), limit) - node_w.begin());
    // busy inner nodes: on a tenth of all paths and more (a suffix; the balanced tree of a flat vocabulary has 15 of them, a skewed one a few more) — at most 64
    const int64_t busy = (int64_t)((double)tot * 0.1);
    s.hs_rep_auto = (int32_t)std::min<int64_t>(64, node_w.end() - std::lower_bound(node_w.begin(), node_w.end(), busy));
    for (int k = 0; k < 32; k++)     // first node on more than k/32 of all paths (weights ascend with the node number)
        s.hs_rep_thr32[k] = (int32_t)(std::upper_bound(node_w.begin(), node_w.end(), (int64_t)((double)tot * k / 32.0)) - node_w.begin());
}

// ------------------------------------------------------------------------------------------ the rules
// Items of one synchronous mini-batch of the owner-computes schedule (update_policy 8, sgns_sorted.hip).  Within a mini-batch the context rows are frozen
// and every row takes its terms without feedback from the other side, so the size is set by TERMS PER LIVE ROW: measured (scripts/quality_sorted.py,
// profiles/r02_quality_sorted.txt) the link-prediction AUC equals the atomics schedule's up to ~120 items per row and mini-batch, slips by 0.001 per ~70
// items beyond and collapses between 320 and 390 (8 ranks: 73 ms per episode at 128 items per row, 69 at 256 — not worth the margin) —
// and the HOTTEST row counts, not the average one: on a Zipf-popular graph a head row took > 1e5 terms of a 96-per-row mini-batch and
// the tables went to NaN within an epoch.  Hence: 128 items per live row, at most 4096 for the hottest row, and no mini-batch below 5e5
// items (the two sorts and ~16 launches per mini-batch need that much to pay): 0 = this vocabulary is too skewed or too small.
static inline int64_t dge_sorted_batch_items(const ScheduleStats& s, int part_n) {
    const int n = std::max(part_n, 1);
    const int64_t live_rows = std::max<int64_t>(1, s.V / n);
    const double hottest = std::min(1.0, s.row_share_max * (double)n);      // its share of one block's terms
    int64_t items = std::min<int64_t>(96ll << 20, 128 * live_rows);
    // (round 5: 4 096 for the busiest row, was 2 048 — on cfg3 that bound was the one that bound (its busiest vertex holds 30x the mean count: 8.8 M items where the
    //  128-a-row rule allows 16 M) and an epoch of the cfg3-sized community graph on 8 ranks ends at the same AUC 0.9596 / loss 0.474 with 18 M-item mini-batches — the
    //  busiest row at ~4 200 terms — as with 9 M, 10 % faster; 36 M (a whole episode, 288 a row) loses it: 0.9565 / 0.497.  scripts/blocks_minibatch_quality.py,
    //  profiles/r05_blocks_minibatch_quality.txt)
    items = std::min<int64_t>(items, (int64_t)(4096.0 / std::max(hottest, 1e-12)));
    // (wide rows: from half a million items on — round 4: a 50 000-row vocabulary with rank^-0.5 popularity lands at 0.9 M and ran 3.4e8 edges/s at D = 256 under this
    //  schedule against 2.1e8 under the atomics the rule used to leave it with: scripts/policy_sweep.py)
    //  — on rows of more than 128 floats: with D = 64 the same vocabulary runs 7.9e8 under atomics against 4.2e8 here; the sorts do not shrink with the row)
    // One block of the multi-GPU schedule on a vocabulary large enough for the lock kernels (>= 32 768 rows a partition): those — the mixed kernel on a skewed
    // vocabulary — are the alternative there, not atomics, and a mini-batch that the busiest row keeps small loses to them: cfg5 at 2 ranks landed at 0.7 M items and
    // ran 4.6e7 edges/s per rank here against 8.6e7 under the mixed kernel at 4 ranks (round 5).  From 4 M items on (cfg3's blocks: 16 .. 18 M).
    if (n >= 2 && s.V / n >= 32768) return items >= (4 << 20) ? items : 0;
    return items >= (s.stride > 128 ? (1 << 19) : (1 << 20)) ? items : 0;
}

// block_head's memo: the head of the latest (ranks, workers) asked for (owned by the model; computed on first use)
struct BlockHeadMemo { int32_t n = 0; int64_t workers = 0, rows = 0; };

// Head of the vocabulary inside ONE BLOCK of an n-rank block schedule (dge_model_set_partition).  A block's live rows are the V / n rows of its
// partition, and a row of the partition takes n times its share of the block's accesses (negatives drawn from the whole table are moved to the
// partition's row nearest below: n rows' worth of draws; contexts: the pairs whose context lies in the partition), so over the locked rows the
// expected failures per try-lock are W * 5 * n^2 * sum_{partition}(q_i^2 + p_i^2) ~ W * 5 * n * sum_{all}(q_i^2 + p_i^2): the rule of
// schedule_stats with the bound divided by n.  And a context row whose own pairs — serialised by its lock — are more than half of what one worker
// trains in the launch (W * n * p_i > 0.5) goes to the atomics side as well.  Rows [0, head) take atomics, the rest stay under the commit locks.
// Round 5, with the hottest rows' chains gone (the accumulator banks), the head size was swept again per graph (profiles/r05_skewed_knobs_*.txt, r05_blocks_head_quality_*.txt):
// a block's speed has a flat optimum — cfg3_zipf 20 000 .. 160 000 rows within 2 %, cfg5 15 000 .. 60 000 (best 30 000: 8.47e7 against 8.31e7 at the 60 320 of the
// 0.1 bound), the cfg3-sized community graph with a Zipf fifth 20 000 .. 40 000 (10 % faster than the 183 340 of the 0.1 bound) — and the embedding does not depend on it
// (AUC / loss equal to the fourth digit from 10 000 to 183 340 rows).  A bound of 0.2 puts all three inside their optimum (44 222 / ~30 000 / 60 380 rows).
static inline int64_t block_head(const ScheduleStats& s, const int64_t* counts, int n, int64_t W, BlockHeadMemo& memo) {
    if (memo.n == n && memo.workers == W) return memo.rows;
    const double power = 0.75, twp = s.neg_norm, tw = (double)std::max<int64_t>(s.total_words, 1);
    double tail = 0.0; int64_t H = s.V;
    const double bound = 0.2 / (5.0 * (double)W * (double)std::max(n, 1));     // (round 5: 0.1 until the accumulator banks; see below)
    while (H > 0) {
        const double c = (double)counts[H - 1];
        const double q = pow(c, power) / twp, pp = c / tw;
        if (tail + q * q + pp * pp >= bound) break;
        tail += q * q + pp * pp; H--;
    }
    int64_t Hs = 0;
    while (Hs < s.V && (double)W * (double)n * (double)counts[Hs] / tw > 0.5) Hs++;
    memo.n = n; memo.workers = W; memo.rows = std::max(H, Hs);
    return memo.rows;
}

// Expected failures per try-lock attempt with the device full of lock workers (48 a compute unit): a try fails when the row is among the ~5 rows another
// worker holds, i.e. with probability ~ workers * 5 * sum_i q_i^2 (q = unigram^0.75 sampling probabilities).
static inline double lock_failures(const ScheduleStats& s) { return (double)((int64_t)s.n_cus * 3 * 16) * 5.0 * s.neg_collision; }
// the busiest row's share caps the workers below a quarter of the device (48 / its share of the tokens < 4096 workers; plan_train then caps the workers at 96 in flight)
static inline bool row_share_caps_workers(const ScheduleStats& s) { return (int64_t)(48.0 / std::max(s.row_share_max, 1e-12)) < 4096; }
// the commit locks are the fast schedule while a try-lock rarely fails: fewer than 0.4 expected failures per attempt on a vocabulary of >= 131 072 rows
static inline bool locks_work(const ScheduleStats& s) { return s.V >= 131072 && lock_failures(s) < 0.4; }
// per-segment descriptors (TableView) for tables of 4 GiB and more
static inline bool tables_need_segments(const ScheduleStats& s) { return (uint64_t)s.V * (uint64_t)s.stride * 4ull >= 0xFFFFFFFFull; }
// ... and DGE_TUNE_FORCE_SEGMENTS selects that code path on small tables too so that the parity tests can cover it
static inline bool big_tables(const ScheduleStats& s, const int64_t* knob) { return tables_need_segments(s) || knob[DGE_TUNE_FORCE_SEGMENTS] > 0; }

// What update_policy 0 resolves to for a device-filling launch over the whole vocabulary on one GPU — 5 (commit locks), 7 (locks, the head by atomics) or 2
// (atomics); the owner-computes schedule (8) is taken instead of 2 where it applies (plan_train).  The rule's constants were fitted on the four bench graphs
// and then checked — and moved — against a sweep of vocabulary size x popularity exponent x row width (scripts/policy_sweep.py, profiles/r04_policy_sweep.txt):
//   * the commit locks are the fast schedule while a try-lock rarely fails: expected failures per attempt ~ workers * 5 * sum q_i^2 < 0.4 on a vocabulary of
//     >= 131 072 rows (round 3: 0.25 and 262 144 — a flat 200 000-row vocabulary runs 1.46e9 edges/s under locks against 1.19e9 owner-computes);
//   * a skewed vocabulary keeps the locks for its tail when the head that has to leave them is at most a quarter of the rows (round 3: an eighth — rank^-0.5
//     popularity over 300 000 rows: 9.5e8 against 7.3e8 owner-computes);
//   * when the busiest row's share caps the workers below a quarter of the device (48 / its share of the tokens < 4096 workers; plan_train then caps the workers at 96 in flight), the lock protocol has
//     nothing to win over atomics (rank^-1 over 300 000 words: 1.37e8 against 5.9e7).
// (the first two conditions alone: a try-lock on a syn1neg row rarely fails — what the hierarchical-softmax kernel's lock form needs; it never locks a context row,
//  so a vocabulary with a handful of rows whose OWN pairs would serialise under a syn0 lock, policy 7 with a tiny head, takes it as well)
static inline bool syn1neg_locks_work(const ScheduleStats& s) { return !row_share_caps_workers(s) && locks_work(s); }
static inline int auto_policy(const ScheduleStats& s, bool hs) {
    if (hs) return 2;
    if (row_share_caps_workers(s)) return 2;
    if (locks_work(s)) return s.hot_rows_serial > 0 ? 7 : 5;
    if (s.V >= 131072 && s.hot_rows_auto <= s.V / 4) return 7;
    return 2;
}

// Rows of 17 .. 32 floats under the atomics policy (the reference's own layerSize 20): half a wave a worker, a row = one request each way (k_sgns_train_small).
// `policy` is the one the launch resolves to.
static inline bool small_rows(const dge_train_config& cfg, const ScheduleStats& s, int policy, int part_n, int32_t L, bool big, const int64_t* knob) {
    return policy == 2 && cfg.use_hs == 0 && part_n <= 1 && cfg.dim > 16 && cfg.dim <= 32 && s.stride == 64 && L <= 64 && !big && knob[DGE_TUNE_SMALL_ROWS] != 0;
}

// The walk-window pair loop's LDS (sgns_kernels.h: k_sgns_train_window): one workgroup of 48 workers a compute unit has the CU's 160 KB.  Fixed: the sigmoid table (4 000 B), the
// table's run form (25 092 B) and the slots' control words — 32 KB set aside — and the workers' centre-delta double buffers (48 x 2 rows).  A slot: L rows of
// deltas and the walk's tokens.  At most 16 slots (a worker scans them with one lane each).
#define DGE_LDS_BYTES 163840
#define DGE_WIN_FIXED_BYTES 32768
#define DGE_WIN_WORKERS 48
#define DGE_WIN_MAX_SLOTS 16
#define DGE_WIN_MIN_SLOTS 4
static inline int64_t window_slot_bytes(int32_t stride, int32_t L) { return (int64_t)L * stride * 4 + (int64_t)((L + 3) & ~3) * 4; }
static inline int window_slots(int32_t stride, int32_t L) {
    const int64_t left = (int64_t)DGE_LDS_BYTES - DGE_WIN_FIXED_BYTES - (int64_t)DGE_WIN_WORKERS * 2 * stride * 4;
    return (int)std::max<int64_t>(0, std::min<int64_t>(DGE_WIN_MAX_SLOTS, left / window_slot_bytes(stride, L)));
}
static inline size_t window_dyn_bytes(int32_t stride, int32_t L, int slots) {
    return (size_t)((int64_t)DGE_WIN_WORKERS * 2 * stride * 4 + (int64_t)slots * window_slot_bytes(stride, L));
}

// ------------------------------------------------------------------------------------------ the plan
// The trainer's forms; the flags below pick the template arguments (sgns_kernels.h, launch_train_b).
enum class TrainForm { Sorted, InOrder, RowRmw, Atomics, SmallRows, Locked, HsCentre };

struct TrainPlan {
    TrainForm form = TrainForm::InOrder;
    bool hs = false;              // k_sgns_train<.., HS, ..>: the hierarchical-softmax term
    bool part = false;            // one block of the multi-GPU schedule (PART)
    bool strict = false;          // k_sgns_train_locked: strict commit (update_policy 6)
    bool hotmix = false;          // k_sgns_train_locked: the head rows by atomics (update_policy 7)
    bool wdog = false;            // k_sgns_train_locked: the watchdog (forced commit locks)
    bool nlock = false;           // k_sgns_train_hsw: the negatives under commit locks
    bool head = false;            // k_sgns_train_hsw with nlock: the head rows by atomics
    int waves = 0;                // k_sgns_train_hsw: training waves a workgroup (3 or 7)
    bool big = false;             // BIG: per-segment table descriptors
    int64_t workers = 0;
    unsigned blocks = 0, threads = 0;
    size_t shmem = 0;
    // the TrainParams fields the rules set (train_rows copies them)
    int32_t hot_rows = 0, acc_rows = 0, acc_drain = 16, syn0_free = 0;
    int32_t hs_hot0 = 0x7fffffff, hs_n_hot = 0, hs_drain = 1, hs_cold = 0, hs_wave = 0, hs_rep0 = 0x7fffffff, hs_rep_n = 0;
    int32_t hs_rep_thr[HS_REP] = {0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff,
                                  0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff};
    uint64_t wd_ticks = 0;
    bool runs_off = false;        // the negative-sampling table, not its run form
    bool walk_counter = false;    // walks handed out by a launch-wide counter (TrainParams::next_walk)
    // k_sgns_train_locked<relaxed> in its walk-window pair loop (k_sgns_train_window, sgns_kernels.h): its own geometry — blocks / threads / shmem above stay those of
    // the per-pair loop, which the same plan would otherwise run
    bool window = false;
    int32_t win_slots = 0;
    unsigned win_blocks = 0;
    size_t win_shmem = 0;
    char error[512] = "";         // why plan_train refused

    // what dge_model_schedule reports as the update policy
    int reported_policy() const {
        switch (form) {
            case TrainForm::Sorted: return 8;
            case TrainForm::InOrder: return 0;
            case TrainForm::RowRmw: return 1;
            case TrainForm::Locked: return hotmix ? 7 : (strict ? 6 : 5);
            case TrainForm::HsCentre: return nlock ? (head ? 7 : 5) : 2;
            default: return 2;
        }
    }
    // which trainer kernel runs (dge_model_kernel): the bench line names it from here, not from the policy number
    std::string kernel_name() const {
        const std::string blk = part ? ", one block" : "";
        switch (form) {
            case TrainForm::Sorted:
                return part ? "k_sorted_phase (owner-computes, one block of the multi-GPU schedule: k_block_emit + 2 item sorts + 2 phases)"
                            : "k_sorted_phase (owner-computes: k_sorted_emit + 2 item sorts + 2 phases)";
            case TrainForm::HsCentre:
                if (!nlock) return "k_sgns_train_hsw<atomics, 3 waves> (hierarchical softmax, a wave per centre)";
                return std::string("k_sgns_train_hsw<negatives under commit locks") + (head ? ", head rows by atomics" : "") + (waves == 7 ? ", 7 waves>" : ", 3 waves>") +
                       " (hierarchical softmax, a wave per centre)";
            case TrainForm::Locked: return std::string("k_sgns_train_locked<") + (strict ? "strict" : "relaxed") + (hotmix ? ", head rows by atomics" : "") + blk + ">";
            case TrainForm::SmallRows: return "k_sgns_train_small<atomics, 32 lanes a worker>";
            default:
                return std::string("k_sgns_train<") + (form == TrainForm::Atomics ? "atomics" : (form == TrainForm::RowRmw ? "row rmw" : "in-order")) +
                       (hs ? ", hierarchical softmax pair by pair" : "") + blk + ">";
        }
    }
};

static inline int plan_fail(TrainPlan* out, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
static inline int plan_fail(TrainPlan* out, int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(out->error, sizeof(out->error), fmt, ap);
    va_end(ap);
    return code;
}

// The schedule of one launch over n_rows compacted walks of up to L tokens (counts: the vocabulary's, descending; knob: a snapshot of the tuning knobs,
// include/dge.h — -1 = the library's own rule).  DGE_OK, or an error code with the reason in out->error.  Touches nothing but *out and the memo.
static inline int plan_train(const dge_train_config& cfg, const ScheduleStats& s, const int64_t* counts, int32_t part_n, int64_t n_rows, int32_t L,
                             const int64_t* knob, BlockHeadMemo& memo, TrainPlan* out) {
    *out = TrainPlan();
    TrainPlan& P = *out;
    const bool part = part_n > 1;
    const bool hs = cfg.use_hs != 0;
    const bool big = big_tables(s, knob);
    P.part = part;

    // auto: where the Hogwild kernels are bound by contention on a FLAT vocabulary — one too small for row locks (they fall back to
    // atomics: cfg2), a block of a schedule of 3 and more ranks (V/N live rows per table) — the owner-computes schedule is the faster
    // one at equal link-prediction AUC (one block of 8 ranks 5.7e8 vs 4.6e8 edges/s, a 100 k-row vocabulary at D = 128 6.8e8 vs 4.2e8:
    // profiles/r02_quality_sorted.txt).  A skewed vocabulary stays with the mixed policy 7: a synchronous mini-batch hands a hot row
    // thousands of terms at once with no feedback between them, and the embedding diverges (dge_sorted_batch_items).
    bool sorted_auto = false;
    if (cfg.update_policy == 0 && cfg.workers == 0 && !hs && !tables_need_segments(s)) {
        if (part) sorted_auto = dge_sorted_batch_items(s, part_n) > 0;                 // (per rank on cfg3, owner-computes vs locks, round 3 with the items made once per batch: N = 2 7.5e8 vs 7.2e8, N = 4 7.8e8 vs 7.4e8, N = 8 7.5e8 vs 4.8e8)
        else sorted_auto = auto_policy(s, hs) == 2 && dge_sorted_batch_items(s, 1) > 0;   // (what used to fall back to atomics)
    }
    const bool allow_unsafe = knob[DGE_TUNE_ALLOW_UNSAFE] > 0;
    const double launch_pairs = (double)n_rows * dge_expected_pairs_per_walk(L, cfg.window) / ((double)part_n * (double)part_n);      // (full-length walks: an upper estimate)
    if ((cfg.update_policy == 8 && cfg.workers != 1) || sorted_auto) {
        // owner-computes schedule (sgns_sorted.hip): items sorted by row, no locks, no atomics, deterministic
        if (hs) return plan_fail(out, DGE_ERR_ARG, "update_policy 8 does not carry the hierarchical-softmax term");
        // FORCED on a vocabulary the rule would not pick it for (dge_sorted_batch_items == 0): a small vocabulary is merely slow, but on a skewed one the busiest row takes
        // thousands of terms of one synchronous mini-batch with no feedback between them and the tables go to NaN within an epoch (profiles/r02_quality_zipf_sorted_diverges.txt;
        // rank^-1 over 50 000 words: 9 % of a million-item mini-batch on one row).  Refused instead (round 5; a mini-batch size set by hand — DGE_TUNE_SORTED_WALKS — is the caller's business).
        if (!sorted_auto && !allow_unsafe && knob[DGE_TUNE_SORTED_WALKS] <= 0 && dge_sorted_batch_items(s, part_n) == 0) {
            const double hottest = std::min(1.0, s.row_share_max * (double)std::max(part_n, 1));
            const double mb_items = std::min((double)(1 << 20), launch_pairs * (double)(cfg.negative + 1));
            if (hottest * mb_items > 8192.0)
                return plan_fail(out, DGE_ERR_ARG, "update_policy 8 (owner-computes) on this vocabulary: its busiest row holds %.2g of the terms, ~%.0f of one synchronous mini-batch "
                                 "with no feedback between them (the schedule keeps that below 4096; far beyond, the tables diverge): use update_policy 0 (auto), 2 or 7", hottest, hottest * mb_items);
        }
        P.form = TrainForm::Sorted;
        return DGE_OK;
    }

    // update policy (see Policy<>, k_sgns_train_locked and dge_train_config.update_policy).  Auto: the commit-lock kernel is the fast one while lock attempts
    // rarely fail (lock_failures).  cfg3 (uniform-ish, 1M rows, 12k workers): 0.07 -> locked, 8.9e8 edges/s.  A Zipf-popular vocabulary (cfg5) gives >> 1: the
    // same kernel spins on its hot rows (measured 5e5 edges/s) while memory-side atomics are indifferent to the skew (5.9e7 = their byte rate) -> atomics.
    // In between (a skewed head over a long tail — cfg5, and what real trip data looks like) the head rows alone are taken out of the lock protocol: policy 7.
    // (auto_policy above; one worker runs in order whatever it says — below)
    int pol = cfg.update_policy == 0 ? auto_policy(s, hs) : cfg.update_policy;
    const bool small = small_rows(cfg, s, pol, part_n, L, big, knob);
    int64_t workers;
    if (cfg.workers == 0) {
        // fill the device: 4 blocks of 16 workers per CU, but never more concurrent walks than half the vocabulary
        // (Hogwild's premise is sparse collisions: measured, a 2.3k-row table keeps 0.99 cosine to the in-order
        // result up to ~1k workers and loses it beyond; the reference ran 8 workers on <= 6.4k rows)
        const int blocks_per_cu = (pol == 5 || pol == 6 || pol == 7) ? (pol == 7 ? (s.stride <= 128 ? DGE_HOTMIX_WAVES : 2) : (s.stride == 64 ? 4 : DGE_LOCKED_WAVES)) : 4;   // (rows of one chunk leave room for a 4th wave per SIMD in the lock kernel; a 5th under atomics gains nothing: cfg2 7.6e8 either way)   // what the kernel's VGPR budget keeps resident
        workers = (int64_t)s.n_cus * blocks_per_cu * 16;
        // Round 5 (scripts/small_vocab_workers.py, profiles/r05_small_vocab_workers*.txt): measured again on the reference's own tract size — 6 408 rows, D = 20, a graph with
        // community structure — with what matters downstream instead of the cosine to the in-order result: held-out link AUC and loss.  Negative sampling: AUC 0.9295 at
        // 3 204 ... 16 384 workers alike (sequential oracle 0.9294, its 8 Hogwild threads 0.9274), loss 0.6928 -> 0.6942 at 9 612 (sequential 0.6924, 8 threads 0.7111);
        // with the hierarchical softmax 9 612 workers keep AUC 0.9213 / loss 0.737 (8 CPU threads: 0.9207 / 0.741) and 12 816 lose it (0.915 / 0.81).  So from 4 096
        // rows on the cap is 1.5 workers a row: cfg1 7.2e8 -> 1.28e9 edges/s, with the tree term 1.64e8 -> 5.1e8.  Below 4 096 rows the round-1 cap stays.
        // The small-row kernel (rows of 17 .. 32 floats without the tree term: k_sgns_train_small) reaches its request-rate ceiling with ONE worker a row — 1.41e9 edges/s
        // at 6 408, 9 612 and 16 384 workers alike, loss 0.6935 / 0.6943 / 0.716 (profiles/r05_small_row_kernel.txt) — so it runs one a row.
        workers = std::min(workers, std::max<int64_t>(64, s.V >= 4096 ? (small ? s.V : s.V * 3 / 2) : s.V / 2));
        // ... nor so many that ONE row has dozens of its updates in flight at once: every one of them is computed from the same stale row, and their
        // sum — along the direction the contexts share — is a gradient step M times too long.  A vocabulary whose busiest row takes 9 % of the tokens
        // (Zipf(1) over 50 000 words: text without sub-sampling, not a flow graph) went to NaN within one launch of 16 384 workers
        // (scripts/policy_sweep.py, round 4); cfg3 with Zipf destinations and cfg5 keep 34 and 18 in flight and train to the atomics-free AUC.
        // Round 5 swept that bound on a graph WITH structure whose busiest vertex holds 2.8 % of the tokens (scripts/hot_row_inflight.py, profiles/r05_hot_row_inflight.txt;
        // sequential oracle AUC 0.7472 / loss 1.988, its 8 Hogwild threads 0.7346 / 2.044): 24 / 48 / 96 in flight 0.7469 / 0.7464 / 0.7454 at loss 1.97, 192: 0.7402 / 2.00,
        // 384: 0.7333 / 2.08 — and the SPEED peaks at 96 (3.2e8 edges/s; 2.7e8 at 48, 3.0e8 at 192: beyond, the busiest rows' atomics queue at the memory side).  So: 96.
        // Copies of the hottest rows (what k_sgns_train_hsw does for the Huffman root) would lift the atomic wall, not this one: staleness caps the in-flight count first.
        workers = std::min(workers, std::max<int64_t>(64, (int64_t)(96.0 / std::max(s.row_share_max, 1e-12))));
        workers = std::min(workers, (n_rows + 15) / 16 * 16);
    } else workers = cfg.workers;
    const bool workers_knob = cfg.workers == 0 && knob[DGE_TUNE_WORKERS] > 0;
    if (workers_knob) workers = std::min<int64_t>(knob[DGE_TUNE_WORKERS], (n_rows + 15) / 16 * 16);     // ablation knob
    const bool workers_auto = cfg.workers == 0 && !workers_knob;      // (the rules below may still move the count)
    if (cfg.update_policy == 0 && workers == 1) pol = 0;                 // one worker: in order
    // FORCED commit locks (5 / 6) on a vocabulary with a busy row: a pair holds its context row's lock for its whole duration, so the pairs of row i run one behind
    // the other — p_i x pairs of them while the launch as a whole should last pairs / W pair-times — and the waiting workers keep hammering that lock word: measured
    // (profiles/r04_policy_sweep.txt) 60x slower at W x p = 6 (rank^-0.5 over 1e6 rows), "minutes" on rank^-1.  Auto moves such rows to the atomics side (7); a forced 5 / 6 is
    // refused beyond W x p = 2 (the community graph's W x p = 1.2 runs 1.8x slower: still a choice).  Same rule inside a block, whose rows take n times their share.
    if ((cfg.update_policy == 5 || cfg.update_policy == 6) && workers > 1 && !allow_unsafe) {
        const double chain = (double)workers * s.row_share_max * (double)std::max(part_n, 1);
        // (and only where that chain is long: a contended hand-over of a row lock takes ~100 us — rank^-0.5 over 1e6 rows: 38 000 pairs of the busiest row in 5 s —, so a
        //  launch whose busiest row has fewer than 50 000 pairs is merely slow for seconds: the edge-case tests on 1- and 3-row vocabularies)
        if (chain > 2.0 && s.row_share_max * (double)std::max(part_n, 1) * launch_pairs > 5e4)
            return plan_fail(out, DGE_ERR_ARG, "update_policy %d (commit locks on every row) on this vocabulary: its busiest row holds %.2g of the tokens, %lld workers x that share = %.1f pairs "
                             "queue behind ONE row lock at any time and the launch would be that row's chain (bound 2): use update_policy 0 (auto) or 7 (the head by atomics)",
                             cfg.update_policy, s.row_share_max, (long long)workers, chain);
    }
    if (pol == 7) {
        // a flat vocabulary with a few busy rows: only those; a skewed one: the whole head
        P.hot_rows = (int32_t)std::min<int64_t>((cfg.update_policy == 0 && lock_failures(s) < 0.25) ? s.hot_rows_serial : std::max(s.hot_rows_auto, s.hot_rows_serial), s.V);
        if (knob[DGE_TUNE_HOT_ROWS] >= 0) P.hot_rows = (int32_t)std::min<int64_t>(knob[DGE_TUNE_HOT_ROWS], s.V);     // ablation knob
        // off unless asked for: measured on cfg3_zipf it buys 2-4 % and shifts the trained scores (profiles/r03_zipf_ablation.txt)
        P.acc_rows = knob[DGE_TUNE_ACC_ROWS] > 0 ? (int32_t)std::min<int64_t>(knob[DGE_TUNE_ACC_ROWS], 64) : 0;       // (the kernel caps it at what its LDS holds)
        if (knob[DGE_TUNE_ACC_DRAIN] > 0) P.acc_drain = (int32_t)std::min<int64_t>(knob[DGE_TUNE_ACC_DRAIN], 1 << 20);
    }
    if (workers == 1 && pol != 5 && pol != 6 && pol != 7 && pol != 2 && pol != 1) pol = 0;   // in-order: plain accesses
    if (pol == 3 || pol == 8) pol = 0;          // (policy 8 with one worker: the in-order schedule)
    switch (pol) {
        case 0: P.form = TrainForm::InOrder; break;
        case 1: P.form = TrainForm::RowRmw; break;
        case 2: P.form = TrainForm::Atomics; break;
        default: P.form = TrainForm::Locked; P.strict = pol == 6; P.hotmix = pol == 7; break;
    }
    if (part && L > 64) return plan_fail(out, DGE_ERR_ARG, "the block schedule keeps a walk's tokens in registers: walks of up to 64 tokens, not %d", L);
    if (part) {
        // One block of the multi-GPU schedule: the live rows are V/part_n per table, so lock attempts collide part_n times
        // as often as on the whole table (measured on cfg3 with bench.py --sim-ranks, profiles/r01_block_schedule_sim.txt).
        P.hot_rows = 0;
        // A skewed vocabulary keeps the head / tail split inside a block (round 4; until then such a block ran with float atomics on every row): the
        // block's own head — block_head, the one-GPU rule with the block's collision rate — by atomics through the workgroup's atomics wave, the tail
        // under the commit locks.  Two resident workgroups of 12 workers a compute unit (k_sgns_train_locked<HOTMIX, PART>).
        const int64_t w_mixed = (int64_t)s.n_cus * 2 * 12;
        const int64_t head_b = (cfg.update_policy == 0 || cfg.update_policy == 7) && workers > 1 && s.V / part_n >= 32768 ? block_head(s, counts, part_n, w_mixed, memo) : 0;
        const int64_t head_knob = knob[DGE_TUNE_HOT_ROWS];
        // with the hierarchical softmax (round 4): the in-order schedule or memory-side atomics, as on one GPU — inner-node rows are split by node % n like the
        // vocabulary rows, every block visits every centre for the path nodes of its target partition (k_sgns_train<.., HS, PART>)
        if (hs || pol == 0) P.form = pol == 0 ? TrainForm::InOrder : TrainForm::Atomics;
        else if (cfg.update_policy == 0) {
            const double per_worker = 5.0 * s.neg_collision * (double)part_n;
            const int64_t w_max = per_worker > 0 ? (int64_t)(0.37 / per_worker) / 256 * 256 : workers;
            if (s.V >= 262144 && w_max >= workers) { P.form = TrainForm::Locked; P.hotmix = false; }     // cfg3: up to 4 ranks
            else if (s.V >= 262144 && w_max >= 4096) {
                // more ranks: also take the pair's syn0 row out of the lock protocol (it is held for the whole pair: at
                // 8 ranks 10 % of the live syn0 rows are locked at any time and every tenth pair is aborted and retried);
                // its update goes out as atomics behind the last unlock.  8 192 workers (2 resident blocks a CU): 4.6e8 edges/s
                // per rank against 3.7e8 with the syn0 locks and 3.6e8 with atomics everywhere.
                P.form = TrainForm::Locked; P.hotmix = true; P.hot_rows = 0; P.syn0_free = 1;
                if (cfg.workers == 0) workers = std::min<int64_t>(workers, (int64_t)s.n_cus * 2 * 16);
            } else if (s.V / part_n >= 32768 && head_b <= s.V / 4) {
                // a skewed vocabulary (cfg5, cfg3 with Zipf destinations): the block's head by atomics, its tail under the locks
                P.form = TrainForm::Locked; P.hotmix = true; P.hot_rows = (int32_t)head_b; P.syn0_free = 0;
                if (cfg.workers == 0) workers = std::min<int64_t>(workers, (int64_t)s.n_cus * 2 * 16);
            } else { P.form = TrainForm::Atomics; P.hotmix = false; }
        }
        else if (pol == 2 || pol == 5) { }
        else if (pol == 7) { P.hot_rows = (int32_t)head_b; P.syn0_free = 1; }      // locks on syn1neg's tail only (the pair's syn0 row by atomics)
        else return plan_fail(out, DGE_ERR_ARG, "the block schedule runs under update_policy 0 (auto), 2, 3, 5 or 7, not %d", cfg.update_policy);
        if (P.form == TrainForm::Locked && P.hotmix) {
            if (head_knob >= 0) P.hot_rows = (int32_t)std::min<int64_t>(head_knob, s.V);                                       // ablation knobs
            if (knob[DGE_TUNE_BLOCK_SYN0_FREE] >= 0) P.syn0_free = knob[DGE_TUNE_BLOCK_SYN0_FREE] > 0 ? 1 : 0;
            // the partition's hottest rows of BOTH tables add up in the atomics wave's LDS accumulators (lk_atomics_wave, LkAcc): in a block one row's atomics are the
            // longest chain of the launch (cfg3_zipf at 8 ranks: 22.6 -> 15.2 ms a block).  Updates a flush: what keeps a row's parked updates — at most one flush short
            // in every workgroup — under 2 048, half of what the owner-computes schedule lets a row take from one stale value (dge_sorted_batch_items); measured on the
            // cfg3-sized Zipf graph at 8 ranks with 512 workgroups: 4 a flush AUC 0.826 / loss 1.280 (banks off 0.817 / 1.285), 8 a flush 0.825 / 1.296, 16 a flush
            // diverges (profiles/r05_blocks_acc_quality_zipf.txt).  (the kernel caps the rows at what its LDS holds: 16 a bank, 8 from 129 floats a row on)
            // (the flush period is set below, once the launch's workgroups are known)
            // ... where that chain is long against the block: the partition's busiest row takes part_n x max(its share of the contexts, K x its share of the negative
            // draws) of the block's pairs, ~78 ns each, against ~3 TB/s of row traffic for a pair.  Where it is short the banks buy nothing and cost a little: the
            // community graph with a Zipf fifth (chain a quarter of the block) loses 0.0034 AUC / 2.3 % of the loss with them and gains 1 % (tests/test_gpu_blocks_scale.py).
            const double top = (double)counts[0];
            const double chain_share = (double)part_n * std::max(top / (double)std::max<int64_t>(s.total_words, 1), (double)cfg.negative * pow(top, 0.75) / s.neg_norm);
            const double pair_s = 8.0 * (double)s.stride * (double)(cfg.negative + 2) / 3e12;
            // (scripts/block_head_rule.py: that ratio is 1.08 on cfg3_zipf — banks: +50 % and a better AUC —, 0.55 on cfg5 — +10 % —, 0.32 on the community graph: on from 0.4)
            const int32_t auto_rows = chain_share * 78e-9 > 0.4 * pair_s ? 16 : 0;
            P.acc_rows = knob[DGE_TUNE_ACC_ROWS] >= 0 ? (int32_t)std::min<int64_t>(knob[DGE_TUNE_ACC_ROWS], 64) : auto_rows;
        }
    }
    if (hs) {
        // dge_model_create admitted policies 0/2/3 only: in order or under atomics, with the tree term
        P.hs = true;
        if (P.form != TrainForm::InOrder) { P.form = TrainForm::Atomics; P.strict = P.hotmix = false; }
        if (P.form == TrainForm::Atomics && workers > 1) {         // (one worker: the sequential schedule — no LDS accumulators, no cold class, every node by atomics it waits for)
            // LDS accumulators for the inner nodes nearest the root: 30 KB a block (3 blocks a CU stay resident beside the atomics wave's boxes)
            const int64_t row_b = (int64_t)s.stride * 4 + 4;
            P.hs_n_hot = (int32_t)std::min<int64_t>(std::max<int64_t>(s.V - 1, 0), 30720 / row_b);
            P.hs_hot0 = (int32_t)(std::max<int64_t>(s.V - 1, 0) - P.hs_n_hot);
            P.hs_drain = 64;
            if (knob[DGE_TUNE_HS_DRAIN] >= 1) P.hs_drain = (int32_t)knob[DGE_TUNE_HS_DRAIN];      // ablation knob
            // the cold end of the tree: plain read-modify-write instead of atomics (see k_sgns_train)
            P.hs_cold = (int32_t)std::min<int64_t>(s.hs_cold_auto, P.hs_hot0);
            if (knob[DGE_TUNE_HS_COLD] >= 0) P.hs_cold = (int32_t)std::min<int64_t>(knob[DGE_TUNE_HS_COLD], P.hs_hot0);
            P.shmem = (size_t)P.hs_n_hot * (size_t)row_b;
        }
    }
    const bool hs_atomics = hs && P.form == TrainForm::Atomics;
    P.threads = workers == 1 ? 64u : 256u;
    P.blocks = (unsigned)((workers * 16 + P.threads - 1) / P.threads);
    // (from 65 536 vocabulary rows on, like the atomics wave below: on the reference's own 6 408-row tract vocabulary the walks in flight are capped by the
    //  vocabulary — 801 waves — and the pair-by-pair kernel's 3 204 groups are faster: 1.64e8 against 1.22e8 edges/s; DGE_TUNE_HS_CENTRE = 1 forces it)
    if (hs_atomics && !part && workers > 1 && s.stride <= 256 && L <= 64 && !big &&
        (knob[DGE_TUNE_HS_CENTRE] > 0 || (knob[DGE_TUNE_HS_CENTRE] < 0 && s.V >= 65536))) {
        // Hierarchical softmax, a wave per centre (k_sgns_train_hsw, round 4): the centre's path nodes stay in the registers of a wave's four groups for all
        // its contexts and their gathered updates leave once per centre.  `workers` = walks in flight = waves that train: two resident workgroups of three
        // such waves (and one atomics wave) a compute unit; never more than an eighth of the vocabulary (a wave works on four context rows at a time).
        P.form = TrainForm::HsCentre;
        int nw = 3;
        // ... and where the negative-sampling kernels would run under commit locks (a flat vocabulary: auto_policy 5), the pair's negatives and the centre's
        // gathered syn1neg update go under the rows' locks instead of out as atomics (k_sgns_train_hsw<.., NLOCK>) — in ONE workgroup of seven training waves a
        // compute unit, which share their LDS accumulators (DGE_TUNE_HS_CENTRE: 1 keeps atomics, 2 = locks in workgroups of three waves, 3 = of seven)
        const int64_t centre_knob = knob[DGE_TUNE_HS_CENTRE];
        // ... and on a SKEWED vocabulary whose head the mixed policy 7 would take out of the lock protocol (round 5): the same kernel with that head by atomics, the tail's
        // negatives under locks (hot_rows; DGE_TUNE_HOT_ROWS sets it by hand)
        const bool mixed_ok = s.V >= 131072 && !row_share_caps_workers(s) && std::max(s.hot_rows_auto, s.hot_rows_serial) <= s.V / 4;
        if (centre_knob == 2 || centre_knob == 3 || (centre_knob < 0 && cfg.update_policy == 0 && (syn1neg_locks_work(s) || mixed_ok))) {
            const bool mixed = !syn1neg_locks_work(s) && mixed_ok && centre_knob < 0;
            P.nlock = true;
            if (!(centre_knob == 2 || s.stride > 128 || mixed)) nw = 7;      // (rows of more than 128 floats: three-wave workgroups only — seven waves' message boxes do not fit the LDS; a head by atomics: three waves to an atomics wave, not seven)
            if (!syn1neg_locks_work(s) && mixed_ok) P.hot_rows = (int32_t)std::min<int64_t>(std::max(s.hot_rows_auto, s.hot_rows_serial), s.V);
            if (knob[DGE_TUNE_HOT_ROWS] >= 0) P.hot_rows = (int32_t)std::min<int64_t>(knob[DGE_TUNE_HOT_ROWS], s.V);
            P.head = P.hot_rows > 0;
        }
        P.waves = nw;
        if (workers_auto)
            workers = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>((int64_t)s.n_cus * (nw == 3 ? (s.stride <= 128 ? 6 : 3) : 7), std::max<int64_t>(1, s.V / 8)), std::max<int64_t>(16, (int64_t)(12.0 / std::max(s.row_share_max, 1e-12)))));      // (wide rows: one three-wave workgroup a compute unit)
        workers = std::max<int64_t>(1, std::min<int64_t>(workers, n_rows));
        P.blocks = (unsigned)((workers + nw - 1) / nw);
        P.threads = (unsigned)(nw + 1) * 64u;
        // an LDS accumulator now takes one addition per CENTRE (16 pairs' worth on cfg3): drained every 4 additions instead of every 64 — every 8 where seven
        // waves share it (the same number of additions parked device-wide: workgroups x drain)
        P.hs_drain = knob[DGE_TUNE_HS_DRAIN] >= 1 ? (int32_t)knob[DGE_TUNE_HS_DRAIN] : (nw == 3 ? 4 : 8);
        // Measured on cfg3 and the cfg3-sized community graph (profiles/r04_hs_waves7.txt; three waves, drain 4: 3.3e8 edges/s, AUC 0.9534): seven waves with 15 KB of
        // accumulators (the 29 nodes next to the root) and a drain every 8 additions 3.6e8 at AUC 0.9533; with 30 KB 3.64e8 / 0.9526, with 60 KB 3.7e8 / 0.9519 — every
        // accumulator is a row whose readers lag workgroups x drain / 2 updates behind, so fewer of them and shared by more waves is the better trade (three waves at
        // drain 8: 3.63e8 / 0.9518).
        // The busiest inner nodes in copies instead of LDS accumulators (k_sgns_train_hsw, HS_REP): the default; DGE_TUNE_HS_HOT_KB > 0 brings the accumulators back
        // (that many KB of them; the drain period then matters again) for comparison.
        const int64_t hot_kb = knob[DGE_TUNE_HS_HOT_KB];
        const int64_t cold_knob = knob[DGE_TUNE_HS_COLD];
        if (hot_kb <= 0 && s.hs_rep_auto > 0 && s.V > 1) {
            const int64_t n_rep = std::min<int64_t>(std::min<int64_t>(s.hs_rep_auto, HS_REP_NODES), s.V - 1);
            P.hs_rep_n = (int32_t)n_rep; P.hs_rep0 = (int32_t)(s.V - 1 - n_rep);      // (the copies: rows V .. of syn1, zero between launches: k_hs_rep_fold)
            // copies per node: ceil(share of the paths x F), F = HS_REP (the root: HS_REP = 16 copies, a node on half the paths 8, ...; DGE_TUNE_HS_COPIES = F for comparison: 4 = the root four copies, ...)
            const int64_t f_knob = knob[DGE_TUNE_HS_COPIES];
            const int F = (int)std::min<int64_t>(HS_REP, f_knob >= 1 ? f_knob : (int64_t)HS_REP);
            for (int k = 1; k < HS_REP; k++) P.hs_rep_thr[k] = k < F ? std::max(s.hs_rep_thr32[std::min(31, k * 32 / F)], P.hs_rep0) : 0x7fffffff;      // more than k copies: share x F > k
            P.hs_rep_thr[0] = 0;
            P.hs_n_hot = 0; P.hs_hot0 = (int32_t)std::max<int64_t>(s.V - 1, 0); P.shmem = 0;
            P.hs_cold = (int32_t)std::min<int64_t>(cold_knob >= 0 ? cold_knob : (int64_t)s.hs_cold_auto, P.hs_rep0);
        } else {                   // LDS accumulators (DGE_TUNE_HS_HOT_KB > 0; or a tree without a busy node): seven waves, one workgroup a compute unit — up to 100 KB; three waves, two workgroups — up to 30 KB each
            const int64_t row_b = (int64_t)s.stride * 4 + 4;
            P.hs_n_hot = (int32_t)std::min<int64_t>(std::max<int64_t>(s.V - 1, 0), (hot_kb > 0 ? std::min<int64_t>(hot_kb, nw == 7 ? 100 : 30) * 1024 : (nw == 7 ? 15360 : 30720)) / row_b);
            P.hs_hot0 = (int32_t)(std::max<int64_t>(s.V - 1, 0) - P.hs_n_hot);
            P.hs_cold = (int32_t)std::min<int64_t>(cold_knob >= 0 ? cold_knob : (int64_t)s.hs_cold_auto, P.hs_hot0);
            P.shmem = (size_t)P.hs_n_hot * (size_t)row_b;
        }
    }
    // (not on small vocabularies, where the worker count is capped at half the rows and every pair is a latency chain: the reference's own
    //  801 x 8 tract graph with hierarchical softmax runs 407 ms per 6.5e7 pairs on its 3 204 workers, 552 ms on 2 400 workers and a wave)
    if (P.form == TrainForm::Atomics && hs && workers > 1 && (knob[DGE_TUNE_HS_WAVE] > 0 || (knob[DGE_TUNE_HS_WAVE] < 0 && s.V >= 65536))) {
        // hierarchical softmax under atomics: every workgroup's fourth wave issues the atomics of its 12 workers (k_sgns_train, lk_atomics_wave)
        P.hs_wave = 1;
        // (three workgroups a compute unit stay resident next to their LDS accumulators and message boxes: DGE_HS_WAVES)
        if (workers_auto) workers = std::max<int64_t>(std::min<int64_t>(workers / 16 * 12, (int64_t)s.n_cus * DGE_HS_WAVES * 12), 2);
        P.blocks = (unsigned)((workers + 11) / 12);
    }
    if (P.form == TrainForm::Locked && P.hotmix && workers > 1) {
        // the mixed kernels keep every workgroup's fourth wave for the head rows' atomics (k_sgns_train_locked): 12 workers a workgroup
        if (workers_auto) workers = std::max<int64_t>(workers / 16 * 12, 2);
        P.blocks = (unsigned)((workers + 11) / 12);
        if (part) P.acc_drain = knob[DGE_TUNE_ACC_DRAIN] > 0 ? (int32_t)std::min<int64_t>(knob[DGE_TUNE_ACC_DRAIN], 1 << 20)
                                                             : (int32_t)std::max<int64_t>(1, std::min<int64_t>(8, 2048 / std::max(P.blocks, 1u)));
    }
    P.workers = workers;
    P.big = big;
    // Walks handed out by a launch-wide counter wherever several workers run, the order of the walks is free (not the in-order schedule) and
    // a worker trains enough walks for the hand-out to even anything out.  Measured on one model in one process (scripts/ab_inproc.py): cfg3
    // 415 against 426 ms per launch, cfg3_zipf 666 against 678, hierarchical softmax 3.24 against 3.28 s, atomics 914 against 925; cfg2 under
    // atomics (6 walks per worker) 5.6 against 5.4 — there the workers keep their fixed walks.
    const bool in_order = P.form == TrainForm::InOrder && !hs && !part;
    P.walk_counter = workers > 1 && n_rows >= 32 * workers && !in_order && !(knob[DGE_TUNE_STATIC_WALKS] > 0);
    // A launch whose length is one busy row's chain of pairs — forced policy 5 or 6 on a vocabulary with such a row — is bound by a pair's latency, not by
    // requests, and the 11 dependent LDS reads of the table's run form are slower than a table look-up that hits the caches (15.4-15.9 s against 12.8 s
    // on the community graph of scripts/quality_scale.py): there the table stays.
    P.runs_off = s.hot_rows_serial > 0 && workers > 1;
    // The lock kernels' watchdog: a worker that is still waiting for a row lock when the launch has run 100x longer than its bytes take at the roofline (+ 5 s) gives up,
    // counts itself in counters[3] and leaves; dge_model_stats then reports DGE_ERR_STATE.  Checked on the waiting paths only (100 MHz s_memrealtime ticks).
    {
        const double bytes = launch_pairs * 8.0 * (double)s.stride * (double)(cfg.negative + 2);
        double budget_s = 5.0 + 100.0 * bytes / 8e12;
        if (knob[DGE_TUNE_WATCHDOG_MS] > 0) budget_s = (double)knob[DGE_TUNE_WATCHDOG_MS] * 1e-3;
        // only where the commit locks on every row were FORCED (update_policy 5 / 6): what auto picks them for cannot make them wait, and the watchdog is its own kernel
        // instantiation so that the headline launch does not pay for it (sgns_kernels.h: WDOG)
        const bool forced_locks = cfg.update_policy == 5 || cfg.update_policy == 6;
        P.wd_ticks = (!forced_locks || knob[DGE_TUNE_WATCHDOG_MS] == 0) ? 0ull : (uint64_t)(budget_s * 1e8);
    }
    P.wdog = P.form == TrainForm::Locked && !P.hotmix && P.wd_ticks != 0;
    // The walk-window pair loop: exactly the instantiation auto picks on a flat vocabulary (relaxed, rows of up to 128 floats, one table descriptor, no head, no
    // block, no watchdog) with more than one worker, where at least four walks' deltas fit the LDS.  Everything else keeps the per-pair loop.
    // (rows of 64 floats: only where the commit locks were asked for by hand.  Auto runs them four waves a SIMD in the per-pair loop — 16 384 workers against the
    //  window's 12 288 — and that comparison has not been measured; the gain is measured at 128 floats, profiles/walk_window_ab.txt)
    const bool win_width = s.stride == 128 || (s.stride == 64 && cfg.update_policy == 5);
    if (P.form == TrainForm::Locked && !P.strict && !P.hotmix && !part && !P.wdog && !big && win_width && workers > 1 && L >= 1 && L <= 64) {
        const int slots = window_slots(s.stride, L);
        if (slots >= DGE_WIN_MIN_SLOTS) {
            P.window = true;
            P.win_slots = slots;
            // (one workgroup a compute unit is all that is resident: more would only queue behind the first and, without the walk counter, train their share late)
            P.win_blocks = (unsigned)std::min<int64_t>((workers + DGE_WIN_WORKERS - 1) / DGE_WIN_WORKERS, std::max(s.n_cus, 1));
            P.win_shmem = window_dyn_bytes(s.stride, L, slots);
        }
    }
    // rows of 17 .. 32 floats under the atomics policy: half a wave a worker (k_sgns_train_small; one worker only when DGE_TUNE_SMALL_ROWS asks for it)
    if (small && P.form == TrainForm::Atomics && (workers > 1 || knob[DGE_TUNE_SMALL_ROWS] > 0)) {
        P.form = TrainForm::SmallRows;
        P.threads = 256u; P.blocks = (unsigned)((workers * 32 + 255) / 256);
    }
    return DGE_OK;
}
