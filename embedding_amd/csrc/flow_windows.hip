// flow_windows.hip — the flow table by hour window (include/dge.h: dge_flows_add_entries, dge_flows_window_edges, dge_graph_add_flow_windows,
// dge_flows_triplets; the rule's per-element pieces: flow_rule.h).  The reference reads taxiFlows through getFlowTo(dst, lo, hi) — a loop over the hours of a
// window around a hash-map look-up — from three places: the cross-time graph DeepWalk trains on (J/CrossTimeGraph.java:25-52), the hand-picked intervals
// (:68-95) and the brute-force triplet search (J/Tracts.java:371-415).  Here all three rest on one primitive, the sparse matrix of window sums of the resident
// table.  Outside the build stamp: nothing here is read or written by a training launch.
//
// Window sums of K windows (k_slot_items of trip_map.hip, generalised): the host lists for each of the 24 hours the windows that hold it; an exclusive scan of
// the entries' window counts places every entry's items; k_win_items writes item (window, rank of ids[s], rank of ids[e]) -> count for every window of the
// entry's hour; then the sort, the reduce-by-key and the decode of trip_flows.h.  The ranks are ranks of ids, so key order is id order.  Nothing of size R^2
// is formed.
//
// Triplets: the five windows' sums are ONE such sorted table (window 0 .. 4 = A .. E); a sum is a binary search in it, absent = 0.
//   k_tri_pairs   one thread per entry of the driving window — A for (t1, t2), B for (t2, t3) and for (t3, t1) — looks the pair's other sums up and applies the
//                 pair's predicate.  A passing pair emits its key: t1 R + t2, t2 R + t3, and for (t3, t1) the key t1 R + t3 with B[t3, t1] as its value; a
//                 failing one the key behind all others.  Sorted, the keys are three edge lists: E12 by (t1, t2), E23 by t2 with t3 ascending, E31 by t1 with
//                 t3 ascending; k_tri_rows gives the latter two their row starts by binary search.
//   k_tri_list    one WAVE per E12 edge.  The lanes take consecutive elements of the shorter of E23[t2] and E31[t1], 64 at a time, search the other list for
//                 the same t3, drop t3 = t1, t2, look B[t3, t2] up and apply the ninth condition; __ballot and the popcount of the lower lanes give a kept
//                 lane its place, so a wave's output is in t3 order.  Two passes — count, exclusive scan, write — so the output stands ascending by
//                 (t1, t2, t3) by construction, without atomics, whatever the geometry.  The loop bounds depend on the edge only, never on a lane; the only
//                 barriers are those of the counters' block reduction, which every thread of the block reaches.
// Counters are integers added with atomicAdd after a block reduction: their values do not depend on the order.
//
// Coherence: no protocol.  Every array is written by one kernel and read by later ones on the same stream.
#include "flow_rule.h"
#include "trip_flows.h"

constexpr int TRI_WAVE = 64;                                 // gfx950: a wave is 64 lanes
constexpr int TRI_WAVES = SEQ_BLOCK / TRI_WAVE;              // E12 edges a block lists
enum { FW_PAIRS_12 = 0, FW_PAIRS_23, FW_PAIRS_31, FW_CANDIDATES, FW_N };

// ------------------------------------------------------------------------------------------ kernels
struct WinCount { const uint64_t* key; const int32_t* hour_first; uint64_t R; int64_t n;
                  __device__ int64_t operator()(int64_t i) const { if (i >= n) return 0; const int64_t h = (int64_t)(key[i] / R / R); return hour_first[h + 1] - hour_first[h]; } };

// entry i -> its items at item_first[i] ..: one for every window that holds its hour (hour_win lists them ascending from hour_first[hour])
__global__ void __launch_bounds__(SEQ_BLOCK) k_win_items(const uint64_t* key, const int64_t* cnt, int64_t n, uint64_t R, const int32_t* hour_first, const int32_t* hour_win,
                                                         const int64_t* item_first, const int32_t* idrank, uint64_t* item_key, int64_t* item_w) {
    const int64_t i = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t kk = key[i], e = kk % R, s = (kk / R) % R;
    const int32_t h = (int32_t)(kk / R / R);
    const uint64_t pair = (uint64_t)idrank[s] * R + (uint64_t)idrank[e];
    const int64_t c = cnt[i];
    int64_t at = item_first[i];
    for (int32_t q = hour_first[h]; q < hour_first[h + 1]; q++, at++) { item_key[at] = (uint64_t)hour_win[q] * R * R + pair; item_w[at] = c; }
}

// first[w] = the first of the sorted window sums that belongs to window w or a later one, w = 0 .. K
__global__ void __launch_bounds__(SEQ_BLOCK) k_win_bounds(const uint64_t* key, int64_t n, uint64_t R, int64_t K, int64_t* first) {
    const int64_t w = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (w <= K) first[w] = coo_lower_bound(key, n, (uint64_t)w * R * R);
}

// W[s, e] of window w in the sorted sums (ranks): absent = 0
__device__ __forceinline__ int64_t tri_sum(const uint64_t* wkey, const int64_t* wsum, int64_t n, uint64_t R, uint64_t w, uint64_t s, uint64_t e) {
    const uint64_t want = (w * R + s) * R + e;
    const int64_t at = coo_lower_bound(wkey, n, want);
    return at < n && wkey[at] == want ? wsum[at] : 0;
}

// which = 0: (t1, t2) over the entries [lo, hi) of window A; 1: (t2, t3) over window B; 2: (t3, t1) over window B
__global__ void __launch_bounds__(SEQ_BLOCK) k_tri_pairs(const uint64_t* wkey, const int64_t* wsum, int64_t n, uint64_t R, int64_t lo, int64_t hi, int32_t which, dge_triplet_rule rule,
                                                         uint64_t* out_key, int64_t* out_val, unsigned long long* counters) {
    const int64_t i = lo + (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    unsigned long long v[1] = {0};
    if (i < hi) {
        const uint64_t kk = wkey[i], e = kk % R, s = (kk / R) % R;
        const int64_t w = wsum[i];
        bool ok = false;
        uint64_t k = 0;
        if (s != e) {
            if (which == 0) {
                ok = fr_pair12(rule, w, tri_sum(wkey, wsum, n, R, 0, e, s), tri_sum(wkey, wsum, n, R, 2, e, s), tri_sum(wkey, wsum, n, R, 2, s, e));
                k = s * R + e;
            } else if (which == 1) {
                ok = fr_pair23(rule, w, tri_sum(wkey, wsum, n, R, 2, s, e), tri_sum(wkey, wsum, n, R, 3, s, e));
                k = s * R + e;
            } else {                             // s = t3, e = t1
                ok = fr_pair31(rule, w, tri_sum(wkey, wsum, n, R, 4, s, e), tri_sum(wkey, wsum, n, R, 2, e, s), tri_sum(wkey, wsum, n, R, 3, e, s), tri_sum(wkey, wsum, n, R, 1, e, s));
                k = e * R + s;
            }
        }
        out_key[i - lo] = ok ? k : ~0ull;
        out_val[i - lo] = w;
        v[0] = ok ? 1 : 0;
    }
    const int which_counter[1] = {FW_PAIRS_12 + which};
    trip_count(v, which_counter, counters);
}

// row_first[r] = the first of the n sorted keys (row R + column) that is in row r or a later one, r = 0 .. R
__global__ void __launch_bounds__(SEQ_BLOCK) k_tri_rows(const uint64_t* key, int64_t n, uint64_t R, int64_t* row_first) {
    const uint64_t r = (uint64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (r <= R) row_first[r] = coo_lower_bound(key, n, r * R);
}

// Wave `edge` of the launch lists E12 edge `edge`.  WRITE = false: count[edge] = its triplets, and the candidates' counter; WRITE = true: the triplets as ids from first[edge] on.
template <bool WRITE>
__global__ void __launch_bounds__(SEQ_BLOCK) k_tri_list(const uint64_t* e12, int64_t n12, const uint64_t* e23, const int64_t* row23, const uint64_t* e31, const int64_t* b31, const int64_t* row31,
                                                        const uint64_t* wkey, const int64_t* wsum, int64_t n, uint64_t R, dge_triplet_rule rule, const int64_t* id_by_rank, int64_t* count,
                                                        const int64_t* first, int64_t* id1, int64_t* id2, int64_t* id3, unsigned long long* counters) {
    const int lane = threadIdx.x % TRI_WAVE;
    const int64_t edge = (int64_t)blockIdx.x * TRI_WAVES + threadIdx.x / TRI_WAVE;
    unsigned long long v[1] = {0};
    if (edge < n12) {                            // (the same for every lane of the wave)
        const uint64_t t1 = e12[edge] / R, t2 = e12[edge] % R;
        const int64_t a0 = row23[t2], a1 = row23[t2 + 1], b0 = row31[t1], b1 = row31[t1 + 1];
        const bool by23 = a1 - a0 <= b1 - b0;    // the shorter list drives, the other one is searched
        const int64_t d0 = by23 ? a0 : b0, d1 = by23 ? a1 : b1, o0 = by23 ? b0 : a0, o1 = by23 ? b1 : a1;
        const uint64_t* drive = by23 ? e23 : e31;
        const uint64_t* other = by23 ? e31 : e23;
        const uint64_t other_row = (by23 ? t1 : t2) * R;
        int64_t done = 0;                        // kept so far by this wave
        for (int64_t base = d0; base < d1; base += TRI_WAVE) {
            const int64_t at = base + lane;
            bool cand = false, keep = false;
            uint64_t t3 = 0;
            if (at < d1) {
                t3 = drive[at] % R;
                const int64_t hit = o0 + coo_lower_bound(other + o0, o1 - o0, other_row + t3);
                cand = hit < o1 && other[hit] == other_row + t3 && t3 != t1 && t3 != t2;
                if (cand) keep = fr_triple(rule, b31[by23 ? hit : at], tri_sum(wkey, wsum, n, R, 1, t3, t2));
            }
            const unsigned long long kept = __ballot(keep);
            if (WRITE) {
                if (keep) {
                    const int64_t to = first[edge] + done + __popcll(kept & ((1ull << lane) - 1));
                    id1[to] = id_by_rank[t1]; id2[to] = id_by_rank[t2]; id3[to] = id_by_rank[t3];
                }
            } else v[0] += cand ? 1 : 0;
            done += __popcll(kept);
        }
        if (!WRITE && lane == 0) count[edge] = done;
    }
    if (!WRITE) {
        const int which[1] = {FW_CANDIDATES};
        trip_count(v, which, counters);
    }
}

// ------------------------------------------------------------------------------------------ host side
namespace {

int windows_check(const dge_hour_window* win, int32_t K, const char* who) {
    if (!win || K < 1) DGE_FAIL(DGE_ERR_ARG, "%s: null windows or K = %d < 1", who, K);
    for (int32_t k = 0; k < K; k++)
        if (!fr_window_ok(win[k]))
            DGE_FAIL(DGE_ERR_ARG, "%s: window %d is (start %d, hours %d): 0 <= start <= 23 and 0 <= hours <= 24 are needed", who, k, win[k].start, win[k].hours);
    return DGE_OK;
}

int rule_check(const dge_triplet_rule* rule, const char* who) {
    static const char* const what[] = {"", "window A", "window B", "window C", "window D", "window E", "min_a (0 .. 2^40)", "min_b (0 .. 2^40)", "ratio (1 .. 65536)"};
    const int fault = fr_rule_fault(*rule);
    if (fault) DGE_FAIL(DGE_ERR_ARG, "%s: the rule's %s is out of bounds", who, what[fault]);
    return DGE_OK;
}

dge_triplet_rule rule_default() {
    dge_triplet_rule r = {};
    r.A = {7, 3}; r.B = {17, 7}; r.C = {17, 6}; r.D = {7, 6}; r.E = {7, 7};
    r.min_a = 30; r.min_b = 70; r.ratio = 2;
    return r;
}

// the window edges on the device, ascending by (window, src id, dst id): the sorted keys (window, rank, rank) and their sums
int win_edges(SeqRun& R, const dge_flows* f, const dge_hour_window* win, int32_t K, const char* who, dge_tmp<uint64_t>& okey, dge_tmp<int64_t>& ow, int64_t* n_out) {
    *n_out = 0;
    const int64_t n = f->n;
    const dge_regions* rg = f->regions;
    const uint64_t Ru = (uint64_t)std::max<int64_t>(rg->R, 1);
    if ((uint64_t)K > (uint64_t)INT64_MAX / (Ru * Ru)) DGE_FAIL(DGE_ERR_RANGE, "%s: the keys (window, s, e) of %d windows over %lld regions do not fit 63 bits", who, K, (long long)rg->R);
    if (n == 0) return DGE_OK;
    std::vector<int32_t> hour_first(25, 0), hour_win;
    for (int32_t h = 0; h < 24; h++) {
        for (int32_t k = 0; k < K; k++) if (fr_window_has(win[k].start, win[k].hours, h)) hour_win.push_back(k);
        hour_first[(size_t)h + 1] = (int32_t)hour_win.size();
    }
    if (hour_win.empty()) return DGE_OK;
    dge_tmp<int32_t> d_first, d_win;
    dge_tmp<int64_t> item_first, iw, sw;
    dge_tmp<uint64_t> ikey, skey;
    SEQ_TRY(seq_alloc(R, d_first, 25, "the hours' windows"));
    SEQ_TRY(seq_alloc(R, d_win, (int64_t)hour_win.size(), "the hours' windows"));
    SEQ_TRY(seq_alloc(R, item_first, n + 1, "the entries' items"));
    DGE_HIP(hipMemcpyAsync(d_first.p, hour_first.data(), 25 * 4, hipMemcpyHostToDevice, R.stream));
    DGE_HIP(hipMemcpyAsync(d_win.p, hour_win.data(), hour_win.size() * 4, hipMemcpyHostToDevice, R.stream));
    DGE_HIP(hipStreamSynchronize(R.stream));     // (the two host vectors may go once this call returns early)
    SEQ_TRY(seq_kernels_begin(R));
    SEQ_TRY(seq_scan(R, rocprim::make_transform_iterator(rocprim::counting_iterator<int64_t>(0), WinCount{f->d_key, d_first.p, Ru, n}), item_first.p, n + 1));
    SEQ_TRY(seq_kernels_end(R));
    int64_t items = 0;
    SEQ_TRY(seq_read_back(R, &items, item_first.p + n, 8));
    if (items == 0) return DGE_OK;
    SEQ_TRY(seq_alloc(R, ikey, items, "the window items"));
    SEQ_TRY(seq_alloc(R, iw, items, "the window items' weights"));
    SEQ_TRY(seq_alloc(R, skey, items, "the sorted window items"));
    SEQ_TRY(seq_alloc(R, sw, items, "the sorted window items' weights"));
    SEQ_TRY(seq_kernels_begin(R));
    hipLaunchKernelGGL(k_win_items, dim3(seq_grid(n)), dim3(SEQ_BLOCK), 0, R.stream, f->d_key, f->d_cnt, n, Ru, d_first.p, d_win.p, item_first.p, rg->d_idrank, ikey.p, iw.p);
    SEQ_TRY(seq_kernels_end(R));
    SEQ_TRY(trip_sort_pairs(R, ikey.p, skey.p, iw.p, sw.p, items, dge_bits((uint64_t)K * Ru * Ru)));
    SEQ_TRY(trip_reduce(R, skey.p, sw.p, items, okey, ow, n_out));
    DGE_HIP(hipGetLastError());
    return DGE_OK;
}

// one pair filter over the entries [lo, hi) of the window sums: the passing pairs' keys ascending in `key` (and their values in `val`), *n_out of them
int tri_pairs(SeqRun& R, const uint64_t* wkey, const int64_t* wsum, int64_t n, uint64_t Ru, int64_t lo, int64_t hi, int32_t which, const dge_triplet_rule& rule, unsigned long long* counters,
              dge_tmp<uint64_t>& key, dge_tmp<int64_t>& val, int64_t* n_out) {
    *n_out = 0;
    const int64_t m = hi - lo;
    SEQ_TRY(seq_alloc(R, key, m, "the pairs"));
    SEQ_TRY(seq_alloc(R, val, m, "the pairs' sums"));
    if (m == 0) return DGE_OK;
    dge_tmp<uint64_t> ukey;
    dge_tmp<int64_t> uval;
    SEQ_TRY(seq_alloc(R, ukey, m, "the unsorted pairs"));
    SEQ_TRY(seq_alloc(R, uval, m, "the unsorted pairs' sums"));
    SEQ_TRY(seq_kernels_begin(R));
    hipLaunchKernelGGL(k_tri_pairs, dim3(seq_grid(m)), dim3(SEQ_BLOCK), 0, R.stream, wkey, wsum, n, Ru, lo, hi, which, rule, ukey.p, uval.p, counters);
    SEQ_TRY(seq_kernels_end(R));
    SEQ_TRY(trip_sort_pairs(R, ukey.p, key.p, uval.p, val.p, m, 64));
    unsigned long long passed = 0;
    SEQ_TRY(seq_read_back(R, &passed, counters + FW_PAIRS_12 + which, 8));
    *n_out = (int64_t)passed;
    return DGE_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------ entries
extern "C" int dge_flows_add_entries(dge_flows* f, const int32_t* hour, const int32_t* src, const int32_t* dst, const int64_t* count, int64_t n) {
    const char* who = "dge_flows_add_entries";
    if (!f || n < 0 || (n > 0 && (!hour || !src || !dst || !count))) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    const dge_regions* rg = f->regions;
    const int64_t Rn = rg->R;
    const uint64_t Ru = (uint64_t)std::max<int64_t>(Rn, 1);
    std::vector<uint64_t> key((size_t)n);
    int64_t added = 0;
    for (int64_t i = 0; i < n; i++) {
        if (hour[i] < 0 || hour[i] > 23) DGE_FAIL(DGE_ERR_ARG, "%s: entry %lld has hour %d: 0 .. 23 is needed", who, (long long)i, hour[i]);
        if (src[i] < 0 || src[i] >= Rn || dst[i] < 0 || dst[i] >= Rn)
            DGE_FAIL(DGE_ERR_ARG, "%s: entry %lld has the region indices (%d, %d): 0 .. %lld is needed", who, (long long)i, src[i], dst[i], (long long)Rn - 1);
        if (count[i] < 1) DGE_FAIL(DGE_ERR_ARG, "%s: entry %lld has count %lld: 1 at least is needed", who, (long long)i, (long long)count[i]);
        if (count[i] > FR_MAX_COUNT) DGE_FAIL(DGE_ERR_RANGE, "%s: entry %lld has count %lld: a key's total may not exceed 2^40", who, (long long)i, (long long)count[i]);
        if ((added += count[i]) > (int64_t)1 << 62) DGE_FAIL(DGE_ERR_RANGE, "%s: the counts up to entry %lld add up to more than 2^62", who, (long long)i);
        key[(size_t)i] = ((uint64_t)hour[i] * Ru + (uint64_t)src[i]) * Ru + (uint64_t)dst[i];
    }
    SEQ_TRY(dge_require_device(rg->device));
    if (n == 0) return DGE_OK;
    SeqRun R;
    SEQ_TRY(seq_open(R, rg->device, who));
    dge_tmp<uint64_t> d_key;
    dge_tmp<int64_t> d_cnt;
    SEQ_TRY(seq_alloc(R, d_key, n, "the entries' keys"));
    SEQ_TRY(seq_alloc(R, d_cnt, n, "the entries' counts"));
    DGE_HIP(hipMemcpyAsync(d_key.p, key.data(), (size_t)n * 8, hipMemcpyHostToDevice, R.stream));
    DGE_HIP(hipMemcpyAsync(d_cnt.p, count, (size_t)n * 8, hipMemcpyHostToDevice, R.stream));
    DGE_HIP(hipStreamSynchronize(R.stream));
    return trip_commit_entries(R, f, d_key.p, d_cnt.p, n, added, (int64_t)FR_MAX_COUNT, who);
}

extern "C" int dge_flows_window_edges(const dge_flows* f, const dge_hour_window* win, int32_t K, int32_t* k, int64_t* src_id, int64_t* dst_id, int64_t* w, int64_t cap, int64_t* n) {
    const char* who = "dge_flows_window_edges";
    if (!n || cap < 0 || (cap > 0 && (!k || !src_id || !dst_id || !w))) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    SEQ_TRY(windows_check(win, K, who));
    if (!f) DGE_FAIL(DGE_ERR_ARG, "%s: null table", who);
    *n = 0;
    if (f->n == 0) return DGE_OK;
    SEQ_TRY(dge_require_device(f->regions->device));
    SeqRun R;
    SEQ_TRY(seq_open(R, f->regions->device, who));
    dge_tmp<uint64_t> okey;
    dge_tmp<int64_t> ow;
    int64_t E = 0;
    SEQ_TRY(win_edges(R, f, win, K, who, okey, ow, &E));
    *n = E;
    if (cap < E) DGE_FAIL(DGE_ERR_CAP, "%s: %lld window edges exceed cap %lld", who, (long long)E, (long long)cap);
    if (E == 0) return DGE_OK;
    SlotArrays A;
    SEQ_TRY(trip_slot_decode(R, f, okey.p, ow.p, E, A));
    SEQ_TRY(seq_read_back(R, k, A.slot.p, (size_t)E * 4));
    SEQ_TRY(seq_read_back(R, src_id, A.src_id.p, (size_t)E * 8));
    SEQ_TRY(seq_read_back(R, dst_id, A.dst_id.p, (size_t)E * 8));
    return seq_read_back(R, w, ow.p, (size_t)E * 8);
}

int dge_flows_windows_check(const dge_hour_window* win, int32_t K, const char* who) { return windows_check(win, K, who); }

int dge_flows_window_keys(const dge_flows* f, const dge_hour_window* win, int32_t K, const char* who, dge_tmp<uint64_t>& key, dge_tmp<int64_t>& w, int64_t* n, double* kernel_ms) {
    *n = 0;
    SeqRun R;
    if (f->n > 0) SEQ_TRY(seq_open(R, f->regions->device, who));
    const int rc = win_edges(R, f, win, K, who, key, w, n);         // (an empty table still gets the range check of K R R)
    *kernel_ms += R.kernel_ms;
    return rc;
}

extern "C" int dge_graph_add_flow_windows(dge_graph* g, const dge_flows* f, const dge_hour_window* win, int32_t K, dge_names* names, dge_od_info* info) {
    const char* who = "dge_graph_add_flow_windows";
    SEQ_TRY(windows_check(win, K, who));
    if (!g || !f) DGE_FAIL(DGE_ERR_ARG, "%s: null argument", who);
    if (g->device != f->regions->device) DGE_FAIL(DGE_ERR_ARG, "%s: the graph is on device %d, the flows on device %d", who, g->device, f->regions->device);
    SEQ_TRY(od_check(g, names, who));
    SEQ_TRY(dge_require_device(g->device));
    SeqRun R;
    SEQ_TRY(seq_open(R, g->device, who));
    dge_tmp<uint64_t> okey;
    dge_tmp<int64_t> ow;
    int64_t E = 0, Rn = 0, S = 0;
    SEQ_TRY(win_edges(R, f, win, K, who, okey, ow, &E));
    SlotArrays A;
    SEQ_TRY(trip_slot_decode(R, f, okey.p, ow.p, E, A));
    SEQ_TRY(od_commit(R, g, names, E, E, K, A.src_id.p, A.dst_id.p, A.w_bits.p, A.slot.p, A.iota.p, who, &Rn, &S));
    if (info) {
        info->bytes = 0; info->lines = 0; info->flows = E; info->edges = E; info->dropped = 0; info->regions = Rn; info->sources = S; info->host_values = 0; info->slices = K; info->reserved = 0;
        info->read_ms = 0; info->kernel_ms = R.kernel_ms;
    }
    return DGE_OK;
}

extern "C" int dge_triplet_rule_default(dge_triplet_rule* rule) {
    if (!rule) DGE_FAIL(DGE_ERR_ARG, "dge_triplet_rule_default: null argument");
    *rule = rule_default();
    return DGE_OK;
}

extern "C" int dge_triplet_rule_check(const dge_triplet_rule* rule, const int64_t sums[13], int32_t* keep) {
    const char* who = "dge_triplet_rule_check";
    if (!sums || !keep) DGE_FAIL(DGE_ERR_ARG, "%s: null argument", who);
    const dge_triplet_rule r = rule ? *rule : rule_default();
    SEQ_TRY(rule_check(&r, who));
    for (int q = 0; q < FR_SUMS; q++)
        if (sums[q] < 0 || sums[q] > 24 * FR_MAX_COUNT) DGE_FAIL(DGE_ERR_ARG, "%s: sum %d is %lld: a window sum lies in 0 .. 24 * 2^40", who, q, (long long)sums[q]);
    *keep = fr_keep(r, sums) ? 1 : 0;
    return DGE_OK;
}

extern "C" int dge_flows_triplets(const dge_flows* f, const dge_triplet_rule* rule, int64_t* id1, int64_t* id2, int64_t* id3, int64_t cap, int64_t* n, dge_triplet_info* info) {
    const char* who = "dge_flows_triplets";
    if (!n || cap < 0 || (cap > 0 && (!id1 || !id2 || !id3))) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    const dge_triplet_rule r = rule ? *rule : rule_default();
    SEQ_TRY(rule_check(&r, who));
    if (!f) DGE_FAIL(DGE_ERR_ARG, "%s: null table", who);
    *n = 0;
    dge_triplet_info I = {};
    if (info) *info = I;
    const dge_regions* rg = f->regions;
    if (f->n == 0 || rg->R < 3) return DGE_OK;
    SEQ_TRY(dge_require_device(rg->device));
    SeqRun R;
    SEQ_TRY(seq_open(R, rg->device, who));
    const uint64_t Ru = (uint64_t)rg->R;
    const dge_hour_window five[5] = {r.A, r.B, r.C, r.D, r.E};
    dge_tmp<uint64_t> wkey, e12, e23, e31;
    dge_tmp<int64_t> wsum, v12, v23, b31, seg, row23, row31, count, first, d_id1, d_id2, d_id3;
    dge_tmp<unsigned long long> counters;
    int64_t nw = 0, n12 = 0, n23 = 0, n31 = 0, bounds[6] = {0, 0, 0, 0, 0, 0}, total = 0;
    unsigned long long c[FW_N];
    SEQ_TRY(win_edges(R, f, five, 5, who, wkey, wsum, &nw));
    SEQ_TRY(seq_alloc(R, counters, FW_N, "the counters"));
    DGE_HIP(hipMemsetAsync(counters.p, 0, FW_N * 8, R.stream));
    if (nw > 0) {
        SEQ_TRY(seq_alloc(R, seg, 6, "the windows' bounds"));
        SEQ_TRY(seq_kernels_begin(R));
        hipLaunchKernelGGL(k_win_bounds, dim3(1), dim3(SEQ_BLOCK), 0, R.stream, wkey.p, nw, Ru, (int64_t)5, seg.p);
        SEQ_TRY(seq_kernels_end(R));
        SEQ_TRY(seq_read_back(R, bounds, seg.p, sizeof(bounds)));
        SEQ_TRY(tri_pairs(R, wkey.p, wsum.p, nw, Ru, bounds[0], bounds[1], 0, r, counters.p, e12, v12, &n12));
        SEQ_TRY(tri_pairs(R, wkey.p, wsum.p, nw, Ru, bounds[1], bounds[2], 1, r, counters.p, e23, v23, &n23));
        SEQ_TRY(tri_pairs(R, wkey.p, wsum.p, nw, Ru, bounds[1], bounds[2], 2, r, counters.p, e31, b31, &n31));
    }
    if (n12 > 0 && n23 > 0 && n31 > 0) {
        const unsigned blocks = (unsigned)((n12 + TRI_WAVES - 1) / TRI_WAVES);
        SEQ_TRY(seq_alloc(R, row23, (int64_t)Ru + 1, "the rows of the (t2, t3) pairs"));
        SEQ_TRY(seq_alloc(R, row31, (int64_t)Ru + 1, "the rows of the (t3, t1) pairs"));
        SEQ_TRY(seq_alloc(R, count, n12 + 1, "the edges' triplets"));
        SEQ_TRY(seq_alloc(R, first, n12 + 1, "the edges' first triplets"));
        DGE_HIP(hipMemsetAsync(count.p, 0, (size_t)(n12 + 1) * 8, R.stream));
        SEQ_TRY(seq_kernels_begin(R));
        hipLaunchKernelGGL(k_tri_rows, dim3(seq_grid((int64_t)Ru + 1)), dim3(SEQ_BLOCK), 0, R.stream, e23.p, n23, Ru, row23.p);
        hipLaunchKernelGGL(k_tri_rows, dim3(seq_grid((int64_t)Ru + 1)), dim3(SEQ_BLOCK), 0, R.stream, e31.p, n31, Ru, row31.p);
        hipLaunchKernelGGL(k_tri_list<false>, dim3(blocks), dim3(SEQ_BLOCK), 0, R.stream, e12.p, n12, e23.p, row23.p, e31.p, b31.p, row31.p, wkey.p, wsum.p, nw, Ru, r, rg->d_id_by_rank, count.p,
                           first.p, (int64_t*)nullptr, (int64_t*)nullptr, (int64_t*)nullptr, counters.p);
        SEQ_TRY(seq_scan(R, count.p, first.p, n12 + 1));
        SEQ_TRY(seq_kernels_end(R));
        SEQ_TRY(seq_read_back(R, &total, first.p + n12, 8));
    }
    SEQ_TRY(seq_read_back(R, c, counters.p, sizeof(c)));
    DGE_HIP(hipGetLastError());
    I.pairs_12 = (int64_t)c[FW_PAIRS_12]; I.pairs_23 = (int64_t)c[FW_PAIRS_23]; I.pairs_31 = (int64_t)c[FW_PAIRS_31]; I.candidates = (int64_t)c[FW_CANDIDATES];
    I.triplets = total; I.kernel_ms = R.kernel_ms;
    *n = total;
    if (info) *info = I;
    if (cap < total) DGE_FAIL(DGE_ERR_CAP, "%s: %lld triplets exceed cap %lld", who, (long long)total, (long long)cap);
    if (total == 0) return DGE_OK;
    SEQ_TRY(seq_alloc(R, d_id1, total, "the triplets' residences"));
    SEQ_TRY(seq_alloc(R, d_id2, total, "the triplets' offices"));
    SEQ_TRY(seq_alloc(R, d_id3, total, "the triplets' night lives"));
    SEQ_TRY(seq_kernels_begin(R));
    hipLaunchKernelGGL(k_tri_list<true>, dim3((unsigned)((n12 + TRI_WAVES - 1) / TRI_WAVES)), dim3(SEQ_BLOCK), 0, R.stream, e12.p, n12, e23.p, row23.p, e31.p, b31.p, row31.p, wkey.p, wsum.p, nw, Ru,
                       r, rg->d_id_by_rank, count.p, first.p, d_id1.p, d_id2.p, d_id3.p, counters.p);
    SEQ_TRY(seq_kernels_end(R));
    DGE_HIP(hipGetLastError());
    if (info) info->kernel_ms = R.kernel_ms;
    SEQ_TRY(seq_read_back(R, id1, d_id1.p, (size_t)total * 8));
    SEQ_TRY(seq_read_back(R, id2, d_id2.p, (size_t)total * 8));
    return seq_read_back(R, id3, d_id3.p, (size_t)total * 8);
}
