// tree.hip — binary CART on resident rows (gfx950) as the fully specified rule of include/dge.h, and its F-fold cross-validated accuracy: the reference's third
// figure of merit (P/embeddingEvaluation_tract.py:201-232, P/binaryClassification_CA.py:33-58).  The per-element pieces, the one comparator among them, live in
// tree_rule.h; this file is what runs them at full concurrency without changing a bit: every quantity that chooses a split is an integer.
//
// Once per call every column's used rows are sorted by value (one radix sort of dim * n 64-bit keys: column, then the order-preserving key of the value; the row
// is the payload).  A batch of trees — all F of a cross-validation where they fit — grows level by level together.  Every column keeps the rows of the batch's
// open nodes as one list, cut into the nodes' segments in (tree, node) order, ascending by value inside a segment; an entry is (tree * n + row) with the row's
// label in the top bit, and the value's key travels beside it.  A level is:
//   a prefix count of the label bits along all lists (one scan over dim * M entries, M = rows in open nodes; a segment's count is a difference),
//   k_tr_cand: a lane per (column, position) scores the cut behind its position where the value changes and a wave reduces to the best per run of one segment,
//   k_tr_best: a wave per node merges the runs of its segment and then the columns — both with tr_better, the comparator of tree_rule.h,
//   the plan (k_tr_plan_a, one scan over the nodes, k_tr_plan_b): children's counts and numbers, the tree arrays, the next level's segments,
//   k_tr_mark: every row of a splitting node is marked left or right from the winning column's list,
//   a prefix count of the left marks, and k_tr_scatter: the stable partition of every list — rows of finished leaves are dropped here.
// So a level costs dim * M whatever the number of nodes; the host reads back one pair of counts per level.  No floating-point operation takes part in choosing
// a split (the two of tr_threshold form the number that is reported), and there is no floating-point atomic.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include <rocprim/iterator/transform_iterator.hpp>

#include "dge_device.h"
#include "tree_rule.h"

#define TR_MAX_DIM 4096
#define TR_ROW_MASK 0x7fffffffu
#define TR_NONE (~0ULL)

extern std::atomic<int64_t> g_dge_tuning[DGE_TUNE_COUNT];      // sgns.hip: the knobs of dge_set_tuning, -1 = the library's own rule

struct tr_node {          // an open node of the level: its segment [start, start + n) of every list
    int32_t start, n, p, tree, id, first;      // tree: number inside the batch; id: node number inside its tree; first: the level's first open node of that tree
};
struct tr_best {
    int32_t f, pos, pL;   // the winning column (-1: none), the last position that goes left, the label-1 rows up to it
};
struct tr_tri {
    int32_t a, b, c;      // splits, open children, rows of open children
};
struct tr_tri_plus {
    __host__ __device__ tr_tri operator()(const tr_tri& x, const tr_tri& y) const { return tr_tri{x.a + y.a, x.b + y.b, x.c + y.c}; }
};
struct tr_label_bit {
    __host__ __device__ uint32_t operator()(uint32_t e) const { return e >> 31; }
};
struct tr_left_flag {
    const uint8_t* mark;
    __host__ __device__ uint32_t operator()(uint32_t e) const { return mark[e & TR_ROW_MASK] == 0 ? 1u : 0u; }
};
struct tr_arrays {        // the trees of a batch back to back; tree t owns [off[t], off[t + 1])
    int32_t* feature;
    double* threshold;
    int32_t* left;
    int64_t* count;
    int64_t* pos;
};

// ------------------------------------------------------------------------------------------ once per call
// key = (column << 32) | key of the value, payload = the used row's number; the least (row, column) of a value that is not finite
__global__ void k_tr_keys(const float* __restrict__ x, const int64_t* __restrict__ used, int64_t n, int dim, uint64_t* __restrict__ keys, uint32_t* __restrict__ rows,
                          unsigned long long* __restrict__ bad) {
    const size_t total = (size_t)n * (size_t)dim, step = (size_t)gridDim.x * blockDim.x;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
        const size_t i = e / (size_t)dim, c = e - i * (size_t)dim;
        const size_t row = used ? (size_t)used[i] : i;
        const uint32_t bits = __float_as_uint(x[row * (size_t)dim + c]);
        if (!tr_finite_bits(bits)) atomicMin(bad, (unsigned long long)e);
        keys[c * (size_t)n + i] = ((uint64_t)c << 32) | tr_key_bits(bits);
        rows[c * (size_t)n + i] = (uint32_t)i;
    }
}

// the batch's first lists: every tree takes a copy of every column's sorted rows (segment = tree), and a row is marked 0 where it trains the tree
__global__ void k_tr_first_lists(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ rows, const uint8_t* __restrict__ y, int64_t n, int dim, int trees,
                                 uint32_t* __restrict__ ent, uint32_t* __restrict__ key) {
    const size_t M = (size_t)trees * (size_t)n, total = M * (size_t)dim, step = (size_t)gridDim.x * blockDim.x;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
        const size_t c = e / M, r = e - c * M, t = r / (size_t)n, i = r - t * (size_t)n;
        const uint32_t row = rows[c * (size_t)n + i];
        ent[e] = (uint32_t)(t * (size_t)n + row) | ((uint32_t)y[row] << 31);
        key[e] = (uint32_t)keys[c * (size_t)n + i];
    }
}
__global__ void k_tr_first_marks(const int32_t* __restrict__ fold, int64_t n, int trees, int tree0, uint8_t* __restrict__ mark, int32_t* __restrict__ seg) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (int64_t)trees * n) return;
    const int64_t t = r / n, i = r - t * n;
    mark[r] = fold[i] == tree0 + (int)t ? 1 : 0;
    seg[r] = (int32_t)t;
}
__global__ void k_tr_roots(tr_arrays T, const int64_t* __restrict__ off, const int64_t* __restrict__ n_t, const int64_t* __restrict__ p_t, int trees) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < trees) { T.count[off[t]] = n_t[t]; T.pos[off[t]] = p_t[t]; }
}

// ------------------------------------------------------------------------------------------ a level
// seg[pos] = the open node whose segment holds pos
__global__ void k_tr_seg(const tr_node* __restrict__ node, int K, int M, int32_t* __restrict__ seg) {
    const int pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= M) return;
    int lo = 0, hi = K - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (node[mid].start <= pos) lo = mid; else hi = mid - 1;
    }
    seg[pos] = lo;
}

// label-1 rows of column c's list from the start of node nd's segment up to and including pos (G: the inclusive prefix count over all lists, modulo 2^32)
__device__ __forceinline__ int32_t tr_count_to(const uint32_t* __restrict__ G, size_t base, const tr_node& nd, int pos) {
    const size_t g0 = base + (size_t)nd.start;
    return (int32_t)(G[base + (size_t)pos] - (g0 ? G[g0 - 1] : 0u));
}

// the candidate behind position pos of column c in node nd (D = 0: none)
__device__ __forceinline__ tr_cand tr_cand_at(const uint32_t* __restrict__ key, const uint32_t* __restrict__ G, size_t base, const tr_node& nd, int pos, int c,
                                              const tr_limits& lim, int32_t* pL_out) {
    tr_cand x{0, 0, c, 0};
    if (pos + 1 >= nd.start + nd.n) return x;
    const uint32_t ka = key[base + (size_t)pos], kb = key[base + (size_t)pos + 1];
    if (ka == kb) return x;
    const int64_t nL = pos - nd.start + 1;
    if (!tr_valid_cut(nd.n, nL, lim)) return x;
    const int32_t pL = tr_count_to(G, base, nd, pos);
    tr_score(nd.n, nd.p, nL, pL, &x.N, &x.D);
    x.a = ka;
    *pL_out = pL;
    return x;
}

// HOT.  grid (ceil(M / 256), dim).  A lane per position of one column; a wave reduces its 64 positions by segment (the segments are runs: seg ascends) and the
// first lane of every run writes the run's best position, or -1, to partial[(wave + segment) * dim + column] — wave + segment grows along the runs of a column,
// so every run has a slot of its own, and the runs of segment k are the slots (first wave of k) + k .. (last wave of k) + k.
__global__ void __launch_bounds__(256) k_tr_cand(const uint32_t* __restrict__ key, const uint32_t* __restrict__ G, const int32_t* __restrict__ seg,
                                                 const tr_node* __restrict__ node, int M, int dim, tr_limits lim, int32_t* __restrict__ partial) {
    const int c = blockIdx.y, pos = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const size_t base = (size_t)c * (size_t)M;
    const bool in = pos < M;
    const int k = in ? seg[pos] : 0x7fffffff;
    tr_cand x{0, 0, c, 0};
    int32_t best = -1;
    if (in) {
        int32_t pL;
        x = tr_cand_at(key, G, base, node[k], pos, c, lim, &pL);
        if (x.D) best = pos;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        tr_cand y;
        y.N = __shfl_down((unsigned long long)x.N, o);
        y.D = __shfl_down((unsigned long long)x.D, o);
        y.a = __shfl_down(x.a, o);
        y.f = c;
        const int32_t yb = __shfl_down(best, o);
        const int yk = __shfl_down(k, o);
        if (lane + o < 64 && yk == k && tr_better(y, x)) { x = y; best = yb; }
    }
    const int before = __shfl_up(k, 1);
    if (in && (lane == 0 || before != k)) partial[((size_t)(pos >> 6) + (size_t)k) * (size_t)dim + (size_t)c] = best;
}

// HOT.  A wave per open node: lane l merges the runs of columns l, l + 64, ..., then the lanes merge.  Every comparison is tr_better.
__global__ void __launch_bounds__(64) k_tr_best(const uint32_t* __restrict__ key, const uint32_t* __restrict__ G, const tr_node* __restrict__ node, int M, int dim,
                                                tr_limits lim, const int32_t* __restrict__ partial, tr_best* __restrict__ out) {
    const int k = blockIdx.x, lane = threadIdx.x;
    const tr_node nd = node[k];
    const int w0 = nd.start >> 6, w1 = (nd.start + nd.n - 1) >> 6;
    tr_cand x{0, 0, 0, 0};
    int32_t bpos = -1, bpL = 0;
    for (int c = lane; c < dim; c += 64) {
        const size_t base = (size_t)c * (size_t)M;
        for (int w = w0; w <= w1; w++) {
            const int32_t pp = partial[((size_t)w + (size_t)k) * (size_t)dim + (size_t)c];
            if (pp < 0) continue;
            int32_t pL = 0;
            const tr_cand y = tr_cand_at(key, G, base, nd, pp, c, lim, &pL);
            if (tr_better(y, x)) { x = y; bpos = pp; bpL = pL; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        tr_cand y;
        y.N = __shfl_xor((unsigned long long)x.N, o);
        y.D = __shfl_xor((unsigned long long)x.D, o);
        y.a = __shfl_xor(x.a, o);
        y.f = __shfl_xor(x.f, o);
        const int32_t yb = __shfl_xor(bpos, o), yp = __shfl_xor(bpL, o);
        if (tr_better(y, x)) { x = y; bpos = yb; bpL = yp; }
    }
    if (lane == 0) out[k] = tr_best{x.D ? x.f : -1, bpos, bpL};
}

// what a node's split makes: the children's rows and label-1 rows and whether they stay open
struct tr_kids {
    int32_t nL, pL, nR, pR;
    bool openL, openR;
};
__device__ __forceinline__ tr_kids tr_kids_of(const tr_node& nd, const tr_best& b, int level, const tr_limits& lim) {
    tr_kids q;
    q.nL = b.pos - nd.start + 1; q.pL = b.pL; q.nR = nd.n - q.nL; q.pR = nd.p - q.pL;
    q.openL = !tr_is_leaf(q.nL, q.pL, level + 1, lim);
    q.openR = !tr_is_leaf(q.nR, q.pR, level + 1, lim);
    return q;
}

__global__ void k_tr_plan_a(const tr_node* __restrict__ node, const tr_best* __restrict__ best, int K, int level, tr_limits lim, tr_tri* __restrict__ tri) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    tr_tri t{0, 0, 0};
    if (best[k].f >= 0) {
        const tr_kids q = tr_kids_of(node[k], best[k], level, lim);
        t.a = 1; t.b = (q.openL ? 1 : 0) + (q.openR ? 1 : 0); t.c = (q.openL ? q.nL : 0) + (q.openR ? q.nR : 0);
    }
    tri[k] = t;
}

// ex: the exclusive sums of tri over the level's nodes.  A node that splits takes the next two numbers of its tree, in node order; its open children become
// nodes of the next level, in that order, with their segments back to back.  dest[2k], dest[2k + 1]: where the rows that go left / right start in the next
// lists (-1: the child is a finished leaf and its rows leave).  splits[tree]: the tree's splits of this level.  totals: the next level's nodes and rows.
__global__ void k_tr_plan_b(const tr_node* __restrict__ node, const tr_best* __restrict__ best, const tr_tri* __restrict__ tri, const tr_tri* __restrict__ ex, int K, int M,
                            int level, tr_limits lim, const uint32_t* __restrict__ key, tr_arrays T, const int64_t* __restrict__ off, const int32_t* __restrict__ next_id,
                            tr_node* __restrict__ node2, int32_t* __restrict__ dest, int32_t* __restrict__ splits, int32_t* __restrict__ totals) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const tr_node nd = node[k];
    const tr_best b = best[k];
    const tr_tri e = ex[k], e0 = ex[nd.first];
    int32_t dl = -1, dr = -1;
    if (b.f >= 0) {
        const tr_kids q = tr_kids_of(nd, b, level, lim);
        const int64_t o = off[nd.tree];
        const int32_t left = next_id[nd.tree] + 2 * (e.a - e0.a);
        const size_t at = (size_t)b.f * (size_t)M + (size_t)b.pos;
        T.feature[o + nd.id] = b.f;
        T.threshold[o + nd.id] = tr_threshold(__uint_as_float(tr_unkey_bits(key[at])), __uint_as_float(tr_unkey_bits(key[at + 1])));
        T.left[o + nd.id] = left;
        T.count[o + left] = q.nL; T.pos[o + left] = q.pL;
        T.count[o + left + 1] = q.nR; T.pos[o + left + 1] = q.pR;
        int32_t idx = e.b, rows = e.c;
        if (q.openL) { node2[idx] = tr_node{rows, q.nL, q.pL, nd.tree, left, e0.b}; dl = rows; idx++; rows += q.nL; }
        if (q.openR) { node2[idx] = tr_node{rows, q.nR, q.pR, nd.tree, left + 1, e0.b}; dr = rows; }
    }
    dest[2 * k] = dl; dest[2 * k + 1] = dr;
    if (k == K - 1 || node[k + 1].tree != nd.tree) splits[nd.tree] = e.a + tri[k].a - e0.a;
    if (k == K - 1) { totals[0] = e.b + tri[k].b; totals[1] = e.c + tri[k].c; }
}
__global__ void k_tr_bump(int32_t* __restrict__ splits, int32_t* __restrict__ next_id, int32_t* __restrict__ depth, int trees, int level) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= trees) return;
    if (splits[t] > 0) { next_id[t] += 2 * splits[t]; depth[t] = level + 1; }
    splits[t] = 0;
}

// every row of a node that splits: 0 = left, 1 = right, read off the winning column's list
__global__ void k_tr_mark(const uint32_t* __restrict__ ent, const int32_t* __restrict__ seg, const tr_best* __restrict__ best, int M, uint8_t* __restrict__ mark) {
    const int pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= M) return;
    const tr_best b = best[seg[pos]];
    if (b.f < 0) return;                                       // its rows leave: the mark is read (as "not left") but decides nothing
    mark[ent[(size_t)b.f * (size_t)M + (size_t)pos] & TR_ROW_MASK] = pos <= b.pos ? 0 : 1;
}

// HOT.  grid (ceil(M / 256), dim).  The stable partition: H is the inclusive prefix count of the left marks along all lists; an entry's place among its node's
// left (right) rows in its column is a difference of two of them.
__global__ void __launch_bounds__(256) k_tr_scatter(const uint32_t* __restrict__ ent, const uint32_t* __restrict__ key, const uint32_t* __restrict__ H,
                                                    const int32_t* __restrict__ seg, const tr_node* __restrict__ node, const int32_t* __restrict__ dest,
                                                    const uint8_t* __restrict__ mark, int M, int M2, uint32_t* __restrict__ ent2, uint32_t* __restrict__ key2) {
    const int c = blockIdx.y, pos = blockIdx.x * 256 + threadIdx.x;
    if (pos >= M) return;
    const int k = seg[pos];
    const int32_t dl = dest[2 * k], dr = dest[2 * k + 1];
    if (dl < 0 && dr < 0) return;
    const size_t base = (size_t)c * (size_t)M;
    const uint32_t e = ent[base + (size_t)pos];
    const bool is_left = mark[e & TR_ROW_MASK] == 0;
    const int32_t d = is_left ? dl : dr;
    if (d < 0) return;
    const int start = node[k].start;
    const size_t g0 = base + (size_t)start;
    const int32_t lefts = (int32_t)(H[base + (size_t)pos] - (g0 ? H[g0 - 1] : 0u));       // up to and including pos
    const int32_t place = is_left ? d + lefts - 1 : d + (pos - start) - lefts;
    const size_t to = (size_t)c * (size_t)M2 + (size_t)place;
    ent2[to] = e;
    key2[to] = key[base + (size_t)pos];
}

// ------------------------------------------------------------------------------------------ prediction
// A lane per row.  trees > 0: the row's tree is its fold (cross-validation: rows outside [tree0, tree0 + trees) are another batch's); the count of rows whose vote
// equals their label goes to correct[fold].  trees == 0: one tree, the vote goes to out (255 on an absent row).  The tree was checked on the host or built here:
// a child's number is greater than its parent's and inside the tree.
__global__ void k_tr_predict(const float* __restrict__ x, const int64_t* __restrict__ used, const uint8_t* __restrict__ present, int64_t n, int dim, tr_arrays T,
                             const int64_t* __restrict__ off, const int32_t* __restrict__ fold, const uint8_t* __restrict__ y, int tree0, int trees,
                             unsigned long long* __restrict__ correct, uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int64_t o = 0;
    if (trees > 0) {
        const int t = fold[i] - tree0;
        if (t < 0 || t >= trees) return;
        o = off[t];
    } else if (present && !present[i]) { out[i] = 255; return; }
    const size_t row = used ? (size_t)used[i] : (size_t)i;
    int32_t k = 0;
    for (;;) {
        const int32_t f = T.feature[o + k];
        if (f < 0) break;
        k = T.left[o + k] + (tr_goes_left(x[row * (size_t)dim + (size_t)f], T.threshold[o + k]) ? 0 : 1);
    }
    const uint8_t vote = tr_vote(T.count[o + k], T.pos[o + k]);
    if (trees > 0) { if (vote == y[i]) atomicAdd(&correct[fold[i]], 1ULL); }
    else out[i] = vote;
}

// ------------------------------------------------------------------------------------------ host
// the scratch of the library's scans: one buffer that only grows, so that a level allocates nothing
struct tr_scratch {
    dge_tmp<uint8_t> t;
    size_t cap = 0;
    const char* who = "";
    int operator()(size_t bytes, void** p) {
        if (bytes > cap) { if (int rc = dge_alloc_for(t, bytes, who)) return rc; cap = bytes; }
        *p = t.p;
        return DGE_OK;
    }
};

static int tree_cfg_check(const char* who, const dge_tree_cfg* cfg, tr_limits* lim) {
    *lim = tr_limits{0, 2, 1};
    if (!cfg) return DGE_OK;
    if (cfg->max_depth < 0) DGE_FAIL(DGE_ERR_ARG, "%s: max_depth = %d must not be negative (0 = no limit)", who, cfg->max_depth);
    if (cfg->min_samples_split < 2) DGE_FAIL(DGE_ERR_ARG, "%s: min_samples_split = %d must be at least 2", who, cfg->min_samples_split);
    if (cfg->min_samples_leaf < 1) DGE_FAIL(DGE_ERR_ARG, "%s: min_samples_leaf = %d must be at least 1", who, cfg->min_samples_leaf);
    *lim = tr_limits{cfg->max_depth, cfg->min_samples_split, cfg->min_samples_leaf};
    return DGE_OK;
}

struct tree_out {         // what a run gives: per tree
    std::vector<int32_t> n_nodes, depth;
    std::vector<int64_t> correct;
    std::vector<int32_t> feature, left;      // tree 0's arrays (keep_arrays)
    std::vector<double> threshold;
    std::vector<int64_t> count, pos;
    int64_t levels = 0;
    int32_t batches = 0;
    float ms = 0.f;
};

// every tree of the call has rows to train on, and no more than the lists hold: tree t trains on the used rows with fold != t
static int tree_counts(const char* who, const ur_rows& u, int trees) {
    for (int t = 0; t < trees; t++) {
        const int64_t nt = u.n - ((size_t)t < u.tested.size() ? u.tested[(size_t)t] : 0);
        if (nt == 0) DGE_FAIL(DGE_ERR_ARG, "%s: fold %d has no training rows", who, t);
        if (nt > TR_MAX_ROWS) DGE_FAIL(DGE_ERR_RANGE, "%s: %lld rows would train tree %d; at most 2^20 may", who, (long long)nt, t);
    }
    return DGE_OK;
}

// The used rows u (tree_counts has passed them), their labels y and folds (u.fold[i] outside 0 .. trees-1: the row trains every tree and tests none), grow `trees`
// trees: tree t trains on the used rows with fold != t.  predict: count the test rows every tree votes right.
static int tree_run(const char* who, const dge_vectors* v, const ur_rows& u, const std::vector<uint8_t>& y, int trees, const tr_limits& lim, bool predict, bool keep_arrays,
                    tree_out* out) {
    const std::vector<int32_t>& fold = u.fold;
    const int dim = v->dim;
    const int64_t n = u.n;
    int rc;
    std::vector<int64_t> n_t((size_t)trees, 0), p_t((size_t)trees, 0);
    for (int t = 0; t < trees; t++)
        for (int64_t i = 0; i < n; i++) if (fold[(size_t)i] != t) { n_t[(size_t)t]++; p_t[(size_t)t] += y[(size_t)i]; }
    const size_t dn = (size_t)dim * (size_t)n;

    // how many trees grow together: what fits half the free memory (about 23 bytes an entry of a list: two lists with keys, the prefix counts, the runs), at most
    // what keeps tree * n + row in 31 bits, and at most what the knob says
    size_t free_b = 0, total_b = 0;
    DGE_HIP(hipMemGetInfo(&free_b, &total_b));
    const size_t per_tree = dn * 23 + (size_t)n * 64 + 4096;
    const size_t fixed = dn * 24;
    int64_t batch = free_b / 2 > fixed ? (int64_t)((free_b / 2 - fixed) / per_tree) : 0;
    batch = std::min<int64_t>(batch, (int64_t)0x7fffffff / (n > 0 ? n : 1));
    const int64_t knob = g_dge_tuning[DGE_TUNE_TREE_BATCH];
    if (knob > 0) batch = std::min(batch, knob);
    batch = std::max<int64_t>(1, std::min<int64_t>(batch, trees));
    if ((int64_t)batch * n > 0x7fffffffLL) DGE_FAIL(DGE_ERR_RANGE, "%s: %lld rows x %d columns are too many for one tree's lists", who, (long long)n, dim);

    dge_used_rows d_used;
    dge_tmp<uint8_t> d_y, d_mark;
    dge_tmp<int32_t> d_fold, d_seg, d_partial, d_dest, d_splits, d_next, d_depth, d_totals;
    dge_tmp<uint64_t> d_keys, d_keys_in;
    dge_tmp<uint32_t> d_rows, d_rows_in, d_ent[2], d_key[2], d_G;
    dge_tmp<unsigned long long> d_bad, d_correct;
    dge_tmp<tr_node> d_node[2];
    dge_tmp<tr_best> d_best;
    dge_tmp<tr_tri> d_tri, d_ex;
    dge_tmp<int64_t> d_off, d_nt, d_pt;
    dge_tmp<int32_t> d_feature, d_left;
    dge_tmp<double> d_threshold;
    dge_tmp<int64_t> d_count, d_pos;
    tr_scratch scratch;
    scratch.who = who;

    if ((rc = d_used.upload(u, who))) return rc;
    const int64_t* dused = d_used.p;
    if ((rc = dge_alloc_for(d_y, (size_t)n, who)) || (rc = dge_alloc_for(d_fold, (size_t)n, who)) || (rc = dge_alloc_for(d_bad, 1, who)) || (rc = dge_alloc_for(d_correct, (size_t)trees, who)) ||
        (rc = dge_alloc_for(d_keys, dn, who)) || (rc = dge_alloc_for(d_rows, dn, who)) || (rc = dge_alloc_for(d_keys_in, dn, who)) || (rc = dge_alloc_for(d_rows_in, dn, who))) return rc;
    DGE_HIP(hipMemcpy(d_y.p, y.data(), (size_t)n, hipMemcpyHostToDevice));
    DGE_HIP(hipMemcpy(d_fold.p, fold.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));

    dge_stopwatch watch;
    if ((rc = watch.start(0))) return rc;
    DGE_HIP(hipMemsetAsync(d_bad.p, 0xff, sizeof(unsigned long long), 0));
    DGE_HIP(hipMemsetAsync(d_correct.p, 0, (size_t)trees * sizeof(unsigned long long), 0));
    {
        const size_t blocks = (dn + 255) / 256;
        hipLaunchKernelGGL(k_tr_keys, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, 0, v->d, dused, n, dim, d_keys_in.p, d_rows_in.p, d_bad.p);
        DGE_HIP(hipGetLastError());
    }
    unsigned long long bad = TR_NONE;
    DGE_HIP(hipMemcpy(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost));
    if (bad != TR_NONE)
        DGE_FAIL(DGE_ERR_ARG, "%s: row %lld, column %lld holds a value that is not finite", who, (long long)u.at((int64_t)(bad / (unsigned long long)dim)), (long long)(bad % (unsigned long long)dim));
    if ((rc = dge_sort_pairs(scratch, d_keys_in.p, d_keys.p, d_rows_in.p, d_rows.p, (int64_t)dn, 32 + dge_bits((uint64_t)dim), 0, true))) return rc;
    (void)hipFree(d_keys_in.release());
    (void)hipFree(d_rows_in.release());

    out->n_nodes.assign((size_t)trees, 0); out->depth.assign((size_t)trees, 0); out->correct.assign((size_t)trees, 0);
    const size_t Mcap = (size_t)batch * (size_t)n, Kcap = Mcap / 2 + (size_t)batch + 1;
    if ((rc = dge_alloc_for(d_ent[0], Mcap * dim, who)) || (rc = dge_alloc_for(d_ent[1], Mcap * dim, who)) || (rc = dge_alloc_for(d_key[0], Mcap * dim, who)) ||
        (rc = dge_alloc_for(d_key[1], Mcap * dim, who)) || (rc = dge_alloc_for(d_G, Mcap * dim, who)) || (rc = dge_alloc_for(d_seg, Mcap, who)) || (rc = dge_alloc_for(d_mark, Mcap, who)) ||
        (rc = dge_alloc_for(d_partial, ((Mcap + 63) / 64 + Kcap) * (size_t)dim, who)) || (rc = dge_alloc_for(d_node[0], Kcap, who)) || (rc = dge_alloc_for(d_node[1], Kcap, who)) ||
        (rc = dge_alloc_for(d_best, Kcap, who)) || (rc = dge_alloc_for(d_tri, Kcap, who)) || (rc = dge_alloc_for(d_ex, Kcap, who)) || (rc = dge_alloc_for(d_dest, 2 * Kcap, who)) ||
        (rc = dge_alloc_for(d_splits, (size_t)batch, who)) || (rc = dge_alloc_for(d_next, (size_t)batch, who)) || (rc = dge_alloc_for(d_depth, (size_t)batch, who)) ||
        (rc = dge_alloc_for(d_totals, 2, who)) || (rc = dge_alloc_for(d_off, (size_t)batch + 1, who)) || (rc = dge_alloc_for(d_nt, (size_t)batch, who)) || (rc = dge_alloc_for(d_pt, (size_t)batch, who))) return rc;

    std::vector<tr_node> nodes;
    std::vector<int32_t> dest, ones;
    std::vector<int64_t> off;
    for (int t0 = 0; t0 < trees; t0 += (int)batch) {
        const int tb = std::min<int>((int)batch, trees - t0);
        out->batches++;
        // the trees' arrays: tree t of the batch may come to 2 n_t - 1 nodes
        off.assign((size_t)tb + 1, 0);
        for (int t = 0; t < tb; t++) off[(size_t)t + 1] = off[(size_t)t] + 2 * n_t[(size_t)(t0 + t)] - 1;
        const size_t cap_nodes = (size_t)off[(size_t)tb];
        if ((rc = dge_alloc_for(d_feature, cap_nodes, who)) || (rc = dge_alloc_for(d_left, cap_nodes, who)) || (rc = dge_alloc_for(d_threshold, cap_nodes, who)) ||
            (rc = dge_alloc_for(d_count, cap_nodes, who)) || (rc = dge_alloc_for(d_pos, cap_nodes, who))) return rc;
        const tr_arrays T{d_feature.p, d_threshold.p, d_left.p, d_count.p, d_pos.p};
        DGE_HIP(hipMemsetAsync(d_feature.p, 0xff, cap_nodes * sizeof(int32_t), 0));
        DGE_HIP(hipMemsetAsync(d_left.p, 0xff, cap_nodes * sizeof(int32_t), 0));
        DGE_HIP(hipMemsetAsync(d_threshold.p, 0, cap_nodes * sizeof(double), 0));
        DGE_HIP(hipMemsetAsync(d_splits.p, 0, (size_t)tb * sizeof(int32_t), 0));
        DGE_HIP(hipMemsetAsync(d_depth.p, 0, (size_t)tb * sizeof(int32_t), 0));
        ones.assign((size_t)tb, 1);
        DGE_HIP(hipMemcpy(d_next.p, ones.data(), (size_t)tb * sizeof(int32_t), hipMemcpyHostToDevice));
        DGE_HIP(hipMemcpy(d_off.p, off.data(), ((size_t)tb + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
        DGE_HIP(hipMemcpy(d_nt.p, n_t.data() + t0, (size_t)tb * sizeof(int64_t), hipMemcpyHostToDevice));
        DGE_HIP(hipMemcpy(d_pt.p, p_t.data() + t0, (size_t)tb * sizeof(int64_t), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_tr_roots, dim3(dge_grid(tb)), dim3(256), 0, 0, T, d_off.p, d_nt.p, d_pt.p, tb);

        // the step in front of level 0: every tree's copy of the sorted columns is one segment, its training rows go "left" into the root's segment
        int K = tb, M = (int)((int64_t)tb * n), cur = 0;
        nodes.clear(); dest.assign(2 * (size_t)tb, -1);
        std::vector<tr_node> first((size_t)tb);
        int M2 = 0;
        for (int t = 0; t < tb; t++) {
            first[(size_t)t] = tr_node{(int32_t)((int64_t)t * n), (int32_t)n, 0, t, 0, t};
            const int64_t nt = n_t[(size_t)(t0 + t)], pt = p_t[(size_t)(t0 + t)];
            if (tr_is_leaf(nt, pt, 0, lim)) continue;
            dest[2 * (size_t)t] = M2;
            nodes.push_back(tr_node{M2, (int32_t)nt, (int32_t)pt, t, 0, (int32_t)nodes.size()});
            M2 += (int)nt;
        }
        if (!nodes.empty()) {
            DGE_HIP(hipMemcpy(d_node[0].p, first.data(), (size_t)tb * sizeof(tr_node), hipMemcpyHostToDevice));
            DGE_HIP(hipMemcpy(d_dest.p, dest.data(), 2 * (size_t)tb * sizeof(int32_t), hipMemcpyHostToDevice));
            {
                const size_t total = (size_t)M * (size_t)dim, blocks = (total + 255) / 256;
                hipLaunchKernelGGL(k_tr_first_lists, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, 0, d_keys.p, d_rows.p, d_y.p, n, dim, tb, d_ent[0].p, d_key[0].p);
                hipLaunchKernelGGL(k_tr_first_marks, dim3(dge_grid(M)), dim3(256), 0, 0, d_fold.p, n, tb, t0, d_mark.p, d_seg.p);
                DGE_HIP(hipGetLastError());
            }
            const size_t flat = (size_t)M * (size_t)dim;
            if ((rc = dge_two_pass(scratch, [&](void* tmp, size_t& bytes) {
                    return rocprim::inclusive_scan(tmp, bytes, rocprim::make_transform_iterator(d_ent[0].p, tr_left_flag{d_mark.p}), d_G.p, flat, rocprim::plus<uint32_t>(), (hipStream_t)0);
                }, 0, false))) return rc;
            hipLaunchKernelGGL(k_tr_scatter, dim3(dge_grid(M), (unsigned)dim), dim3(256), 0, 0, d_ent[0].p, d_key[0].p, d_G.p, d_seg.p, d_node[0].p, d_dest.p, d_mark.p, M, M2,
                               d_ent[1].p, d_key[1].p);
            DGE_HIP(hipGetLastError());
            DGE_HIP(hipMemcpyAsync(d_node[1].p, nodes.data(), nodes.size() * sizeof(tr_node), hipMemcpyHostToDevice, 0));
            DGE_HIP(hipStreamSynchronize(0));                  // `nodes` and `first` are host memory the copies above read
            cur = 1; K = (int)nodes.size(); M = M2;
        } else K = 0;

        for (int level = 0; K > 0; level++) {
            out->levels++;
            uint32_t* ent = d_ent[cur].p; uint32_t* key = d_key[cur].p;
            tr_node* node = d_node[cur].p;
            const size_t flat = (size_t)M * (size_t)dim;
            hipLaunchKernelGGL(k_tr_seg, dim3(dge_grid(M)), dim3(256), 0, 0, node, K, M, d_seg.p);
            if ((rc = dge_two_pass(scratch, [&](void* tmp, size_t& bytes) {
                    return rocprim::inclusive_scan(tmp, bytes, rocprim::make_transform_iterator(ent, tr_label_bit{}), d_G.p, flat, rocprim::plus<uint32_t>(), (hipStream_t)0);
                }, 0, false))) return rc;
            hipLaunchKernelGGL(k_tr_cand, dim3(dge_grid(M), (unsigned)dim), dim3(256), 0, 0, key, d_G.p, d_seg.p, node, M, dim, lim, d_partial.p);
            hipLaunchKernelGGL(k_tr_best, dim3((unsigned)K), dim3(64), 0, 0, key, d_G.p, node, M, dim, lim, d_partial.p, d_best.p);
            hipLaunchKernelGGL(k_tr_plan_a, dim3(dge_grid(K)), dim3(256), 0, 0, node, d_best.p, K, level, lim, d_tri.p);
            DGE_HIP(hipGetLastError());
            if ((rc = dge_two_pass(scratch, [&](void* tmp, size_t& bytes) {
                    return rocprim::exclusive_scan(tmp, bytes, d_tri.p, d_ex.p, tr_tri{0, 0, 0}, (size_t)K, tr_tri_plus(), (hipStream_t)0);
                }, 0, false))) return rc;
            hipLaunchKernelGGL(k_tr_plan_b, dim3(dge_grid(K)), dim3(256), 0, 0, node, d_best.p, d_tri.p, d_ex.p, K, M, level, lim, key, T, d_off.p, d_next.p, d_node[1 - cur].p,
                               d_dest.p, d_splits.p, d_totals.p);
            hipLaunchKernelGGL(k_tr_bump, dim3(dge_grid(tb)), dim3(256), 0, 0, d_splits.p, d_next.p, d_depth.p, tb, level);
            DGE_HIP(hipGetLastError());
            int32_t totals[2] = {0, 0};
            DGE_HIP(hipMemcpy(totals, d_totals.p, sizeof totals, hipMemcpyDeviceToHost));      // the level's one read-back
            const int K2 = totals[0], M2n = totals[1];
            if (K2 < 0 || (size_t)K2 > Kcap || M2n < 0 || M2n > M) DGE_FAIL(DGE_ERR_STATE, "%s: level %d planned %d nodes on %d rows out of %d", who, level, K2, M2n, M);
            if (K2 > 0) {
                hipLaunchKernelGGL(k_tr_mark, dim3(dge_grid(M)), dim3(256), 0, 0, ent, d_seg.p, d_best.p, M, d_mark.p);
                if ((rc = dge_two_pass(scratch, [&](void* tmp, size_t& bytes) {
                        return rocprim::inclusive_scan(tmp, bytes, rocprim::make_transform_iterator(ent, tr_left_flag{d_mark.p}), d_G.p, flat, rocprim::plus<uint32_t>(), (hipStream_t)0);
                    }, 0, false))) return rc;
                hipLaunchKernelGGL(k_tr_scatter, dim3(dge_grid(M), (unsigned)dim), dim3(256), 0, 0, ent, key, d_G.p, d_seg.p, node, d_dest.p, d_mark.p, M, M2n, d_ent[1 - cur].p,
                                   d_key[1 - cur].p);
                DGE_HIP(hipGetLastError());
            }
            cur = 1 - cur; K = K2; M = M2n;
        }

        if (predict) {
            hipLaunchKernelGGL(k_tr_predict, dim3(dge_grid(n)), dim3(256), 0, 0, v->d, dused, (const uint8_t*)nullptr, n, dim, T, d_off.p, d_fold.p, d_y.p, t0, tb, d_correct.p,
                               (uint8_t*)nullptr);
            DGE_HIP(hipGetLastError());
        }
        std::vector<int32_t> nn((size_t)tb), dd((size_t)tb);
        DGE_HIP(hipMemcpy(nn.data(), d_next.p, (size_t)tb * sizeof(int32_t), hipMemcpyDeviceToHost));
        DGE_HIP(hipMemcpy(dd.data(), d_depth.p, (size_t)tb * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int t = 0; t < tb; t++) { out->n_nodes[(size_t)(t0 + t)] = nn[(size_t)t]; out->depth[(size_t)(t0 + t)] = dd[(size_t)t]; }
        if (keep_arrays && t0 == 0) {
            const size_t m = (size_t)nn[0];
            out->feature.resize(m); out->left.resize(m); out->threshold.resize(m); out->count.resize(m); out->pos.resize(m);
            DGE_HIP(hipMemcpy(out->feature.data(), d_feature.p, m * sizeof(int32_t), hipMemcpyDeviceToHost));
            DGE_HIP(hipMemcpy(out->left.data(), d_left.p, m * sizeof(int32_t), hipMemcpyDeviceToHost));
            DGE_HIP(hipMemcpy(out->threshold.data(), d_threshold.p, m * sizeof(double), hipMemcpyDeviceToHost));
            DGE_HIP(hipMemcpy(out->count.data(), d_count.p, m * sizeof(int64_t), hipMemcpyDeviceToHost));
            DGE_HIP(hipMemcpy(out->pos.data(), d_pos.p, m * sizeof(int64_t), hipMemcpyDeviceToHost));
        }
    }
    if ((rc = watch.stop(&out->ms))) return rc;
    if (predict) {
        std::vector<unsigned long long> c((size_t)trees);
        DGE_HIP(hipMemcpy(c.data(), d_correct.p, (size_t)trees * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (int t = 0; t < trees; t++) out->correct[(size_t)t] = (int64_t)c[(size_t)t];
    }
    return DGE_OK;
}

static void tree_fill_info(dge_tree_info* info, int64_t rows, const tree_out& o) {
    if (!info) return;
    info->rows = rows; info->n_nodes = 0; info->depth = 0;
    for (size_t t = 0; t < o.n_nodes.size(); t++) { info->n_nodes += o.n_nodes[t]; info->depth = std::max(info->depth, o.depth[t]); }
    info->levels = (int32_t)o.levels; info->trees = (int32_t)o.n_nodes.size(); info->batches = o.batches; info->kernel_ms = o.ms;
}

// the walk of both fits and both cross-validations: pres the present bytes (nullptr: every row); the first offence in the entry's words
static int tree_intake(const char* who, int64_t rows, const uint8_t* pres, const uint8_t* y, const uint8_t* select, const int32_t* fold, int32_t n_folds, ur_rows* u) {
    ur_intake(ur_in{rows, pres, select, fold, n_folds, y, 1}, u);
    if (!fold) ur_no_folds(u);
    if (u->kind == UR_FOLD) DGE_FAIL(DGE_ERR_ARG, "%s: row %lld has fold %d, outside -1 .. %d", who, (long long)u->bad_row, u->bad_value, n_folds - 1);
    if (u->kind == UR_LABEL) DGE_FAIL(DGE_ERR_ARG, "%s: row %lld has label %d; labels are 0 or 1", who, (long long)u->bad_row, u->bad_value);
    if (!fold && u->n == 0) DGE_FAIL(DGE_ERR_ARG, "%s: no row to train on", who);
    return fold ? tree_counts(who, *u, n_folds) : DGE_OK;
}

static int tree_fit_run(const char* who, const dge_vectors* v, const ur_rows& u, const uint8_t* y, const tr_limits& lim, int64_t cap, int32_t* feature, double* threshold,
                        int32_t* left, int64_t* count, int64_t* pos, dge_tree_info* info) {
    int rc = tree_counts(who, u, 1);
    if (rc) return rc;
    tree_out o;
    if ((rc = tree_run(who, v, u, ur_gather_labels(u, y, 1), 1, lim, false, true, &o))) return rc;
    const int64_t m = o.n_nodes[0];
    if (m > cap) {
        if (info) info->n_nodes = m;
        DGE_FAIL(DGE_ERR_CAP, "%s: the tree has %lld nodes, the arrays hold %lld", who, (long long)m, (long long)cap);
    }
    memcpy(feature, o.feature.data(), (size_t)m * sizeof(int32_t));
    memcpy(threshold, o.threshold.data(), (size_t)m * sizeof(double));
    memcpy(left, o.left.data(), (size_t)m * sizeof(int32_t));
    memcpy(count, o.count.data(), (size_t)m * sizeof(int64_t));
    memcpy(pos, o.pos.data(), (size_t)m * sizeof(int64_t));
    tree_fill_info(info, u.n, o);
    return DGE_OK;
}

static int tree_cv_run(const char* who, const dge_vectors* v, const ur_rows& u, const uint8_t* y, int32_t n_folds, const tr_limits& lim, int64_t* correct, int64_t* tested,
                       int32_t* n_nodes, int32_t* depth, dge_tree_info* info) {
    tree_out o;
    if (int rc = tree_run(who, v, u, ur_gather_labels(u, y, 1), n_folds, lim, true, false, &o)) return rc;
    for (int t = 0; t < n_folds; t++) { correct[t] = o.correct[(size_t)t]; tested[t] = u.tested[(size_t)t]; if (n_nodes) n_nodes[t] = o.n_nodes[(size_t)t]; if (depth) depth[t] = o.depth[(size_t)t]; }
    tree_fill_info(info, u.n, o);
    return DGE_OK;
}

// a *_vectors entry behind its limit checks: the device, the present bytes, the walk
static int tree_vectors_intake(const char* who, const dge_vectors* v, const uint8_t* y, const uint8_t* select, const int32_t* fold, int32_t n_folds, ur_rows* u) {
    int rc = dge_require_device(v->device);
    dge_present pres;
    if (rc || (rc = pres.load(v))) return rc;
    return tree_intake(who, v->rows, pres.p, y, select, fold, n_folds, u);
}

extern "C" int dge_tree_fit_vectors(const dge_vectors* v, const uint8_t* y, const uint8_t* select, const dge_tree_cfg* cfg, int64_t cap, int32_t* feature, double* threshold,
                                    int32_t* left, int64_t* count, int64_t* pos, dge_tree_info* info) {
    const char* who = "dge_tree_fit_vectors";
    if (!v || !y || !feature || !threshold || !left || !count || !pos || cap < 0) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    tr_limits lim;
    ur_rows u;
    int rc = tree_cfg_check(who, cfg, &lim);
    if (rc || (rc = dge_range_check(who, "dim", v->dim, TR_MAX_DIM)) || (rc = tree_vectors_intake(who, v, y, select, nullptr, 0, &u))) return rc;
    return tree_fit_run(who, v, u, y, lim, cap, feature, threshold, left, count, pos, info);
}

extern "C" int dge_tree_fit(int device, const float* features, int64_t n_rows, int32_t dim, const uint8_t* y, const uint8_t* select, const dge_tree_cfg* cfg, int64_t cap,
                            int32_t* feature, double* threshold, int32_t* left, int64_t* count, int64_t* pos, dge_tree_info* info) {
    const char* who = "dge_tree_fit";
    if (!features || !y || !feature || !threshold || !left || !count || !pos || n_rows < 0 || dim < 0 || cap < 0) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    tr_limits lim;
    ur_rows u;
    int rc = tree_cfg_check(who, cfg, &lim);
    if (rc || (rc = dge_range_check(who, "dim", dim, TR_MAX_DIM)) || (rc = tree_intake(who, n_rows, nullptr, y, select, nullptr, 0, &u))) return rc;
    if (u.n > TR_MAX_ROWS) DGE_FAIL(DGE_ERR_RANGE, "%s: %lld rows would train the tree; at most 2^20 may", who, (long long)u.n);
    dge_vectors_guard g;
    if ((rc = dge_vectors_from_host(device, features, n_rows, dim, nullptr, &g.v))) return rc;
    return tree_fit_run(who, g.v, u, y, lim, cap, feature, threshold, left, count, pos, info);
}

extern "C" int dge_tree_cv_vectors(const dge_vectors* v, const uint8_t* y, const int32_t* fold, int32_t n_folds, const dge_tree_cfg* cfg, int64_t* correct, int64_t* tested,
                                   int32_t* n_nodes, int32_t* depth, dge_tree_info* info) {
    const char* who = "dge_tree_cv_vectors";
    if (!v || !y || !fold || !correct || !tested) DGE_FAIL(DGE_ERR_ARG, "%s: null argument", who);
    tr_limits lim;
    ur_rows u;
    int rc = tree_cfg_check(who, cfg, &lim);
    if (rc || (rc = dge_range_check(who, "n_folds", n_folds, TR_MAX_FOLDS)) || (rc = dge_range_check(who, "dim", v->dim, TR_MAX_DIM))) return rc;
    for (int64_t i = 0; i < v->rows; i++)                          // every row's fold before a device is looked for, the labels behind the present bytes
        if (fold[i] < -1 || fold[i] >= n_folds) DGE_FAIL(DGE_ERR_ARG, "%s: row %lld has fold %d, outside -1 .. %d", who, (long long)i, fold[i], n_folds - 1);
    if ((rc = tree_vectors_intake(who, v, y, nullptr, fold, n_folds, &u))) return rc;
    return tree_cv_run(who, v, u, y, n_folds, lim, correct, tested, n_nodes, depth, info);
}

extern "C" int dge_tree_cv(int device, const float* features, int64_t n_rows, int32_t dim, const uint8_t* y, const int32_t* fold, int32_t n_folds, const dge_tree_cfg* cfg,
                           int64_t* correct, int64_t* tested, int32_t* n_nodes, int32_t* depth, dge_tree_info* info) {
    const char* who = "dge_tree_cv";
    if (!features || !y || !fold || !correct || !tested || n_rows < 0 || dim < 0) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    tr_limits lim;
    ur_rows u;
    int rc = tree_cfg_check(who, cfg, &lim);
    if (rc || (rc = dge_range_check(who, "n_folds", n_folds, TR_MAX_FOLDS)) || (rc = dge_range_check(who, "dim", dim, TR_MAX_DIM)) ||
        (rc = tree_intake(who, n_rows, nullptr, y, nullptr, fold, n_folds, &u))) return rc;
    dge_vectors_guard g;
    if ((rc = dge_vectors_from_host(device, features, n_rows, dim, nullptr, &g.v))) return rc;
    return tree_cv_run(who, g.v, u, y, n_folds, lim, correct, tested, n_nodes, depth, info);
}

extern "C" int dge_tree_predict_vectors(const dge_vectors* v, int64_t n_nodes, const int32_t* feature, const double* threshold, const int32_t* left, const int64_t* count,
                                        const int64_t* pos, uint8_t* out_labels) {
    const char* who = "dge_tree_predict_vectors";
    if (!v || !feature || !threshold || !left || !count || !pos || !out_labels) DGE_FAIL(DGE_ERR_ARG, "%s: null argument", who);
    if (n_nodes < 1 || n_nodes > 2 * TR_MAX_ROWS) DGE_FAIL(DGE_ERR_ARG, "%s: n_nodes = %lld is outside 1 .. 2^21", who, (long long)n_nodes);
    // a tree the kernel can walk blindly: every inner node names a column of the rows and two children behind it and inside the tree
    for (int64_t k = 0; k < n_nodes; k++) {
        if (feature[k] == -1) continue;
        if (feature[k] < 0 || feature[k] >= v->dim) DGE_FAIL(DGE_ERR_ARG, "%s: node %lld tests column %d; the rows have %d", who, (long long)k, feature[k], v->dim);
        if ((int64_t)left[k] <= k || (int64_t)left[k] + 1 >= n_nodes) DGE_FAIL(DGE_ERR_ARG, "%s: node %lld has children %lld and %lld, outside %lld .. %lld", who, (long long)k, (long long)left[k], (long long)left[k] + 1, (long long)k + 1, (long long)n_nodes - 1);
    }
    int rc;
    if ((rc = dge_require_device(v->device))) return rc;
    const size_t m = (size_t)n_nodes;
    dge_tmp<int32_t> d_feature, d_left;
    dge_tmp<double> d_threshold;
    dge_tmp<int64_t> d_count, d_pos;
    dge_tmp<uint8_t> d_out;
    if ((rc = dge_alloc_for(d_feature, m, who)) || (rc = dge_alloc_for(d_left, m, who)) || (rc = dge_alloc_for(d_threshold, m, who)) || (rc = dge_alloc_for(d_count, m, who)) ||
        (rc = dge_alloc_for(d_pos, m, who)) || (rc = dge_alloc_for(d_out, (size_t)v->rows, who))) return rc;
    DGE_HIP(hipMemcpy(d_feature.p, feature, m * sizeof(int32_t), hipMemcpyHostToDevice));
    DGE_HIP(hipMemcpy(d_left.p, left, m * sizeof(int32_t), hipMemcpyHostToDevice));
    DGE_HIP(hipMemcpy(d_threshold.p, threshold, m * sizeof(double), hipMemcpyHostToDevice));
    DGE_HIP(hipMemcpy(d_count.p, count, m * sizeof(int64_t), hipMemcpyHostToDevice));
    DGE_HIP(hipMemcpy(d_pos.p, pos, m * sizeof(int64_t), hipMemcpyHostToDevice));
    if (v->rows) {
        const tr_arrays T{d_feature.p, d_threshold.p, d_left.p, d_count.p, d_pos.p};
        hipLaunchKernelGGL(k_tr_predict, dim3(dge_grid(v->rows)), dim3(256), 0, 0, v->d, (const int64_t*)nullptr, v->d_present, v->rows, v->dim, T, (const int64_t*)nullptr,
                           (const int32_t*)nullptr, (const uint8_t*)nullptr, 0, 0, (unsigned long long*)nullptr, d_out.p);
        DGE_HIP(hipGetLastError());
        DGE_HIP(hipMemcpy(out_labels, d_out.p, (size_t)v->rows, hipMemcpyDeviceToHost));
    }
    return DGE_OK;
}
