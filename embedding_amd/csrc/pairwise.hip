// pairwise.hip — the reference's headline figure per slice on resident rows (gfx950): evalute_by_pairwise_similarity of
// P/embeddingEvaluation_tract.py:285-367 (nDCG@k of every method's neighbour lists under the POI ground truth, precision@k against the ground's nearest
// rel_m, coverage), as the rule of include/dge.h.  The per-element arithmetic lives in pairwise_rule.h; this file runs it without changing a bit.
//
// The estimated lists come from knn.hip's strip kernel, set by set, on the members' feature rows gathered into a stack (k_pw_gather) and mapped back to region
// numbers (k_pw_map_back).  The ground side is binary64 VALU only — no MFMA, no floating-point atomic — and is built in the simpler of the forms the design
// allows: the ideal lists in a pass of their own, the ranks in a second pass that serves every set at once.
//   k_pw_norms   a lane per ground row: its sum of squares and whether it has a direction.
//   k_pw_ideal   a lane per query region; the block's query rows stay in LDS, all n ground rows stream through LDS in tiles, a lane keeps the kmax least
//                keys (distance, region) of its region in LDS under a threshold that only tightens, and ends with the ideal DCG chain.
//   k_pw_rank    a workgroup per region r: the keys of r's neighbours in every set where r is tested are sorted once in LDS (bitonic, padded with keys that sort
//                last); every column c forms dist(r, c) once, finds its place among them by bisection and counts itself in an integer LDS histogram; the
//                histogram's prefix sums are the ranks.  Integer counters: the order of the columns cannot change them.
//   k_pw_score   a lane per (set, region): the DCG chain over the list, cut at every k of the call, and the hits.
// The means are the host's: a plain ascending sum over the tested regions.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dge_device.h"
#include "pairwise_rule.h"

#define PW_RANK_THREADS 256
#define PW_LDS_CAP (160 * 1024)

struct pw_ground {                       // what every ground kernel reads
    const float* x;                      // [n x g]
    const double* ss;                    // [n]
    const uint8_t* live;                 // [n]
    int n, g;
};

__global__ void k_pw_norms(const float* __restrict__ x, const uint8_t* __restrict__ present, int n, int g, double* __restrict__ ss, uint8_t* __restrict__ live) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const float* row = x + (size_t)r * g;
    double s = 0.0;
    for (int j = 0; j < g; j++) s = pw_step(s, row[j], row[j]);
    ss[r] = s;
    live[r] = (!present || present[r]) && pw_live(s) ? 1 : 0;
}

// dist(r, c) with r's row wherever the caller holds it (LDS) and c's row in global memory
__device__ __forceinline__ double pw_dist_to(const pw_ground& G, const float* row_r, double ss_r, bool live_r, int c) {
    return pw_dist_rows(row_r, G.x + (size_t)c * G.g, G.g, ss_r, G.ss[c], live_r, G.live[c] != 0);
}

// HOT.  blockDim.x = QB query regions, a lane each.  LDS: Ld [QB][kmax] binary64, the tile's sums of squares [tc] binary64, Li [QB][kmax], the tile's live flags
// [tc], the query rows [QB][g | 1] (an odd pitch: the lanes of a wave read one column of different rows), the column tile [tc][g] (every lane reads the same
// element: a broadcast).  The loop over a tile's columns reads LDS only: a workgroup is one wave, and nothing would hide a global load per column.
__global__ void k_pw_ideal(pw_ground G, int kmax, int tc, const double* __restrict__ disc, const int32_t* __restrict__ ks, int n_k, int32_t* __restrict__ out_idx,
                           double* __restrict__ out_dist, double* __restrict__ ideal) {
    extern __shared__ double pw_lds[];
    const int QB = blockDim.x, t = threadIdx.x, q0 = blockIdx.x * QB, q = q0 + t, n = G.n, g = G.g, pitch = g | 1;
    double* Ld = pw_lds;
    double* Tss = Ld + (size_t)QB * kmax;
    int32_t* Li = (int32_t*)(Tss + tc);
    int32_t* Tlive = Li + (size_t)QB * kmax;
    float* Q = (float*)(Tlive + tc);
    float* T = Q + (size_t)QB * pitch;
    for (int e = t; e < QB * g; e += QB) {
        const int row = e / g, j = e - row * g;
        Q[row * pitch + j] = q0 + row < n ? G.x[(size_t)(q0 + row) * g + j] : 0.0f;
    }
    double* ld = Ld + (size_t)t * kmax;
    int32_t* li = Li + (size_t)t * kmax;
    for (int i = 0; i < kmax; i++) { ld[i] = (double)INFINITY; li[i] = INT_MAX; }
    const bool mine = q < n;
    const double ss_q = mine ? G.ss[q] : 0.0;
    const bool live_q = mine && G.live[q] != 0;
    const float* row_q = Q + (size_t)t * pitch;
    double thr_d = (double)INFINITY;
    int32_t thr_i = INT_MAX;
    for (int c0 = 0; c0 < n; c0 += tc) {
        const int cn = n - c0 < tc ? n - c0 : tc;
        __syncthreads();                                          // the last tile is read, and (first trip) Q is written
        for (int e = t; e < cn * g; e += QB) T[e] = G.x[(size_t)c0 * g + e];
        for (int e = t; e < cn; e += QB) { Tss[e] = G.ss[c0 + e]; Tlive[e] = G.live[c0 + e]; }
        __syncthreads();
        if (!mine) continue;
        for (int cc = 0; cc < cn; cc++) {
            const int c = c0 + cc;
            if (c == q) continue;
            const double d = pw_dist_rows(row_q, T + cc * g, g, ss_q, Tss[cc], live_q, Tlive[cc] != 0);
            if (!pw_key_less(d, c, thr_d, thr_i)) continue;
            int pos = kmax - 1;                                   // rare once the list has warmed up
            while (pos > 0 && pw_key_less(d, c, ld[pos - 1], li[pos - 1])) { ld[pos] = ld[pos - 1]; li[pos] = li[pos - 1]; pos--; }
            ld[pos] = d; li[pos] = c;
            thr_d = ld[kmax - 1]; thr_i = li[kmax - 1];
        }
    }
    if (!mine) return;
    double acc = 0.0;
    int j = 0;
    for (int i = 0; i < kmax; i++) {
        if (out_idx) { out_idx[(size_t)q * kmax + i] = li[i]; out_dist[(size_t)q * kmax + i] = ld[i]; }
        if (ideal) {
            acc = pw_gain(acc, ld[i], disc[i]);
            if (j < n_k && i == ks[j] - 1) { ideal[(size_t)j * n + q] = acc; j++; }
        }
    }
}

// the key of slot e = s * kmax + i of region r: (dist(r, nb), nb), or the pad (+inf, INT_MAX) where r is not tested in s or e is past the slots
__device__ __forceinline__ bool pw_slot_key(const pw_ground& G, const float* row_r, double ss_r, bool live_r, int r, int e, int kmax, int n_sets,
                                            const int32_t* __restrict__ lists, const uint8_t* __restrict__ tested, double* d, int32_t* c) {
    const int s = e / kmax, i = e - s * kmax;
    if (s < n_sets && tested[(size_t)s * G.n + r]) {
        const int32_t nb = lists[((size_t)s * G.n + r) * kmax + i];
        *d = pw_dist_to(G, row_r, ss_r, live_r, nb); *c = nb;
        return true;
    }
    *d = (double)INFINITY; *c = INT_MAX;
    return false;
}

// HOT.  One workgroup per region; Tp: n_sets * kmax rounded up to a power of two.  LDS: kd [Tp] binary64, kc [Tp], hist [Tp + 1], part [256], the row [g].
__global__ void __launch_bounds__(PW_RANK_THREADS) k_pw_rank(pw_ground G, int kmax, int n_sets, int Tp, const int32_t* __restrict__ lists,
                                                             const uint8_t* __restrict__ tested, int rel_m, uint8_t* __restrict__ hit) {
    extern __shared__ double pw_lds[];
    double* kd = pw_lds;
    int32_t* kc = (int32_t*)(kd + Tp);
    int32_t* hist = kc + Tp;
    int32_t* part = hist + Tp + 1;
    float* row_r = (float*)(part + PW_RANK_THREADS);
    const int t = threadIdx.x, r = blockIdx.x, n = G.n, g = G.g;
    if (!__syncthreads_or(t < n_sets && tested[(size_t)t * n + r])) return;          // the whole workgroup leaves together
    for (int j = t; j < g; j += PW_RANK_THREADS) row_r[j] = G.x[(size_t)r * g + j];
    const double ss_r = G.ss[r];
    const bool live_r = G.live[r] != 0;
    __syncthreads();
    for (int e = t; e < Tp; e += PW_RANK_THREADS) {
        pw_slot_key(G, row_r, ss_r, live_r, r, e, kmax, n_sets, lists, tested, &kd[e], &kc[e]);
        hist[e] = 0;
    }
    if (t == 0) hist[Tp] = 0;
    for (int k2 = 2; k2 <= Tp; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int e = t; e < Tp; e += PW_RANK_THREADS) {
                const int l = e ^ j;
                if (l <= e) continue;
                const double da = kd[e], db = kd[l];
                const int32_t ca = kc[e], cb = kc[l];
                const bool up = (e & k2) == 0;
                if (up ? pw_key_less(db, cb, da, ca) : pw_key_less(da, ca, db, cb)) { kd[e] = db; kc[e] = cb; kd[l] = da; kc[l] = ca; }
            }
        }
    __syncthreads();
    // column c counts for every sorted key above its own: hist[p], p = the number of sorted keys <= key(c)
    for (int c = t; c < n; c += PW_RANK_THREADS) {
        if (c == r) continue;
        const double d = pw_dist_to(G, row_r, ss_r, live_r, c);
        int lo = 0, hi = Tp;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (pw_key_less(d, c, kd[mid], kc[mid])) hi = mid; else lo = mid + 1;
        }
        atomicAdd(&hist[lo], 1);
    }
    __syncthreads();
    // hist[i] := hist[0] + .. + hist[i], the rank of sorted key i
    const int per = (Tp + PW_RANK_THREADS - 1) / PW_RANK_THREADS, e0 = t * per, e1 = e0 + per < Tp ? e0 + per : Tp;
    int sum = 0;
    for (int e = e0; e < e1; e++) sum += hist[e];
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int w = 0; w < PW_RANK_THREADS; w++) { const int v = part[w]; part[w] = run; run += v; }
    }
    __syncthreads();
    int run = part[t];
    for (int e = e0; e < e1; e++) { run += hist[e]; hist[e] = run; }
    __syncthreads();
    for (int e = t; e < n_sets * kmax; e += PW_RANK_THREADS) {
        double d; int32_t c;
        if (!pw_slot_key(G, row_r, ss_r, live_r, r, e, kmax, n_sets, lists, tested, &d, &c)) continue;
        int lo = 0, hi = Tp;                                       // the first sorted key that is not below this one: the key itself (equal keys share a rank)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (pw_key_less(kd[mid], kc[mid], d, c)) lo = mid + 1; else hi = mid;
        }
        const int s = e / kmax, i = e - s * kmax;
        hit[((size_t)s * n + r) * kmax + i] = hist[lo] < rel_m ? 1 : 0;
    }
}

// a lane per (set, region).  ratio, hits: [n_sets x n_k x n], 0 where the region is not tested.
__global__ void k_pw_score(pw_ground G, int kmax, int n_sets, const int32_t* __restrict__ lists, const uint8_t* __restrict__ tested, const uint8_t* __restrict__ hit,
                           const double* __restrict__ disc, const int32_t* __restrict__ ks, int n_k, const double* __restrict__ ideal, double* __restrict__ ratio,
                           int32_t* __restrict__ hits) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int n = G.n;
    if (e >= (size_t)n_sets * n) return;
    const int s = (int)(e / n), r = (int)(e - (size_t)s * n);
    if (!tested[e]) {
        for (int j = 0; j < n_k; j++) { ratio[((size_t)s * n_k + j) * n + r] = 0.0; hits[((size_t)s * n_k + j) * n + r] = 0; }
        return;
    }
    const float* row_r = G.x + (size_t)r * G.g;
    const double ss_r = G.ss[r];
    const bool live_r = G.live[r] != 0;
    double acc = 0.0;
    int h = 0, j = 0;
    for (int i = 0; i < kmax; i++) {
        const int32_t nb = lists[e * kmax + i];
        acc = pw_gain(acc, pw_dist_to(G, row_r, ss_r, live_r, nb), disc[i]);
        if (hit && hit[e * kmax + i]) h++;
        if (j < n_k && i == ks[j] - 1) {
            ratio[((size_t)s * n_k + j) * n + r] = pw_ratio(acc, ideal[(size_t)j * n + r]);
            hits[((size_t)s * n_k + j) * n + r] = h;
            j++;
        }
    }
}

// the members' feature rows of one set, stacked in region order
__global__ void k_pw_gather(const float* __restrict__ f, const int64_t* __restrict__ rows, int m, int D, float* __restrict__ stack) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)m * D) return;
    const size_t j = e / D, c = e - j * D;
    stack[e] = f[(size_t)rows[j] * D + c];
}
// lists of the stack's rows -> lists of the set's regions, in region numbers
__global__ void k_pw_map_back(const int32_t* __restrict__ idx, const int32_t* __restrict__ region, int m, int kmax, int32_t* __restrict__ lists_s) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)m * kmax) return;
    const size_t j = e / kmax, i = e - j * kmax;
    lists_s[(size_t)region[j] * kmax + i] = region[idx[e]];
}

// ------------------------------------------------------------------------------------------ the host side
struct pw_ground_dev {
    dge_tmp<double> ss;
    dge_tmp<uint8_t> live;
    pw_ground G;
    int make(const dge_vectors* gnd, const char* who) {
        const int n = (int)gnd->rows;
        int rc;
        if ((rc = dge_alloc_for(ss, (size_t)n, who)) || (rc = dge_alloc_for(live, (size_t)n, who))) return rc;
        hipLaunchKernelGGL(k_pw_norms, dim3(dge_grid(n)), dim3(256), 0, 0, gnd->d, gnd->n_present == gnd->rows ? (const uint8_t*)nullptr : gnd->d_present, n, gnd->dim, ss.p, live.p);
        DGE_HIP(hipGetLastError());
        G.x = gnd->d; G.ss = ss.p; G.live = live.p; G.n = n; G.g = gnd->dim;
        return DGE_OK;
    }
};

// the ideal pass: the block is 64, 32 or 16 query regions, the most that keep the LDS within 64 KB (several workgroups a compute unit)
static int pw_launch_ideal(const pw_ground& G, int kmax, const double* d_disc, const int32_t* d_ks, int n_k, int32_t* d_idx, double* d_dist, double* d_ideal, const char* who) {
    const int g = G.g, pitch = g | 1;
    int tc = 4096 / g;
    tc = tc > 64 ? 64 : (tc < 8 ? 8 : tc);
    auto bytes = [&](int qb) { return ((size_t)qb * kmax + tc) * 12 + ((size_t)qb * pitch + (size_t)tc * g) * 4; };
    int qb = 64;
    while (qb > 16 && bytes(qb) > 64 * 1024) qb >>= 1;            // 16 regions at kmax = 128, g = 256 take 58 KB: the loop always ends inside the limit
    const size_t lds = bytes(qb);
    if (lds > PW_LDS_CAP) DGE_FAIL(DGE_ERR_ARG, "%s: lists of %d with ground rows of %d values need more than the 160 KB of LDS", who, kmax, g);
    (void)hipFuncSetAttribute((const void*)k_pw_ideal, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_pw_ideal, dim3((G.n + qb - 1) / qb), dim3(qb), lds, 0, G, kmax, tc, d_disc, d_ks, n_k, d_idx, d_dist, d_ideal);
    DGE_HIP(hipGetLastError());
    return DGE_OK;
}

static int pw_ground_args(const char* who, const dge_vectors* gnd, int64_t need) {
    if (gnd->rows < 2 || gnd->rows > 0x7fffffffLL) DGE_FAIL(DGE_ERR_ARG, "%s: %lld ground rows: 2 .. 2^31 - 1 regions", who, (long long)gnd->rows);
    if (gnd->dim < 1 || gnd->dim > PW_MAX_DIM) DGE_FAIL(DGE_ERR_ARG, "%s: ground dim = %d is outside 1 .. %d", who, gnd->dim, PW_MAX_DIM);
    if (gnd->rows - 1 < need) DGE_FAIL(DGE_ERR_ARG, "%s: lists of %lld need more than %lld other regions (n - 1 < kmax)", who, (long long)need, (long long)(gnd->rows - 1));
    return DGE_OK;
}

extern "C" int dge_pairwise_ground_vectors(const dge_vectors* gnd, int32_t m, int32_t* idx, double* dist) {
    const char* who = "dge_pairwise_ground_vectors";
    if (!gnd || !idx || !dist) DGE_FAIL(DGE_ERR_ARG, "%s: null argument", who);
    if (m < 1 || m > PW_MAX_K) DGE_FAIL(DGE_ERR_ARG, "%s: m = %d is outside 1 .. %d", who, m, PW_MAX_K);
    int rc = pw_ground_args(who, gnd, m);
    if (rc) return rc;
    if ((rc = dge_require_device(gnd->device))) return rc;
    const size_t n = (size_t)gnd->rows;
    pw_ground_dev gd;
    dge_tmp<int32_t> d_idx; dge_tmp<double> d_dist;
    if ((rc = gd.make(gnd, who)) || (rc = dge_alloc_for(d_idx, n * m, who)) || (rc = dge_alloc_for(d_dist, n * m, who))) return rc;
    if ((rc = pw_launch_ideal(gd.G, m, nullptr, nullptr, 0, d_idx.p, d_dist.p, nullptr, who))) return rc;
    DGE_HIP(hipMemcpy(idx, d_idx.p, n * m * sizeof(int32_t), hipMemcpyDeviceToHost));
    DGE_HIP(hipMemcpy(dist, d_dist.p, n * m * sizeof(double), hipMemcpyDeviceToHost));
    return DGE_OK;
}

extern "C" int dge_pairwise_eval_vectors(const dge_vectors* f, const dge_vectors* gnd, const int64_t* row_of, int32_t n_sets, const uint8_t* test, const int32_t* ks,
                                         int32_t n_k, int32_t rel_m, double* ndcg, double* precision, int64_t* members, int64_t* tested, double* ratio, int32_t* hits,
                                         int32_t* lists, double* ideal, dge_pairwise_info* info) {
    const char* who = "dge_pairwise_eval_vectors";
    // ---- everything a host can check, before a device is looked for
    if (!f || !gnd || !row_of || !ks || !ndcg || !members || !tested) DGE_FAIL(DGE_ERR_ARG, "%s: null argument", who);
    if (n_sets < 1 || n_sets > PW_MAX_SETS) DGE_FAIL(DGE_ERR_ARG, "%s: n_sets = %d is outside 1 .. %d", who, n_sets, PW_MAX_SETS);
    if (n_k < 1 || n_k > PW_MAX_NK) DGE_FAIL(DGE_ERR_ARG, "%s: n_k = %d is outside 1 .. %d", who, n_k, PW_MAX_NK);
    for (int j = 0; j < n_k; j++) {
        if (ks[j] < 1 || ks[j] > PW_MAX_K) DGE_FAIL(DGE_ERR_ARG, "%s: ks[%d] = %d is outside 1 .. %d", who, j, ks[j], PW_MAX_K);
        if (j && ks[j] <= ks[j - 1]) DGE_FAIL(DGE_ERR_ARG, "%s: ks[%d] = %d after ks[%d] = %d: ks must be strictly ascending", who, j, ks[j], j - 1, ks[j - 1]);
    }
    const int kmax = ks[n_k - 1];
    int rc = pw_ground_args(who, gnd, kmax);
    if (rc) return rc;
    const int64_t V = f->rows;
    const int n = (int)gnd->rows, D = f->dim;
    if (V < 1 || V > 0x7fffffffLL) DGE_FAIL(DGE_ERR_ARG, "%s: %lld feature rows", who, (long long)V);
    if (D < 1 || D > PW_MAX_DIM) DGE_FAIL(DGE_ERR_ARG, "%s: dim = %d is outside 1 .. %d", who, D, PW_MAX_DIM);
    if (rel_m < 0 || rel_m > n - 1) DGE_FAIL(DGE_ERR_ARG, "%s: rel_m = %d is outside 0 .. n - 1 = %d", who, rel_m, n - 1);
    if ((rel_m != 0) != (precision != nullptr)) DGE_FAIL(DGE_ERR_ARG, "%s: precision must be NULL if and only if rel_m == 0 (rel_m = %d)", who, rel_m);
    if (f->device != gnd->device) DGE_FAIL(DGE_ERR_ARG, "%s: the features and the ground rows are on devices %d and %d", who, f->device, gnd->device);
    {
        std::vector<int64_t> named;
        for (int s = 0; s < n_sets; s++) {
            named.clear();
            for (int i = 0; i < n; i++) {
                const int64_t row = row_of[(size_t)s * n + i];
                if (row < -1 || row >= V) DGE_FAIL(DGE_ERR_ARG, "%s: set %d, region %d: row_of = %lld is outside -1 .. %lld", who, s, i, (long long)row, (long long)(V - 1));
                if (row >= 0) named.push_back(row);
            }
            std::sort(named.begin(), named.end());
            for (size_t j = 1; j < named.size(); j++)
                if (named[j] == named[j - 1]) DGE_FAIL(DGE_ERR_ARG, "%s: set %d names feature row %lld twice", who, s, (long long)named[j]);
        }
    }
    // ---- the device; the presence of a row is the one check that needs its data
    if ((rc = dge_require_device(f->device))) return rc;
    dge_present pres;
    if ((rc = pres.load(f))) return rc;
    std::vector<int32_t> region; std::vector<int64_t> rows; std::vector<size_t> first((size_t)n_sets + 1, 0);
    std::vector<uint8_t> h_tested((size_t)n_sets * n, 0);
    std::vector<int64_t> n_members((size_t)n_sets), n_tested((size_t)n_sets, 0);
    for (int s = 0; s < n_sets; s++) {
        for (int i = 0; i < n; i++) {
            const int64_t row = row_of[(size_t)s * n + i];
            if (row < 0 || (pres.p && !pres.p[row])) continue;
            region.push_back(i); rows.push_back(row);
            if (!test || test[i]) { h_tested[(size_t)s * n + i] = 1; n_tested[s]++; }
        }
        first[s + 1] = region.size();
        n_members[s] = (int64_t)(first[s + 1] - first[s]);
    }
    for (int s = 0; s < n_sets; s++)
        if (n_members[s] < kmax + 1) DGE_FAIL(DGE_ERR_ARG, "%s: set %d has %lld members: lists of %d need at least %d", who, s, (long long)n_members[s], kmax, kmax + 1);
    const int64_t m_max = *std::max_element(n_members.begin(), n_members.end());
    const size_t total = region.size(), cells = (size_t)n_sets * n;

    std::vector<double> h_disc((size_t)kmax);
    for (int i = 0; i < kmax; i++) h_disc[i] = pw_disc_host(i);
    dge_tmp<double> d_disc, d_ideal, d_ratio; dge_tmp<int32_t> d_ks, d_region, d_lists, d_hits, d_oi; dge_tmp<int64_t> d_rows; dge_tmp<uint8_t> d_tested, d_hit;
    dge_tmp<float> d_stack, d_xn, d_inv, d_od;
    if ((rc = dge_alloc_for(d_disc, (size_t)kmax, who)) || (rc = dge_alloc_for(d_ks, (size_t)n_k, who)) || (rc = dge_alloc_for(d_region, total, who)) ||
        (rc = dge_alloc_for(d_rows, total, who)) || (rc = dge_alloc_for(d_tested, cells, who)) || (rc = dge_alloc_for(d_lists, cells * kmax, who)) ||
        (rc = dge_alloc_for(d_ideal, (size_t)n_k * n, who)) || (rc = dge_alloc_for(d_ratio, cells * n_k, who)) || (rc = dge_alloc_for(d_hits, cells * n_k, who)) ||
        (rc = dge_alloc_for(d_stack, (size_t)m_max * D, who)) || (rc = dge_alloc_for(d_xn, (size_t)m_max * 256, who)) || (rc = dge_alloc_for(d_inv, (size_t)m_max, who)) ||
        (rc = dge_alloc_for(d_od, (size_t)m_max * kmax, who)) || (rc = dge_alloc_for(d_oi, (size_t)m_max * kmax, who))) return rc;
    if (rel_m && (rc = dge_alloc_for(d_hit, cells * kmax, who))) return rc;
    DGE_HIP(hipMemcpy(d_disc.p, h_disc.data(), (size_t)kmax * sizeof(double), hipMemcpyHostToDevice));
    DGE_HIP(hipMemcpy(d_ks.p, ks, (size_t)n_k * sizeof(int32_t), hipMemcpyHostToDevice));
    DGE_HIP(hipMemcpy(d_region.p, region.data(), total * sizeof(int32_t), hipMemcpyHostToDevice));
    DGE_HIP(hipMemcpy(d_rows.p, rows.data(), total * sizeof(int64_t), hipMemcpyHostToDevice));
    DGE_HIP(hipMemcpy(d_tested.p, h_tested.data(), cells, hipMemcpyHostToDevice));
    DGE_HIP(hipMemsetAsync(d_lists.p, 0xff, cells * kmax * sizeof(int32_t), 0));          // -1 rows for non-members

    // ---- the estimated lists, set by set: exactly dge_knn_cosine on the stacked members
    double knn_ms = 0.0;
    for (int s = 0; s < n_sets; s++) {
        const int m = (int)n_members[s];
        hipLaunchKernelGGL(k_pw_gather, dim3(dge_grid((int64_t)m * D)), dim3(256), 0, 0, f->d, d_rows.p + first[s], m, D, d_stack.p);
        double ms = 0.0;
        if ((rc = dge_knn_device(d_stack.p, nullptr, m, D, kmax, d_inv.p, d_xn.p, d_oi.p, d_od.p, &ms))) return rc;
        knn_ms += ms;
        hipLaunchKernelGGL(k_pw_map_back, dim3(dge_grid((int64_t)m * kmax)), dim3(256), 0, 0, d_oi.p, d_region.p + first[s], m, kmax, d_lists.p + (size_t)s * n * kmax);
        DGE_HIP(hipGetLastError());
    }

    // ---- the ground side
    pw_ground_dev gd;
    dge_stopwatch watch;
    float ground_ms = 0.f, score_ms = 0.f;
    if ((rc = watch.start(0))) return rc;
    if ((rc = gd.make(gnd, who))) return rc;
    if ((rc = pw_launch_ideal(gd.G, kmax, d_disc.p, d_ks.p, n_k, nullptr, nullptr, d_ideal.p, who))) return rc;
    int Tp = 2;
    while (Tp < n_sets * kmax) Tp <<= 1;
    if (rel_m) {
        const size_t lds = (size_t)Tp * 12 + ((size_t)Tp + 1 + PW_RANK_THREADS) * 4 + (size_t)gd.G.g * 4;
        (void)hipFuncSetAttribute((const void*)k_pw_rank, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k_pw_rank, dim3(n), dim3(PW_RANK_THREADS), lds, 0, gd.G, kmax, n_sets, Tp, d_lists.p, d_tested.p, rel_m, d_hit.p);
        DGE_HIP(hipGetLastError());
    }
    if ((rc = watch.stop(&ground_ms))) return rc;
    if ((rc = watch.start(0))) return rc;
    hipLaunchKernelGGL(k_pw_score, dim3(dge_grid((int64_t)cells)), dim3(256), 0, 0, gd.G, kmax, n_sets, d_lists.p, d_tested.p, rel_m ? d_hit.p : (const uint8_t*)nullptr, d_disc.p,
                       d_ks.p, n_k, d_ideal.p, d_ratio.p, d_hits.p);
    DGE_HIP(hipGetLastError());
    if ((rc = watch.stop(&score_ms))) return rc;

    // ---- the means: plain ascending sums over the tested regions, on the host
    std::vector<double> h_ratio(cells * n_k);
    std::vector<int32_t> h_hits(cells * n_k);
    DGE_HIP(hipMemcpy(h_ratio.data(), d_ratio.p, cells * n_k * sizeof(double), hipMemcpyDeviceToHost));
    DGE_HIP(hipMemcpy(h_hits.data(), d_hits.p, cells * n_k * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (lists) DGE_HIP(hipMemcpy(lists, d_lists.p, cells * kmax * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (ideal) DGE_HIP(hipMemcpy(ideal, d_ideal.p, (size_t)n_k * n * sizeof(double), hipMemcpyDeviceToHost));
    int64_t tested_total = 0;
    for (int s = 0; s < n_sets; s++) {
        members[s] = n_members[s]; tested[s] = n_tested[s]; tested_total += n_tested[s];
        for (int j = 0; j < n_k; j++) {
            const double* rr = h_ratio.data() + ((size_t)s * n_k + j) * n;
            const int32_t* hh = h_hits.data() + ((size_t)s * n_k + j) * n;
            double sum = 0.0;
            int64_t hsum = 0;
            for (int r = 0; r < n; r++)
                if (h_tested[(size_t)s * n + r]) { sum = sum + rr[r]; hsum += hh[r]; }
            ndcg[(size_t)s * n_k + j] = n_tested[s] ? sum / (double)n_tested[s] : 0.0;
            if (precision) precision[(size_t)s * n_k + j] = n_tested[s] ? (double)hsum / (double)((int64_t)ks[j] * n_tested[s]) : 0.0;
        }
    }
    if (ratio) memcpy(ratio, h_ratio.data(), cells * n_k * sizeof(double));
    if (hits) memcpy(hits, h_hits.data(), cells * n_k * sizeof(int32_t));
    if (info) {
        info->regions = n; info->members = (int64_t)total; info->tested = tested_total; info->threshold_keys = rel_m ? Tp : 0;
        info->knn_ms = knn_ms; info->ground_ms = ground_ms; info->score_ms = score_ms;
    }
    return DGE_OK;
}
