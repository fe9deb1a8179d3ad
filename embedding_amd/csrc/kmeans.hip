// kmeans.hip — k-means on resident rows (gfx950) as the fully specified rule of include/dge.h, and the reference's clustering accuracy on top of it
// (P/embeddingEvaluation_tract.py:539-571).  The per-element arithmetic lives in kmeans_rule.h; this file is what runs it at full concurrency without
// changing a bit: the sums that decide anything are int64 (order-free) or binary64 sums in the order the rule fixes.
//
// The assignment pass is the hot path: n * k * dim binary64 FMAs over rows read once.  A workgroup of four waves takes tiles of 64 rows.  A tile goes
// through LDS (coalesced global reads, then lane r of every wave owns row r, pitch dim | 1: no bank conflict); the centres sit in LDS transposed
// ([column][centre]), so that a wave reads the KG centres of its group at one column from one address — a broadcast.  The centres are dealt to the waves
// in groups of KG (KG accumulators a lane, chains in ascending column), each wave keeps its least (d, c), wave 0 merges the four.  Then the tile's rows
// are put in label order in LDS and every thread owns a column (and a slice of the rows when dim < 256): it quantises and adds up runs of equal label in
// registers and touches global memory once per run — 64-bit integer atomics, exact in any order.  No floating-point atomic anywhere.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <vector>

#include "dge_device.h"
#include "kmeans_rule.h"
#include "cluster_match.h"

#define KM_TILE 64

// seeding: d of every selected row to the centre chosen last, dmin = min(dmin, d), and the sum of every block of KM_BLOCK rows' dmin.  A workgroup is one
// block of the blocked sum; the rows go through LDS 32 columns at a time (32 lanes read 128 consecutive bytes of a row), a lane owns a row.
__global__ void __launch_bounds__(KM_BLOCK) k_km_dmin(const float* __restrict__ x, const int64_t* __restrict__ sel, int64_t n, int dim,
                                                      const float* __restrict__ centre, int first, double* __restrict__ dmin, double* __restrict__ block_sums) {
    __shared__ float tile[KM_BLOCK * 33];
    __shared__ float cen[KM_MAX_DIM];
    __shared__ double vals[KM_BLOCK];
    const int t = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * KM_BLOCK;
    for (int j = t; j < dim; j += KM_BLOCK) cen[j] = centre[j];
    double acc = 0.0;
    for (int j0 = 0; j0 < dim; j0 += 32) {
        const int w = dim - j0 < 32 ? dim - j0 : 32;
        __syncthreads();
        for (int e = t; e < KM_BLOCK * 32; e += KM_BLOCK) {
            const int r = e >> 5, c = e & 31;
            const int64_t i = i0 + r;
            float v = 0.0f;
            if (i < n && c < w) v = x[(size_t)(sel ? sel[i] : i) * (size_t)dim + (size_t)(j0 + c)];
            tile[r * 33 + c] = v;
        }
        __syncthreads();
        for (int c = 0; c < w; c++) acc = km_dist_step(acc, tile[t * 33 + c], cen[j0 + c]);
    }
    const int64_t i = i0 + t;
    double d = acc;
    if (i < n) {
        if (!first) { const double o = dmin[i]; if (o < d) d = o; }
        dmin[i] = d;
    }
    vals[t] = d;
    __syncthreads();
    if (t == 0) block_sums[blockIdx.x] = km_block_sum(vals, 0, n - i0 < KM_BLOCK ? n - i0 : (int64_t)KM_BLOCK);
}

// the sums of the blocks of any binary64 array (the inertia's)
__global__ void __launch_bounds__(KM_BLOCK) k_km_block_sums(const double* __restrict__ v, int64_t n, double* __restrict__ block_sums) {
    __shared__ double vals[KM_BLOCK];
    const int64_t i0 = (int64_t)blockIdx.x * KM_BLOCK, i = i0 + threadIdx.x;
    vals[threadIdx.x] = i < n ? v[i] : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) block_sums[blockIdx.x] = km_block_sum(vals, 0, n - i0 < KM_BLOCK ? n - i0 : (int64_t)KM_BLOCK);
}

// one workgroup: the next centre.  forced >= 0: that selected row.  Else thread 0 walks the blocked sum of dmin to u * total (km_walk); where no row
// exceeds the target, all threads look for the greatest dmin, least row among equals.  The row is copied into centre_out.
__global__ void __launch_bounds__(KM_BLOCK) k_km_pick(const float* __restrict__ x, const int64_t* __restrict__ sel, int64_t n, int dim, const double* __restrict__ dmin,
                                                      const double* __restrict__ block_sums, double u, int64_t forced, float* __restrict__ centre_out) {
    __shared__ int64_t pick;
    __shared__ double best_v[KM_BLOCK];
    __shared__ int64_t best_i[KM_BLOCK];
    const int t = threadIdx.x;
    if (t == 0) {
        if (forced >= 0) pick = forced;
        else {
            const double total = km_sum_blocks(block_sums, (n + KM_BLOCK - 1) / KM_BLOCK);
            pick = km_walk(dmin, block_sums, n, u * total);
        }
    }
    __syncthreads();
    if (pick < 0) {                                           // the same for every thread
        double bv = -1.0;
        int64_t bi = n;
        for (int64_t i = t; i < n; i += KM_BLOCK) { const double v = dmin[i]; if (v > bv) { bv = v; bi = i; } }
        best_v[t] = bv; best_i[t] = bi;
        __syncthreads();
        for (int o = KM_BLOCK / 2; o > 0; o >>= 1) {
            if (t < o && (best_v[t + o] > best_v[t] || (best_v[t + o] == best_v[t] && best_i[t + o] < best_i[t]))) { best_v[t] = best_v[t + o]; best_i[t] = best_i[t + o]; }
            __syncthreads();
        }
        if (t == 0) pick = best_i[0];
        __syncthreads();
    }
    const size_t row = sel ? (size_t)sel[pick] : (size_t)pick;
    for (int j = t; j < dim; j += KM_BLOCK) centre_out[j] = x[row * (size_t)dim + (size_t)j];
}

__global__ void k_km_update(const unsigned long long* __restrict__ S, const unsigned long long* __restrict__ count, int k, int dim, int s, float* __restrict__ centres) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= k * dim) return;
    const int64_t cnt = (int64_t)count[e / dim];
    if (cnt > 0) centres[e] = km_centre_from_sum((int64_t)S[e], cnt, s);          // a centre without a member keeps its position
}

// The assignment pass (see the head of the file).  KG: centres of one group; the launch picks the least of 1, 2, 4, 8, 16 with 4 * KG >= k, so that the
// four waves share the centres of a small k too.  Dynamic LDS: tile [64][P] floats, then the centres [dim][KP], KP = k rounded up to a multiple of KG.
template <int KG>
__global__ void __launch_bounds__(256) k_km_assign(const float* __restrict__ x, const int64_t* __restrict__ sel, int64_t n, int dim, int k, int s,
                                                   const float* __restrict__ centres, int32_t* __restrict__ labels, double* __restrict__ dist,
                                                   unsigned long long* __restrict__ S, unsigned long long* __restrict__ count, unsigned* __restrict__ changed) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double cand_d[4][KM_TILE];
    __shared__ int cand_c[4][KM_TILE];
    __shared__ int lab[KM_TILE], order[KM_TILE], hist[KM_MAX_K + 1], start[KM_MAX_K + 1];
    const int P = dim | 1, KP = (k + KG - 1) / KG * KG;
    float* tile = lds;
    float* cen = lds + KM_TILE * P;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;

    for (int e = t; e < dim * KP; e += 256) {
        const int j = e / KP, c = e - j * KP;
        cen[e] = c < k ? centres[c * dim + j] : 0.0f;
    }
    const int64_t n_tiles = (n + KM_TILE - 1) / KM_TILE;
    // the accumulation's split of the 256 threads: a column each, and `parts` slices of the tile's rows where dim leaves threads over
    const int parts = 256 / dim < 1 ? 1 : (256 / dim > KM_TILE ? KM_TILE : 256 / dim);
    const int per = (KM_TILE + parts - 1) / parts;

    for (int64_t ti = blockIdx.x; ti < n_tiles; ti += gridDim.x) {
        const int64_t i0 = ti * KM_TILE;
        const int nv = n - i0 < KM_TILE ? (int)(n - i0) : KM_TILE;
        __syncthreads();                                      // the tile before is done with (and, the first time, the centres are in)
        for (int e = t; e < KM_TILE * dim; e += 256) {
            const int r = e / dim, j = e - r * dim;
            float v = 0.0f;
            if (r < nv) v = x[(size_t)(sel ? sel[i0 + r] : i0 + r) * (size_t)dim + (size_t)j];
            tile[r * P + j] = v;
        }
        if (t <= k) hist[t] = 0;
        __syncthreads();

        // chains: this wave's groups of centres, ascending, for the row of this lane
        double best_d = INFINITY;
        int best_c = 0x7fffffff;
        const float* xr = tile + lane * P;
        for (int c0 = wave * KG; c0 < k; c0 += 4 * KG) {
            double acc[KG];
#pragma unroll
            for (int g = 0; g < KG; g++) acc[g] = 0.0;
            const float* cj = cen + c0;
#pragma unroll 4                                              // every chain keeps its order; the unrolled columns are independent work for the scheduler
            for (int j = 0; j < dim; j++, cj += KP) {
                const float xv = xr[j];
                if constexpr (KG >= 4) {
#pragma unroll
                    for (int q = 0; q < KG / 4; q++) {
                        const float4 c4 = *(const float4*)(cj + 4 * q);
                        acc[4 * q + 0] = km_dist_step(acc[4 * q + 0], xv, c4.x);
                        acc[4 * q + 1] = km_dist_step(acc[4 * q + 1], xv, c4.y);
                        acc[4 * q + 2] = km_dist_step(acc[4 * q + 2], xv, c4.z);
                        acc[4 * q + 3] = km_dist_step(acc[4 * q + 3], xv, c4.w);
                    }
                } else {
#pragma unroll
                    for (int g = 0; g < KG; g++) acc[g] = km_dist_step(acc[g], xv, cj[g]);
                }
            }
#pragma unroll
            for (int g = 0; g < KG; g++)
                if (c0 + g < k && acc[g] < best_d) { best_d = acc[g]; best_c = c0 + g; }      // ascending c, strict <: the least c among equals
        }
        cand_d[wave][lane] = best_d; cand_c[wave][lane] = best_c;
        __syncthreads();

        if (wave == 0) {
            double bd = cand_d[0][lane];
            int bc = cand_c[0][lane];
#pragma unroll
            for (int w = 1; w < 4; w++) {
                const double d = cand_d[w][lane];
                const int c = cand_c[w][lane];
                if (d < bd || (d == bd && c < bc)) { bd = d; bc = c; }
            }
            const bool valid = lane < nv;
            bool ch = false;
            if (valid) {
                ch = labels[i0 + lane] != bc;
                labels[i0 + lane] = bc;
                dist[i0 + lane] = bd;
            }
            const int l = valid ? bc : k;                     // rows past the end sort behind every label
            lab[lane] = l;
            atomicAdd(&hist[l], 1);
            const unsigned long long moved = __ballot(ch);
            if (lane == 0 && moved) atomicAdd(changed, (unsigned)__popcll(moved));
        }
        __syncthreads();
        if (t == 0) { int a = 0; for (int c = 0; c <= k; c++) { start[c] = a; a += hist[c]; } }
        __syncthreads();
        if (wave == 0) order[atomicAdd(&start[lab[lane]], 1)] = lane;      // the tile's rows in label order (any order inside a label: the sums are integers)
        if (t < k && hist[t] > 0) atomicAdd(&count[t], (unsigned long long)hist[t]);
        __syncthreads();

        // fixed-point sums: thread = (column j, slice of the ordered rows); one global atomic per run of equal labels
        const int part = t / dim, j = t - part * dim;
        if (part < parts) {
            const int lo = part * per, hi = lo + per < nv ? lo + per : nv;
            int cur = -1;
            int64_t acc = 0;
            for (int p = lo; p < hi; p++) {
                const int r = order[p], c = lab[r];
                const int64_t q = km_quantise(tile[r * P + j], s);
                if (c != cur) {
                    if (cur >= 0) atomicAdd(&S[(size_t)cur * dim + j], (unsigned long long)acc);
                    cur = c; acc = q;
                } else acc += q;
            }
            if (cur >= 0) atomicAdd(&S[(size_t)cur * dim + j], (unsigned long long)acc);
        }
    }
}

template <int KG>
static int launch_assign(const float* x, const int64_t* sel, int64_t n, int dim, int k, int s, const float* cen, int32_t* lab, double* d,
                         unsigned long long* S, unsigned long long* count, unsigned* changed) {
    const int KP = (k + KG - 1) / KG * KG;
    const size_t lds = ((size_t)KM_TILE * (size_t)(dim | 1) + (size_t)dim * (size_t)KP) * sizeof(float);
    DGE_HIP(hipFuncSetAttribute((const void*)k_km_assign<KG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int64_t n_tiles = (n + KM_TILE - 1) / KM_TILE;
    hipLaunchKernelGGL((k_km_assign<KG>), dim3((unsigned)(n_tiles < 2048 ? n_tiles : 2048)), dim3(256), lds, 0, x, sel, n, dim, k, s, cen, lab, d, S, count, changed);
    DGE_HIP(hipGetLastError());
    return DGE_OK;
}

static int assign_pass(const float* x, const int64_t* sel, int64_t n, int dim, int k, int s, const float* cen, int32_t* lab, double* d, unsigned long long* S,
                       unsigned long long* count, unsigned* changed) {
    if (k <= 4) return launch_assign<1>(x, sel, n, dim, k, s, cen, lab, d, S, count, changed);
    if (k <= 8) return launch_assign<2>(x, sel, n, dim, k, s, cen, lab, d, S, count, changed);
    if (k <= 16) return launch_assign<4>(x, sel, n, dim, k, s, cen, lab, d, S, count, changed);
    if (k <= 32) return launch_assign<8>(x, sel, n, dim, k, s, cen, lab, d, S, count, changed);
    return launch_assign<16>(x, sel, n, dim, k, s, cen, lab, d, S, count, changed);
}

static int kmeans_cfg_check(const char* who, const dge_kmeans_cfg* cfg) {
    if (int rc = dge_range_check(who, "k", cfg->k, KM_MAX_K)) return rc;
    if (cfg->n_init < 1) DGE_FAIL(DGE_ERR_ARG, "%s: n_init = %d must be at least 1", who, cfg->n_init);
    if (cfg->max_iter < 1) DGE_FAIL(DGE_ERR_ARG, "%s: max_iter = %d must be at least 1", who, cfg->max_iter);
    return DGE_OK;
}

// u: the used rows (present and, with a mask, selected)
static int kmeans_run(const char* who, const dge_vectors* v, const ur_rows& u, const dge_kmeans_cfg* cfg, const float* init, int32_t* labels, float* centres,
                      dge_kmeans_info* info) {
    int rc;
    const int dim = v->dim, k = cfg->k;
    const int64_t n = u.n;
    if (n < k) DGE_FAIL(DGE_ERR_ARG, "%s: k = %d exceeds the %lld selected rows", who, k, (long long)n);
    if (n > 0x7fffffffLL) DGE_FAIL(DGE_ERR_ARG, "%s: %lld selected rows exceed 2^31 - 1", who, (long long)n);
    const int64_t n_blocks = (n + KM_BLOCK - 1) / KM_BLOCK;
    const size_t kd = (size_t)k * (size_t)dim;

    dge_used_rows d_sel;
    dge_tmp<unsigned> d_changed;
    dge_tmp<unsigned long long> d_bad, d_S, d_count;
    dge_tmp<double> d_dmin, d_bs, d_dist[2];
    dge_tmp<int32_t> d_lab[2];
    dge_tmp<float> d_cen[2];
    if ((rc = d_sel.upload(u, nullptr))) return rc;
    const int64_t* dsel = d_sel.p;
    if ((rc = d_changed.alloc(1)) || (rc = d_bad.alloc(2)) || (rc = d_S.alloc(kd)) || (rc = d_count.alloc((size_t)k)) ||
        (rc = d_dmin.alloc((size_t)n)) || (rc = d_bs.alloc((size_t)n_blocks)) || (rc = d_dist[0].alloc((size_t)n)) || (rc = d_dist[1].alloc((size_t)n)) ||
        (rc = d_lab[0].alloc((size_t)n)) || (rc = d_lab[1].alloc((size_t)n)) || (rc = d_cen[0].alloc(kd)) || (rc = d_cen[1].alloc(kd))) return rc;

    dge_stopwatch watch;
    if ((rc = watch.start(0))) return rc;

    // max |x| and the finite check
    unsigned max_bits = 0;
    int64_t bad = -1;
    if ((rc = dge_scan_rows<true>(v->d, dsel, n, dim, d_bad.p, 0, &max_bits, &bad))) return rc;
    if (bad >= 0) DGE_FAIL(DGE_ERR_ARG, "%s: row %lld holds a value that is not finite", who, (long long)u.at(bad / dim));
    float max_abs;
    memcpy(&max_abs, &max_bits, sizeof max_abs);
    const int s = km_scale_bits(max_abs, n);

    const int n_init = init ? 1 : cfg->n_init;
    int best = -1, best_slot = 0, best_iter = 0, best_empty = 0;
    double best_inertia = 0.0;
    int64_t total_iter = 0;
    std::vector<double> bs((size_t)n_blocks);
    std::vector<unsigned long long> cnt((size_t)k);
    for (int r = 0; r < n_init; r++) {
        const int slot = best < 0 ? 0 : 1 - best_slot;        // never the buffers of the best restart so far
        float* cen = d_cen[slot].p;
        int32_t* lab = d_lab[slot].p;
        double* dist = d_dist[slot].p;
        if (init) DGE_HIP(hipMemcpy(cen, init, kd * sizeof(float), hipMemcpyHostToDevice));
        else {
            hipLaunchKernelGGL(k_km_pick, dim3(1), dim3(KM_BLOCK), 0, 0, v->d, dsel, n, dim, d_dmin.p, d_bs.p, 0.0, km_first_pick(cfg->seed, r, k, n), cen);
            for (int c = 1; c < k; c++) {
                hipLaunchKernelGGL(k_km_dmin, dim3((unsigned)n_blocks), dim3(KM_BLOCK), 0, 0, v->d, dsel, n, dim, cen + (size_t)(c - 1) * dim, c == 1 ? 1 : 0, d_dmin.p, d_bs.p);
                hipLaunchKernelGGL(k_km_pick, dim3(1), dim3(KM_BLOCK), 0, 0, v->d, dsel, n, dim, d_dmin.p, d_bs.p, km_draw(cfg->seed, r, k, c), (int64_t)-1, cen + (size_t)c * dim);
            }
            DGE_HIP(hipGetLastError());
        }
        DGE_HIP(hipMemsetAsync(lab, 0xff, (size_t)n * sizeof(int32_t), 0));      // -1: the first pass counts every row
        int iter = 0;
        for (;;) {
            DGE_HIP(hipMemsetAsync(d_S.p, 0, kd * sizeof(unsigned long long), 0));
            DGE_HIP(hipMemsetAsync(d_count.p, 0, (size_t)k * sizeof(unsigned long long), 0));
            DGE_HIP(hipMemsetAsync(d_changed.p, 0, sizeof(unsigned), 0));
            if ((rc = assign_pass(v->d, dsel, n, dim, k, s, cen, lab, dist, d_S.p, d_count.p, d_changed.p))) return rc;
            iter++;
            unsigned changed = 0;
            DGE_HIP(hipMemcpy(&changed, d_changed.p, sizeof changed, hipMemcpyDeviceToHost));
            if (changed == 0 || iter == cfg->max_iter) break;
            hipLaunchKernelGGL(k_km_update, dim3((unsigned)((kd + 255) / 256)), dim3(256), 0, 0, d_S.p, d_count.p, k, dim, s, cen);
            DGE_HIP(hipGetLastError());
        }
        total_iter += iter;
        hipLaunchKernelGGL(k_km_block_sums, dim3((unsigned)n_blocks), dim3(KM_BLOCK), 0, 0, dist, n, d_bs.p);
        DGE_HIP(hipGetLastError());
        DGE_HIP(hipMemcpy(bs.data(), d_bs.p, (size_t)n_blocks * sizeof(double), hipMemcpyDeviceToHost));
        DGE_HIP(hipMemcpy(cnt.data(), d_count.p, (size_t)k * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        const double inertia = km_sum_blocks(bs.data(), n_blocks);
        if (best < 0 || inertia < best_inertia) {             // least inertia, then the lower restart
            best = r; best_slot = slot; best_inertia = inertia; best_iter = iter; best_empty = 0;
            for (int c = 0; c < k; c++) if (cnt[(size_t)c] == 0) best_empty++;
        }
    }
    float ms = 0.f;
    if ((rc = watch.stop(&ms))) return rc;

    // outputs last: an error above leaves them as they were
    std::vector<int32_t> lab((size_t)n);
    std::vector<float> cen(kd);
    DGE_HIP(hipMemcpy(lab.data(), d_lab[best_slot].p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    DGE_HIP(hipMemcpy(cen.data(), d_cen[best_slot].p, kd * sizeof(float), hipMemcpyDeviceToHost));
    ur_scatter_back<int32_t>(labels, u, -1, lab.data());
    memcpy(centres, cen.data(), kd * sizeof(float));
    if (info) {
        info->rows = n; info->best_restart = best; info->iterations = best_iter; info->total_iterations = total_iter; info->scale_bits = s;
        info->empty = best_empty; info->inertia = best_inertia; info->kernel_ms = ms;
    }
    return DGE_OK;
}

// what both entries refuse before they look for a device
static int kmeans_limits(const char* who, const dge_kmeans_cfg* cfg, int32_t dim) {
    if (int rc = kmeans_cfg_check(who, cfg)) return rc;
    return dge_range_check(who, "dim", dim, KM_MAX_DIM);
}

extern "C" int dge_kmeans_vectors(const dge_vectors* v, const uint8_t* select, const dge_kmeans_cfg* cfg, const float* init_centres, int32_t* labels, float* centres,
                                  dge_kmeans_info* info) {
    const char* who = "dge_kmeans_vectors";
    if (!v || !cfg || !labels || !centres) DGE_FAIL(DGE_ERR_ARG, "%s: null argument", who);
    int rc = kmeans_limits(who, cfg, v->dim);
    if (rc) return rc;
    if (select == nullptr && v->n_present < cfg->k) DGE_FAIL(DGE_ERR_ARG, "%s: k = %d exceeds the %lld selected rows", who, cfg->k, (long long)v->n_present);
    if ((rc = dge_require_device(v->device))) return rc;
    dge_present pres;
    if ((rc = pres.load(v))) return rc;
    ur_rows u;
    ur_intake(ur_in{v->rows, pres.p, select}, &u);
    return kmeans_run(who, v, u, cfg, init_centres, labels, centres, info);
}

extern "C" int dge_kmeans(int device, const float* features, int64_t n_rows, int32_t dim, const uint8_t* select, const dge_kmeans_cfg* cfg, const float* init_centres,
                          int32_t* labels, float* centres, dge_kmeans_info* info) {
    const char* who = "dge_kmeans";
    if (!features || !cfg || !labels || !centres || n_rows < 0 || dim < 0) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    int rc = kmeans_limits(who, cfg, dim);
    if (rc) return rc;
    ur_rows u;
    ur_intake(ur_in{n_rows, nullptr, select}, &u);
    if (u.n < cfg->k) DGE_FAIL(DGE_ERR_ARG, "%s: k = %d exceeds the %lld selected rows", who, cfg->k, (long long)u.n);
    dge_vectors_guard g;
    if ((rc = dge_vectors_from_host(device, features, n_rows, dim, nullptr, &g.v))) return rc;
    return kmeans_run(who, g.v, u, cfg, init_centres, labels, centres, info);
}

extern "C" int dge_cluster_accuracy(const int32_t* labels, const int32_t* gnd, int64_t n_rows, int32_t k, int64_t* cnt, int32_t* map, double* accuracy) {
    if (!labels || !gnd || !accuracy || n_rows < 0) DGE_FAIL(DGE_ERR_ARG, "dge_cluster_accuracy: null or negative argument");
    if (int rc = dge_range_check("dge_cluster_accuracy", "k", k, KM_MAX_K)) return rc;
    std::vector<int64_t> table((size_t)k * (size_t)k);
    std::vector<int32_t> m((size_t)k, -1);
    int64_t n_gnd = 0;
    const int64_t bad = cm_contingency(labels, gnd, n_rows, k, table.data(), &n_gnd);
    if (bad >= 0) DGE_FAIL(DGE_ERR_ARG, "dge_cluster_accuracy: row %lld holds a label outside -1 .. %d", (long long)bad, k - 1);
    const int64_t hit = cm_greedy_map(table.data(), k, m.data());
    if (cnt) memcpy(cnt, table.data(), table.size() * sizeof(int64_t));
    if (map) memcpy(map, m.data(), m.size() * sizeof(int32_t));
    *accuracy = cm_accuracy(hit, n_gnd);
    return DGE_OK;
}
