// line.hip — LINE, the edge-sampled embedding of the reference's "LINE" baseline (P/flowFeatureGeneration_tract.py:54-73, regression-eval.sh:14-27), on gfx950 as
// the fully specified rule of include/dge.h.  The per-element arithmetic lives in line_rule.h; this file is what runs it at full concurrency without changing a bit.
//
// Both tables are int64 fixed point (2^-32 a unit) and every gradient term is quantised before it is added, so a mini-batch is a set of 64-bit integer atomic
// adds into delta tables: their sum does not depend on order, launch geometry or timing.  Per call: the entries are checked and sorted by (src, dst) (the intake
// shared with nmf.hip, coo_entries.h), the edge and negative tables are two rocPRIM prefix sums.  Per chunk of batches one draw kernel, a lane per draw, does the binary searches and
// leaves int32 [samples x (K + 2)]: u, v, the K negatives.  Per batch: k_line_grad — one DPP row of 16 lanes per sample, lane l holds columns l, l + 16, ... of
// u's row in registers across the K + 1 targets; partial l of the rule's dot is lane l's fma chain, the fold is four row rotations (dge_row16_ror), which leave the sum in every
// lane; u's K + 1 terms are summed as integers in registers and added once per cell — and k_line_apply over the batch's (K + 2) * count row ids, which claims a
// delta cell with an exchange-with-zero (a duplicate finds 0 and skips), adds it to the table and folds the batch number into one word by an integer minimum
// when a cell leaves the bound.  The host reads that word once, at the end.  No floating-point atomic anywhere.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <vector>

#include "coo_entries.h"
#include "line_rule.h"

#define LINE_NONE (~0ULL)
#define LINE_CHUNK (1LL << 20)          // samples drawn by one launch of the draw kernel (rounded to whole batches)

typedef unsigned long long line_u64;

// ------------------------------------------------------------------------------------------ the entries, once per call
// a weight for the shared intake (coo_entries.h): kind 1 is not a finite integer >= 0, kind 2 is >= 2^31
struct LineWeight {
    static __device__ int kind(double v) {
        return !isfinite(v) || v < 0.0 || v != rint(v) ? COO_KIND1 : v >= (double)LINE_MAX_WEIGHT ? COO_KIND2 : v == 0.0 ? COO_ZEROS : COO_KEEP;
    }
};

// edge e: its ends, its weight as an integer, and the mark of both ends
__global__ void __launch_bounds__(256) k_line_edges(const uint64_t* __restrict__ key, const int64_t* __restrict__ idx, const double* __restrict__ w, int64_t kept, int64_t n,
                                                    int32_t* __restrict__ es, int32_t* __restrict__ ed, int64_t* __restrict__ ew, uint8_t* __restrict__ touched) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= kept) return;
    const uint64_t k = key[p], i = k / (uint64_t)n, j = k - i * (uint64_t)n;
    es[p] = (int32_t)i; ed[p] = (int32_t)j; ew[p] = (int64_t)w[idx[p]];
    touched[i] = 1; touched[j] = 1;
}

// nw[v] from d[v], the weight of the edges whose source is v: they are the run of sorted keys in [v * n, (v + 1) * n), and C is the prefix sum over the edges
__global__ void __launch_bounds__(256) k_line_neg_weights(const uint64_t* __restrict__ key, const int64_t* __restrict__ C, int64_t kept, int64_t n, int64_t* __restrict__ nw) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const int64_t at[2] = {coo_lower_bound(key, kept, (uint64_t)v * (uint64_t)n), coo_lower_bound(key, kept, (uint64_t)(v + 1) * (uint64_t)n)};
    const int64_t d = (at[1] ? C[at[1] - 1] : 0) - (at[0] ? C[at[0] - 1] : 0);
    nw[v] = line_neg_weight(d);
}

__global__ void __launch_bounds__(256) k_line_init(int64_t* __restrict__ PX, int64_t cells, int dim, uint64_t seed2) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= cells) return;
    PX[t] = line_init_cell(seed2, (uint64_t)t, dim);
}

// ------------------------------------------------------------------------------------------ the draws of a chunk of batches
// a lane per draw: out[s][0] = u, out[s][1] = v of the edge of sample first + s, out[s][1 + d] = negative d
__global__ void __launch_bounds__(256) k_line_draw(const int64_t* __restrict__ C, int64_t kept, int64_t W, const int32_t* __restrict__ es, const int32_t* __restrict__ ed,
                                                   const int64_t* __restrict__ NC, int64_t n, int64_t N, uint64_t seed, int64_t first, int64_t count, int K,
                                                   int32_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= count * (K + 1)) return;
    const int64_t s = t / (K + 1);
    const int d = (int)(t - s * (K + 1));
    const uint64_t r = line_draw(seed, (uint64_t)(first + s), (uint64_t)d);
    int32_t* o = out + (size_t)s * (size_t)(K + 2);
    if (d == 0) {
        const int64_t e = line_search(C, kept, r, W);
        o[0] = es[e]; o[1] = ed[e];
    } else o[1 + d] = (int32_t)line_search(NC, n, r, N);
}

// ------------------------------------------------------------------------------------------ a batch
// the fold of the 16 partials, one per lane: p[l] + p[l + s] for s = 8, 4, 2, 1.  A rotation instead of a shift gives every lane, not only lane 0, the rule's
// sum: addition commutes, so after the step s the row holds the rule's values with period s, and lane l reads what the rule's lane l mod s reads.
__device__ __forceinline__ double line_fold(double p) {
    p = p + dge_row16_ror<8>(p);
    p = p + dge_row16_ror<4>(p);
    p = p + dge_row16_ror<2>(p);
    p = p + dge_row16_ror<1>(p);
    return p;
}

// the gradients of a batch into the delta tables.  RB: the columns a lane holds, the least of 1, 2, 4, 8, 16 that is at least ceil(dim / 16).
template <int RB>
__global__ void __launch_bounds__(256) k_line_grad(const int32_t* __restrict__ draws, int64_t count, int K, int dim, int order, const int64_t* __restrict__ PX,
                                                   const int64_t* __restrict__ PY, int64_t* __restrict__ DX, int64_t* __restrict__ DY, const double* __restrict__ T, double rho,
                                                   const line_u64* __restrict__ flag) {
    const int64_t s = ((int64_t)blockIdx.x * 256 + threadIdx.x) / NMF_LANES;       // a DPP row of 16 lanes is one sample: its lanes leave together
    const int l = threadIdx.x & (NMF_LANES - 1);
    if (s >= count) return;
    if (*flag != LINE_NONE) return;                                                 // a batch before this one left the bound: the call fails, nothing more is added
    const int32_t* dr = draws + (size_t)s * (size_t)(K + 2);
    const size_t u = (size_t)dr[0] * (size_t)dim;
    const int64_t* PB = order == 1 ? PX : PY;
    int64_t* DB = order == 1 ? DX : DY;
    double A[RB];
    int64_t acc[RB];
#pragma unroll
    for (int r = 0; r < RB; r++) {
        const int j = l + NMF_LANES * r;
        A[r] = j < dim ? line_value(PX[u + j]) : 0.0;
        acc[r] = 0;
    }
    for (int d = 0; d <= K; d++) {
        const size_t t = (size_t)dr[1 + d] * (size_t)dim;
        double B[RB];
        double p = 0.0;
#pragma unroll
        for (int r = 0; r < RB; r++) {
            const int j = l + NMF_LANES * r;
            B[r] = 0.0;
            if (j < dim) { B[r] = line_value(PB[t + j]); p = nmf_seg_step(p, A[r], B[r]); }
        }
        const double g = line_g(d == 0 ? 1.0 : 0.0, line_sig(T, line_fold(p)), rho);
#pragma unroll
        for (int r = 0; r < RB; r++) {
            const int j = l + NMF_LANES * r;
            if (j < dim) {
                atomicAdd((line_u64*)(DB + t + j), (line_u64)line_term(g, A[r]));
                acc[r] += line_term(g, B[r]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RB; r++) {
        const int j = l + NMF_LANES * r;
        if (j < dim && acc[r] != 0) atomicAdd((line_u64*)(DX + u + j), (line_u64)acc[r]);
    }
}

// P += delta over the rows the batch names, delta back to zero; a cell outside the bound folds the batch number into *flag
__global__ void __launch_bounds__(256) k_line_apply(const int32_t* __restrict__ draws, int64_t count, int K, int dim, int order, int64_t* __restrict__ PX, int64_t* __restrict__ PY,
                                                    int64_t* __restrict__ DX, int64_t* __restrict__ DY, line_u64 batch, line_u64* __restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= count * (K + 2) * dim) return;
    const int64_t i = t / dim;
    const int j = (int)(t - i * dim);
    const bool target = (i % (K + 2)) != 0 && order != 1;
    int64_t* P = target ? PY : PX;
    int64_t* D = target ? DY : DX;
    const size_t cell = (size_t)draws[i] * (size_t)dim + (size_t)j;
    const int64_t d = (int64_t)atomicExch((line_u64*)(D + cell), 0ULL);
    if (d == 0) return;
    const int64_t v = P[cell] + d;
    P[cell] = v;
    if (line_cell_over(v)) atomicMin(flag, batch);
}

// ------------------------------------------------------------------------------------------ host side
namespace {

void grad(int64_t count, const int32_t* draws, const dge_line_cfg* cfg, const int64_t* PX, const int64_t* PY, int64_t* DX, int64_t* DY, const double* T, double rho,
          const line_u64* flag) {
    const dim3 grid(dge_grid(count * NMF_LANES)), block(256);
    const int K = cfg->negative, dim = cfg->dim, order = cfg->order;
    if (dim <= 16) hipLaunchKernelGGL((k_line_grad<1>), grid, block, 0, 0, draws, count, K, dim, order, PX, PY, DX, DY, T, rho, flag);
    else if (dim <= 32) hipLaunchKernelGGL((k_line_grad<2>), grid, block, 0, 0, draws, count, K, dim, order, PX, PY, DX, DY, T, rho, flag);
    else if (dim <= 64) hipLaunchKernelGGL((k_line_grad<4>), grid, block, 0, 0, draws, count, K, dim, order, PX, PY, DX, DY, T, rho, flag);
    else if (dim <= 128) hipLaunchKernelGGL((k_line_grad<8>), grid, block, 0, 0, draws, count, K, dim, order, PX, PY, DX, DY, T, rho, flag);
    else hipLaunchKernelGGL((k_line_grad<16>), grid, block, 0, 0, draws, count, K, dim, order, PX, PY, DX, DY, T, rho, flag);
}

int cfg_check(const char* who, const dge_line_cfg* cfg, int64_t n) {
    if (cfg->dim < 1 || cfg->dim > LINE_MAX_DIM) DGE_FAIL(DGE_ERR_ARG, "%s: dim = %d is outside 1 .. %d", who, cfg->dim, LINE_MAX_DIM);
    if (cfg->order != 1 && cfg->order != 2) DGE_FAIL(DGE_ERR_ARG, "%s: order = %d is neither 1 nor 2", who, cfg->order);
    if (cfg->negative < 0 || cfg->negative > LINE_MAX_NEG) DGE_FAIL(DGE_ERR_ARG, "%s: negative = %d is outside 0 .. %d", who, cfg->negative, LINE_MAX_NEG);
    if (cfg->batch < 1 || cfg->batch > LINE_MAX_BATCH) DGE_FAIL(DGE_ERR_ARG, "%s: batch = %d is outside 1 .. %d", who, cfg->batch, LINE_MAX_BATCH);
    if (cfg->samples < 1 || cfg->samples > LINE_MAX_SAMPLES) DGE_FAIL(DGE_ERR_ARG, "%s: samples = %lld is outside 1 .. 2^40", who, (long long)cfg->samples);
    if (!(cfg->rho0 > 0.0 && cfg->rho0 <= 1.0)) DGE_FAIL(DGE_ERR_ARG, "%s: rho0 = %g is outside (0, 1]", who, cfg->rho0);
    if (n < 1 || n > LINE_MAX_N) DGE_FAIL(DGE_ERR_ARG, "%s: n = %lld is outside 1 .. 2^22", who, (long long)n);
    return DGE_OK;
}

// the rule on device entries (src, dst, w: device arrays of ne input entries).  init_X / init_Y: host arrays or NULL (init_Y only with init_X).
int line_run(const char* who, const int32_t* d_src, const int32_t* d_dst, const double* d_w, int64_t ne, int64_t n, const dge_line_cfg* cfg, const double* init_X, const double* init_Y,
             double* X, double* Y, uint8_t* touched, dge_line_info* info) {
    int rc;
    const int dim = cfg->dim, K = cfg->negative;
    const size_t cells = (size_t)n * (size_t)dim;
    dge_stopwatch watch;
    if ((rc = watch.start(0))) return rc;

    // ---- the entries: checks, the order by (src, dst) (the shared intake)
    coo_entries E;
    if ((rc = coo_intake<LineWeight, false>(d_src, d_dst, d_w, ne, n, n, INT64_MAX, E))) return rc;
    switch (E.fault) {
    case COO_RANGE: DGE_FAIL(DGE_ERR_ARG, "%s: entry %lld names a vertex outside 0 .. %lld", who, (long long)E.at, (long long)n - 1);
    case COO_KIND1: DGE_FAIL(DGE_ERR_ARG, "%s: entry %lld holds a weight that is not a finite integer >= 0", who, (long long)E.at);
    case COO_KIND2: DGE_FAIL(DGE_ERR_ARG, "%s: entry %lld holds a weight >= 2^31", who, (long long)E.at);
    case COO_ZEROS: DGE_FAIL(DGE_ERR_ARG, "%s: no entry is left: all %lld weights are zero", who, (long long)ne);
    case COO_DUP: DGE_FAIL(DGE_ERR_ARG, "%s: entry %lld repeats the source and destination of an earlier entry", who, (long long)E.at);
    }
    const int64_t zeros = E.zeros, kept = E.kept;
    line_u64* d_flag = E.d_c.p + COO_SPARE;                 // LINE_NONE so far: the least batch that left the bound

    // ---- the edge table and the negative table
    dge_tmp<int32_t> es, ed, draws;
    dge_tmp<int64_t> ew, C, nw, NC;
    dge_tmp<uint8_t> d_touched;
    if ((rc = es.alloc((size_t)kept)) || (rc = ed.alloc((size_t)kept)) || (rc = ew.alloc((size_t)kept)) || (rc = C.alloc((size_t)kept)) || (rc = nw.alloc((size_t)n)) ||
        (rc = NC.alloc((size_t)n)) || (rc = d_touched.alloc((size_t)n))) return rc;
    DGE_HIP(hipMemset(d_touched.p, 0, (size_t)n));
    hipLaunchKernelGGL(k_line_edges, dim3(dge_grid(kept)), dim3(256), 0, 0, E.skey.p, E.sidx.p, d_w, kept, n, es.p, ed.p, ew.p, d_touched.p);
    DGE_HIP(hipGetLastError());
    if ((rc = dge_inclusive_sum(dge_scratch(), (const int64_t*)ew.p, C.p, kept, 0, true))) return rc;
    int64_t W = 0, N = 0;
    DGE_HIP(hipMemcpy(&W, C.p + (kept - 1), sizeof W, hipMemcpyDeviceToHost));
    if (W >= LINE_MAX_TOTAL) DGE_FAIL(DGE_ERR_ARG, "%s: the total weight %lld is not below 2^40", who, (long long)W);
    hipLaunchKernelGGL(k_line_neg_weights, dim3(dge_grid(n)), dim3(256), 0, 0, E.skey.p, C.p, kept, n, nw.p);
    DGE_HIP(hipGetLastError());
    if ((rc = dge_inclusive_sum(dge_scratch(), (const int64_t*)nw.p, NC.p, n, 0, true))) return rc;
    DGE_HIP(hipMemcpy(&N, NC.p + (n - 1), sizeof N, hipMemcpyDeviceToHost));

    // ---- the tables, their deltas, the sigmoid table
    dge_tmp<int64_t> PX, PY, DX, DY;
    dge_tmp<double> T;
    if ((rc = PX.alloc(cells)) || (rc = PY.alloc(cells)) || (rc = DX.alloc(cells)) || (rc = DY.alloc(cfg->order == 2 ? cells : 1)) || (rc = T.alloc(LINE_SIG_N))) return rc;
    DGE_HIP(hipMemset(DX.p, 0, cells * sizeof(int64_t)));
    DGE_HIP(hipMemset(DY.p, 0, (cfg->order == 2 ? cells : 1) * sizeof(int64_t)));
    std::vector<int64_t> host(cells);
    if (init_X) {
        for (size_t t = 0; t < cells; t++) host[t] = line_quant(init_X[t]);
        DGE_HIP(hipMemcpy(PX.p, host.data(), cells * sizeof(int64_t), hipMemcpyHostToDevice));
    } else {
        hipLaunchKernelGGL(k_line_init, dim3(dge_grid((int64_t)cells)), dim3(256), 0, 0, PX.p, (int64_t)cells, dim, line_seed2(cfg->seed));
        DGE_HIP(hipGetLastError());
    }
    if (init_Y) {
        for (size_t t = 0; t < cells; t++) host[t] = line_quant(init_Y[t]);
        DGE_HIP(hipMemcpy(PY.p, host.data(), cells * sizeof(int64_t), hipMemcpyHostToDevice));
    } else DGE_HIP(hipMemset(PY.p, 0, cells * sizeof(int64_t)));
    {
        double sig[LINE_SIG_N];
        for (int k = 0; k < LINE_SIG_N; k++) sig[k] = line_sig_entry(k);
        DGE_HIP(hipMemcpy(T.p, sig, sizeof sig, hipMemcpyHostToDevice));
    }

    // ---- the batches: nothing below waits for the device until the last batch is queued
    const int64_t samples = cfg->samples, batch = cfg->batch;
    const int64_t batches = (samples + batch - 1) / batch;
    const int64_t chunk = (LINE_CHUNK / batch > 0 ? LINE_CHUNK / batch : 1) * batch;
    if ((rc = draws.alloc((size_t)(chunk < samples ? chunk : samples) * (size_t)(K + 2)))) return rc;
    for (int64_t first = 0; first < samples; first += chunk) {
        const int64_t count = samples - first < chunk ? samples - first : chunk;
        hipLaunchKernelGGL(k_line_draw, dim3(dge_grid(count * (K + 1))), dim3(256), 0, 0, C.p, kept, W, es.p, ed.p, NC.p, n, N, cfg->seed, first, count, K, draws.p);
        for (int64_t o = 0; o < count; o += batch) {
            const int64_t cnt = count - o < batch ? count - o : batch;
            const int32_t* dr = draws.p + (size_t)o * (size_t)(K + 2);
            grad(cnt, dr, cfg, PX.p, PY.p, DX.p, DY.p, T.p, line_rho(cfg->rho0, first + o, samples), d_flag);
            hipLaunchKernelGGL(k_line_apply, dim3(dge_grid(cnt * (K + 2) * dim)), dim3(256), 0, 0, dr, cnt, K, dim, cfg->order, PX.p, PY.p, DX.p, DY.p,
                               (line_u64)((first + o) / batch), d_flag);
        }
        DGE_HIP(hipGetLastError());
    }
    float ms = 0.f;
    if ((rc = watch.stop(&ms))) return rc;
    line_u64 over = LINE_NONE;
    DGE_HIP(hipMemcpy(&over, d_flag, sizeof over, hipMemcpyDeviceToHost));
    if (over != LINE_NONE)
        DGE_FAIL(DGE_ERR_ARG, "%s: after batch %lld a table holds a value outside (-256, 256): the rule's bound is left (a smaller rho0 or initial values keep it)", who, (long long)over);

    // outputs last: an error above leaves them as they were
    std::vector<int64_t> hostY(Y ? cells : 0);
    std::vector<uint8_t> hostT(touched ? (size_t)n : 0);
    DGE_HIP(hipMemcpy(host.data(), PX.p, cells * sizeof(int64_t), hipMemcpyDeviceToHost));
    int64_t big = 0;
    {
        std::vector<int64_t> all(Y ? 0 : cells);
        int64_t* y = Y ? hostY.data() : all.data();
        DGE_HIP(hipMemcpy(y, PY.p, cells * sizeof(int64_t), hipMemcpyDeviceToHost));
        for (size_t t = 0; t < cells; t++) {
            const int64_t a = host[t] < 0 ? -host[t] : host[t], b = y[t] < 0 ? -y[t] : y[t];
            if (a > big) big = a;
            if (b > big) big = b;
        }
    }
    if (touched) DGE_HIP(hipMemcpy(hostT.data(), d_touched.p, (size_t)n, hipMemcpyDeviceToHost));
    for (size_t t = 0; t < cells; t++) X[t] = line_value(host[t]);
    if (Y) for (size_t t = 0; t < cells; t++) Y[t] = line_value(hostY[t]);
    if (touched) memcpy(touched, hostT.data(), (size_t)n);
    if (info) {
        info->vertices = n; info->entries = kept; info->zeros = zeros; info->batches = batches; info->samples = samples; info->total_weight = W; info->neg_total = N;
        info->max_abs = line_value(big); info->kernel_ms = ms;
    }
    return DGE_OK;
}

int init_check(const char* who, const char* name, const double* v, size_t cells) {
    for (size_t t = 0; t < cells; t++)
        if (!(isfinite(v[t]) && fabs(v[t]) < LINE_INIT_LIMIT)) DGE_FAIL(DGE_ERR_ARG, "%s: %s[%lld] is not a finite value inside (-256, 256)", who, name, (long long)t);
    return DGE_OK;
}

}  // namespace

extern "C" int dge_line_coo(int device, const int32_t* src, const int32_t* dst, const double* w, int64_t n_entries, int64_t n, const dge_line_cfg* cfg, const double* init_X,
                            const double* init_Y, double* X, double* Y, uint8_t* touched, dge_line_info* info) {
    const char* who = "dge_line_coo";
    if (!src || !dst || !w || !cfg || !X) DGE_FAIL(DGE_ERR_ARG, "%s: null argument", who);
    if (init_Y && !init_X) DGE_FAIL(DGE_ERR_ARG, "%s: null argument: init_Y comes only together with init_X", who);
    int rc = cfg_check(who, cfg, n);
    if (rc) return rc;
    if (n_entries < 1 || n_entries > 0x7fffffffLL) DGE_FAIL(DGE_ERR_ARG, "%s: n_entries = %lld is outside 1 .. 2^31 - 1", who, (long long)n_entries);
    const size_t cells = (size_t)n * (size_t)cfg->dim;
    if (init_X && (rc = init_check(who, "init_X", init_X, cells))) return rc;
    if (init_Y && (rc = init_check(who, "init_Y", init_Y, cells))) return rc;
    if ((rc = dge_require_device(device))) return rc;
    dge_tmp<int32_t> d_src, d_dst;
    dge_tmp<double> d_w;
    if ((rc = coo_upload(src, dst, w, n_entries, d_src, d_dst, d_w))) return rc;
    return line_run(who, d_src.p, d_dst.p, d_w.p, n_entries, n, cfg, init_X, init_Y, X, Y, touched, info);
}

extern "C" int dge_line_flows(const dge_flows* f, int32_t T, int32_t mode, int32_t slot, const uint8_t* select, const dge_line_cfg* cfg, double* X, double* Y, uint8_t* touched,
                              int64_t* region_index, dge_line_info* info) {
    const char* who = "dge_line_flows";
    if (!f || !cfg || !X) DGE_FAIL(DGE_ERR_ARG, "%s: null argument", who);
    int rc = cfg_check(who, cfg, 1);
    if (rc) return rc;
    dge_tmp<int32_t> d_src, d_dst;
    dge_tmp<double> d_w;
    int64_t ne = 0;
    std::vector<int64_t> regions;
    if ((rc = dge_flows_slot_coo(f, T, mode, slot, select, who, d_src, d_dst, d_w, &ne, regions))) return rc;
    const int64_t n = (int64_t)regions.size();
    if ((rc = cfg_check(who, cfg, n))) return rc;
    if ((rc = line_run(who, d_src.p, d_dst.p, d_w.p, ne, n, cfg, nullptr, nullptr, X, Y, touched, info))) return rc;
    if (region_index) memcpy(region_index, regions.data(), (size_t)n * sizeof(int64_t));
    return DGE_OK;
}
