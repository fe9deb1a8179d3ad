// eval.hip — held-out evaluation on the device (include/dge.h: dge_model_score_pairs, dge_model_eval_links, dge_model_eval_sgns): pair scores,
// link-prediction AUC and the negative-sampling loss, read from syn0 / syn1neg where they lie.
//
// The model is only read.  Nothing here touches the trainer's per-call buffers (d_sen / d_len / d_wb carry a memo of the corpus rows they were
// derived from, sgns_model.h: a training launch skips its compaction when the memo matches) — walks are compacted into LDS — nor its counters, lock
// words, event list or plan.
//
// Layout: a row is `stride` floats (dim rounded up to 64, zero padded), 16-byte aligned.  A 16-lane group takes a row as DCH = stride / 64 float4
// per lane (lane l holds floats 4l .. 4l+3 of every 64-float chunk: each load instruction of a group is one 256-byte run), four groups a wave.
// ev_dot is the ONE dot product of this file: per lane four accumulators over its DCH float4 in chunk order, (a0 + a1) + (a2 + a3), then an xor
// butterfly over the 16 lanes (8, 4, 2, 1).  Its association order depends on DCH alone, and every step of the butterfly adds the same two numbers
// in both lanes, so all 16 lanes end with the same bits and the three entries give one pair the same score.  (-ffp-contract=off: the fused
// operations are the ones written.)
//
// Visibility of the trained rows: the trainer leaves them through write-through stores and memory-side atomics, and these kernels start behind it
// on the same stream — a dependent kernel boundary, after which plain loads read what the predecessor wrote (DESIGN.md, section "Held-out evaluation").
//
// Reduction: counts (pairs, negatives, skipped, wins, ties) are integers; the two loss sums are doubles.  Work is assigned statically (workgroup b
// takes steps / walks [b * per_block, (b + 1) * per_block), its group q every 16th of them), every workgroup adds its threads' sums up in a fixed
// tree and writes one partial; one final workgroup adds the partials (thread t: partials t, t + 256, ... in order, then the same tree).  No
// floating-point atomics: the same call returns the same bits.
#include <math.h>

#include "dge_device.h"
#include "sgns_kernels.h"      // neg_table_row; dge_algos.h (dge_mix64), dge_internal.h
#include "sgns_model.h"

enum { EV_PAIRS = 0, EV_NEGS, EV_SKIP, EV_WINS, EV_TIES, EV_NI };
struct EvalPartial { long long n[EV_NI]; double s[2]; };      // s[0] = sum softplus(-pos), s[1] = sum softplus(neg)

template <int DCH>
__device__ __forceinline__ void ev_load_row(const float* __restrict__ tab, int64_t row, int stride, int lane, float4 (&x)[DCH]) {
    const float4* p = reinterpret_cast<const float4*>(tab + row * (int64_t)stride) + lane;
#pragma unroll
    for (int k = 0; k < DCH; k++) x[k] = p[16 * k];
}

template <int DCH>
__device__ __forceinline__ float ev_dot(const float4 (&x)[DCH], const float4 (&y)[DCH]) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int k = 0; k < DCH; k++) {
        a0 = fmaf(x[k].x, y[k].x, a0); a1 = fmaf(x[k].y, y[k].y, a1);
        a2 = fmaf(x[k].z, y[k].z, a2); a3 = fmaf(x[k].w, y[k].w, a3);
    }
    float a = (a0 + a1) + (a2 + a3);
    a += __shfl_xor(a, 8, 16); a += __shfl_xor(a, 4, 16); a += __shfl_xor(a, 2, 16); a += __shfl_xor(a, 1, 16);
    return a;
}

__device__ __forceinline__ int32_t ev_row(const int32_t* __restrict__ remap, int32_t NV, int64_t v) {
    return (v >= 0 && v < (int64_t)NV) ? remap[v] : -1;
}

__device__ __forceinline__ double ev_softplus(double x) { return x > 0.0 ? x + log1p(exp(-x)) : log1p(exp(x)); }

// every thread's sums -> out (one record): a fixed tree over the workgroup's threads (blockDim.x is a power of two <= 256)
__device__ __forceinline__ void ev_block_reduce(const long long (&n)[EV_NI], double s0, double s1, EvalPartial* out) {
    __shared__ long long r_n[EV_NI][256];
    __shared__ double r_s[2][256];
    const int t = threadIdx.x;
#pragma unroll
    for (int q = 0; q < EV_NI; q++) r_n[q][t] = n[q];
    r_s[0][t] = s0; r_s[1][t] = s1;
    __syncthreads();
    for (int h = (int)blockDim.x >> 1; h > 0; h >>= 1) {
        if (t < h) {
#pragma unroll
            for (int q = 0; q < EV_NI; q++) r_n[q][t] += r_n[q][t + h];
            r_s[0][t] += r_s[0][t + h]; r_s[1][t] += r_s[1][t + h];
        }
        __syncthreads();
    }
    if (t == 0) {
#pragma unroll
        for (int q = 0; q < EV_NI; q++) out->n[q] = r_n[q][0];
        out->s[0] = r_s[0][0]; out->s[1] = r_s[1][0];
    }
}

__global__ void __launch_bounds__(256) k_eval_final(const EvalPartial* __restrict__ part, int n_part, EvalPartial* __restrict__ out) {
    long long n[EV_NI] = {0, 0, 0, 0, 0};
    double s0 = 0.0, s1 = 0.0;
    for (int i = threadIdx.x; i < n_part; i += (int)blockDim.x) {
#pragma unroll
        for (int q = 0; q < EV_NI; q++) n[q] += part[i].n[q];
        s0 += part[i].s[0]; s1 += part[i].s[1];
    }
    ev_block_reduce(n, s0, s1, out);
}

// ------------------------------------------------------------------------------------------ dge_model_score_pairs
template <int DCH>
__global__ void __launch_bounds__(256) k_eval_score(const float* __restrict__ syn0, const float* __restrict__ syn1neg, const int32_t* __restrict__ remap,
                                                    int32_t NV, int stride, const int32_t* __restrict__ ctx, const int32_t* __restrict__ tgt, int64_t n,
                                                    float* __restrict__ score) {
    const int lane = threadIdx.x & 15;
    const int64_t g0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4, ng = ((int64_t)gridDim.x * blockDim.x) >> 4;
    for (int64_t i = g0; i < n; i += ng) {
        const int32_t rc = ev_row(remap, NV, ctx[i]), rt = ev_row(remap, NV, tgt[i]);
        float s = __builtin_nanf("");
        if (rc >= 0 && rt >= 0) {
            float4 x[DCH], y[DCH];
            ev_load_row<DCH>(syn0, rc, stride, lane, x); ev_load_row<DCH>(syn1neg, rt, stride, lane, y);
            s = ev_dot<DCH>(x, y);
        }
        if (lane == 0) score[i] = s;
    }
}

// ------------------------------------------------------------------------------------------ dge_model_eval_links
// a 16-lane group per walk step; lane 0 takes the positive's loss term, lane 1 the negative's
template <int DCH>
__global__ void __launch_bounds__(256) k_eval_links(const float* __restrict__ syn0, const float* __restrict__ syn1neg, const int32_t* __restrict__ remap,
                                                    int32_t NV, int stride, const int32_t* __restrict__ walks, int64_t row0, int64_t n_steps, int32_t L,
                                                    int32_t R, uint64_t seed, int64_t per_block, EvalPartial* __restrict__ part) {
    const int lane = threadIdx.x & 15, grp = threadIdx.x >> 4;
    long long cnt[EV_NI] = {0, 0, 0, 0, 0};
    double s0 = 0.0, s1 = 0.0;
    const int64_t begin = (int64_t)blockIdx.x * per_block, end = begin + per_block < n_steps ? begin + per_block : n_steps;
    const int32_t L1 = L - 1;
    for (int64_t s = begin + grp; s < end; s += 16) {
        const int64_t i = s / L1, g = row0 + i;
        const int32_t j = (int32_t)(s - i * L1);
        const int32_t a = walks[g * L + j], b = walks[g * L + j + 1];
        if (a < 0 || b < 0) continue;
        const int64_t r = (int64_t)(b / R) * R + (int64_t)(dge_mix64(seed + (uint64_t)g * (uint64_t)L + (uint64_t)j) % (uint64_t)R);
        const int32_t ra = ev_row(remap, NV, a), rb = ev_row(remap, NV, b), rr = ev_row(remap, NV, r);
        if (ra < 0 || rb < 0 || rr < 0) { cnt[EV_SKIP]++; continue; }
        float4 y[DCH], x[DCH], z[DCH];
        ev_load_row<DCH>(syn1neg, ra, stride, lane, y);
        ev_load_row<DCH>(syn0, rb, stride, lane, x);
        ev_load_row<DCH>(syn0, rr, stride, lane, z);
        const float pos = ev_dot<DCH>(x, y), neg = ev_dot<DCH>(z, y);
        cnt[EV_PAIRS]++; cnt[EV_NEGS]++;
        cnt[EV_WINS] += pos > neg; cnt[EV_TIES] += pos == neg;
        if (lane < 2) {
            const double v = ev_softplus(lane == 0 ? -(double)pos : (double)neg);
            if (lane == 0) s0 += v; else s1 += v;
        }
    }
    if (lane != 0) {          // the counts are the same in the 16 lanes of a group: lane 0 reports them
#pragma unroll
        for (int q = 0; q < EV_NI; q++) cnt[q] = 0;
    }
    ev_block_reduce(cnt, s0, s1, part + blockIdx.x);
}

// ------------------------------------------------------------------------------------------ dge_model_eval_sgns
// A 16-lane group per walk: the walk's vocabulary rows are left-packed into the group's slice of LDS (as k_remap_compact packs them for the trainer), then
// for every centre its syn1neg row stays in registers across its up to 2 W contexts.  The K negatives of a pair: lane k draws slot and row k, the
// rows are broadcast one by one; lane k keeps score k for its loss term, and the positive's goes to the first lane without a negative.
template <int DCH>
__global__ void __launch_bounds__(256) k_eval_sgns(const float* __restrict__ syn0, const float* __restrict__ syn1neg, const int32_t* __restrict__ remap,
                                                   int32_t NV, int stride, const uint4* __restrict__ ctab, uint64_t T, const int32_t* __restrict__ walks,
                                                   int64_t row0, int64_t n_rows, int32_t L, int32_t W, int32_t K, uint64_t seed, int64_t per_block,
                                                   EvalPartial* __restrict__ part) {
    extern __shared__ int32_t s_tok[];        // [groups of the workgroup][L]
    const int lane = threadIdx.x & 15, grp = threadIdx.x >> 4, n_grp = (int)blockDim.x >> 4, sh = threadIdx.x & 48;
    int32_t* tok = s_tok + (size_t)grp * L;
    long long cnt[EV_NI] = {0, 0, 0, 0, 0};
    double s0 = 0.0, s1 = 0.0;
    const int64_t begin = (int64_t)blockIdx.x * per_block, end = begin + per_block < n_rows ? begin + per_block : n_rows;
    for (int64_t wi = begin + grp; wi < end; wi += n_grp) {
        const int64_t g = row0 + wi;
        const int32_t* in = walks + g * L;
        int n = 0;
        for (int j0 = 0; j0 < L; j0 += 16) {
            const int j = j0 + lane;
            const int32_t v = j < L ? ev_row(remap, NV, in[j]) : -1;
            const unsigned keep = (unsigned)(__ballot(v >= 0) >> sh) & 0xFFFFu;
            if (v >= 0) tok[n + __popc(keep & ((1u << lane) - 1u))] = v;
            n += __popc(keep);
        }
        __builtin_amdgcn_wave_barrier();
        for (int i = 0; i < n; i++) {
            const int32_t ri = tok[i];
            float4 y[DCH];
            ev_load_row<DCH>(syn1neg, ri, stride, lane, y);
            const int lo = i - W > 0 ? i - W : 0, hi = i + W < n - 1 ? i + W : n - 1;
            for (int c = lo; c <= hi; c++) {
                if (c == i) continue;
                float4 x[DCH];
                ev_load_row<DCH>(syn0, tok[c], stride, lane, x);
                const float pos = ev_dot<DCH>(x, y);
                cnt[EV_PAIRS]++;
                const uint64_t base = (((uint64_t)g * (uint64_t)L + (uint64_t)i) * (uint64_t)L + (uint64_t)c) * (uint64_t)K;
                bool pos_done = false;
                for (int k0 = 0; k0 < K; k0 += 16) {
                    const int nb = K - k0 < 16 ? K - k0 : 16;
                    int32_t row = 0;
                    if (lane < nb) row = neg_table_row(ctab, dge_mix64(seed + base + (uint64_t)(k0 + lane)) % T);
                    double xv = 0.0;
                    int kind = 0;                  // 1: a negative's term, 2: the positive's
                    int32_t rq = __shfl(row, 0, 16);
                    float4 z[DCH];
                    ev_load_row<DCH>(syn1neg, rq, stride, lane, z);
                    for (int q = 0; q < nb; q++) {
                        // the next row is on its way while this one is scored (the last round asks for its own row again: no branch around the loads)
                        const int32_t rn = __shfl(row, q + 1 < nb ? q + 1 : q, 16);
                        float4 zn[DCH];
                        ev_load_row<DCH>(syn1neg, rn, stride, lane, zn);
                        const float neg = ev_dot<DCH>(x, z);
                        const bool ok = rq != ri;
                        cnt[EV_NEGS] += ok; cnt[EV_SKIP] += !ok;
                        cnt[EV_WINS] += ok && pos > neg; cnt[EV_TIES] += ok && pos == neg;
                        if (lane == q && ok) { xv = (double)neg; kind = 1; }
                        rq = rn;
#pragma unroll
                        for (int k = 0; k < DCH; k++) z[k] = zn[k];
                    }
                    if (!pos_done && nb < 16) {
                        if (lane == nb) { xv = -(double)pos; kind = 2; }
                        pos_done = true;
                    }
                    if (kind) {
                        const double v = ev_softplus(xv);
                        if (kind == 1) s1 += v; else s0 += v;
                    }
                }
                if (!pos_done && lane == 0) s0 += ev_softplus(-(double)pos);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (lane != 0) {
#pragma unroll
        for (int q = 0; q < EV_NI; q++) cnt[q] = 0;
    }
    ev_block_reduce(cnt, s0, s1, part + blockIdx.x);
}

// ------------------------------------------------------------------------------------------ host side
#define EV_SWITCH_DCH(dch, CALL)                                                                       \
    switch (dch) {                                                                                     \
        case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break; \
        case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break; case 8: CALL(8); break; \
        default: DGE_FAIL(DGE_ERR_ARG, "evaluation: rows of %d floats are not supported", (dch) * 64);  \
    }

static int ev_check(const dge_model* m, const char* who) {
    if (!m) DGE_FAIL(DGE_ERR_ARG, "%s: null model", who);
    if (m->part_n > 1) DGE_FAIL(DGE_ERR_STATE, "%s: a partition is set (n_parts = %d): the tables are in pieces — call dge_model_set_partition(m, 1, 0, 0) first", who, m->part_n);
    return DGE_OK;
}

static int ev_check_walks(const dge_model* m, const dge_walks* w, int64_t row0, int64_t n_rows, const dge_eval_result* out, const char* who) {
    if (!w || !out) DGE_FAIL(DGE_ERR_ARG, "%s: null argument", who);
    if (row0 < 0 || n_rows < 0 || row0 > w->n || n_rows > w->n - row0) DGE_FAIL(DGE_ERR_ARG, "%s: rows [%lld, %lld + %lld) are outside the corpus of %lld walks", who, (long long)row0, (long long)row0, (long long)n_rows, (long long)w->n);
    if (w->device != m->device) DGE_FAIL(DGE_ERR_ARG, "%s: the corpus lies on device %d, the model on device %d", who, w->device, m->device);
    return DGE_OK;
}

static void ev_empty(dge_eval_result* out) {
    out->pairs = out->negatives = out->skipped = 0;
    out->auc = out->loss = nan(""); out->kernel_ms = 0.0;
}

// the partials of `blocks` workgroups -> one record on the host; *ms = event time from t's start to behind the final kernel
static int ev_finish(dge_model* m, dge_stopwatch& t, const EvalPartial* d_part, int blocks, EvalPartial* d_total, EvalPartial* total, double* ms) {
    hipLaunchKernelGGL(k_eval_final, dim3(1), dim3(256), 0, m->stream, d_part, blocks, d_total);
    DGE_HIP(hipGetLastError());
    float f = 0.f;
    if (int rc = t.stop(&f)) return rc;
    *ms = (double)f;
    DGE_HIP(hipMemcpy(total, d_total, sizeof(EvalPartial), hipMemcpyDeviceToHost));
    return DGE_OK;
}

// statically assigned work: `items` over at most 8 workgroups a compute unit, at least `min_per_block` items each
static void ev_geometry(const dge_model* m, int64_t items, int64_t min_per_block, int* blocks, int64_t* per_block) {
    const int64_t max_blocks = (int64_t)std::max(m->n_cus, 1) * 8;
    int64_t b = std::min(max_blocks, std::max<int64_t>(1, (items + min_per_block - 1) / min_per_block));
    *per_block = (items + b - 1) / b;
    *blocks = (int)((items + *per_block - 1) / *per_block);
}

extern "C" int dge_model_score_pairs(dge_model* m, const int32_t* d_ctx, const int32_t* d_tgt, int64_t n, float* d_score) {
    int rc = ev_check(m, "dge_model_score_pairs");
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!d_ctx || !d_tgt || !d_score))) DGE_FAIL(DGE_ERR_ARG, "dge_model_score_pairs: null or negative argument");
    if (n == 0) return DGE_OK;
    DGE_HIP(hipSetDevice(m->device));
    DGE_HIP(hipDeviceSynchronize());            // the caller's id buffers may still be in flight on a stream of theirs
    const int blocks = (int)std::min<int64_t>((int64_t)std::max(m->n_cus, 1) * 8, (n + 15) / 16);
#define EV_CALL(N) hipLaunchKernelGGL((k_eval_score<N>), dim3(blocks), dim3(256), 0, m->stream, m->d_syn0, m->d_syn1neg, m->d_remap, m->NV, m->stride, d_ctx, d_tgt, n, d_score)
    EV_SWITCH_DCH(m->stride / 64, EV_CALL)
#undef EV_CALL
    DGE_HIP(hipGetLastError());
    DGE_HIP(hipStreamSynchronize(m->stream));
    return DGE_OK;
}

extern "C" int dge_model_eval_links(dge_model* m, const dge_walks* w, int64_t row0, int64_t n_rows, int32_t regions_per_slice, uint64_t seed,
                                    dge_eval_result* out) {
    int rc = ev_check(m, "dge_model_eval_links");
    if (rc) return rc;
    if ((rc = ev_check_walks(m, w, row0, n_rows, out, "dge_model_eval_links"))) return rc;
    if (regions_per_slice <= 0) DGE_FAIL(DGE_ERR_ARG, "dge_model_eval_links: regions_per_slice must be positive");
    ev_empty(out);
    const int64_t n_steps = n_rows * (int64_t)std::max(w->L - 1, 0);
    if (n_steps == 0) return DGE_OK;
    DGE_HIP(hipSetDevice(m->device));
    if ((rc = dge_walks_order(w, m->stream))) return rc;      // behind another model's launch that still writes the corpus
    int blocks; int64_t per_block;
    ev_geometry(m, n_steps, 64, &blocks, &per_block);
    dge_tmp<EvalPartial> d_part;
    if ((rc = d_part.alloc((size_t)blocks + 1))) return rc;
    dge_stopwatch t;
    if ((rc = t.start(m->stream))) return rc;
#define EV_CALL(N) hipLaunchKernelGGL((k_eval_links<N>), dim3(blocks), dim3(256), 0, m->stream, m->d_syn0, m->d_syn1neg, m->d_remap, m->NV, m->stride, w->d, row0, n_steps, w->L, regions_per_slice, seed, per_block, d_part.p)
    EV_SWITCH_DCH(m->stride / 64, EV_CALL)
#undef EV_CALL
    DGE_HIP(hipGetLastError());
    EvalPartial tot;
    if ((rc = ev_finish(m, t, d_part.p, blocks, d_part.p + blocks, &tot, &out->kernel_ms))) return rc;
    out->pairs = tot.n[EV_PAIRS]; out->negatives = tot.n[EV_NEGS]; out->skipped = tot.n[EV_SKIP];
    if (out->negatives > 0) out->auc = ((double)tot.n[EV_WINS] + 0.5 * (double)tot.n[EV_TIES]) / (double)out->negatives;
    if (out->pairs > 0) out->loss = tot.s[0] / (double)out->pairs + tot.s[1] / (double)out->negatives;
    return DGE_OK;
}

extern "C" int dge_model_eval_sgns(dge_model* m, const dge_walks* w, int64_t row0, int64_t n_rows, uint64_t seed, dge_eval_result* out) {
    int rc = ev_check(m, "dge_model_eval_sgns");
    if (rc) return rc;
    if ((rc = ev_check_walks(m, w, row0, n_rows, out, "dge_model_eval_sgns"))) return rc;
    ev_empty(out);
    if (n_rows == 0 || w->L <= 0) return DGE_OK;
    // groups a workgroup: as many as keep the packed walks within 48 KB of LDS (next to the 14 KB of the reduction)
    int groups = 16;
    while (groups > 1 && (size_t)groups * (size_t)w->L * sizeof(int32_t) > 49152) groups >>= 1;
    const size_t lds = (size_t)groups * (size_t)w->L * sizeof(int32_t);
    if (lds > 49152) DGE_FAIL(DGE_ERR_ARG, "dge_model_eval_sgns: walks of %d tokens exceed the 12288 a workgroup can pack", w->L);
    DGE_HIP(hipSetDevice(m->device));
    if ((rc = dge_walks_order(w, m->stream))) return rc;      // behind another model's launch that still writes the corpus
    int blocks; int64_t per_block;
    ev_geometry(m, n_rows, groups, &blocks, &per_block);
    dge_tmp<EvalPartial> d_part;
    if ((rc = d_part.alloc((size_t)blocks + 1))) return rc;
    dge_stopwatch t;
    if ((rc = t.start(m->stream))) return rc;
#define EV_CALL(N) hipLaunchKernelGGL((k_eval_sgns<N>), dim3(blocks), dim3(16 * groups), lds, m->stream, m->d_syn0, m->d_syn1neg, m->d_remap, m->NV, m->stride, m->d_ctab, (uint64_t)m->T, w->d, row0, n_rows, w->L, m->cfg.window, m->cfg.negative, seed, per_block, d_part.p)
    EV_SWITCH_DCH(m->stride / 64, EV_CALL)
#undef EV_CALL
    DGE_HIP(hipGetLastError());
    EvalPartial tot;
    if ((rc = ev_finish(m, t, d_part.p, blocks, d_part.p + blocks, &tot, &out->kernel_ms))) return rc;
    out->pairs = tot.n[EV_PAIRS]; out->negatives = tot.n[EV_NEGS]; out->skipped = tot.n[EV_SKIP];
    if (out->negatives > 0) out->auc = ((double)tot.n[EV_WINS] + 0.5 * (double)tot.n[EV_TIES]) / (double)out->negatives;
    if (out->pairs > 0) out->loss = (tot.s[0] + tot.s[1]) / (double)out->pairs;
    return DGE_OK;
}
