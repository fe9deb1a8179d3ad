// svm.hip — RBF C-SVC on resident rows (gfx950) as the fully specified rule of include/dge.h, and its F-fold cross-validated accuracy for many label columns
// at once: the SVM line of the reference's classification table (P/binaryClassification_CA.py:38,55-57).  The per-element pieces live in svm_rule.h; this
// file is what runs them at full concurrency without changing a bit.
//
// Once per call the kernel matrix K of all used rows is computed (k_sv_kernel: 16 x 16 tiles, both row tiles staged in LDS, a lane per (i, j), the fma chain
// over the columns in order) and shared by every problem of the call.  A problem — one label column, one set of training rows — is solved by one workgroup
// (k_sv_solve); all problems of the call are one grid.  A lane owns the rows t = lane (mod workgroup).  An iteration is two block reductions, (m, i, M) and
// (score, j), each by wave shuffles and then through LDS, both under the total orders of svm_rule.h, and one pass over the rows that takes the gradient step
// and the next iteration's (m, i, M) together; the rows K(i, .) and K(j, .) are read along the row, coalesced.  alpha, G and the sign live in LDS where the
// used rows fit, else in a per-problem scratch in global memory: both forms run the same device function, and a problem's state is touched by its own
// workgroup only.  The host launches the solver in slices of launch_iters iterations; the state is saved between the launches, a problem that has stopped
// leaves at once, and the loop ends when none is left: no kernel here loops unbounded.
// The decision: the support rows of every problem are compacted by a prefix count (k_sv_compact) and one wave per (problem, tested row) takes the blocked
// sum (k_sv_decide).  Double-precision VALU only, no MFMA, no floating-point atomic; per-fold counts are integer atomics.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dge_device.h"
#include "svm_rule.h"

#define SV_TILE 16
#define SV_CHUNK 32               // columns of a row tile staged at once
#define SV_LDS_ROWS 3584          // used rows whose state (17 bytes a row) fits the 64 KiB of LDS a workgroup may take, beside the reductions' scratch
#define SV_MAX_WAVES 16
#define SV_LAUNCH_ITERS 1024      // the default slice
#define SV_LAUNCH_CAP 65536       // and the longest one

struct sv_ctl {                   // a problem between two launches
    int64_t iters;
    double bias;
    int32_t stopped, converged;
};

// ------------------------------------------------------------------------------------------ once per call
// HOT.  grid (ceil(n / 16), ceil(n / 16)), 256 lanes: lane (ti, tj) of the tile takes the chain of K(i, j).  Both halves of the matrix are computed: t only
// changes sign between them, so the bits are equal.  Rows past n read as 0 and write nothing.
__global__ void __launch_bounds__(256) k_sv_kernel(const float* __restrict__ x, const int64_t* __restrict__ used, int n, int dim, double gamma, double* __restrict__ K) {
    __shared__ float A[SV_TILE][SV_CHUNK + 1], B[SV_TILE][SV_CHUNK + 1];
    const int tid = threadIdx.x, tj = tid & (SV_TILE - 1), ti = tid / SV_TILE;
    const int i0 = blockIdx.y * SV_TILE, j0 = blockIdx.x * SV_TILE;
    double acc = 0.0;
    for (int c0 = 0; c0 < dim; c0 += SV_CHUNK) {
        for (int e = tid; e < SV_TILE * SV_CHUNK; e += 256) {
            const int r = e / SV_CHUNK, c = e - r * SV_CHUNK;
            const bool col = c0 + c < dim;
            const int ra = i0 + r, rb = j0 + r;
            float a = 0.0f, b = 0.0f;
            if (col && ra < n) a = x[(size_t)(used ? used[ra] : ra) * (size_t)dim + (size_t)(c0 + c)];
            if (col && rb < n) b = x[(size_t)(used ? used[rb] : rb) * (size_t)dim + (size_t)(c0 + c)];
            A[r][c] = a; B[r][c] = b;
        }
        __syncthreads();
        const int cn = dim - c0 < SV_CHUNK ? dim - c0 : SV_CHUNK;
        for (int c = 0; c < cn; c++) acc = km_dist_step(acc, A[ti][c], B[tj][c]);
        __syncthreads();
    }
    const int i = i0 + ti, j = j0 + tj;
    if (i < n && j < n) K[(size_t)i * (size_t)n + (size_t)j] = sv_kernel_of(acc, gamma);
}

// the state every problem starts from: problem p = label * F + f trains the used rows with fold != f
__global__ void k_sv_init(const uint8_t* __restrict__ y, const int32_t* __restrict__ fold, int n, int F, int P, double* __restrict__ alpha, double* __restrict__ G,
                          int8_t* __restrict__ sgn) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)P * (size_t)n) return;
    const int p = (int)(e / (size_t)n), t = (int)(e - (size_t)p * (size_t)n), l = p / F, f = p - l * F;
    alpha[e] = 0.0; G[e] = -1.0;
    sgn[e] = fold[t] == f ? 0 : (y[(size_t)l * (size_t)n + (size_t)t] ? 1 : -1);
}

// ------------------------------------------------------------------------------------------ the solver
// the block's (m, i, M): wave shuffles under sv_up_better, the waves' results through LDS, every lane merges them in wave order.  One barrier; the scratch
// of the other reduction lies between two uses of this one, so nobody still reads what the next use writes.
__device__ __forceinline__ sv_front sv_reduce_front(sv_front f, double* r_m, double* r_M, int32_t* r_i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sv_front_merge(f, __shfl_xor(f.m, o), __shfl_xor(f.M, o), __shfl_xor(f.i, o));
    const int wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) { r_m[wave] = f.m; r_M[wave] = f.M; r_i[wave] = f.i; }
    __syncthreads();
    sv_front g = sv_front_none();
    for (int w = 0; w < waves; w++) sv_front_merge(g, r_m[w], r_M[w], r_i[w]);
    return g;
}
__device__ __forceinline__ sv_pick sv_reduce_pick(sv_pick p, double* r_s, int32_t* r_j) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double sc = __shfl_xor(p.score, o);
        const int32_t j = __shfl_xor(p.j, o);
        if (sv_score_better(sc, j, p.score, p.j)) { p.score = sc; p.j = j; }
    }
    const int wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) { r_s[wave] = p.score; r_j[wave] = p.j; }
    __syncthreads();
    sv_pick g = sv_pick_none();
    for (int w = 0; w < waves; w++) if (sv_score_better(r_s[w], r_j[w], g.score, g.j)) { g.score = r_s[w]; g.j = r_j[w]; }
    return g;
}

// HOT.  One workgroup per problem; at most launch_iters iterations.  alpha, G, sgn: the problem's state, in LDS or in global memory.
__device__ __forceinline__ void sv_solve_slice(const double* __restrict__ K, int n, double C, double eps, int64_t max_iter, int launch_iters, double* alpha, double* G,
                                               const int8_t* sgn, sv_ctl* ctl, int* __restrict__ active) {
    __shared__ double r_m[SV_MAX_WAVES], r_M[SV_MAX_WAVES], r_s[SV_MAX_WAVES];
    __shared__ int32_t r_i[SV_MAX_WAVES], r_j[SV_MAX_WAVES];
    const int tid = threadIdx.x, bs = blockDim.x;
    sv_front mine = sv_front_none();
    for (int t = tid; t < n; t += bs) {
        const int s = sgn[t];
        if (s) sv_front_row(mine, t, s, alpha[t], G[t], C);
    }
    int64_t it = ctl->iters;
    bool stopped = false;
    int converged = 0;
    sv_front f;
    for (int step = 0;; step++) {
        f = sv_reduce_front(mine, r_m, r_M, r_i);
        if (sv_front_closed(f, eps)) { stopped = true; converged = 1; break; }
        if (it == max_iter) { stopped = true; break; }
        if (step == launch_iters) break;
        const int i = f.i;
        const double* Ki = K + (size_t)i * (size_t)n;
        sv_pick pk = sv_pick_none();
        for (int t = tid; t < n; t += bs) {
            const int s = sgn[t];
            if (s) sv_pick_row(pk, t, s, alpha[t], G[t], C, f.m, Ki[t]);
        }
        pk = sv_reduce_pick(pk, r_s, r_j);
        if (pk.j == SV_NONE) { stopped = true; break; }       // cannot happen while G is finite (the row of M is a candidate); never index K with it
        const int j = pk.j;
        const double* Kj = K + (size_t)j * (size_t)n;
        const int si = sgn[i], sj = sgn[j];
        const sv_move mv = sv_step(f.m, sv_v(sj, G[j]), Ki[j], si, sj, alpha[i], alpha[j], C);
        __syncthreads();                                       // every lane has read alpha[i], alpha[j], G[j] before their owners write them
        mine = sv_front_none();
        for (int t = tid; t < n; t += bs) {
            const int s = sgn[t];
            if (!s) continue;
            double a = alpha[t];
            if (t == i) { a = mv.ai; alpha[t] = a; }
            else if (t == j) { a = mv.aj; alpha[t] = a; }
            const double g = sv_grad(G[t], s, si, sj, Ki[t], Kj[t], mv.Di, mv.Dj);
            G[t] = g;
            sv_front_row(mine, t, s, a, g, C);
        }
        it++;
    }
    if (tid == 0) {
        ctl->iters = it;
        if (stopped) { ctl->stopped = 1; ctl->converged = converged; ctl->bias = sv_bias(f); }
        else atomicAdd(active, 1);
    }
}

template <bool LDS>
__global__ void __launch_bounds__(1024) k_sv_solve(const double* __restrict__ K, int n, double C, double eps, int64_t max_iter, int launch_iters, double* alpha_g, double* G_g,
                                                   const int8_t* sgn_g, sv_ctl* ctl, int* __restrict__ active) {
    extern __shared__ double sv_state[];
    const int p = blockIdx.x;
    if (ctl[p].stopped) return;                                // the whole workgroup
    double* alpha = alpha_g + (size_t)p * (size_t)n;
    double* G = G_g + (size_t)p * (size_t)n;
    const int8_t* sgn = sgn_g + (size_t)p * (size_t)n;
    if (LDS) {
        double* a_l = sv_state;
        double* g_l = sv_state + n;
        int8_t* s_l = (int8_t*)(sv_state + 2 * (size_t)n);
        for (int t = threadIdx.x; t < n; t += blockDim.x) { a_l[t] = alpha[t]; g_l[t] = G[t]; s_l[t] = sgn[t]; }
        __syncthreads();
        sv_solve_slice(K, n, C, eps, max_iter, launch_iters, a_l, g_l, s_l, ctl + p, active);
        __syncthreads();
        for (int t = threadIdx.x; t < n; t += blockDim.x) { alpha[t] = a_l[t]; G[t] = g_l[t]; }
    } else {
        sv_solve_slice(K, n, C, eps, max_iter, launch_iters, alpha, G, sgn, ctl + p, active);
    }
}

// ------------------------------------------------------------------------------------------ the decision
// One workgroup of 256 per problem: the rows with alpha > 0, ascending, by a prefix count (ballots inside a wave, the waves' totals through LDS).
// coef_all[p][t] = s * alpha (0 on a row that does not train).
__global__ void __launch_bounds__(256) k_sv_compact(const double* __restrict__ alpha, const int8_t* __restrict__ sgn, int n, int32_t* __restrict__ sup, double* __restrict__ sup_coef,
                                                    int32_t* __restrict__ n_sup, double* __restrict__ coef_all) {
    __shared__ int wsum[4];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t base = (size_t)p * (size_t)n;
    int done = 0;
    for (int t0 = 0; t0 < n; t0 += 256) {
        const int t = t0 + tid;
        double c = 0.0;
        if (t < n) {
            const int s = sgn[base + t];
            const double a = alpha[base + t];
            c = sv_coef(s, a);
            coef_all[base + t] = c;
        }
        const bool flag = c != 0.0;
        const unsigned long long ballot = __ballot(flag);
        const int rank = __popcll(ballot & ((1ULL << lane) - 1ULL));
        if (lane == 0) wsum[wave] = __popcll(ballot);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 4; w++) { if (w < wave) before += wsum[w]; total += wsum[w]; }
        if (flag) { sup[base + done + before + rank] = t; sup_coef[base + done + before + rank] = c; }
        done += total;
        __syncthreads();
    }
    if (tid == 0) n_sup[p] = done;
}

// HOT.  One wave per (model, row).  K != nullptr: the rows are the call's used rows, the model of row r for label l is problem l * F + fold[r], K(u, r) is read
// from the matrix, and a vote that equals the label counts for the problem.  K == nullptr: model l is problem l, K(u, r) is computed from the rows of sv and
// x, and an absent row of x gives NaN and is not read (the plain form: a lane runs a whole dim-long chain per support row and reads the row of x again each
// time; no time of it was taken).  256 terms at a time go through LDS and lane 0 adds them in order: that chain is the rule's.
__global__ void __launch_bounds__(64) k_sv_decide(const double* __restrict__ K, int n_sv, const float* __restrict__ svx, const float* __restrict__ x,
                                                  const uint8_t* __restrict__ x_present, int n_x, int dim, double gamma, const int32_t* __restrict__ fold, int F,
                                                  const uint8_t* __restrict__ y, const int32_t* __restrict__ sup, const double* __restrict__ sup_coef,
                                                  const int32_t* __restrict__ n_sup, const sv_ctl* __restrict__ ctl, const double* __restrict__ bias_in,
                                                  double* __restrict__ out, unsigned long long* __restrict__ correct) {
    __shared__ double term[SV_BLOCK];
    const int lane = threadIdx.x;
    const size_t w = blockIdx.x;
    const int l = (int)(w / (size_t)n_x), r = (int)(w - (size_t)l * (size_t)n_x);
    const int p = K ? l * F + fold[r] : l;
    if (!K && x_present && !x_present[r]) {
        if (lane == 0) out[w] = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }
    const size_t base = (size_t)p * (size_t)n_sv;
    const int ns = n_sup[p];
    double total = 0.0;
    for (int lo = 0; lo < ns; lo += SV_BLOCK) {
        const int cnt = ns - lo < SV_BLOCK ? ns - lo : SV_BLOCK;
        for (int k = lane; k < cnt; k += 64) {
            const int u = sup[base + lo + k];
            const double kv = K ? K[(size_t)r * (size_t)n_sv + (size_t)u] : sv_kernel(svx + (size_t)u * (size_t)dim, x + (size_t)r * (size_t)dim, dim, gamma);
            term[k] = sv_term(sup_coef[base + lo + k], kv);
        }
        __syncthreads();
        if (lane == 0) {
            double s = 0.0;
            for (int k = 0; k < cnt; k++) s += term[k];
            total += s;
        }
        __syncthreads();
    }
    if (lane == 0) {
        const double f = (ctl ? ctl[p].bias : bias_in[p]) + total;
        out[w] = f;
        if (correct && (f > 0.0 ? 1 : 0) == y[(size_t)l * (size_t)n_x + (size_t)r]) atomicAdd(&correct[p], 1ULL);
    }
}

// ------------------------------------------------------------------------------------------ host
static int svm_cfg_check(const char* who, const dge_svm_cfg* cfg, int32_t dim, dge_svm_cfg* c) {
    c->C = 1.0; c->gamma = dim > 0 ? 1.0 / (double)dim : 1.0; c->eps = 1e-3; c->max_iter = 10000000; c->state = 0; c->launch_iters = 0;
    if (!cfg) return DGE_OK;
    if (!(cfg->C > 0.0) || !(cfg->C < INFINITY)) DGE_FAIL(DGE_ERR_ARG, "%s: C = %g is not a finite number > 0", who, cfg->C);
    if (!(cfg->gamma > 0.0) || !(cfg->gamma < INFINITY)) DGE_FAIL(DGE_ERR_ARG, "%s: gamma = %g is not a finite number > 0", who, cfg->gamma);
    if (!(cfg->eps > 0.0)) DGE_FAIL(DGE_ERR_ARG, "%s: eps = %g is not > 0", who, cfg->eps);
    if (cfg->max_iter < 0) DGE_FAIL(DGE_ERR_ARG, "%s: max_iter = %lld must not be negative", who, (long long)cfg->max_iter);
    if (cfg->state < 0 || cfg->state > 2) DGE_FAIL(DGE_ERR_ARG, "%s: state = %d is outside 0 .. 2", who, cfg->state);
    if (cfg->launch_iters < 0) DGE_FAIL(DGE_ERR_ARG, "%s: launch_iters = %d must not be negative (0 = the library's default)", who, cfg->launch_iters);
    *c = *cfg;
    return DGE_OK;
}

// The walk of both fits and both cross-validations: pres the present bytes (nullptr: every row); the first offence in the entry's words, then what the count
// of used rows decides: problem (label, f) trains the used rows with fold != f.
static int svm_intake(const char* who, int64_t rows, const uint8_t* pres, const uint8_t* y, int32_t n_labels, const uint8_t* select, const int32_t* fold, int32_t n_folds,
                      const dge_svm_cfg& cfg, ur_rows* u) {
    ur_intake(ur_in{rows, pres, select, fold, n_folds, y, n_labels}, u);
    if (!fold) ur_no_folds(u);
    if (u->kind == UR_FOLD) DGE_FAIL(DGE_ERR_ARG, "%s: row %lld has fold %d, outside -1 .. %d", who, (long long)u->bad_row, u->bad_value, n_folds - 1);
    if (u->kind == UR_LABEL) DGE_FAIL(DGE_ERR_ARG, "%s: row %lld has label %d in column %d; labels are 0 or 1", who, (long long)u->bad_row, u->bad_value, u->bad_col);
    const int64_t n = u->n;
    if (n < 2) DGE_FAIL(DGE_ERR_ARG, "%s: %lld used rows; at least 2 are needed", who, (long long)n);
    if (n > SV_MAX_ROWS) DGE_FAIL(DGE_ERR_RANGE, "%s: %lld used rows; at most %d may (the kernel matrix is held whole)", who, (long long)n, SV_MAX_ROWS);
    for (size_t f = 0; f < u->tested.size(); f++)
        if (n - u->tested[f] == 0) DGE_FAIL(DGE_ERR_ARG, "%s: fold %d has no training rows", who, (int)f);
    if (cfg.state == 1 && n > SV_LDS_ROWS) DGE_FAIL(DGE_ERR_ARG, "%s: state = 1 holds at most %d used rows in LDS; the call has %lld", who, SV_LDS_ROWS, (long long)n);
    return DGE_OK;
}
// a *_vectors entry behind its limit checks: the device, the present bytes, the walk
static int svm_vectors_intake(const char* who, const dge_vectors* v, const uint8_t* y, int32_t n_labels, const uint8_t* select, const int32_t* fold, int32_t n_folds,
                              const dge_svm_cfg& cfg, ur_rows* u) {
    int rc = dge_require_device(v->device);
    dge_present pres;
    if (rc || (rc = pres.load(v))) return rc;
    return svm_intake(who, v->rows, pres.p, y, n_labels, select, fold, n_folds, cfg, u);
}

struct svm_out {              // per problem p = label * F + f; per (label, used row) where it says so
    std::vector<double> coef;             // [P x n]
    std::vector<double> bias;
    std::vector<int64_t> iters, support, correct;
    std::vector<int32_t> converged;
    std::vector<double> decision;         // [n_labels x n]
    int64_t launches = 0;
    float ms = 0.f;
};

// The used rows u (svm_intake has passed them), their labels yu [n_labels x n] and folds u.fold [n] (-1: trains every problem): the problems (label, f), f < F.
// decide: the held-out decision of every used row, and the votes that equal the label per problem.
static int svm_run(const char* who, const dge_vectors* v, const ur_rows& u, const std::vector<uint8_t>& yu, int n_labels, int F, const dge_svm_cfg& cfg, bool decide,
                   bool want_coef, svm_out* out) {
    const std::vector<int32_t>& fu = u.fold;
    const int dim = v->dim;
    const int n = (int)u.n;
    const int P = n_labels * F;
    int rc;
    const bool lds = cfg.state == 1 || (cfg.state == 0 && n <= SV_LDS_ROWS);
    const int slice = cfg.launch_iters == 0 ? SV_LAUNCH_ITERS : std::min<int>(cfg.launch_iters, SV_LAUNCH_CAP);

    // the values first: a table that is refused pays for the row numbers and one word, not for the kernel matrix
    dge_used_rows d_used;
    dge_tmp<unsigned long long> d_bad, d_correct;
    if ((rc = d_used.upload(u, who)) || (rc = dge_alloc_for(d_bad, 1, who))) return rc;
    const int64_t* dused = d_used.p;
    int64_t bad = -1;
    if ((rc = dge_scan_rows<false>(v->d, dused, n, dim, d_bad.p, 0, nullptr, &bad))) return rc;
    if (bad >= 0) DGE_FAIL(DGE_ERR_ARG, "%s: row %lld, column %lld holds a value that is not finite", who, (long long)u.at(bad / dim), (long long)(bad % dim));

    const size_t nn = (size_t)n * (size_t)n, Pn = (size_t)P * (size_t)n;
    size_t free_b = 0, total_b = 0;
    DGE_HIP(hipMemGetInfo(&free_b, &total_b));
    const size_t need = nn * 8 + Pn * (8 + 8 + 1 + 4 + 8 + 8) + (size_t)n_labels * (size_t)n * 9 + (size_t)n * 12 + (1u << 20);
    if (need > free_b) DGE_FAIL(DGE_ERR_CAP, "%s: %zu bytes of device memory are needed (%zu of them the kernel matrix of %d rows); %zu are free", who, need, nn * 8, n, free_b);

    dge_tmp<uint8_t> d_y;
    dge_tmp<int32_t> d_fold, d_sup, d_nsup;
    dge_tmp<int> d_active;
    dge_tmp<double> d_K, d_alpha, d_G, d_supc, d_coef, d_dec;
    dge_tmp<int8_t> d_sgn;
    dge_tmp<sv_ctl> d_ctl;
    if ((rc = dge_alloc_for(d_y, (size_t)n_labels * (size_t)n, who)) || (rc = dge_alloc_for(d_fold, (size_t)n, who)) || (rc = dge_alloc_for(d_K, nn, who)) ||
        (rc = dge_alloc_for(d_alpha, Pn, who)) || (rc = dge_alloc_for(d_G, Pn, who)) || (rc = dge_alloc_for(d_sgn, Pn, who)) || (rc = dge_alloc_for(d_ctl, (size_t)P, who)) ||
        (rc = dge_alloc_for(d_active, 1, who)) || (rc = dge_alloc_for(d_sup, Pn, who)) || (rc = dge_alloc_for(d_supc, Pn, who)) || (rc = dge_alloc_for(d_nsup, (size_t)P, who)) ||
        (rc = dge_alloc_for(d_coef, Pn, who)) || (rc = dge_alloc_for(d_correct, (size_t)P, who)) || (rc = dge_alloc_for(d_dec, decide ? (size_t)n_labels * (size_t)n : 1, who))) return rc;
    DGE_HIP(hipMemcpy(d_y.p, yu.data(), (size_t)n_labels * (size_t)n, hipMemcpyHostToDevice));
    DGE_HIP(hipMemcpy(d_fold.p, fu.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));

    dge_stopwatch watch;
    if ((rc = watch.start(0))) return rc;
    {
        const unsigned tiles = (unsigned)((n + SV_TILE - 1) / SV_TILE);
        hipLaunchKernelGGL(k_sv_kernel, dim3(tiles, tiles), dim3(256), 0, 0, v->d, dused, n, dim, cfg.gamma, d_K.p);
        hipLaunchKernelGGL(k_sv_init, dim3(dge_grid((int64_t)Pn)), dim3(256), 0, 0, d_y.p, d_fold.p, n, F, P, d_alpha.p, d_G.p, d_sgn.p);
        DGE_HIP(hipGetLastError());
    }
    DGE_HIP(hipMemsetAsync(d_ctl.p, 0, (size_t)P * sizeof(sv_ctl), 0));
    DGE_HIP(hipMemsetAsync(d_correct.p, 0, (size_t)P * sizeof(unsigned long long), 0));

    // the workgroup: four rows a lane where the largest training set allows it, 64 .. 1024 lanes
    int train_max = 0;
    for (int f = 0; f < F; f++) {
        int train = 0;
        for (int t = 0; t < n; t++) if (fu[(size_t)t] != f) train++;
        train_max = std::max(train_max, train);
    }
    int wg = 64;
    while (wg < 1024 && wg * 4 < train_max) wg <<= 1;
    const size_t lds_bytes = lds ? (((size_t)n * 17 + 7) & ~(size_t)7) : 0;
    for (;;) {
        DGE_HIP(hipMemsetAsync(d_active.p, 0, sizeof(int), 0));
        if (lds) hipLaunchKernelGGL(k_sv_solve<true>, dim3((unsigned)P), dim3((unsigned)wg), lds_bytes, 0, d_K.p, n, cfg.C, cfg.eps, cfg.max_iter, slice, d_alpha.p, d_G.p, d_sgn.p, d_ctl.p, d_active.p);
        else hipLaunchKernelGGL(k_sv_solve<false>, dim3((unsigned)P), dim3((unsigned)wg), 0, 0, d_K.p, n, cfg.C, cfg.eps, cfg.max_iter, slice, d_alpha.p, d_G.p, d_sgn.p, d_ctl.p, d_active.p);
        DGE_HIP(hipGetLastError());
        out->launches++;
        int active = 0;
        DGE_HIP(hipMemcpy(&active, d_active.p, sizeof active, hipMemcpyDeviceToHost));      // the slice's one read-back
        if (active == 0) break;
    }
    hipLaunchKernelGGL(k_sv_compact, dim3((unsigned)P), dim3(256), 0, 0, d_alpha.p, d_sgn.p, n, d_sup.p, d_supc.p, d_nsup.p, d_coef.p);
    DGE_HIP(hipGetLastError());
    if (decide) {
        hipLaunchKernelGGL(k_sv_decide, dim3((unsigned)((size_t)n_labels * (size_t)n)), dim3(64), 0, 0, d_K.p, n, (const float*)nullptr, (const float*)nullptr, (const uint8_t*)nullptr, n,
                           dim, cfg.gamma, d_fold.p, F, d_y.p, d_sup.p, d_supc.p, d_nsup.p, d_ctl.p, (const double*)nullptr, d_dec.p, d_correct.p);
        DGE_HIP(hipGetLastError());
    }
    if ((rc = watch.stop(&out->ms))) return rc;

    std::vector<sv_ctl> ctl((size_t)P);
    std::vector<int32_t> nsup((size_t)P);
    DGE_HIP(hipMemcpy(ctl.data(), d_ctl.p, (size_t)P * sizeof(sv_ctl), hipMemcpyDeviceToHost));
    DGE_HIP(hipMemcpy(nsup.data(), d_nsup.p, (size_t)P * sizeof(int32_t), hipMemcpyDeviceToHost));
    out->bias.resize((size_t)P); out->iters.resize((size_t)P); out->support.resize((size_t)P); out->converged.resize((size_t)P); out->correct.assign((size_t)P, 0);
    for (int p = 0; p < P; p++) {
        out->bias[(size_t)p] = ctl[(size_t)p].bias; out->iters[(size_t)p] = ctl[(size_t)p].iters; out->converged[(size_t)p] = ctl[(size_t)p].converged;
        out->support[(size_t)p] = nsup[(size_t)p];
    }
    if (want_coef) {
        out->coef.resize(Pn);
        DGE_HIP(hipMemcpy(out->coef.data(), d_coef.p, Pn * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (decide) {
        std::vector<unsigned long long> c((size_t)P);
        DGE_HIP(hipMemcpy(c.data(), d_correct.p, (size_t)P * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (int p = 0; p < P; p++) out->correct[(size_t)p] = (int64_t)c[(size_t)p];
        out->decision.resize((size_t)n_labels * (size_t)n);
        DGE_HIP(hipMemcpy(out->decision.data(), d_dec.p, out->decision.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    return DGE_OK;
}

static void svm_fill_info(dge_svm_info* info, int64_t rows, const svm_out& o) {
    if (!info) return;
    info->rows = rows; info->problems = (int64_t)o.iters.size(); info->iterations = 0; info->max_iterations = 0; info->not_converged = 0; info->support = 0;
    for (size_t p = 0; p < o.iters.size(); p++) {
        info->iterations += o.iters[p]; info->max_iterations = std::max(info->max_iterations, o.iters[p]); info->support += o.support[p];
        if (!o.converged[p]) info->not_converged++;
    }
    info->kernel_bytes = rows * rows * 8; info->launches = o.launches; info->kernel_ms = o.ms;
}

static int svm_fit_run(const char* who, const dge_vectors* v, const ur_rows& u, const uint8_t* y, int32_t n_labels, const dge_svm_cfg& cfg, double* coef, double* bias,
                       int64_t* iterations, int32_t* converged, dge_svm_info* info) {
    svm_out o;
    if (int rc = svm_run(who, v, u, ur_gather_labels(u, y, n_labels), n_labels, 1, cfg, false, true, &o)) return rc;
    for (int l = 0; l < n_labels; l++) {
        ur_scatter_back(coef + (size_t)l * (size_t)v->rows, u, __builtin_nan(""), o.coef.data() + (size_t)l * (size_t)u.n);
        bias[l] = o.bias[(size_t)l];
        if (iterations) iterations[l] = o.iters[(size_t)l];
        if (converged) converged[l] = o.converged[(size_t)l];
    }
    svm_fill_info(info, u.n, o);
    return DGE_OK;
}

static int svm_cv_run(const char* who, const dge_vectors* v, const ur_rows& u, const uint8_t* y, int32_t n_labels, int32_t n_folds, const dge_svm_cfg& cfg, int64_t* correct,
                      int64_t* tested, int64_t* iterations, int64_t* support, int32_t* converged, double* decision, dge_svm_info* info) {
    svm_out o;
    if (int rc = svm_run(who, v, u, ur_gather_labels(u, y, n_labels), n_labels, n_folds, cfg, true, false, &o)) return rc;
    for (int f = 0; f < n_folds; f++) tested[f] = u.tested[(size_t)f];
    for (int p = 0; p < n_labels * n_folds; p++) {
        correct[p] = o.correct[(size_t)p];
        if (iterations) iterations[p] = o.iters[(size_t)p];
        if (support) support[p] = o.support[(size_t)p];
        if (converged) converged[p] = o.converged[(size_t)p];
    }
    if (decision)
        for (int l = 0; l < n_labels; l++) ur_scatter_back(decision + (size_t)l * (size_t)v->rows, u, __builtin_nan(""), o.decision.data() + (size_t)l * (size_t)u.n);
    svm_fill_info(info, u.n, o);
    return DGE_OK;
}

static int svm_decision_run(const char* who, const dge_vectors* sv, const double* coef, const double* bias, int32_t n_models, double gamma, const dge_vectors* x, double* out) {
    int rc;
    if ((rc = dge_range_check(who, "dim", sv->dim, SV_MAX_DIM))) return rc;
    if (x->dim != sv->dim) DGE_FAIL(DGE_ERR_ARG, "%s: the rows of x have %d columns, the support rows %d", who, x->dim, sv->dim);
    if (x->device != sv->device) DGE_FAIL(DGE_ERR_ARG, "%s: x lives on device %d, the support rows on device %d", who, x->device, sv->device);
    if (sv->rows > 0x7fffffffLL / 2 || x->rows > 0x7fffffffLL / 2) DGE_FAIL(DGE_ERR_RANGE, "%s: more than 2^30 rows", who);
    if ((rc = dge_require_device(sv->device))) return rc;
    dge_present pres;
    if ((rc = pres.load(sv))) return rc;
    const int64_t R = sv->rows, X = x->rows;
    // the support lists on the host: the rows with a coefficient that is neither 0 nor NaN, ascending
    std::vector<int32_t> sup((size_t)n_models * (size_t)R), nsup((size_t)n_models, 0);
    std::vector<double> supc((size_t)n_models * (size_t)R);
    for (int l = 0; l < n_models; l++)
        for (int64_t i = 0; i < R; i++) {
            const double c = coef[(size_t)l * (size_t)R + (size_t)i];
            if (c == 0.0 || c != c) continue;
            if (pres.p && !pres.p[i]) DGE_FAIL(DGE_ERR_ARG, "%s: model %d has a coefficient on row %lld, which is absent", who, l, (long long)i);
            const size_t at = (size_t)l * (size_t)R + (size_t)nsup[(size_t)l]++;
            sup[at] = (int32_t)i; supc[at] = c;
        }
    if (X == 0) return DGE_OK;
    if ((uint64_t)n_models * (uint64_t)X > 0x7fffffffULL) DGE_FAIL(DGE_ERR_RANGE, "%s: %d models x %lld rows are more than 2^31 - 1 decisions of one call", who, n_models, (long long)X);
    dge_tmp<int32_t> d_sup, d_nsup;
    dge_tmp<double> d_supc, d_bias, d_out;
    const size_t lists = std::max<size_t>(sup.size(), 1), outs = (size_t)n_models * (size_t)X;
    if ((rc = dge_alloc_for(d_sup, lists, who)) || (rc = dge_alloc_for(d_supc, lists, who)) || (rc = dge_alloc_for(d_nsup, (size_t)n_models, who)) || (rc = dge_alloc_for(d_bias, (size_t)n_models, who)) ||
        (rc = dge_alloc_for(d_out, outs, who))) return rc;
    if (!sup.empty()) {
        DGE_HIP(hipMemcpy(d_sup.p, sup.data(), sup.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        DGE_HIP(hipMemcpy(d_supc.p, supc.data(), supc.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    DGE_HIP(hipMemcpy(d_nsup.p, nsup.data(), (size_t)n_models * sizeof(int32_t), hipMemcpyHostToDevice));
    DGE_HIP(hipMemcpy(d_bias.p, bias, (size_t)n_models * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_sv_decide, dim3((unsigned)outs), dim3(64), 0, 0, (const double*)nullptr, (int)R, sv->d, x->d, x->n_present == x->rows ? (const uint8_t*)nullptr : x->d_present, (int)X,
                       sv->dim, gamma, (const int32_t*)nullptr, 1, (const uint8_t*)nullptr, d_sup.p, d_supc.p, d_nsup.p, (const sv_ctl*)nullptr, d_bias.p, d_out.p,
                       (unsigned long long*)nullptr);
    DGE_HIP(hipGetLastError());
    DGE_HIP(hipMemcpy(out, d_out.p, outs * sizeof(double), hipMemcpyDeviceToHost));
    return DGE_OK;
}

extern "C" int dge_svm_fit_vectors(const dge_vectors* v, const uint8_t* y, int32_t n_labels, const uint8_t* select, const dge_svm_cfg* cfg, double* coef, double* bias,
                                   int64_t* iterations, int32_t* converged, dge_svm_info* info) {
    const char* who = "dge_svm_fit_vectors";
    if (!v || !y || !coef || !bias || n_labels < 0) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    dge_svm_cfg c;
    ur_rows u;
    int rc = dge_range_check(who, "n_labels", n_labels, SV_MAX_LABELS);
    if (rc || (rc = svm_cfg_check(who, cfg, v->dim, &c)) || (rc = dge_range_check(who, "dim", v->dim, SV_MAX_DIM)) || (rc = svm_vectors_intake(who, v, y, n_labels, select, nullptr, 0, c, &u))) return rc;
    return svm_fit_run(who, v, u, y, n_labels, c, coef, bias, iterations, converged, info);
}

extern "C" int dge_svm_fit(int device, const float* features, int64_t n_rows, int32_t dim, const uint8_t* y, int32_t n_labels, const uint8_t* select, const dge_svm_cfg* cfg,
                           double* coef, double* bias, int64_t* iterations, int32_t* converged, dge_svm_info* info) {
    const char* who = "dge_svm_fit";
    if (!features || !y || !coef || !bias || n_rows < 0 || dim < 0 || n_labels < 0) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    dge_svm_cfg c;
    ur_rows u;
    int rc = dge_range_check(who, "dim", dim, SV_MAX_DIM);
    if (rc || (rc = dge_range_check(who, "n_labels", n_labels, SV_MAX_LABELS)) || (rc = svm_cfg_check(who, cfg, dim, &c)) || (rc = svm_intake(who, n_rows, nullptr, y, n_labels, select, nullptr, 0, c, &u))) return rc;
    dge_vectors_guard g;
    if ((rc = dge_vectors_from_host(device, features, n_rows, dim, nullptr, &g.v))) return rc;
    return svm_fit_run(who, g.v, u, y, n_labels, c, coef, bias, iterations, converged, info);
}

extern "C" int dge_svm_cv_vectors(const dge_vectors* v, const uint8_t* y, int32_t n_labels, const int32_t* fold, int32_t n_folds, const dge_svm_cfg* cfg, int64_t* correct,
                                  int64_t* tested, int64_t* iterations, int64_t* support, int32_t* converged, double* decision, dge_svm_info* info) {
    const char* who = "dge_svm_cv_vectors";
    if (!v || !y || !fold || !correct || !tested || n_labels < 0 || n_folds < 0) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    dge_svm_cfg c;
    ur_rows u;
    int rc = dge_range_check(who, "n_labels", n_labels, SV_MAX_LABELS);
    if (rc || (rc = dge_range_check(who, "n_folds", n_folds, SV_MAX_FOLDS)) || (rc = svm_cfg_check(who, cfg, v->dim, &c)) || (rc = dge_range_check(who, "dim", v->dim, SV_MAX_DIM))) return rc;
    for (int64_t i = 0; i < v->rows; i++)                          // every row's fold before a device is looked for, the labels behind the present bytes
        if (fold[i] < -1 || fold[i] >= n_folds) DGE_FAIL(DGE_ERR_ARG, "%s: row %lld has fold %d, outside -1 .. %d", who, (long long)i, fold[i], n_folds - 1);
    if ((rc = svm_vectors_intake(who, v, y, n_labels, nullptr, fold, n_folds, c, &u))) return rc;
    return svm_cv_run(who, v, u, y, n_labels, n_folds, c, correct, tested, iterations, support, converged, decision, info);
}

extern "C" int dge_svm_cv(int device, const float* features, int64_t n_rows, int32_t dim, const uint8_t* y, int32_t n_labels, const int32_t* fold, int32_t n_folds,
                          const dge_svm_cfg* cfg, int64_t* correct, int64_t* tested, int64_t* iterations, int64_t* support, int32_t* converged, double* decision,
                          dge_svm_info* info) {
    const char* who = "dge_svm_cv";
    if (!features || !y || !fold || !correct || !tested || n_rows < 0 || dim < 0 || n_labels < 0 || n_folds < 0) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    dge_svm_cfg c;
    ur_rows u;
    int rc = dge_range_check(who, "dim", dim, SV_MAX_DIM);
    if (rc || (rc = dge_range_check(who, "n_labels", n_labels, SV_MAX_LABELS)) || (rc = dge_range_check(who, "n_folds", n_folds, SV_MAX_FOLDS)) || (rc = svm_cfg_check(who, cfg, dim, &c)) ||
        (rc = svm_intake(who, n_rows, nullptr, y, n_labels, nullptr, fold, n_folds, c, &u))) return rc;
    dge_vectors_guard g;
    if ((rc = dge_vectors_from_host(device, features, n_rows, dim, nullptr, &g.v))) return rc;
    return svm_cv_run(who, g.v, u, y, n_labels, n_folds, c, correct, tested, iterations, support, converged, decision, info);
}

static int svm_decision_args(const char* who, int32_t n_models, double gamma) {
    if (int rc = dge_range_check(who, "n_models", n_models, SV_MAX_LABELS * SV_MAX_FOLDS)) return rc;
    if (!(gamma > 0.0) || !(gamma < INFINITY)) DGE_FAIL(DGE_ERR_ARG, "%s: gamma = %g is not a finite number > 0", who, gamma);
    return DGE_OK;
}

extern "C" int dge_svm_decision_vectors(const dge_vectors* sv, const double* coef, const double* bias, int32_t n_models, double gamma, const dge_vectors* x, double* out) {
    const char* who = "dge_svm_decision_vectors";
    if (!sv || !coef || !bias || !x || !out || n_models < 0) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    if (int rc = svm_decision_args(who, n_models, gamma)) return rc;
    return svm_decision_run(who, sv, coef, bias, n_models, gamma, x, out);
}

extern "C" int dge_svm_decision(int device, const float* sv_features, int64_t n_sv, int32_t dim, const double* coef, const double* bias, int32_t n_models, double gamma,
                                const float* x_features, int64_t n_x, double* out) {
    const char* who = "dge_svm_decision";
    if (!sv_features || !coef || !bias || !out || n_sv < 0 || dim < 0 || n_models < 0 || n_x < 0) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    int rc = dge_range_check(who, "dim", dim, SV_MAX_DIM);
    if (rc || (rc = svm_decision_args(who, n_models, gamma))) return rc;
    dge_vectors_guard sv, x;
    if ((rc = dge_vectors_from_host(device, sv_features, n_sv, dim, nullptr, &sv.v))) return rc;
    if (x_features && (rc = dge_vectors_from_host(device, x_features, n_x, dim, nullptr, &x.v))) return rc;
    return svm_decision_run(who, sv.v, coef, bias, n_models, gamma, x.v ? x.v : sv.v, out);
}
