// ridge.hip — leave-one-out ridge regression on resident rows (gfx950) as the fully specified rule of include/dge.h: the reference's fourth figure of merit, the
// regression error of regression-eval.sh:43-49 (P/tf_linear_regression.py:61-83), with the closed-form fit and the leverage identity in place of n refits.  The
// per-element pieces live in ridge_rule.h; this file is what runs them at full concurrency without changing a bit: every element's chain keeps the order the
// rule fixes, whatever the schedule around it.  Plain binary64 VALU fma throughout — no MFMA (its accumulation order is not ours to fix), no floating-point
// atomic.
//   k_rg_moments   a workgroup takes one block of 256 used rows and one 64 x 64 square of the moments of [Z | Y]: the rows go through LDS 32 at a time, a thread
//                  holds a 4 x 4 register tile and runs each entry's 256-row chain; k_rg_fold adds a chunk's block partials, in block order, to the totals
//   k_rg_factor    one workgroup per lambda: LDL' left-looking, column by column, L kept column-major (the lanes that own rows i read it coalesced) and
//                  row-major (the back substitution's reads); then a wave per target runs the two substitutions
//   k_rg_leverage  a wave takes four rows at a time, lane l owns the elements j = l (mod 64): k ascending, u[k] broadcast from its owner, every lane updates its
//                  j > k — the column-oriented order of the same per-element chain; an element of L is read once per wave-batch of rows
//   k_rg_predict   a lane per row, the rows through LDS as in k-means' seeding: the prediction chain, and with targets the left-out error and the block
//                  sums of |e|
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <vector>

#include "dge_device.h"
#include "ridge_rule.h"

#define RG_TILE 64              // a workgroup's square of moment entries
#define RG_STEP 32              // rows of a block in LDS at a time
#define RG_ROWS 4               // rows of one wave-batch of the leverage kernel
#define RG_DEFAULT_CHUNK 64     // blocks of one chunk of block partials
#define RG_MAX_MODELS (RG_MAX_LAMBDA * RG_MAX_TARGETS)

extern std::atomic<int64_t> g_dge_tuning[DGE_TUNE_COUNT];      // sgns.hip: the knobs of dge_set_tuning, -1 = the library's own rule

// column c of [Z | Y] for one used row: 1, the features, the targets; 0 from column `lim` on
__device__ __forceinline__ double rg_col(const float* xr, const double* yr, int P, int lim, int c) {
    if (c >= lim) return 0.0;
    return c == 0 ? 1.0 : (c < P ? (double)xr[c - 1] : yr[c - P]);
}

// block blk0 + blockIdx.x of the used rows, square (ta, tb) = blockIdx.y of the moments M [P x (P + T)]; squares below the diagonal are left out (G is read
// from its upper triangle).  part: [blocks of the chunk][P x (P + T)]
__global__ void __launch_bounds__(256) k_rg_moments(const float* __restrict__ x, const int64_t* __restrict__ sel, const double* __restrict__ y, int64_t n, int dim, int T,
                                                    int64_t blk0, int tiles_b, double* __restrict__ part) {
    __shared__ double As[RG_STEP][RG_TILE], Bs[RG_STEP][RG_TILE];
    const int ta = blockIdx.y / tiles_b, tb = blockIdx.y - ta * tiles_b;
    if (tb < ta) return;
    const int P = dim + 1, W = P + T;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int64_t i0 = (blk0 + blockIdx.x) * RG_BLOCK;
    const int nv = n - i0 < RG_BLOCK ? (int)(n - i0) : RG_BLOCK;
    double acc[4][4];
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc[p][q] = 0.0;
    for (int r0 = 0; r0 < nv; r0 += RG_STEP) {
        const int rows_here = nv - r0 < RG_STEP ? nv - r0 : RG_STEP;
        __syncthreads();
        for (int e = t; e < RG_STEP * RG_TILE; e += 256) {
            const int r = e >> 6, c = e & 63;
            if (r < rows_here) {
                const int64_t i = i0 + r0 + r;
                const float* xr = x + (size_t)(sel ? sel[i] : i) * (size_t)dim;
                const double* yr = y + (size_t)i * (size_t)T;
                As[r][c] = rg_col(xr, yr, P, P, ta * RG_TILE + c);
                Bs[r][c] = rg_col(xr, yr, P, W, tb * RG_TILE + c);
            }
        }
        __syncthreads();
        for (int r = 0; r < rows_here; r++) {
            double a[4], b[4];
#pragma unroll
            for (int p = 0; p < 4; p++) { a[p] = As[r][ty + 16 * p]; b[p] = Bs[r][tx + 16 * p]; }
#pragma unroll
            for (int p = 0; p < 4; p++)
#pragma unroll
                for (int q = 0; q < 4; q++) acc[p][q] = rg_moment_step(acc[p][q], a[p], b[q]);
        }
    }
    double* out = part + (size_t)blockIdx.x * (size_t)P * (size_t)W;
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int a = ta * RG_TILE + ty + 16 * p, b = tb * RG_TILE + tx + 16 * q;
            if (a < P && b < W) out[(size_t)a * W + b] = acc[p][q];
        }
}

// M[q] += the chunk's block partials, in block order (M starts at +0.0)
__global__ void k_rg_fold(const double* __restrict__ part, int blocks, int P, int W, double* __restrict__ M) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= P * W) return;
    const int a = q / W, b = q - a * W;
    if (b / RG_TILE < a / RG_TILE) return;                    // a square no workgroup computed
    double s = M[q];
    for (int k = 0; k < blocks; k++) s += part[(size_t)k * (size_t)P * (size_t)W + q];
    M[q] = s;
}

// u := L^-1 u for R vectors of a wave at once; lane l holds the elements j = s * 64 + l in u[.][s].  Lc: column-major unit lower L, L[j][k] at k * P + j.
template <int NS, int R>
__device__ __forceinline__ void rg_forward(const double* Lc, int P, double (&u)[R][NS], int lane) {
#pragma unroll
    for (int ks = 0; ks < NS; ks++) {
        const int kend = P - 1 - ks * 64 < 64 ? P - 1 - ks * 64 : 64;      // k < P - 1: the last element has nothing behind it
        for (int kl = 0; kl < kend; kl++) {
            const int k = ks * 64 + kl;
            double uk[R];
#pragma unroll
            for (int r = 0; r < R; r++) uk[r] = __shfl(u[r][ks], kl);
#pragma unroll
            for (int s = ks; s < NS; s++) {
                const int j = s * 64 + lane;
                if (j > k && j < P) {
                    const double lv = Lc[(size_t)k * P + j];
#pragma unroll
                    for (int r = 0; r < R; r++) u[r][s] = rg_sub_step(u[r][s], lv, uk[r]);
                }
            }
        }
    }
}

// b := L^-T b; Lr: row-major L, L[k][j] at k * P + j.  k descending, b[k] broadcast, every lane updates its j < k
template <int NS>
__device__ __forceinline__ void rg_backward(const double* Lr, int P, double (&b)[NS], int lane) {
#pragma unroll
    for (int ks = NS - 1; ks >= 0; ks--) {
        const int ktop = P - 1 - ks * 64 < 63 ? P - 1 - ks * 64 : 63;
        for (int kl = ktop; kl >= 0; kl--) {
            const int k = ks * 64 + kl;
            if (k == 0) break;
            const double bk = __shfl(b[ks], kl);
#pragma unroll
            for (int s = 0; s <= ks; s++) {
                const int j = s * 64 + lane;
                if (j < k) b[s] = rg_sub_step(b[s], Lr[(size_t)k * P + j], bk);
            }
        }
    }
}

// one workgroup per lambda.  M: the moments; Lc, Lr [nl][P x P]; d, inv [nl][P]; beta [nl][T][P]; fail[l]: the first column whose pivot is not > 0 (-1: none)
template <int NS>
__global__ void __launch_bounds__(256) k_rg_factor(const double* __restrict__ M, int P, int T, const double* __restrict__ lambda, double* Lc, double* Lr,
                                                   double* __restrict__ d, double* __restrict__ inv, double* __restrict__ beta, int* __restrict__ fail) {
    __shared__ double tk[RG_MAX_DIM + 1], ds[RG_MAX_DIM + 1];
    __shared__ double dj;
    const int l = blockIdx.x, t = threadIdx.x, W = P + T;
    double* Lcl = Lc + (size_t)l * P * P;
    double* Lrl = Lr + (size_t)l * P * P;
    const double lam = lambda[l];
    for (int j = 0; j < P; j++) {
        for (int k = t; k < j; k += 256) tk[k] = rg_ldl_t(Lrl[(size_t)j * P + k], ds[k]);
        __syncthreads();
        double hold[2] = {0.0, 0.0};                          // P <= 257: a thread owns at most two rows of a column
#pragma unroll
        for (int it = 0; it < 2; it++) {
            const int i = j + t + 256 * it;
            if (i < P) {
                double acc = i == j ? rg_diag(M[(size_t)j * W + j], j, lam) : M[(size_t)j * W + i];
                for (int k = 0; k < j; k++) acc = rg_sub_step(acc, Lcl[(size_t)k * P + i], tk[k]);
                hold[it] = acc;
                if (i == j) dj = acc;
            }
        }
        __syncthreads();
        const double pivot = dj;
        if (!(pivot > 0.0)) {                                 // the same for every thread
            if (t == 0) fail[l] = j;
            return;
        }
#pragma unroll
        for (int it = 0; it < 2; it++) {
            const int i = j + t + 256 * it;
            if (i < P) {
                const double v = i == j ? 1.0 : hold[it] / pivot;
                Lcl[(size_t)j * P + i] = v;
                Lrl[(size_t)i * P + j] = v;
                if (i == j) { ds[j] = pivot; d[(size_t)l * P + j] = pivot; inv[(size_t)l * P + j] = 1.0 / pivot; }
            }
        }
        __syncthreads();
    }
    // coefficients: a wave per target
    const int lane = t & 63, wave = t >> 6;
    for (int tt = wave; tt < T; tt += 4) {
        double w[1][NS];
#pragma unroll
        for (int s = 0; s < NS; s++) { const int j = s * 64 + lane; w[0][s] = j < P ? M[(size_t)j * W + P + tt] : 0.0; }
        rg_forward<NS, 1>(Lcl, P, w, lane);
#pragma unroll
        for (int s = 0; s < NS; s++) { const int j = s * 64 + lane; if (j < P) w[0][s] = w[0][s] / ds[j]; }
        rg_backward<NS>(Lrl, P, w[0], lane);
#pragma unroll
        for (int s = 0; s < NS; s++) { const int j = s * 64 + lane; if (j < P) beta[((size_t)l * T + tt) * P + j] = w[0][s]; }
    }
}

// h[l][i] for lambda l = blockIdx.y; bad[l]: the least used row with 1 - h not > 0; max_bits: the greatest h of the call as its bits (h >= 0: the bits order)
template <int NS>
__global__ void __launch_bounds__(256) k_rg_leverage(const float* __restrict__ x, const int64_t* __restrict__ sel, int64_t n, int dim, const double* __restrict__ Lc,
                                                     const double* __restrict__ inv, double* __restrict__ h, unsigned long long* __restrict__ bad,
                                                     unsigned long long* __restrict__ max_bits) {
    __shared__ double inv_s[NS * 64];
    __shared__ double us[4][RG_ROWS][NS * 64];
    const int P = dim + 1, l = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const double* Lcl = Lc + (size_t)l * P * P;
    for (int j = t; j < NS * 64; j += 256) inv_s[j] = j < P ? inv[(size_t)l * P + j] : 0.0;
    const int64_t n_batches = (n + 4 * RG_ROWS - 1) / (4 * RG_ROWS);
    for (int64_t bt = blockIdx.x; bt < n_batches; bt += gridDim.x) {      // the same trips for every wave of the workgroup
        const int64_t base = bt * (4 * RG_ROWS) + wave * RG_ROWS;
        double u[RG_ROWS][NS];
#pragma unroll
        for (int r = 0; r < RG_ROWS; r++) {
            const int64_t i = base + r;
            const float* xr = i < n ? x + (size_t)(sel ? sel[i] : i) * (size_t)dim : nullptr;
#pragma unroll
            for (int s = 0; s < NS; s++) { const int j = s * 64 + lane; u[r][s] = (xr && j < P) ? rg_z(xr, j) : 0.0; }
        }
        rg_forward<NS, RG_ROWS>(Lcl, P, u, lane);
        __syncthreads();                                      // the batch before is read (and, the first time, inv_s is in)
#pragma unroll
        for (int r = 0; r < RG_ROWS; r++)
#pragma unroll
            for (int s = 0; s < NS; s++) us[wave][r][s * 64 + lane] = u[r][s];
        __syncthreads();
        if (lane < RG_ROWS && base + lane < n) {
            const double* ur = us[wave][lane];
            double acc = 0.0;
            for (int j = 0; j < P; j++) acc = rg_lev_step(acc, ur[j], inv_s[j]);
            const int64_t i = base + lane;
            h[(size_t)l * (size_t)n + (size_t)i] = acc;
            if (!(1.0 - acc > 0.0)) atomicMin(&bad[l], (unsigned long long)i);
            atomicMax(max_bits, (unsigned long long)__double_as_longlong(acc));
        }
    }
}

// model m = blockIdx.y (beta [models][P]) on block blockIdx.x of the rows, a lane per row.  Without y: out[m][i] = the prediction, NaN on an absent row (which
// is not read).  With y [n x T] and h [models / T][n]: e = (y - p) / (1 - h), out[m][i] = y - e where out is wanted, block_sums[m][block] = the block's sum of |e|
__global__ void __launch_bounds__(RG_BLOCK) k_rg_predict(const float* __restrict__ x, const int64_t* __restrict__ sel, const uint8_t* __restrict__ present, int64_t n, int dim,
                                                         const double* __restrict__ beta, const double* __restrict__ y, int T, const double* __restrict__ h,
                                                         double* __restrict__ out, double* __restrict__ block_sums) {
    __shared__ float tile[RG_BLOCK * 33];
    __shared__ double bs[RG_MAX_DIM + 1];
    __shared__ double vals[RG_BLOCK];
    const int t = threadIdx.x, P = dim + 1, m = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.x * RG_BLOCK;
    for (int j = t; j < P; j += RG_BLOCK) bs[j] = beta[(size_t)m * P + j];
    __syncthreads();
    double p = bs[0];
    for (int j0 = 0; j0 < dim; j0 += 32) {
        const int w = dim - j0 < 32 ? dim - j0 : 32;
        __syncthreads();
        for (int e = t; e < RG_BLOCK * 32; e += RG_BLOCK) {
            const int r = e >> 5, c = e & 31;
            const int64_t i = i0 + r;
            float v = 0.0f;
            if (i < n && c < w) {
                const size_t row = sel ? (size_t)sel[i] : (size_t)i;
                if (!present || present[row]) v = x[row * (size_t)dim + (size_t)(j0 + c)];
            }
            tile[r * 33 + c] = v;
        }
        __syncthreads();
        for (int c = 0; c < w; c++) p = rg_pred_step(p, (double)tile[t * 33 + c], bs[1 + j0 + c]);
    }
    const int64_t i = i0 + t;
    if (!y) {
        if (i < n) out[(size_t)m * (size_t)n + (size_t)i] = (present && !present[i]) ? (double)NAN : p;
        return;
    }
    double e = 0.0;
    if (i < n) {
        const int l = m / T, tt = m - l * T;
        const double yv = y[(size_t)i * (size_t)T + tt];
        e = (yv - p) / (1.0 - h[(size_t)l * (size_t)n + (size_t)i]);
        if (out) out[(size_t)m * (size_t)n + (size_t)i] = yv - e;
    }
    vals[t] = fabs(e);
    __syncthreads();
    if (t == 0) {
        const int nv = n - i0 < RG_BLOCK ? (int)(n - i0) : RG_BLOCK;
        double s = 0.0;
        for (int r = 0; r < nv; r++) s += vals[r];
        block_sums[(size_t)m * (size_t)gridDim.x + blockIdx.x] = s;
    }
}

template <int NS>
static void launch_factor(const double* M, int P, int T, int nl, const double* lambda, double* Lc, double* Lr, double* d, double* inv, double* beta, int* fail) {
    hipLaunchKernelGGL((k_rg_factor<NS>), dim3((unsigned)nl), dim3(256), 0, 0, M, P, T, lambda, Lc, Lr, d, inv, beta, fail);
}
template <int NS>
static void launch_leverage(const float* x, const int64_t* sel, int64_t n, int dim, int nl, const double* Lc, const double* inv, double* h, unsigned long long* bad,
                            unsigned long long* max_bits) {
    const int64_t n_batches = (n + 4 * RG_ROWS - 1) / (4 * RG_ROWS);
    hipLaunchKernelGGL((k_rg_leverage<NS>), dim3((unsigned)(n_batches < 4096 ? n_batches : 4096), (unsigned)nl), dim3(256), 0, 0, x, sel, n, dim, Lc, inv, h, bad, max_bits);
}
#define RG_BY_SLICES(P, call, ...)                             \
    switch (((P) + 63) / 64) {                                 \
        case 1: call<1>(__VA_ARGS__); break;                   \
        case 2: call<2>(__VA_ARGS__); break;                   \
        case 3: call<3>(__VA_ARGS__); break;                   \
        case 4: call<4>(__VA_ARGS__); break;                   \
        default: call<5>(__VA_ARGS__); break;                  \
    }

static int ridge_limits(const char* who, int dim, int n_targets, const double* lambda, int n_lambda) {
    int rc = dge_range_check(who, "dim", dim, RG_MAX_DIM);
    if (rc || (rc = dge_range_check(who, "n_targets", n_targets, RG_MAX_TARGETS)) || (rc = dge_range_check(who, "n_lambda", n_lambda, RG_MAX_LAMBDA))) return rc;
    for (int l = 0; l < n_lambda; l++)
        if (!(lambda[l] >= 0.0) || !(lambda[l] <= 1.7976931348623157e308)) DGE_FAIL(DGE_ERR_ARG, "%s: lambda[%d] = %g is not a finite number >= 0", who, l, lambda[l]);
    return DGE_OK;
}

// u: the used rows (present and, with a mask, selected) with the first of them that holds a target that is not finite
static int ridge_run(const char* who, const dge_vectors* v, const ur_rows& u, const double* y, int T, const double* lambda, int nl, double* mae, double* mre, double* beta,
                     double* loo_pred, dge_ridge_info* info) {
    int rc;
    const int dim = v->dim, P = dim + 1, W = P + T, models = nl * T;
    const int64_t rows = v->rows, n = u.n;
    if (n < 2) DGE_FAIL(DGE_ERR_ARG, "%s: %lld used rows; leave-one-out needs at least 2", who, (long long)n);
    if (n > 0x7fffffffLL) DGE_FAIL(DGE_ERR_ARG, "%s: %lld used rows exceed 2^31 - 1", who, (long long)n);
    const int64_t n_blocks = (n + RG_BLOCK - 1) / RG_BLOCK;
    const int64_t knob = g_dge_tuning[DGE_TUNE_RIDGE_CHUNK];
    const int64_t chunk = std::min<int64_t>(knob > 0 ? knob : RG_DEFAULT_CHUNK, n_blocks);
    const int64_t n_chunks = (n_blocks + chunk - 1) / chunk;
    const std::vector<double> yu = ur_gather_targets(u, y, T);

    const size_t PW = (size_t)P * W, PP = (size_t)P * P;
    dge_used_rows d_sel;
    dge_tmp<unsigned long long> d_bad;                        // [0]: the scan's, [1 .. nl]: the leverage's, [nl + 1]: the greatest h
    dge_tmp<int> d_fail;
    dge_tmp<double> d_y, d_lambda, d_part, d_M, d_Lc, d_Lr, d_d, d_inv, d_beta, d_h, d_out, d_bs;
    if ((rc = d_sel.upload(u, nullptr))) return rc;
    const int64_t* dsel = d_sel.p;
    if ((rc = d_bad.alloc((size_t)nl + 2)) || (rc = d_fail.alloc((size_t)nl)) || (rc = d_y.alloc(yu.size())) || (rc = d_lambda.alloc((size_t)nl)) ||
        (rc = d_part.alloc((size_t)chunk * PW)) || (rc = d_M.alloc(PW)) || (rc = d_Lc.alloc((size_t)nl * PP)) || (rc = d_Lr.alloc((size_t)nl * PP)) ||
        (rc = d_d.alloc((size_t)nl * P)) || (rc = d_inv.alloc((size_t)nl * P)) || (rc = d_beta.alloc((size_t)models * P)) || (rc = d_h.alloc((size_t)nl * (size_t)n)) ||
        (rc = d_bs.alloc((size_t)models * (size_t)n_blocks)) || (loo_pred && (rc = d_out.alloc((size_t)models * (size_t)n)))) return rc;
    DGE_HIP(hipMemcpy(d_y.p, yu.data(), yu.size() * sizeof(double), hipMemcpyHostToDevice));
    DGE_HIP(hipMemcpy(d_lambda.p, lambda, (size_t)nl * sizeof(double), hipMemcpyHostToDevice));

    dge_stopwatch watch;
    if ((rc = watch.start(0))) return rc;
    DGE_HIP(hipMemsetAsync(d_bad.p + nl + 1, 0, sizeof(unsigned long long), 0));
    DGE_HIP(hipMemsetAsync(d_fail.p, 0xff, (size_t)nl * sizeof(int), 0));
    int64_t bad_x = -1;
    if ((rc = dge_scan_rows<false>(v->d, dsel, n, dim, d_bad.p, nl, nullptr, &bad_x))) return rc;      // the leverage's nl words are armed with the scan's
    if (bad_x >= 0 || u.kind == UR_TARGET) {
        const int64_t ix = bad_x < 0 ? -1 : u.at(bad_x / dim);
        DGE_FAIL(DGE_ERR_ARG, "%s: row %lld holds a feature or a target that is not finite", who, (long long)(ix < 0 || (u.kind == UR_TARGET && u.bad_row < ix) ? u.bad_row : ix));
    }

    // moments: chunk by chunk, the block partials folded in block order
    DGE_HIP(hipMemsetAsync(d_M.p, 0, PW * sizeof(double), 0));
    const int tiles_a = (P + RG_TILE - 1) / RG_TILE, tiles_b = (W + RG_TILE - 1) / RG_TILE;
    for (int64_t b0 = 0; b0 < n_blocks; b0 += chunk) {
        const int64_t nb = std::min<int64_t>(chunk, n_blocks - b0);
        hipLaunchKernelGGL(k_rg_moments, dim3((unsigned)nb, (unsigned)(tiles_a * tiles_b)), dim3(256), 0, 0, v->d, dsel, d_y.p, n, dim, T, b0, tiles_b, d_part.p);
        hipLaunchKernelGGL(k_rg_fold, dim3(dge_grid((int64_t)PW)), dim3(256), 0, 0, d_part.p, (int)nb, P, W, d_M.p);
        DGE_HIP(hipGetLastError());
    }

    RG_BY_SLICES(P, launch_factor, d_M.p, P, T, nl, d_lambda.p, d_Lc.p, d_Lr.p, d_d.p, d_inv.p, d_beta.p, d_fail.p);
    DGE_HIP(hipGetLastError());
    std::vector<int> fail((size_t)nl);
    DGE_HIP(hipMemcpy(fail.data(), d_fail.p, (size_t)nl * sizeof(int), hipMemcpyDeviceToHost));
    for (int l = 0; l < nl; l++)
        if (fail[(size_t)l] >= 0)
            DGE_FAIL(DGE_ERR_ARG, "%s: the pivot of column %d under lambda[%d] = %g is not positive: the columns are collinear, or the penalty is too small for them", who,
                     fail[(size_t)l], l, lambda[l]);

    RG_BY_SLICES(P, launch_leverage, v->d, dsel, n, dim, nl, d_Lc.p, d_inv.p, d_h.p, d_bad.p + 1, d_bad.p + nl + 1);
    DGE_HIP(hipGetLastError());
    std::vector<unsigned long long> lev((size_t)nl + 1);
    DGE_HIP(hipMemcpy(lev.data(), d_bad.p + 1, ((size_t)nl + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int l = 0; l < nl; l++)
        if (lev[(size_t)l] != ~0ULL)
            DGE_FAIL(DGE_ERR_ARG, "%s: row %lld has leverage 1 under lambda[%d] = %g: leaving it out leaves nothing to predict it from", who,
                     (long long)u.at((int64_t)lev[(size_t)l]), l, lambda[l]);

    hipLaunchKernelGGL(k_rg_predict, dim3((unsigned)n_blocks, (unsigned)models), dim3(RG_BLOCK), 0, 0, v->d, dsel, (const uint8_t*)nullptr, n, dim, d_beta.p, d_y.p, T, d_h.p,
                       d_out.p, d_bs.p);
    DGE_HIP(hipGetLastError());
    float ms = 0.f;
    if ((rc = watch.stop(&ms))) return rc;

    std::vector<double> bs((size_t)models * (size_t)n_blocks), dd((size_t)nl * P), c0((size_t)T), bet, out;
    DGE_HIP(hipMemcpy(bs.data(), d_bs.p, bs.size() * sizeof(double), hipMemcpyDeviceToHost));
    DGE_HIP(hipMemcpy(dd.data(), d_d.p, dd.size() * sizeof(double), hipMemcpyDeviceToHost));
    DGE_HIP(hipMemcpy(c0.data(), d_M.p + P, (size_t)T * sizeof(double), hipMemcpyDeviceToHost));      // c[t][0]: the blocked sum of y[.][t]
    if (beta) { bet.resize((size_t)models * P); DGE_HIP(hipMemcpy(bet.data(), d_beta.p, bet.size() * sizeof(double), hipMemcpyDeviceToHost)); }
    if (loo_pred) { out.resize((size_t)models * (size_t)n); DGE_HIP(hipMemcpy(out.data(), d_out.p, out.size() * sizeof(double), hipMemcpyDeviceToHost)); }

    // outputs last: an error above leaves them as they were
    for (int m = 0; m < models; m++) {
        double s = 0.0;
        for (int64_t b = 0; b < n_blocks; b++) s += bs[(size_t)m * (size_t)n_blocks + (size_t)b];
        mae[m] = s / (double)n;
        mre[m] = mae[m] / (c0[(size_t)(m % T)] / (double)n);
    }
    if (beta) memcpy(beta, bet.data(), bet.size() * sizeof(double));
    if (loo_pred)
        for (int m = 0; m < models; m++) ur_scatter_back(loo_pred + (size_t)m * (size_t)rows, u, (double)NAN, out.data() + (size_t)m * (size_t)n);
    if (info) {
        info->rows = n; info->blocks = n_blocks; info->chunks = n_chunks;
        info->min_pivot = dd[0];
        for (double p : dd) if (p < info->min_pivot) info->min_pivot = p;
        memcpy(&info->max_leverage, &lev[(size_t)nl], sizeof(double));
        info->kernel_ms = ms;
    }
    return DGE_OK;
}

extern "C" int dge_ridge_loo_vectors(const dge_vectors* v, const double* y, int32_t n_targets, const uint8_t* select, const double* lambda, int32_t n_lambda, double* mae,
                                     double* mre, double* beta, double* loo_pred, dge_ridge_info* info) {
    const char* who = "dge_ridge_loo_vectors";
    if (!v || !y || !lambda || !mae || !mre) DGE_FAIL(DGE_ERR_ARG, "%s: null argument", who);
    int rc = ridge_limits(who, v->dim, n_targets, lambda, n_lambda);
    if (rc || (rc = dge_require_device(v->device))) return rc;
    dge_present pres;
    if ((rc = pres.load(v))) return rc;
    ur_rows u;
    ur_intake(ur_in{v->rows, pres.p, select, nullptr, 0, nullptr, 0, y, n_targets}, &u);
    return ridge_run(who, v, u, y, n_targets, lambda, n_lambda, mae, mre, beta, loo_pred, info);
}

extern "C" int dge_ridge_loo(int device, const float* features, int64_t n_rows, int32_t dim, const double* y, int32_t n_targets, const uint8_t* select, const double* lambda,
                             int32_t n_lambda, double* mae, double* mre, double* beta, double* loo_pred, dge_ridge_info* info) {
    const char* who = "dge_ridge_loo";
    if (!features || !y || !lambda || !mae || !mre || n_rows < 0 || dim < 0) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    int rc = ridge_limits(who, dim, n_targets, lambda, n_lambda);
    if (rc) return rc;
    ur_rows u;
    ur_intake(ur_in{n_rows, nullptr, select, nullptr, 0, nullptr, 0, y, n_targets}, &u);
    if (u.kind == UR_TARGET) DGE_FAIL(DGE_ERR_ARG, "%s: row %lld holds a feature or a target that is not finite", who, (long long)u.bad_row);
    if (u.n < 2) DGE_FAIL(DGE_ERR_ARG, "%s: %lld used rows; leave-one-out needs at least 2", who, (long long)u.n);
    dge_vectors_guard g;
    if ((rc = dge_vectors_from_host(device, features, n_rows, dim, nullptr, &g.v))) return rc;
    return ridge_run(who, g.v, u, y, n_targets, lambda, n_lambda, mae, mre, beta, loo_pred, info);
}

extern "C" int dge_ridge_predict_vectors(const dge_vectors* v, const double* beta, int32_t n_models, double* out) {
    const char* who = "dge_ridge_predict_vectors";
    if (!v || !beta || !out) DGE_FAIL(DGE_ERR_ARG, "%s: null argument", who);
    int rc = dge_range_check(who, "n_models", n_models, RG_MAX_MODELS);
    if (rc || (rc = dge_range_check(who, "dim", v->dim, RG_MAX_DIM)) || (rc = dge_require_device(v->device))) return rc;
    if (v->rows == 0) return DGE_OK;
    if (v->rows > 0x7fffffffLL * RG_BLOCK) DGE_FAIL(DGE_ERR_ARG, "%s: %lld rows exceed 2^39", who, (long long)v->rows);
    const int P = v->dim + 1;
    dge_tmp<double> d_beta, d_out;
    if ((rc = d_beta.alloc((size_t)n_models * P)) || (rc = d_out.alloc((size_t)n_models * (size_t)v->rows))) return rc;
    DGE_HIP(hipMemcpy(d_beta.p, beta, (size_t)n_models * P * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_rg_predict, dim3(dge_grid(v->rows, RG_BLOCK), (unsigned)n_models), dim3(RG_BLOCK), 0, 0, v->d, (const int64_t*)nullptr,
                       v->n_present == v->rows ? (const uint8_t*)nullptr : v->d_present, v->rows, v->dim, d_beta.p, (const double*)nullptr, 1, (const double*)nullptr, d_out.p,
                       (double*)nullptr);
    DGE_HIP(hipGetLastError());
    DGE_HIP(hipMemcpy(out, d_out.p, (size_t)n_models * (size_t)v->rows * sizeof(double), hipMemcpyDeviceToHost));
    return DGE_OK;
}
