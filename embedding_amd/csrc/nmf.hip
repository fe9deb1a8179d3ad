// nmf.hip — non-negative matrix factorisation of a sparse matrix (gfx950) as the fully specified rule of include/dge.h: the reference's "MF" baseline
// (P/matrixFactorization_tract.py:26-45, P/flowFeatureGeneration_tract.py:29-40) without a dense R x R array.  The per-element arithmetic lives in nmf_rule.h;
// this file is what runs it at full concurrency without changing a bit.
//
// Everything here is a memory-bound sparse pass.  The shared intake (coo_entries.h) checks the entries and sorts the kept ones by (row, column); a second sort of (column, row) gives the permutation that
// lists them by column.  W is held [n x rank] and H transposed, [m x rank], so that the rank values a pass gathers for an entry are one contiguous run; H is
// turned back on the host at the end.  One pass forms P (and Q = V / P) per entry.  A segment sum — over a row's or a column's entries — is done by 16 lanes,
// four segments a wave: lane l takes the products l, l + 16, ... of the segment into `rank` accumulators, then four DPP row shifts (dge_row16_shl) fold the 16 partials as the rule
// says (8, 4, 2, 1), without LDS.  The blocked sums, the Gram matrices and the update with its floor are small kernels over n or m values.  No atomic on a
// floating-point value anywhere: the only atomics are integer minima / maxima of the input scan, which are the same in any order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <vector>

#include "coo_entries.h"
#include "nmf_rule.h"

// ------------------------------------------------------------------------------------------ the entries, once per call
// a value of the matrix for the shared intake (coo_entries.h): kind 1 is not finite, kind 2 is negative
struct NmfValue {
    static __device__ int kind(double v) { return !isfinite(v) ? COO_KIND1 : v < 0.0 ? COO_KIND2 : v == 0.0 ? COO_ZEROS : COO_KEEP; }
};

// the entries by row: row, column and value of each, and its key for the order by column
__global__ void __launch_bounds__(256) k_nmf_by_row(const uint64_t* __restrict__ key, const int64_t* __restrict__ idx, const double* __restrict__ val, int64_t kept, int64_t n, int64_t m,
                                                    int32_t* __restrict__ ri, int32_t* __restrict__ ci, double* __restrict__ V, uint64_t* __restrict__ key2, int32_t* __restrict__ pos) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= kept) return;
    const uint64_t k = key[p], i = k / (uint64_t)m, j = k - i * (uint64_t)m;
    ri[p] = (int32_t)i; ci[p] = (int32_t)j; V[p] = val[idx[p]];
    key2[p] = j * (uint64_t)n + i;
    pos[p] = (int32_t)p;
}

// the entries by column: the row of each and its value (Q goes through perm every pass, V once here)
__global__ void __launch_bounds__(256) k_nmf_by_col(const uint64_t* __restrict__ key2, const int32_t* __restrict__ perm, const double* __restrict__ V, int64_t kept, int64_t n,
                                                    int32_t* __restrict__ crow, double* __restrict__ cV) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= kept) return;
    crow[c] = (int32_t)(key2[c] % (uint64_t)n);
    cV[c] = V[perm[c]];
}

// ptr[x] = the first sorted entry whose key is at least x * stride, x = 0 .. count
__global__ void __launch_bounds__(256) k_nmf_ptr(const uint64_t* __restrict__ key, int64_t kept, uint64_t stride, int64_t count, int64_t* __restrict__ ptr) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x > count) return;
    ptr[x] = coo_lower_bound(key, kept, (uint64_t)x * stride);
}

// X[x][r] = nmf_init(seed, base + x * sx + r * sr, vmax)
__global__ void __launch_bounds__(256) k_nmf_init(double* __restrict__ X, int64_t cnt, int rank, uint64_t seed, uint64_t base, uint64_t sx, uint64_t sr, double vmax) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= cnt * rank) return;
    const uint64_t x = (uint64_t)(t / rank), r = (uint64_t)(t % rank);
    X[t] = nmf_init(seed, base + x * sx + r * sr, vmax);
}

// ------------------------------------------------------------------------------------------ the passes of an iteration
// per entry: P by the chain; what: 0 Q = V / P, 1 the divergence objective's term V log(V / P) - V, 2 the Euclidean objective's term (V - P)^2 - P^2
__global__ void __launch_bounds__(256) k_nmf_entries(const int32_t* __restrict__ ri, const int32_t* __restrict__ ci, const double* __restrict__ V, const double* __restrict__ W,
                                                     const double* __restrict__ Ht, int rank, int64_t kept, int what, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= kept) return;
    const double p = nmf_p(W + (size_t)ri[e] * (size_t)rank, 1, Ht + (size_t)ci[e] * (size_t)rank, 1, rank);
    const double v = V[e];
    double o;
    if (what == 0) o = v / p;
    else if (what == 1) o = v * log(v / p) - v;
    else { const double d = v - p; o = d * d - p * p; }
    out[e] = o;
}

// the segment sums of every row (or column): out[g][r] = SEGMENT SUM over the entries c of segment g of Y[other[c]][r] * b[c], b[c] = val[perm[c]] or val[c].
// RB: the accumulators a lane holds, the least of 4, 10, 16, 32 that is at least rank.
template <int RB>
__global__ void __launch_bounds__(256) k_nmf_segments(const int64_t* __restrict__ ptr, const int32_t* __restrict__ other, const double* __restrict__ val, const int32_t* __restrict__ perm,
                                                      const double* __restrict__ Y, int rank, int64_t cnt, double* __restrict__ out) {
    const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) / NMF_LANES;       // a DPP row of 16 lanes is one segment: its lanes leave together
    const int l = threadIdx.x & (NMF_LANES - 1);
    if (g >= cnt) return;
    double acc[RB];
#pragma unroll
    for (int r = 0; r < RB; r++) acc[r] = 0.0;
    const int64_t hi = ptr[g + 1];
    for (int64_t c = ptr[g] + l; c < hi; c += NMF_LANES) {
        const double b = perm ? val[perm[c]] : val[c];
        const double* y = Y + (size_t)other[c] * (size_t)rank;
#pragma unroll
        for (int r = 0; r < RB; r++)
            if (r < rank) acc[r] = nmf_seg_step(acc[r], y[r], b);
    }
#pragma unroll
    for (int r = 0; r < RB; r++) {
        double p = acc[r];
        p = p + dge_row16_shl<8>(p);
        p = p + dge_row16_shl<4>(p);
        p = p + dge_row16_shl<2>(p);
        p = p + dge_row16_shl<1>(p);
        acc[r] = p;
    }
    if (l == 0) {
        double* o = out + (size_t)g * (size_t)rank;
#pragma unroll
        for (int r = 0; r < RB; r++)
            if (r < rank) o[r] = acc[r];
    }
}

// the block sums of the columns of X [cnt x rank]: bs[b][r]; a workgroup is one block of the blocked sum, thread r adds column r
__global__ void __launch_bounds__(NMF_MAX_RANK) k_nmf_col_blocks(const double* __restrict__ X, int64_t cnt, int rank, double* __restrict__ bs) {
    const int r = threadIdx.x;
    if (r >= rank) return;
    const int64_t lo = (int64_t)blockIdx.x * NMF_BLOCK, hi = lo + NMF_BLOCK < cnt ? lo + NMF_BLOCK : cnt;
    bs[(size_t)blockIdx.x * (size_t)rank + r] = nmf_block_sum(X + r, rank, lo, hi);
}

// the block sums of the Gram matrix of X: bs[b][r * rank + s] over the block's rounded products X[i][r] * X[i][s]
__global__ void __launch_bounds__(256) k_nmf_gram_blocks(const double* __restrict__ X, int64_t cnt, int rank, double* __restrict__ bs) {
    const int64_t lo = (int64_t)blockIdx.x * NMF_BLOCK, hi = lo + NMF_BLOCK < cnt ? lo + NMF_BLOCK : cnt;
    for (int p = threadIdx.x; p < rank * rank; p += 256) {
        const int r = p / rank, s = p - r * rank;
        bs[(size_t)blockIdx.x * (size_t)(rank * rank) + p] = nmf_block_dot(X + r, X + s, rank, lo, hi);
    }
}

// out[c] = the block sums of component c added in block order
__global__ void __launch_bounds__(256) k_nmf_sum_blocks(const double* __restrict__ bs, int64_t n_blocks, int comps, double* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= comps) return;
    out[c] = nmf_sum_blocks(bs + c, comps, n_blocks);
}

// X[x][r] = floor(X[x][r] * (num[x][r] / den)), den = d[r] (divergence) or the chain over s of G[r][s] * X[x][s] on the OLD values of the row (Euclidean;
// g_rows != 0: G is read as G[r * rank + s], else as G[s * rank + r] — the rule's two index orders)
template <int RB>
__global__ void __launch_bounds__(256) k_nmf_update(double* __restrict__ X, int64_t cnt, int rank, const double* __restrict__ num, const double* __restrict__ d,
                                                    const double* __restrict__ G, int g_rows) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= cnt) return;
    double* row = X + (size_t)x * (size_t)rank;
    const double* nu = num + (size_t)x * (size_t)rank;
    double old[RB];
#pragma unroll
    for (int r = 0; r < RB; r++) old[r] = r < rank ? row[r] : 0.0;
#pragma unroll
    for (int r = 0; r < RB; r++) {
        if (r < rank) {
            double den;
            if (d) den = d[r];
            else {
                den = 0.0;
#pragma unroll
                for (int s = 0; s < RB; s++)
                    if (s < rank) den = fma(g_rows ? G[r * rank + s] : G[s * rank + r], old[s], den);
            }
            row[r] = nmf_update(old[r], nu[r], den);
        }
    }
}

// ------------------------------------------------------------------------------------------ host side
namespace {

int segments(const int64_t* ptr, const int32_t* other, const double* val, const int32_t* perm, const double* Y, int rank, int64_t cnt, double* out) {
    const dim3 grid(dge_grid(cnt * NMF_LANES)), block(256);
    if (rank <= 4) hipLaunchKernelGGL((k_nmf_segments<4>), grid, block, 0, 0, ptr, other, val, perm, Y, rank, cnt, out);
    else if (rank <= 10) hipLaunchKernelGGL((k_nmf_segments<10>), grid, block, 0, 0, ptr, other, val, perm, Y, rank, cnt, out);
    else if (rank <= 16) hipLaunchKernelGGL((k_nmf_segments<16>), grid, block, 0, 0, ptr, other, val, perm, Y, rank, cnt, out);
    else hipLaunchKernelGGL((k_nmf_segments<32>), grid, block, 0, 0, ptr, other, val, perm, Y, rank, cnt, out);
    DGE_HIP(hipGetLastError());
    return DGE_OK;
}

int update(double* X, int64_t cnt, int rank, const double* num, const double* d, const double* G, int g_rows) {
    const dim3 grid(dge_grid(cnt)), block(256);
    if (rank <= 4) hipLaunchKernelGGL((k_nmf_update<4>), grid, block, 0, 0, X, cnt, rank, num, d, G, g_rows);
    else if (rank <= 10) hipLaunchKernelGGL((k_nmf_update<10>), grid, block, 0, 0, X, cnt, rank, num, d, G, g_rows);
    else if (rank <= 16) hipLaunchKernelGGL((k_nmf_update<16>), grid, block, 0, 0, X, cnt, rank, num, d, G, g_rows);
    else hipLaunchKernelGGL((k_nmf_update<32>), grid, block, 0, 0, X, cnt, rank, num, d, G, g_rows);
    DGE_HIP(hipGetLastError());
    return DGE_OK;
}

// the blocked column sums of X [cnt x rank] into out[rank], or of its Gram matrix into out[rank x rank]; bs: scratch of ceil(cnt / 256) * comps values
int blocked(const double* X, int64_t cnt, int rank, bool gram, double* bs, double* out) {
    const int64_t n_blocks = (cnt + NMF_BLOCK - 1) / NMF_BLOCK;
    const int comps = gram ? rank * rank : rank;
    if (gram) hipLaunchKernelGGL(k_nmf_gram_blocks, dim3((unsigned)n_blocks), dim3(256), 0, 0, X, cnt, rank, bs);
    else hipLaunchKernelGGL(k_nmf_col_blocks, dim3((unsigned)n_blocks), dim3(NMF_MAX_RANK), 0, 0, X, cnt, rank, bs);
    hipLaunchKernelGGL(k_nmf_sum_blocks, dim3(dge_grid(comps)), dim3(256), 0, 0, bs, n_blocks, comps, out);
    DGE_HIP(hipGetLastError());
    return DGE_OK;
}

int cfg_check(const char* who, const dge_nmf_cfg* cfg, int64_t n, int64_t m) {
    if (cfg->rank < 1 || cfg->rank > NMF_MAX_RANK) DGE_FAIL(DGE_ERR_ARG, "%s: rank = %d is outside 1 .. %d", who, cfg->rank, NMF_MAX_RANK);
    if (cfg->max_iter < 1 || cfg->max_iter > NMF_MAX_ITER) DGE_FAIL(DGE_ERR_ARG, "%s: max_iter = %d is outside 1 .. %d", who, cfg->max_iter, NMF_MAX_ITER);
    if (cfg->update != 0 && cfg->update != 1) DGE_FAIL(DGE_ERR_ARG, "%s: update = %d is neither 0 (divergence) nor 1 (euclidean)", who, cfg->update);
    if (n < 1 || n > 0x7fffffffLL) DGE_FAIL(DGE_ERR_ARG, "%s: n = %lld is outside 1 .. 2^31 - 1", who, (long long)n);
    if (m < 1 || m > 0x7fffffffLL) DGE_FAIL(DGE_ERR_ARG, "%s: m = %lld is outside 1 .. 2^31 - 1", who, (long long)m);
    return DGE_OK;
}

// the rule on device entries (row, col, val: device arrays of ne input entries).  init_W / init_H: host arrays or NULL (both or neither).
int nmf_run(const char* who, const int32_t* d_row, const int32_t* d_col, const double* d_val, int64_t ne, int64_t n, int64_t m, const dge_nmf_cfg* cfg, const double* init_W,
            const double* init_H, double* W, double* H, dge_nmf_info* info) {
    int rc;
    const int rank = cfg->rank;
    const size_t nW = (size_t)n * (size_t)rank, nH = (size_t)m * (size_t)rank;
    dge_stopwatch watch;
    if ((rc = watch.start(0))) return rc;

    // ---- the entries: checks and the order by row (the shared intake), the order by column
    coo_entries E;
    if ((rc = coo_intake<NmfValue, true>(d_row, d_col, d_val, ne, n, m, 0x7fffffffLL, E))) return rc;
    switch (E.fault) {
    case COO_RANGE: DGE_FAIL(DGE_ERR_ARG, "%s: entry %lld lies outside the %lld x %lld matrix", who, (long long)E.at, (long long)n, (long long)m);
    case COO_KIND1: DGE_FAIL(DGE_ERR_ARG, "%s: entry %lld holds a value that is not finite", who, (long long)E.at);
    case COO_KIND2: DGE_FAIL(DGE_ERR_ARG, "%s: entry %lld holds a negative value", who, (long long)E.at);
    case COO_ZEROS: DGE_FAIL(DGE_ERR_ARG, "%s: no entry is left: all %lld values are zero", who, (long long)ne);
    case COO_MANY: DGE_FAIL(DGE_ERR_ARG, "%s: %lld entries exceed 2^31 - 1", who, (long long)E.kept);
    case COO_DUP: DGE_FAIL(DGE_ERR_ARG, "%s: entry %lld repeats the row and column of an earlier entry", who, (long long)E.at);
    }
    const int64_t zeros = E.zeros, kept = E.kept;
    const double vmax = E.vmax;

    dge_tmp<uint64_t> key2, skey2;
    dge_tmp<int64_t> rptr, cptr;
    dge_tmp<int32_t> ri, ci, pos, perm, crow;
    dge_tmp<double> V, cV, Q;
    if ((rc = ri.alloc((size_t)kept)) || (rc = ci.alloc((size_t)kept)) || (rc = pos.alloc((size_t)kept)) || (rc = perm.alloc((size_t)kept)) || (rc = crow.alloc((size_t)kept)) ||
        (rc = V.alloc((size_t)kept)) || (rc = cV.alloc((size_t)kept)) || (rc = Q.alloc((size_t)kept)) || (rc = key2.alloc((size_t)kept)) || (rc = skey2.alloc((size_t)kept)) ||
        (rc = rptr.alloc((size_t)n + 1)) || (rc = cptr.alloc((size_t)m + 1))) return rc;
    hipLaunchKernelGGL(k_nmf_by_row, dim3(dge_grid(kept)), dim3(256), 0, 0, E.skey.p, E.sidx.p, d_val, kept, n, m, ri.p, ci.p, V.p, key2.p, pos.p);
    DGE_HIP(hipGetLastError());
    if ((rc = dge_sort_pairs(dge_scratch(), (const uint64_t*)key2.p, skey2.p, (const int32_t*)pos.p, perm.p, kept, dge_bits((uint64_t)n * (uint64_t)m), 0, true))) return rc;
    hipLaunchKernelGGL(k_nmf_by_col, dim3(dge_grid(kept)), dim3(256), 0, 0, skey2.p, perm.p, V.p, kept, n, crow.p, cV.p);
    hipLaunchKernelGGL(k_nmf_ptr, dim3(dge_grid(n + 1)), dim3(256), 0, 0, E.skey.p, kept, (uint64_t)m, n, rptr.p);
    hipLaunchKernelGGL(k_nmf_ptr, dim3(dge_grid(m + 1)), dim3(256), 0, 0, skey2.p, kept, (uint64_t)n, m, cptr.p);
    DGE_HIP(hipGetLastError());

    // ---- the factors: W [n x rank], H transposed [m x rank]
    const int64_t big = n > m ? n : m, big_blocks = (big + NMF_BLOCK - 1) / NMF_BLOCK, kept_blocks = (kept + NMF_BLOCK - 1) / NMF_BLOCK;
    const size_t n_bs = (size_t)big_blocks * rank * rank > (size_t)kept_blocks ? (size_t)big_blocks * rank * rank : (size_t)kept_blocks;      // the objective's terms are summed through it too
    dge_tmp<double> dW, dHt, num, bs, small;
    if ((rc = dW.alloc(nW)) || (rc = dHt.alloc(nH)) || (rc = num.alloc((size_t)big * rank)) || (rc = bs.alloc(n_bs)) ||
        (rc = small.alloc(2 * NMF_MAX_RANK * NMF_MAX_RANK))) return rc;
    double* d_a = small.p;                                   // rank or rank^2 values
    double* d_b = small.p + NMF_MAX_RANK * NMF_MAX_RANK;
    std::vector<double> hostW, hostHt(nH);
    if (init_W) {
        hostW.resize(nW);
        for (size_t t = 0; t < nW; t++) hostW[t] = nmf_floor(init_W[t]);
        for (int r = 0; r < rank; r++)
            for (int64_t j = 0; j < m; j++) hostHt[(size_t)j * rank + r] = nmf_floor(init_H[(size_t)r * (size_t)m + (size_t)j]);
        DGE_HIP(hipMemcpy(dW.p, hostW.data(), nW * sizeof(double), hipMemcpyHostToDevice));
        DGE_HIP(hipMemcpy(dHt.p, hostHt.data(), nH * sizeof(double), hipMemcpyHostToDevice));
    } else {
        hipLaunchKernelGGL(k_nmf_init, dim3(dge_grid((int64_t)nW)), dim3(256), 0, 0, dW.p, n, rank, cfg->seed, (uint64_t)0, (uint64_t)rank, (uint64_t)1, vmax);
        hipLaunchKernelGGL(k_nmf_init, dim3(dge_grid((int64_t)nH)), dim3(256), 0, 0, dHt.p, m, rank, cfg->seed, (uint64_t)n * (uint64_t)rank, (uint64_t)1, (uint64_t)m, vmax);
        DGE_HIP(hipGetLastError());
    }

    const dim3 egrid(dge_grid(kept)), eblock(256);
    for (int it = 0; it < cfg->max_iter; it++) {
        if (cfg->update == 0) {
            hipLaunchKernelGGL(k_nmf_entries, egrid, eblock, 0, 0, ri.p, ci.p, V.p, dW.p, dHt.p, rank, kept, 0, Q.p);
            if ((rc = segments(cptr.p, crow.p, Q.p, perm.p, dW.p, rank, m, num.p))) return rc;
            if ((rc = blocked(dW.p, n, rank, false, bs.p, d_a))) return rc;
            if ((rc = update(dHt.p, m, rank, num.p, d_a, nullptr, 0))) return rc;
            hipLaunchKernelGGL(k_nmf_entries, egrid, eblock, 0, 0, ri.p, ci.p, V.p, dW.p, dHt.p, rank, kept, 0, Q.p);
            if ((rc = segments(rptr.p, ci.p, Q.p, nullptr, dHt.p, rank, n, num.p))) return rc;
            if ((rc = blocked(dHt.p, m, rank, false, bs.p, d_a))) return rc;
            if ((rc = update(dW.p, n, rank, num.p, d_a, nullptr, 0))) return rc;
        } else {
            if ((rc = segments(cptr.p, crow.p, cV.p, nullptr, dW.p, rank, m, num.p))) return rc;
            if ((rc = blocked(dW.p, n, rank, true, bs.p, d_a))) return rc;
            if ((rc = update(dHt.p, m, rank, num.p, nullptr, d_a, 1))) return rc;
            if ((rc = segments(rptr.p, ci.p, V.p, nullptr, dHt.p, rank, n, num.p))) return rc;
            if ((rc = blocked(dHt.p, m, rank, true, bs.p, d_a))) return rc;
            if ((rc = update(dW.p, n, rank, num.p, nullptr, d_a, 0))) return rc;
        }
    }

    // ---- the objective of the final factors (outside the exact rule: the device's log is not libm's)
    double objective = 0.0;
    {
        const bool eu = cfg->update == 1;
        const int comps = eu ? rank * rank : rank;
        std::vector<double> a((size_t)comps), b((size_t)comps);
        double terms = 0.0;
        hipLaunchKernelGGL(k_nmf_entries, egrid, eblock, 0, 0, ri.p, ci.p, V.p, dW.p, dHt.p, rank, kept, eu ? 2 : 1, Q.p);
        DGE_HIP(hipGetLastError());
        if ((rc = blocked(Q.p, kept, 1, false, bs.p, d_a))) return rc;
        DGE_HIP(hipMemcpy(&terms, d_a, sizeof terms, hipMemcpyDeviceToHost));
        if ((rc = blocked(dW.p, n, rank, eu, bs.p, d_a)) || (rc = blocked(dHt.p, m, rank, eu, bs.p, d_b))) return rc;
        DGE_HIP(hipMemcpy(a.data(), d_a, (size_t)comps * sizeof(double), hipMemcpyDeviceToHost));
        DGE_HIP(hipMemcpy(b.data(), d_b, (size_t)comps * sizeof(double), hipMemcpyDeviceToHost));
        double cross = 0.0;
        for (int t = 0; t < comps; t++) cross += a[(size_t)t] * b[(size_t)t];
        objective = terms + cross;
    }
    float ms = 0.f;
    if ((rc = watch.stop(&ms))) return rc;

    // outputs last: an error above leaves them as they were
    hostW.resize(nW);
    DGE_HIP(hipMemcpy(hostW.data(), dW.p, nW * sizeof(double), hipMemcpyDeviceToHost));
    DGE_HIP(hipMemcpy(hostHt.data(), dHt.p, nH * sizeof(double), hipMemcpyDeviceToHost));
    memcpy(W, hostW.data(), nW * sizeof(double));
    for (int r = 0; r < rank; r++)
        for (int64_t j = 0; j < m; j++) H[(size_t)r * (size_t)m + (size_t)j] = hostHt[(size_t)j * rank + r];
    if (info) {
        info->rows = n; info->cols = m; info->entries = kept; info->zeros = zeros; info->iterations = cfg->max_iter; info->reserved = 0;
        info->vmax = vmax; info->objective = objective; info->kernel_ms = ms;
    }
    return DGE_OK;
}

}  // namespace

extern "C" int dge_nmf_coo(int device, const int32_t* row, const int32_t* col, const double* val, int64_t n_entries, int64_t n, int64_t m, const dge_nmf_cfg* cfg,
                           const double* init_W, const double* init_H, double* W, double* H, dge_nmf_info* info) {
    const char* who = "dge_nmf_coo";
    if (!row || !col || !val || !cfg || !W || !H) DGE_FAIL(DGE_ERR_ARG, "%s: null argument", who);
    if ((init_W == nullptr) != (init_H == nullptr)) DGE_FAIL(DGE_ERR_ARG, "%s: null argument: init_W and init_H come together", who);
    int rc = cfg_check(who, cfg, n, m);
    if (rc) return rc;
    if (n_entries < 1 || n_entries > 0x7fffffffLL) DGE_FAIL(DGE_ERR_ARG, "%s: n_entries = %lld is outside 1 .. 2^31 - 1", who, (long long)n_entries);
    if (init_W) {
        const size_t nW = (size_t)n * (size_t)cfg->rank, nH = (size_t)m * (size_t)cfg->rank;
        for (size_t t = 0; t < nW; t++) if (!(isfinite(init_W[t]) && init_W[t] >= 0.0)) DGE_FAIL(DGE_ERR_ARG, "%s: init_W[%lld] is not a finite value >= 0", who, (long long)t);
        for (size_t t = 0; t < nH; t++) if (!(isfinite(init_H[t]) && init_H[t] >= 0.0)) DGE_FAIL(DGE_ERR_ARG, "%s: init_H[%lld] is not a finite value >= 0", who, (long long)t);
    }
    if ((rc = dge_require_device(device))) return rc;
    dge_tmp<int32_t> d_row, d_col;
    dge_tmp<double> d_val;
    if ((rc = coo_upload(row, col, val, n_entries, d_row, d_col, d_val))) return rc;
    return nmf_run(who, d_row.p, d_col.p, d_val.p, n_entries, n, m, cfg, init_W, init_H, W, H, info);
}

extern "C" int dge_nmf_flows(const dge_flows* f, int32_t T, int32_t mode, int32_t slot, const uint8_t* select, const dge_nmf_cfg* cfg, double* W, double* H, int64_t* region_index,
                             dge_nmf_info* info) {
    const char* who = "dge_nmf_flows";
    if (!f || !cfg || !W || !H) DGE_FAIL(DGE_ERR_ARG, "%s: null argument", who);
    int rc = cfg_check(who, cfg, 1, 1);
    if (rc) return rc;
    dge_tmp<int32_t> d_row, d_col;
    dge_tmp<double> d_val;
    int64_t ne = 0;
    std::vector<int64_t> regions;
    if ((rc = dge_flows_slot_coo(f, T, mode, slot, select, who, d_row, d_col, d_val, &ne, regions))) return rc;
    const int64_t n = (int64_t)regions.size();
    if ((rc = nmf_run(who, d_row.p, d_col.p, d_val.p, ne, n, n, cfg, nullptr, nullptr, W, H, info))) return rc;
    if (region_index) memcpy(region_index, regions.data(), (size_t)n * sizeof(int64_t));
    return DGE_OK;
}
