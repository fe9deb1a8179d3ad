// sgns_selftest.hip — test entry points of libdge.so (gfx950): the commit-lock protocol, the atomics wave and the LDS accumulators of the trainers run in
// isolation on the device primitives of sgns_kernels.h, each with an exact conservation check; and the `.vec` number formatter against snprintf.
// Nothing here is reached by a training launch: outside the build stamp (dge_build_stamp, include/dge.h).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dge_algos.h"
#include "dge_internal.h"
#include "sgns_kernels.h"
#include "fmt_g9.h"

// ------------------------------------------------------------------------------------------ lock protocol self-test
// Conservation check of the commit-lock protocol used by k_sgns_train_locked, with the same primitives
// (row_trylock / rowA_load sc1 / rowA_store sc1 / workgroup release fence / row_unlock): every worker repeatedly picks
// NEG_BATCH pseudo-random rows, wins their locks in try-lock rounds and adds 1.0 to every element of each row it won.
// If exclusion, read freshness or write visibility failed anywhere on the chip, some increment would be lost:
// at the end every element of row r must equal the exact number of increments of row r (counted with integer atomics).
template <int DCH, int LAUX, int SAUX, int FENCE>
__global__ void __launch_bounds__(256)
k_selftest_locked_rows(float* table, int* locks, unsigned long long* counts, int32_t n_rows, int stride, int64_t n_workers,
                       int iters, uint64_t seed) {
    const int lane = threadIdx.x & 15;
    const int64_t worker = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    if (worker >= n_workers) return;
    const TableView tv = make_view(table, n_rows, stride);
    for (int it = 0; it < iters; it++) {
        int32_t t = -1;
        if (lane < NEG_BATCH) t = (int32_t)(dge_mix64(seed + (uint64_t)((worker * iters + it) * 16 + lane)) % (uint64_t)n_rows);
        int32_t tg[NEG_BATCH];
#pragma unroll
        for (int q = 0; q < NEG_BATCH; q++) tg[q] = __shfl(t, q, 16);
        unsigned pending = (1u << NEG_BATCH) - 1u;
        while (pending) {
            const bool want = lane < NEG_BATCH && ((pending >> lane) & 1u);
            const bool won = want ? row_trylock(locks, t) : false;
            const unsigned long long bal = __ballot(won);
            const unsigned got = (unsigned)(bal >> (threadIdx.x & 48)) & ((1u << NEG_BATCH) - 1u) & pending;
            if (FENCE & 1) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            Row<DCH> rr[NEG_BATCH];
#pragma unroll
            for (int q = 0; q < NEG_BATCH; q++) rowA_load<DCH, LAUX, false>(rr[q], tv, ((got >> q) & 1u) ? tg[q] : 0, lane);
#pragma unroll
            for (int q = 0; q < NEG_BATCH; q++)
                if ((got >> q) & 1u) {
#pragma unroll
                    for (int c = 0; c < DCH; c++) { rr[q].v[c].x += 1.f; rr[q].v[c].y += 1.f; rr[q].v[c].z += 1.f; rr[q].v[c].w += 1.f; }
                    rowA_store<DCH, SAUX, false>(rr[q], tv, tg[q], lane);
                }
            if (FENCE & 4) {
                float acc = 0.f;
#pragma unroll
                for (int q = 0; q < NEG_BATCH; q++) if ((got >> q) & 1u) acc += row_probe_lines(tv, tg[q], lane, stride / 32);
                asm volatile("" :: "v"(acc));
            }
            if (FENCE & 2) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); else __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (won) { row_unlock<(FENCE & 4) != 0>(locks, t); atomicAdd(&counts[t], 1ULL); }
            pending &= ~got;
            if (pending) __builtin_amdgcn_s_sleep(2);
        }
    }
}

extern "C" int dge_selftest_locked_rows(int device, int32_t n_rows, int64_t n_workers, int32_t iters, uint64_t seed, int32_t commit,
                                        int64_t* total_increments, double* max_abs_error) {
    if (n_rows <= 0 || n_workers <= 0 || iters <= 0 || !total_increments || !max_abs_error) DGE_FAIL(DGE_ERR_ARG, "dge_selftest_locked_rows: bad argument");
    int rc = dge_require_device(device);
    if (rc) return rc;
    const int stride = 128;
    float* d_tab = nullptr; int* d_locks = nullptr; unsigned long long* d_cnt = nullptr;
    if ((rc = dge_dev_alloc(&d_tab, (size_t)n_rows * stride))) return rc;
    if ((rc = dge_dev_alloc(&d_locks, (size_t)n_rows))) return rc;
    if ((rc = dge_dev_alloc(&d_cnt, (size_t)n_rows))) return rc;
    DGE_HIP(hipMemset(d_tab, 0, (size_t)n_rows * stride * sizeof(float)));
    DGE_HIP(hipMemset(d_locks, 0, (size_t)n_rows * sizeof(int)));
    DGE_HIP(hipMemset(d_cnt, 0, (size_t)n_rows * sizeof(unsigned long long)));
    unsigned blocks = (unsigned)((n_workers * 16 + 255) / 256);
#define ST_LAUNCH(L, S, F) hipLaunchKernelGGL((k_selftest_locked_rows<2, L, S, F>), dim3(blocks), dim3(256), 0, 0, d_tab, d_locks, d_cnt, n_rows, stride, n_workers, iters, seed)
    switch (commit) {
        case 0: ST_LAUNCH(16, 16, 0); break;      // relaxed commit of policy 5: sc1 both sides, the wave drains its stores
        case 1: ST_LAUNCH(16, 16, 4); break;      // strict commit of policy 6: + one returning atomic per stored 128-B line
        case 2: ST_LAUNCH(16, 16, 2); break;      // agent-scope release fence (buffer_wbl2): also lossless, 19x slower in the trainer
        default: DGE_FAIL(DGE_ERR_ARG, "dge_selftest_locked_rows: commit must be 0, 1 or 2");
    }
#undef ST_LAUNCH
    DGE_HIP(hipGetLastError());
    DGE_HIP(hipDeviceSynchronize());
    std::vector<float> tab((size_t)n_rows * stride); std::vector<unsigned long long> cnt((size_t)n_rows); std::vector<int> lk((size_t)n_rows);
    DGE_HIP(hipMemcpy(tab.data(), d_tab, tab.size() * sizeof(float), hipMemcpyDeviceToHost));
    DGE_HIP(hipMemcpy(cnt.data(), d_cnt, cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    DGE_HIP(hipMemcpy(lk.data(), d_locks, lk.size() * sizeof(int), hipMemcpyDeviceToHost));
    dge_dev_free(d_tab); dge_dev_free(d_locks); dge_dev_free(d_cnt);
    double worst = 0.0; int64_t total = 0;
    for (int32_t r = 0; r < n_rows; r++) {
        total += (int64_t)cnt[(size_t)r];
        if (lk[(size_t)r] != 0) worst = 1e30;                       // a lock was left held
        for (int c = 0; c < stride; c++) worst = std::max(worst, fabs((double)tab[(size_t)r * stride + c] - (double)cnt[(size_t)r]));
    }
    *total_increments = total; *max_abs_error = worst;
    return DGE_OK;
}

// The atomics wave in isolation (lk_post / lk_atomics_wave with its LDS accumulators of the hottest rows): the 12 workers of every workgroup post
// messages "add 1.0 to every element of these rows" — half of the rows among the n_acc hottest — and afterwards every element of row r must equal
// the number of times r was posted (counted with integer atomics; integers < 2^24 are exact in float): nothing parked in LDS may be lost or added twice.
// Messages alternate between kind 1 (syn1neg: bank 0) and kind 2 (syn0: bank 1); with div > 1 the rows are those of one block of a div-rank schedule:
// kind 1 rows = 1 (mod div), kind 2 rows = div - 1 (mod div), a slot = the row's rank inside its partition.
__global__ void __launch_bounds__(256) k_selftest_atomics_wave(float* table, unsigned long long* counts, int32_t n_rows, int stride, int iters, uint64_t seed, int n_acc, int drain, int div) {
    constexpr int DCH = 2;
    __shared__ __attribute__((aligned(16))) float s_mb[LK_MB_WORKERS * 2 * LkBox<DCH>::FLOATS];
    __shared__ int s_mb_flag[LK_MB_WORKERS * 2];
    __shared__ int s_mb_done;
    __shared__ float s_acc[2 * LK_ACC_ROWS(DCH) * DCH * 64];
    __shared__ int s_acc_cnt[2 * LK_ACC_ROWS(DCH)];
    if (threadIdx.x < LK_MB_WORKERS * 2) s_mb_flag[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_mb_done = 0;
    for (int i = threadIdx.x; i < 2 * LK_ACC_ROWS(DCH) * DCH * 64; i += blockDim.x) s_acc[i] = 0.f;
    if (threadIdx.x < 2 * LK_ACC_ROWS(DCH)) s_acc_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 15, wk = threadIdx.x >> 4;
    TableView tv = make_view(table, n_rows, stride);
    tv.valid = (uint32_t)stride;
    const int part_tgt = 1 % div, part_ctx = div - 1, n_part = n_rows / div;       // (rows of a partition: part, part + div, ... — n_rows >= div)
    if (wk >= LK_MB_WORKERS) {
        const int n = min(n_acc, LK_ACC_ROWS(DCH));
        lk_atomics_wave<DCH>(s_mb, s_mb_flag, &s_mb_done, LK_MB_WORKERS, tv, tv, tv, LkAcc{s_acc, s_acc_cnt, n, n, max(drain, 1), div, part_tgt, part_ctx});
        return;
    }
    unsigned n_posts = 0;
    Row<DCH> ones;
#pragma unroll
    for (int c = 0; c < DCH; c++) ones.v[c] = make_float4(1.f, 1.f, 1.f, 1.f);
    const int64_t worker = (int64_t)blockIdx.x * LK_MB_WORKERS + wk;
    for (int it = 0; it < iters; it++) {
        int32_t row = -1;
        if (lane < NEG_BATCH) {
            const uint64_t hsh = dge_mix64(seed + (uint64_t)((worker * iters + it) * 16 + lane));
            const int32_t rank = (int32_t)((hsh & 1ull) ? (hsh >> 1) % (uint64_t)min(8, n_part) : (hsh >> 1) % (uint64_t)n_part);
            row = rank * div + ((it & 1) ? part_ctx : part_tgt);
            atomicAdd(&counts[row], 1ULL);
        }
        lk_post<DCH>(s_mb, s_mb_flag, wk, n_posts, (it & 1) ? 2 : 1, row, 1.0f, ones, lane);
    }
    if (lane == 0) __hip_atomic_fetch_add(&s_mb_done, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

extern "C" int dge_selftest_atomics_wave(int device, int32_t n_rows, int32_t n_acc, int32_t drain, int32_t blocks, int32_t iters, uint64_t seed,
                                         int64_t* total_updates, double* max_abs_error) {
    return dge_selftest_atomics_wave_block(device, n_rows, n_acc, drain, 1, blocks, iters, seed, total_updates, max_abs_error);
}
extern "C" int dge_selftest_atomics_wave_block(int device, int32_t n_rows, int32_t n_acc, int32_t drain, int32_t div, int32_t blocks, int32_t iters, uint64_t seed,
                                               int64_t* total_updates, double* max_abs_error) {
    if (n_rows <= 0 || blocks <= 0 || iters <= 0 || n_acc < 0 || drain <= 0 || div <= 0 || n_rows < div || !total_updates || !max_abs_error)
        DGE_FAIL(DGE_ERR_ARG, "dge_selftest_atomics_wave: bad argument");
    int rc = dge_require_device(device);
    if (rc) return rc;
    const int stride = 128;
    float* d_tab = nullptr; unsigned long long* d_cnt = nullptr;
    if ((rc = dge_dev_alloc(&d_tab, (size_t)n_rows * stride))) return rc;
    if ((rc = dge_dev_alloc(&d_cnt, (size_t)n_rows))) return rc;
    DGE_HIP(hipMemset(d_tab, 0, (size_t)n_rows * stride * sizeof(float)));
    DGE_HIP(hipMemset(d_cnt, 0, (size_t)n_rows * sizeof(unsigned long long)));
    hipLaunchKernelGGL(k_selftest_atomics_wave, dim3((unsigned)blocks), dim3(256), 0, 0, d_tab, d_cnt, n_rows, stride, iters, seed, n_acc, drain, div);
    DGE_HIP(hipGetLastError());
    DGE_HIP(hipDeviceSynchronize());
    std::vector<float> tab((size_t)n_rows * stride); std::vector<unsigned long long> cnt((size_t)n_rows);
    DGE_HIP(hipMemcpy(tab.data(), d_tab, tab.size() * sizeof(float), hipMemcpyDeviceToHost));
    DGE_HIP(hipMemcpy(cnt.data(), d_cnt, cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    dge_dev_free(d_tab); dge_dev_free(d_cnt);
    double worst = 0.0; int64_t total = 0;
    for (int32_t r = 0; r < n_rows; r++) {
        total += (int64_t)cnt[(size_t)r];
        for (int c = 0; c < stride; c++) worst = std::max(worst, fabs((double)tab[(size_t)r * stride + c] - (double)cnt[(size_t)r]));
    }
    *total_updates = total; *max_abs_error = worst;
    return DGE_OK;
}

// hot_add / hot_drain_block in isolation: every worker adds 1.0 to every element of pseudo-random hot rows `iters` times;
// afterwards each row must hold exactly the number of additions it received (integers < 2^24 are exact in float).
__global__ void __launch_bounds__(256) k_selftest_hot_add(float* rows, unsigned long long* hits, int n_hot, int drain, int iters, uint64_t seed, int64_t n_workers) {
    const int lane = threadIdx.x & 15;
    const int64_t worker = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    float* s_hot = s_dyn;
    int* s_cnt = (int*)(s_dyn + (size_t)n_hot * 64);
    for (int i = threadIdx.x; i < n_hot * 65; i += blockDim.x) s_dyn[i] = 0.f;
    __syncthreads();
    const TableView t = make_view(rows, n_hot, 64);
    Row<1> one; one.v[0] = make_float4(1.f, 1.f, 1.f, 1.f);
    if (worker < n_workers) {
        uint64_t s = dge_mix64(seed + (uint64_t)worker);
        for (int it = 0; it < iters; it++) {
            s = s * DGE_W2V_MULT + 11;
            // skewed like a Huffman path: slot k with probability ~2^-(k+1)
            int slot = min(n_hot - 1, (int)__builtin_ctzll((s >> 20) | (1ull << 40)));
            slot = n_hot - 1 - slot;
            hot_add<1>(s_hot, s_cnt, slot, drain, t, slot, lane, 1.0f, one);
            if (lane == 0) atomicAdd(&hits[slot], 1ULL);
        }
    }
    hot_drain_block(s_hot, n_hot * 64, rows);
}

extern "C" int dge_selftest_hot_add(int device, int32_t n_hot, int64_t n_workers, int32_t iters, int32_t drain, uint64_t seed,
                                    int64_t* total_additions, double* max_abs_error) {
    if (n_hot <= 0 || n_hot > 118 || n_workers <= 0 || iters <= 0 || drain <= 0 || !total_additions || !max_abs_error)
        DGE_FAIL(DGE_ERR_ARG, "dge_selftest_hot_add: bad argument");
    int rc = dge_require_device(device);
    if (rc) return rc;
    dge_tmp<float> d_rows; dge_tmp<unsigned long long> d_hits;
    if ((rc = d_rows.alloc((size_t)n_hot * 64))) return rc;
    if ((rc = d_hits.alloc((size_t)n_hot))) return rc;
    DGE_HIP(hipMemset(d_rows.p, 0, (size_t)n_hot * 64 * sizeof(float)));
    DGE_HIP(hipMemset(d_hits.p, 0, (size_t)n_hot * sizeof(unsigned long long)));
    const unsigned blocks = (unsigned)((n_workers * 16 + 255) / 256);
    hipLaunchKernelGGL(k_selftest_hot_add, dim3(blocks), dim3(256), (size_t)n_hot * 65 * 4, 0, d_rows.p, d_hits.p, n_hot, drain, iters, seed, n_workers);
    DGE_HIP(hipGetLastError());
    DGE_HIP(hipDeviceSynchronize());
    std::vector<float> rows((size_t)n_hot * 64); std::vector<unsigned long long> hits((size_t)n_hot);
    DGE_HIP(hipMemcpy(rows.data(), d_rows.p, rows.size() * sizeof(float), hipMemcpyDeviceToHost));
    DGE_HIP(hipMemcpy(hits.data(), d_hits.p, hits.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    int64_t total = 0; double worst = 0;
    for (int r = 0; r < n_hot; r++) {
        total += (int64_t)hits[(size_t)r];
        for (int e = 0; e < 64; e++) worst = std::max(worst, fabs((double)rows[(size_t)r * 64 + e] - (double)hits[(size_t)r]));
    }
    *total_additions = total; *max_abs_error = worst;
    return DGE_OK;
}

// dge_fmt_g9 (fmt_g9.h) against snprintf("%.9g") on `n` pseudo-random floats: half of them random bit patterns, half values of an embedding's range; host code only
extern "C" int dge_selftest_fmt_g9(int64_t n, uint64_t seed, int64_t* fast_path, int64_t* mismatches) {
    if (n < 0 || !fast_path || !mismatches) DGE_FAIL(DGE_ERR_ARG, "dge_selftest_fmt_g9: bad argument");
    int64_t fast = 0, bad = 0;
    uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
    char a[64], b[64];
    for (int64_t i = 0; i < n; i++) {
        s = dge_mix64(s + (uint64_t)i);
        uint32_t u = (uint32_t)(s >> 32);
        float f;
        if (i & 1) memcpy(&f, &u, 4);
        else f = (float)(((double)(s & 0xFFFFFFFFull) / 4294967296.0 * 2.0 - 1.0) * ((i & 6) == 0 ? 1e-3 : ((i & 6) == 2 ? 1.0 : 40.0)));
        char* e = dge_fmt_g9(f, a);
        if (!e) continue;
        *e = 0; fast++;
        snprintf(b, sizeof(b), "%.9g", (double)f);
        if (strcmp(a, b) != 0) bad++;
    }
    *fast_path = fast; *mismatches = bad;
    return DGE_OK;
}
