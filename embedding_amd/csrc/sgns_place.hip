// sgns_place.hip — which memory the trainer's tables lie in (libdge.so, gfx950): the table probe behind dge_model_create's allocations, the row-rate probe
// and the placement search.  All of it moves a launch's TIME, never the bytes or requests of a pair, so this file is outside the build stamp
// (dge_build_stamp, include/dge.h): the search trains through dge_model_train like any caller and puts tables, counters and plan back when it is done.
#include <algorithm>
#include <map>
#include <mutex>
#include <vector>

#include "dge_internal.h"
#include "sgns_kernels.h"      // TableView, neg_table_row: the probes read rows the way the trainers do
#include "sgns_model.h"

// ------------------------------------------------------------------------------------------ where the tables lie
// Which memory a table of random rows lies in decides how fast rows can be read AND WRITTEN BACK in it: allocations of half a gigabyte fall into
// two classes 15 % apart (a microbenchmark of random 512-byte rows read and stored back reaches 6.3 or 7.3 TB/s on them, nothing in between),
// a launch of the lock kernel takes 412-415 ms with both tables in fast memory and 473-479 ms with both in slow memory, and no property of
// the allocation visible from user space tells the classes apart (profiles/r03_placement.txt: not contiguity, alignment, page-table fragments,
// position or the neighbours) — but a 2-millisecond probe does.  So a table is the best of several virtual-memory allocations under that
// probe: candidates are created one after the other (all held, or the allocator would hand the same memory out again) until the fast class has
// shown (the best at least 14 % above the worst: probe rates come in three levels, ~4150 / ~4620 / ~4810 GB/s) or TABLE_CANDIDATES have been seen;
// the best stays.  Fast memory is 1 allocation in 2 ... 6 on most boxes; candidates are hipMalloc and virtual-memory allocations in turn.
#define TABLE_CANDIDATES 32
typedef unsigned int pv4u __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256) k_probe_table(char* base, uint64_t rows, int iters, float* sink) {
    const int lane = threadIdx.x & 15;
    const uint64_t group = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    uint64_t s = 0x9E3779B97F4A7C15ull * (group + 1);
    float acc = 0.f;
    for (int i = 0; i < iters; i += 8) {
        pv4u v[8][2]; char* pp[8];
#pragma unroll
        for (int z = 0; z < 8; z++) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            pp[z] = base + ((s >> 20) % rows) * 512u + (uint32_t)lane * 16u;
            v[z][0] = __builtin_nontemporal_load((pv4u*)pp[z]); v[z][1] = __builtin_nontemporal_load((pv4u*)(pp[z] + 256));
        }
#pragma unroll
        for (int z = 0; z < 8; z++) {
            acc += __uint_as_float(v[z][0].x ^ v[z][1].y);
            __hip_atomic_store((unsigned*)pp[z], v[z][0].x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);              // the same bytes back, write-through
            __hip_atomic_store((unsigned*)(pp[z] + 256), v[z][1].x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (acc == 12345.678f) sink[0] = acc;
}
struct VmAlloc { size_t bytes; hipMemGenericAllocationHandle_t h; };
static std::map<void*, VmAlloc> g_vm_allocs;
static std::mutex g_vm_mu;
static int vm_alloc(void** out, size_t bytes, int device) {
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned; prop.location.type = hipMemLocationTypeDevice; prop.location.id = device;
    const size_t g = (size_t)2 << 20, sz = (bytes + g - 1) / g * g;
    hipMemGenericAllocationHandle_t h;
    if (hipMemCreate(&h, sz, &prop, 0) != hipSuccess) { (void)hipGetLastError(); return DGE_ERR_DEVICE; }
    void* va = nullptr;
    if (hipMemAddressReserve(&va, sz, g, nullptr, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipMemRelease(h); return DGE_ERR_DEVICE; }
    hipMemAccessDesc acc = {}; acc.location = prop.location; acc.flags = hipMemAccessFlagsProtReadWrite;
    if (hipMemMap(va, sz, 0, h, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipMemAddressFree(va, sz); (void)hipMemRelease(h); return DGE_ERR_DEVICE; }
    if (hipMemSetAccess(va, sz, &acc, 1) != hipSuccess) { (void)hipGetLastError(); (void)hipMemUnmap(va, sz); (void)hipMemAddressFree(va, sz); (void)hipMemRelease(h); return DGE_ERR_DEVICE; }
    { std::lock_guard<std::mutex> lk(g_vm_mu); g_vm_allocs[va] = VmAlloc{sz, h}; }
    *out = va;
    return DGE_OK;
}
// frees what dge_table_alloc (or hipMalloc) returned
void dge_table_free(void* p) {
    if (!p) return;
    VmAlloc a{0, {}};
    { std::lock_guard<std::mutex> lk(g_vm_mu); auto it = g_vm_allocs.find(p); if (it != g_vm_allocs.end()) { a = it->second; g_vm_allocs.erase(it); } }
    if (a.bytes) { (void)hipMemUnmap(p, a.bytes); (void)hipMemRelease(a.h); (void)hipMemAddressFree(p, a.bytes); }
    else (void)hipFree(p);
}
int dge_table_alloc(float** out, size_t floats, int device, hipStream_t st, int* seen, double* rate_best, double* rate_worst) {
    *out = nullptr;
    const size_t bytes = floats * sizeof(float);
    if (seen) *seen = 0;
    // small tables live in the caches: nothing to choose (and the probe needs rows to draw from)
    size_t free_b = 0, total_b = 0;
    // (and tables of 2 GiB and more are left to hipMalloc.  Round 3: the runtime aborted inside the probing of a 4.5 GB virtual-memory allocation.  Round 4: creating
    //  nine models of 2 x 3.4 GB in one process — ~100 virtual-memory allocations of 3.4 GB made, probed and released — ended twice in four runs inside this function,
    //  once as "Memory access fault by GPU node" under the probe kernel, once as an abort() of the runtime (tests/test_gpu_configs.py, full-size cfg5 on 8 ranks).
    //  The placement classes were measured on half-gigabyte tables; above 2 GiB the choice is not worth a process.)
    if (bytes < ((size_t)64 << 20) || bytes >= ((size_t)2 << 30) || hipMemGetInfo(&free_b, &total_b) != hipSuccess) return dge_dev_alloc(out, floats);
    const int n_max = (int)std::max<size_t>(1, std::min<size_t>(TABLE_CANDIDATES, free_b / 4 / bytes));      // candidates may take a quarter of the free memory
    dge_tmp<float> sink;
    int rc = sink.alloc(4);
    if (rc) return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { if (e0) (void)hipEventDestroy(e0); (void)hipGetLastError(); return dge_dev_alloc(out, floats); }
    std::vector<void*> cand; std::vector<double> rate;
    double best = 0, worst = 1e30;
    for (int k = 0; k < n_max; k++) {
        // candidates alternate between the two kinds of allocation: which kind the fast memory turns up in differs from box to box (on some every
        // hipMalloc allocation is slow and one virtual-memory allocation in two is fast, on others 24 virtual-memory allocations in a row are slow)
        void* q = nullptr;
        if (k & 1) { if (vm_alloc(&q, bytes, device) != DGE_OK) break; }       // (the virtual-memory API refused, or memory ran out: what we have, or hipMalloc below)
        else if (hipMalloc(&q, bytes) != hipSuccess) { (void)hipGetLastError(); break; }
        double r = 0;
        bool ok = hipMemsetAsync(q, 0, bytes, st) == hipSuccess;
        for (int rep = 0; rep < 3 && ok; rep++) {
            ok = hipEventRecord(e0, st) == hipSuccess;
            hipLaunchKernelGGL(k_probe_table, dim3(4096), dim3(256), 0, st, (char*)q, (uint64_t)(bytes / 512), 64, sink.p);
            ok = ok && hipEventRecord(e1, st) == hipSuccess && hipEventSynchronize(e1) == hipSuccess;
            float ms = 0.f;
            if (ok && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms > 0) r = std::max(r, 65536.0 * 64 * 1024.0 / (ms * 1e-3) / 1e9);
        }
        if (!ok) { (void)hipGetLastError(); dge_table_free(q); break; }
        cand.push_back(q); rate.push_back(r);
        best = std::max(best, r); worst = std::min(worst, r);
        if (cand.size() >= 2 && best >= 1.14 * worst) break;                   // the fast class has shown (an intermediate one, ~11 % above the slowest, exists too)
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (cand.empty()) return dge_dev_alloc(out, floats);
    size_t pick = 0;
    for (size_t k = 1; k < cand.size(); k++) if (rate[k] > rate[pick]) pick = k;
    for (size_t k = 0; k < cand.size(); k++) if (k != pick) dge_table_free(cand[k]);
    *out = (float*)cand[pick];
    if (seen) *seen = (int)cand.size();
    if (rate_best) *rate_best = best;
    if (rate_worst) *rate_worst = worst;
    return DGE_OK;
}

// ---- dge_model_row_rates: how fast THIS model's memory answers the three things the lock kernel does to it — rows read at random, rows read and
// written back (write-through stores, as a commit does), exchanges on random lock words.  Two models of one process can differ by 15 % in
// training speed while the device's copy rate does not move (profiles/r02_box_drift.txt): the difference follows the allocation, and this
// probe shows which access it is without training anything.  16 lanes per row, 8 rows in flight per group; tables below 4 GiB.
template <int MODE>
__global__ void __launch_bounds__(256) k_probe_rows(float* t0, float* t1, int* locks, const uint4* ctab, int64_t T, int64_t V, int32_t stride, int64_t reads_per_group,
                                                    float* sink) {
    const int lane = threadIdx.x & 15;
    const int64_t group = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    uint64_t s = dge_mix64(0x9E3779B97F4A7C15ull * (uint64_t)(group + 1));
    const TableView v0 = make_view(t0, V, stride), v1 = make_view(t1, V, stride);
    float acc = 0.f;
    if (MODE == 3) {
        for (int64_t i = 0; i < reads_per_group; i += 4) {
            int32_t t[4];
#pragma unroll
            for (int z = 0; z < 4; z++) { s = s * DGE_W2V_MULT + 11; t[z] = neg_table_row(ctab, ((s >> 16) + (uint64_t)lane * 0x9E3779B1ull) % (uint64_t)T); }
            acc += (float)(t[0] ^ t[1] ^ t[2] ^ t[3]);
        }
    } else if (MODE == 2) {
        for (int64_t i = 0; i < reads_per_group; i++) {
            s = s * DGE_W2V_MULT + 11;
            const int64_t w = (int64_t)(((s >> 16) + (uint64_t)lane * 0x9E3779B1ull) % (uint64_t)(2 * V));
            acc += (float)__hip_atomic_exchange(&locks[w], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else {
        for (int64_t i = 0; i < reads_per_group; i += 8) {
            v4u v[8]; uint32_t off[8]; uint32_t mix = 0;
#pragma unroll
            for (int z = 0; z < 8; z++) {
                s = s * DGE_W2V_MULT + 11;
                off[z] = (uint32_t)((s >> 16) % (uint64_t)V) * v0.row_bytes + (uint32_t)lane * 16u;
                v[z] = __builtin_amdgcn_raw_buffer_load_b128((z & 1) ? v1.rsrc : v0.rsrc, (int)off[z], 0, 0);
                for (uint32_t c = 256; c < v0.row_bytes; c += 256) {
                    const v4u u = __builtin_amdgcn_raw_buffer_load_b128((z & 1) ? v1.rsrc : v0.rsrc, (int)(off[z] + c), 0, 0);
                    mix ^= u.x;
                }
            }
#pragma unroll
            for (int z = 0; z < 8; z++) {
                acc += __uint_as_float(v[z].x ^ mix);
                if (MODE == 1) {           // the same bytes back, write-through (aux 16 = sc1), every 256-byte piece of the row
                    for (uint32_t c = 0; c < v0.row_bytes; c += 256) {
                        const v4u u = c ? __builtin_amdgcn_raw_buffer_load_b128((z & 1) ? v1.rsrc : v0.rsrc, (int)(off[z] + c), 0, 0) : v[z];
                        __builtin_amdgcn_raw_buffer_store_b128(u, (z & 1) ? v1.rsrc : v0.rsrc, (int)(off[z] + c), 0, 16);
                    }
                }
            }
        }
    }
    if (acc == 12345.678f) sink[0] = acc;                 // keeps the loads alive
}

extern "C" int dge_model_row_rates(dge_model* m, double* read_gb_per_s, double* rewrite_gb_per_s, double* lock_exchanges_per_s, double* table_lookups_per_s) {
    if (!m) DGE_FAIL(DGE_ERR_ARG, "dge_model_row_rates: null model");
    if ((uint64_t)m->V * (uint64_t)m->stride * 4ull >= 0xFFFFFFFFull) DGE_FAIL(DGE_ERR_ARG, "dge_model_row_rates: tables of 4 GiB and more are not probed");
    DGE_HIP(hipSetDevice(m->device));
    int rc = dge_drain_events(m);
    if (rc) return rc;
    DGE_HIP(hipStreamSynchronize(m->stream));
    const int64_t groups = 256 * 16 * 16, reads = 256;     // 65 536 groups x 256 rows
    dge_tmp<float> sink;
    if ((rc = sink.alloc(4))) return rc;
    hipEvent_t e0, e1;
    DGE_HIP(hipEventCreate(&e0)); DGE_HIP(hipEventCreate(&e1));
    double best[4] = {0, 0, 0, 0};
    for (int mode = 0; mode < 4; mode++) {
        for (int r = 0; r < 3; r++) {
            DGE_HIP(hipEventRecord(e0, m->stream));
            const dim3 grid((unsigned)(groups * 16 / 256));
#define PROBE(M) hipLaunchKernelGGL(k_probe_rows<M>, grid, dim3(256), 0, m->stream, m->d_syn0, m->d_syn1neg, m->d_locks, m->d_ctab, m->T, m->V, m->stride, reads, sink.p)
            if (mode == 0) PROBE(0); else if (mode == 1) PROBE(1); else if (mode == 2) PROBE(2); else PROBE(3);
#undef PROBE
            DGE_HIP(hipEventRecord(e1, m->stream));
            DGE_HIP(hipEventSynchronize(e1));
            float ms = 0.f; DGE_HIP(hipEventElapsedTime(&ms, e0, e1));
            const double n = (double)groups * reads;
            const double rate = mode >= 2 ? n * 16.0 / (ms * 1e-3) : n * m->stride * 4.0 * (mode == 1 ? 2.0 : 1.0) / (ms * 1e-3) / 1e9;
            if (rate > best[mode]) best[mode] = rate;
        }
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    DGE_HIP(hipGetLastError());
    if (read_gb_per_s) *read_gb_per_s = best[0];
    if (rewrite_gb_per_s) *rewrite_gb_per_s = best[1];
    if (lock_exchanges_per_s) *lock_exchanges_per_s = best[2];
    if (table_lookups_per_s) *table_lookups_per_s = best[3];
    return DGE_OK;
}

// ---- dge_model_tune_placement.  Which physical memory hipMalloc hands an array decides a training launch's duration by up to 15 %, array by
// array, and no allocation rule (contiguous blocks, aligned ranges, shuffled 2 MiB chunks) nor any cheap probe of the memory predicts it
// (profiles/r02_box_drift.txt, profiles/r03_placement.txt).  So the library searches with the only probe that works, the caller's own launch:
// rows [row0, row0 + n_rows) of `w` are trained once for a baseline; then, one array at a time (negative-sampling table, lock words, syn1neg,
// syn0), a copy in freshly allocated memory takes the array's place, the same rows are trained again, and the faster placement stays.
// Rejected placements are only freed at the end (the allocator would hand the same memory out again).  The tables' contents and the
// model's counters are saved first and restored last: training results are exactly those of an untuned model.
static int tune_time_launch(dge_model* m, const dge_walks* w, int64_t row0, int64_t n_rows, double* ms) {
    hipEvent_t a = nullptr, b = nullptr;
    DGE_HIP(hipEventCreate(&a));
    if (hipEventCreate(&b) != hipSuccess || hipEventRecord(a, m->stream) != hipSuccess) {
        (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b);
        DGE_FAIL(DGE_ERR_DEVICE, "dge_model_tune_placement: cannot time the probe launch");
    }
    int rc = dge_model_train(m, w, row0, n_rows, 0, 0, 0, 1.0, std::max<int64_t>(w->n, 1));
    if (rc == DGE_OK) {
        if (hipEventRecord(b, m->stream) != hipSuccess || hipEventSynchronize(b) != hipSuccess) { dge_set_error("dge_model_tune_placement: the probe launch failed"); rc = DGE_ERR_DEVICE; }
        float t = 0.f;
        if (rc == DGE_OK && hipEventElapsedTime(&t, a, b) == hipSuccess) *ms = t;
    }
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    return rc;
}

extern "C" int dge_model_tune_placement(dge_model* m, const dge_walks* w, int64_t row0, int64_t n_rows, int32_t candidates, double* ms_before, double* ms_after,
                                        int32_t* arrays_moved) {
    if (!m || !w || row0 < 0 || n_rows <= 0 || row0 + n_rows > w->n || candidates < 1) DGE_FAIL(DGE_ERR_ARG, "dge_model_tune_placement: bad argument");
    if (w->device != m->device) DGE_FAIL(DGE_ERR_ARG, "dge_model_tune_placement: corpus and model live on different devices");
    DGE_HIP(hipSetDevice(m->device));
    int rc = dge_drain_events(m);
    if (rc) return rc;
    if (ms_before) *ms_before = 0; if (ms_after) *ms_after = 0; if (arrays_moved) *arrays_moved = 0;
    if (m->V == 0) return DGE_OK;
    hipStream_t st = m->stream;
    const size_t tab_bytes = ((size_t)m->V * (size_t)m->stride + 64) * sizeof(float);
    const size_t lock_bytes = 2 * ((size_t)m->V + 1) * sizeof(int), ctab_bytes = ((size_t)m->ctab_blocks + 1) * sizeof(uint4);
    // what a probe launch changes: the two tables (syn1 too under hierarchical softmax), the counters, the launch statistics
    dge_tmp<char> keep0, keep1, keep2;
    if ((rc = keep0.alloc(tab_bytes)) || (rc = keep1.alloc(tab_bytes))) return rc;
    if (m->d_syn1 && (rc = keep2.alloc(tab_bytes))) return rc;
    unsigned long long counters[3] = {0, 0, 0};
    DGE_HIP(hipMemcpyAsync(keep0.p, m->d_syn0, tab_bytes, hipMemcpyDeviceToDevice, st));
    DGE_HIP(hipMemcpyAsync(keep1.p, m->d_syn1neg, tab_bytes, hipMemcpyDeviceToDevice, st));
    if (m->d_syn1) DGE_HIP(hipMemcpyAsync(keep2.p, m->d_syn1, tab_bytes, hipMemcpyDeviceToDevice, st));
    DGE_HIP(hipMemcpyAsync(counters, m->d_counters, sizeof(counters), hipMemcpyDeviceToHost, st));
    DGE_HIP(hipStreamSynchronize(st));
    const double k_ms = m->kernel_ms, w_ms = m->walk_ms; const int64_t launches = m->launches;
    const TrainPlan last_plan = m->last_plan; const bool has_plan = m->has_plan;

    std::vector<void*> graveyard;
    double best = 0, first = 0;
    int moved = 0;
    // Every probe starts from the tables as they were: a launch's duration depends on them under hierarchical softmax (a path node whose dot product
    // has left the sigmoid's table is skipped), and probes that train the same walks again and again get faster by themselves — the search then
    // "found" 24 improvements and 723 -> 280 ms on a model whose launches did not change (profiles/r03_final_numbers.txt).
    auto reset_tables = [&]() -> int {
        DGE_HIP(hipMemcpyAsync(m->d_syn0, keep0.p, tab_bytes, hipMemcpyDeviceToDevice, st));
        DGE_HIP(hipMemcpyAsync(m->d_syn1neg, keep1.p, tab_bytes, hipMemcpyDeviceToDevice, st));
        if (m->d_syn1) DGE_HIP(hipMemcpyAsync(m->d_syn1, keep2.p, tab_bytes, hipMemcpyDeviceToDevice, st));
        return DGE_OK;
    };
    rc = tune_time_launch(m, w, row0, n_rows, &best);          // warm-up (work buffers, the owner-computes schedule's lazy allocations)
    if (rc == DGE_OK) rc = reset_tables();
    if (rc == DGE_OK) rc = tune_time_launch(m, w, row0, n_rows, &best);
    first = best;
    struct Slot { void** p; size_t bytes; };
    Slot slots[4] = {{(void**)&m->d_ctab, ctab_bytes}, {(void**)&m->d_locks, lock_bytes}, {(void**)&m->d_syn1neg, tab_bytes}, {(void**)&m->d_syn0, tab_bytes}};
    // A pass tries every array in up to candidates - 1 other allocations.  A pass that found nothing ends the search (a model that started
    // well costs one pass); one that did means the model started badly, and arrays it left alone may still be badly placed: passes go on while
    // they find something, at most six (a single pass left one process in three at 119.4 -> 115.7 ms: 447.8 ms per launch where its neighbours ran
    // 414; at most three passes left one in six at 112.4: 434.5; profiles/r03_bench_repeat_search.txt).
    for (int pass = 0; pass < 6 && rc == DGE_OK; pass++) {
        const int moved_before = moved;
        for (int a = 0; a < 4 && rc == DGE_OK; a++)
            for (int c = 1; c < candidates && rc == DGE_OK; c++) {
                void* fresh = nullptr;
                if (hipMalloc(&fresh, slots[a].bytes) != hipSuccess) { (void)hipGetLastError(); break; }      // out of memory: keep what we have
                void* old = *slots[a].p;
                if (hipMemcpyAsync(fresh, old, slots[a].bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) { (void)hipFree(fresh); dge_set_error("dge_model_tune_placement: copy failed"); rc = DGE_ERR_DEVICE; break; }
                *slots[a].p = fresh;
                double t = 0;
                rc = reset_tables();
                if (rc == DGE_OK) rc = tune_time_launch(m, w, row0, n_rows, &t);
                if (rc == DGE_OK && t < best * 0.995) { best = t; graveyard.push_back(old); moved++; break; }      // this array is well placed now: next array
                else { *slots[a].p = old; graveyard.push_back(fresh); }
            }
        if (moved == moved_before) break;
    }
    hipError_t e = hipStreamSynchronize(st);
    for (void* g : graveyard) dge_table_free(g);                  // (a table that came from dge_table_alloc is a virtual-memory allocation)
    if (rc == DGE_OK && e != hipSuccess) { dge_set_error("dge_model_tune_placement: %s", hipGetErrorName(e)); rc = DGE_ERR_DEVICE; }
    // put everything back as it was before the probes
    DGE_HIP(hipMemcpyAsync(m->d_syn0, keep0.p, tab_bytes, hipMemcpyDeviceToDevice, st));
    DGE_HIP(hipMemcpyAsync(m->d_syn1neg, keep1.p, tab_bytes, hipMemcpyDeviceToDevice, st));
    if (m->d_syn1) DGE_HIP(hipMemcpyAsync(m->d_syn1, keep2.p, tab_bytes, hipMemcpyDeviceToDevice, st));
    DGE_HIP(hipMemsetAsync(m->d_locks, 0, lock_bytes, st));
    DGE_HIP(hipMemcpyAsync(m->d_counters, counters, sizeof(counters), hipMemcpyHostToDevice, st));
    DGE_HIP(hipStreamSynchronize(st));
    int rc2 = dge_drain_events(m);
    m->kernel_ms = k_ms; m->walk_ms = w_ms; m->launches = launches;
    m->last_plan = last_plan; m->has_plan = has_plan;
    m->seen_gen = 0;                                           // (the next launch derives its rows again)
    if (rc == DGE_OK) rc = rc2;
    if (ms_before) *ms_before = first; if (ms_after) *ms_after = best; if (arrays_moved) *arrays_moved = moved;
    m->search_runs++; m->search_ms_before = first; m->search_ms_after = best; m->search_moved = moved;
    return rc;
}

extern "C" int dge_model_placement_search(const dge_model* m, int32_t* runs, double* ms_before, double* ms_after, int32_t* arrays_moved) {
    if (!m) DGE_FAIL(DGE_ERR_ARG, "dge_model_placement_search: null model");
    if (runs) *runs = m->search_runs;
    if (ms_before) *ms_before = m->search_ms_before;
    if (ms_after) *ms_after = m->search_ms_after;
    if (arrays_moved) *arrays_moved = m->search_moved;
    return DGE_OK;
}

extern "C" int dge_model_table_placement(const dge_model* m, int32_t table, int32_t* candidates, double* best_gb_per_s, double* worst_gb_per_s) {
    if (!m || table < 0 || table > 2) DGE_FAIL(DGE_ERR_ARG, "dge_model_table_placement: table is 0 (syn0), 1 (syn1neg) or 2 (syn1)");
    if (candidates) *candidates = m->placed_seen[table];
    if (best_gb_per_s) *best_gb_per_s = m->placed_best[table];
    if (worst_gb_per_s) *worst_gb_per_s = m->placed_worst[table];
    return DGE_OK;
}
