// dge_internal.h — handle layouts, error plumbing and the counted host waits shared by every translation unit of libdge.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <string_view>
#include <unordered_set>
#include <vector>

#include "../../include/dge.h"

void dge_set_error(const char* fmt, ...);

#define DGE_FAIL(code, ...)            \
    do {                               \
        dge_set_error(__VA_ARGS__);    \
        return (code);                 \
    } while (0)

#define DGE_HIP(expr)                                                                         \
    do {                                                                                      \
        hipError_t e__ = (expr);                                                              \
        if (e__ != hipSuccess) {                                                              \
            dge_set_error("HIP error %s at %s:%d: %s", hipGetErrorName(e__), __FILE__, __LINE__, #expr); \
            return DGE_ERR_DEVICE;                                                            \
        }                                                                                     \
    } while (0)

// Host synchronisations the library performs (blocking stream / device / event waits and blocking copies), counted process-wide: a multi-GPU episode must not
// contain any in steady state (tests count them: dge_host_sync_count, include/dge.h).  Every call site below goes through these wrappers.
extern std::atomic<int64_t> g_dge_host_syncs;
static inline hipError_t dge_counted_stream_sync(hipStream_t s) { g_dge_host_syncs.fetch_add(1, std::memory_order_relaxed); return hipStreamSynchronize(s); }
static inline hipError_t dge_counted_device_sync() { g_dge_host_syncs.fetch_add(1, std::memory_order_relaxed); return hipDeviceSynchronize(); }
static inline hipError_t dge_counted_event_sync(hipEvent_t e) { g_dge_host_syncs.fetch_add(1, std::memory_order_relaxed); return hipEventSynchronize(e); }
static inline hipError_t dge_counted_memcpy(void* d, const void* s, size_t n, hipMemcpyKind k) { g_dge_host_syncs.fetch_add(1, std::memory_order_relaxed); return hipMemcpy(d, s, n, k); }
#define hipStreamSynchronize(s) dge_counted_stream_sync(s)
#define hipDeviceSynchronize() dge_counted_device_sync()
#define hipEventSynchronize(e) dge_counted_event_sync(e)
#define hipMemcpy(d, s, n, k) dge_counted_memcpy((d), (s), (n), (k))

int dge_require_device(int device);   // DGE_OK when `device` is a usable gfx950 device, sets it current

template <typename T>
static inline int dge_dev_alloc(T** p, size_t n) {
    *p = nullptr;
    if (n == 0) n = 1;
    DGE_HIP(hipMalloc((void**)p, n * sizeof(T)));
    return DGE_OK;
}
static inline void dge_dev_free(void* p) { if (p) (void)hipFree(p); }

// a device buffer with one owner: the scratch of one call, freed on every exit path, or a member of a handle's group, moved in once it is finished
template <typename T>
struct dge_tmp {
    T* p = nullptr;
    dge_tmp() = default;
    dge_tmp(std::nullptr_t) {}                         // `= nullptr` in a handle reads as the raw member did
    dge_tmp(const dge_tmp&) = delete;
    dge_tmp& operator=(const dge_tmp&) = delete;
    dge_tmp(dge_tmp&& o) noexcept : p(o.release()) {}
    dge_tmp& operator=(dge_tmp&& o) noexcept { if (this != &o) { if (p) (void)hipFree(p); p = o.release(); } return *this; }
    ~dge_tmp() { if (p) (void)hipFree(p); }
    int alloc(size_t n) { if (p) { (void)hipFree(p); p = nullptr; } return dge_dev_alloc(&p, n); }
    T* release() { T* q = p; p = nullptr; return q; }
    template <typename U>             // takes over the buffer of o, whose elements are as wide as T (bits parsed as uint32_t that are float32 from here on)
    void adopt(dge_tmp<U>&& o) { static_assert(sizeof(U) == sizeof(T), "adopt: the element sizes differ"); if (p) (void)hipFree(p); p = reinterpret_cast<T*>(o.release()); }
    operator T*() const { return p; }
};
static_assert(sizeof(dge_tmp<float>) == sizeof(float*), "a dge_tmp member lies in a handle as the raw pointer did");

// One alias slot as the walk kernel reads it: 32 bytes (two 16-byte loads of one aligned sector), the ONLY memory access of a walk
// step.  nbr_alias already resolves alias[i] to the neighbour it points at ("alias == -1" -> nbr itself), and the slot carries the
// row bounds of both candidates, so the next step needs no row_ptr look-up: one dependent round trip per step instead of two.
struct __attribute__((aligned(32))) dge_slot {
    double prob;
    int32_t nbr;
    int32_t nbr_alias;
    uint32_t base, k;               // edges of nbr:       [base, base + k)   (the store holds fewer than 2^32 edges)
    uint32_t base_alias, k_alias;   // edges of nbr_alias
};

// What a graph owns on the device, in four groups.  A group frees its arrays when it goes and moves as a whole: assigning an empty one is the free, and an entry
// that replaces a group builds the new one in a local and moves it in after the last step that can fail (graph.hip).  alloc: the arrays at their sizes, no content.
struct dge_coo {                   // the COO staging in insertion order (allEdges, J/LayeredGraph.java:142)
    dge_tmp<int32_t> src, dst;
    dge_tmp<double> w;
    int64_t n = 0, cap = 0;
    int alloc(int64_t c) { cap = c; int rc = src.alloc((size_t)c); if (!rc) rc = dst.alloc((size_t)c); if (!rc) rc = w.alloc((size_t)c); return rc; }
};
struct dge_csr {                   // built: row_ptr is there (an allocation is never null, dge_dev_alloc)
    dge_tmp<int64_t> row_ptr;      // [V + 1]
    dge_tmp<int32_t> nbr;          // [E]
    dge_tmp<double> w, outdeg;     // [E], [V]
    int32_t V = 0;
    int64_t E = 0;
    bool built() const { return row_ptr.p != nullptr; }
    int alloc(int32_t v, int64_t e) {
        V = v; E = e;
        int rc = row_ptr.alloc((size_t)v + 1); if (!rc) rc = nbr.alloc((size_t)e); if (!rc) rc = w.alloc((size_t)e); if (!rc) rc = outdeg.alloc((size_t)v);
        return rc;
    }
};
struct dge_tables {                // alias tables of n slots and the walk kernel's form of them: the edges' (n = E), the sources' (n = S)
    dge_tmp<double> prob;
    dge_tmp<int32_t> alias;
    dge_tmp<dge_slot> slots;
    int alloc(int64_t n) { int rc = prob.alloc((size_t)n); if (!rc) rc = alias.alloc((size_t)n); if (!rc) rc = slots.alloc((size_t)n); return rc; }
};
struct dge_sources {               // J/LayeredGraph.java:145-148
    dge_tmp<int32_t> srcv;
    dge_tmp<double> w;
    dge_tables tables;
    int64_t S = 0;
    double weight_sum = 0.0;
    int stream_sum = 0;            // how set_sources summed (0 running +=, 1 DoubleStream.sum())
    bool sum_fixed = false;        // the host assigned sourceWeightSum itself (dge_graph_set_source_weight_sum)
};

struct dge_graph {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    dge_coo coo;
    int32_t max_id = -1;
    dge_csr csr;                   // "the CSR is built" is csr.built(): no flag beside it
    dge_tables tables;
    dge_sources src;
    // alias_built: the tables (tables, src.tables) are complete and made from the present CSR, outDegree, sources and weight sum.  It stays a flag
    // (the trainer reads it by this name): dge_graph_build_alias sets it with the tables it moves in, every entry that changes one of those inputs clears it, and
    // the CSR never goes without its tables (drop_tables).
    bool alias_built = false;
    void drop_tables() { tables = dge_tables{}; alias_built = false; }
    // the region ids of a graph made from .od text (od_read.hip), ascending: vertex h*R + i is region od_regions[i] in slice h
    std::vector<int64_t> od_regions;
};
// back to what dge_graph_create left (the device of g is current: the groups free device memory)
static inline void dge_graph_reset(dge_graph* g) {
    g->coo = dge_coo{}; g->csr = dge_csr{}; g->src = dge_sources{}; g->drop_tables();
    g->max_id = -1;
    g->od_regions.clear();
}
// what the builders ask of the graph they fill (od_commit.h, spatial.hip): no edges, no reserved vertices, no sources
static inline bool dge_graph_fresh(const dge_graph* g) { return g->coo.n == 0 && g->max_id < 0 && g->src.S == 0 && !g->src.srcv.p && g->od_regions.empty(); }

// dge_walks and dge_vectors own their arrays as dge_tmp members: delete is the free; a creator builds the handle in a unique_ptr and releases it into *out last
struct dge_walks {
    int device = 0;
    int64_t n = 0;
    int32_t L = 0;
    dge_tmp<int32_t> d = nullptr;
    uint64_t gen = 0;          // changes whenever the library writes the corpus (a trainer may keep what it derived from an unchanged one)
    // The corpus's last ASYNCHRONOUS use: dge_model_train and dge_model_walk_and_train return with their launches queued on the model's stream and record `used`
    // behind them (dge_walks_mark).  Every other entry that touches d goes behind it: dge_walks_order where it enqueues work, dge_walks_settle before a blocking
    // copy.  A chain of marks on different streams holds, because a stream first orders itself behind the mark it replaces.  mutable: readers mark a const corpus.
    mutable hipEvent_t used = nullptr;
    mutable hipStream_t used_on = nullptr;
    mutable bool used_pending = false;      // recorded, and no host wait of the library is known to have passed it
    ~dge_walks() { if (used) (void)hipEventDestroy(used); }
};
uint64_t dge_next_generation();
// `s` waits for the corpus's last asynchronous use; nothing to do when that use is on `s` itself.  No host wait.
static inline int dge_walks_order(const dge_walks* w, hipStream_t s) {
    if (w->used_pending && w->used_on != s) DGE_HIP(hipStreamWaitEvent(s, w->used, 0));
    return DGE_OK;
}
// work that uses the corpus has just been queued on `s`
static inline int dge_walks_mark(const dge_walks* w, hipStream_t s) {
    if (!w->used) DGE_HIP(hipEventCreateWithFlags(&w->used, hipEventDisableTiming));
    DGE_HIP(hipEventRecord(w->used, s));
    w->used_on = s; w->used_pending = true;
    return DGE_OK;
}
// the host waits for the corpus's last asynchronous use (one counted wait, and only while one is pending)
static inline int dge_walks_settle(const dge_walks* w) {
    if (w->used_pending) { DGE_HIP(hipEventSynchronize(w->used)); w->used_pending = false; }
    return DGE_OK;
}
// a host wait that covers the last use has just been made (the device, or a stream that dge_walks_order put behind it)
static inline void dge_walks_settled(const dge_walks* w) { w->used_pending = false; }

// interned strings, id = position: a host object, no device involved.  seq_ingest.hip fills it, seq_write.hip reads ptr / len
struct dge_names {
    std::vector<std::unique_ptr<char[]>> blobs;     // NUL-terminated strings back to back; a blob never moves once it is in
    std::vector<const char*> ptr;                   // id -> string
    std::vector<int64_t> len;
    int64_t bytes = 0;                              // sum of len
    std::unordered_set<std::string_view> index;     // for dge_names_add's duplicate check; built on the first add after an ingest appended names
    size_t indexed = 0;
};

// resident float32 [rows x dim], row-major, and one present byte per row: vec_read.hip makes it, sgns_io.hip (dge_model_load_vectors) and knn.hip read it
struct dge_vectors {
    int device = 0;
    int64_t rows = 0;
    int32_t dim = 0;
    dge_tmp<float> d = nullptr;
    dge_tmp<uint8_t> d_present = nullptr;
    int64_t n_present = 0;
};

// region rings with their cell index (trip_map.hip makes and reads it; spatial.hip reads the segments and keeps the centroids)
struct dge_regions {
    int device = 0;
    std::atomic<int> refs{1};
    int64_t R = 0, n_rings = 0, n_segs = 0, max_cand = 0;
    int32_t grid = 1;
    double box[4] = {0, 0, 0, 0};                // x0, y0, x1, y1
    double invx = 0, invy = 0;
    std::vector<int64_t> ids;
    double* d_seg = nullptr;                     // [n_segs][4]: ax ay bx by
    int64_t* d_seg_first = nullptr;              // [R + 1]
    double* d_box = nullptr;                     // [R][4]
    int64_t* d_cell_first = nullptr;             // [G*G + 1]
    int32_t* d_cand = nullptr;
    int32_t* d_idrank = nullptr;                 // region -> rank of its id
    int64_t* d_id_by_rank = nullptr;             // rank -> id
    // the regions' centroids (spatial.hip): computed on the device on first use and kept, on the device and on the host
    mutable std::mutex cent_mutex;               // the first use may come from several threads at once: the fill happens under it, once
    mutable bool cent_done = false;
    mutable double* d_cent = nullptr;            // [R][2]
    mutable std::vector<double> cent;
    ~dge_regions() { for (void* p : {(void*)d_seg, (void*)d_seg_first, (void*)d_box, (void*)d_cell_first, (void*)d_cand, (void*)d_idrank, (void*)d_id_by_rank, (void*)d_cent}) dge_dev_free(p); }
};

// the flow table of trip_map.hip as trip_text.hip needs it: the trips of a text gather in a table of their own over the same regions, merged at the end
int dge_flows_device(const dge_flows* f);
int dge_flows_like(const dge_flows* f, dge_flows** out);          // an empty table over f's regions
int dge_flows_merge(dge_flows* f, const dge_flows* part);          // part's table and counters into f; on error f is as it was

// the edges dge_flows_slot_edges gives for `slot`, restricted to the regions with a non-zero select byte (NULL: all) and re-indexed in ascending region index, as
// device entries (row = source, col = destination, val = weight) in no particular order; regions: the selected region indices, ascending (nmf.hip reads it)
int dge_flows_slot_coo(const dge_flows* f, int32_t T, int32_t mode, int32_t slot, const uint8_t* select, const char* who, dge_tmp<int32_t>& row, dge_tmp<int32_t>& col,
                       dge_tmp<double>& val, int64_t* n_entries, std::vector<int64_t>& regions);

// The two edge sources of the flow table as flow_text.hip takes them: the edges of dge_flows_slot_edges (trip_map.hip) and of dge_flows_window_edges
// (flow_windows.hip) as they stand on the device before the decode — the keys (slice * R + rank of the src id) * R + rank of the dst id, R = max(regions, 1),
// ascending, with their int64 weights; *n of them (0: the arrays may be null).  The two checks are those entries' own; kernel_ms is added to.
int dge_flows_slot_check(int32_t T, int32_t mode, const char* who);
int dge_flows_windows_check(const dge_hour_window* win, int32_t K, const char* who);
int dge_flows_slot_keys(const dge_flows* f, int32_t T, int32_t mode, const char* who, dge_tmp<uint64_t>& key, dge_tmp<int64_t>& w, int64_t* n, double* kernel_ms);
int dge_flows_window_keys(const dge_flows* f, const dge_hour_window* win, int32_t K, const char* who, dge_tmp<uint64_t>& key, dge_tmp<int64_t>& w, int64_t* n, double* kernel_ms);

int dge_graph_ensure_csr(dge_graph* g);
// The two ways another translation unit hands a graph its edges (graph.hip); neither can leave g half-way.
// The edges of n_vertices vertices as COO arrays of coo.n entries: g stands where dge_graph_add_edges and dge_graph_reserve_vertices would leave it.
void dge_graph_adopt_coo(dge_graph* g, dge_coo&& coo, int32_t n_vertices);
// the end state of keepNearestKVertices: the store becomes the given CSR with its recomputed outDegree, the tables are void, the sources' weights are refreshed
// (DoubleStream.sum(), no host-fixed sum).  dge_graph_keep_top_k ends in it; spatial.hip hands its edges over through it.  On error g is as it was.
int dge_graph_adopt_pruned(dge_graph* g, dge_csr&& csr);
// launches the strided walk kernel on `stream`; rows [row0,row0+n) of out (row length L)
int dge_launch_walks_strided(const dge_graph* g, hipStream_t stream, int32_t* d_out, int64_t n, int32_t L,
                             int64_t seed, int64_t first_index, int32_t* d_deadend_count);

// knn.hip's device form for other translation units: x [n x D] in device memory -> the k nearest other rows of every row (d_oi, d_od: [n x k]); d_present may be
// null; d_inv [n] and d_xn [n x 256] are scratch the caller owns.  k is bounded only by the strip kernel's LDS (DGE_ERR_ARG beyond it).  One host wait.
int dge_knn_device(const float* d_x, const uint8_t* d_present, int n, int D, int k, float* d_inv, float* d_xn, int32_t* d_oi, float* d_od, double* ms_kernel);
