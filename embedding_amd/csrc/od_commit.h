// od_commit.h — the commit path that od_read.hip (.od text) and trip_map.hip (dge_graph_add_flows) share: flows with their ids, weights and slices already on the
// device become the layered graph.  Flow r of `rows` is kept when keepx[r + 1] != keepx[r] and is then edge keepx[r] (keepx: an exclusive scan of the keep
// flags, rows + 1 entries); E = keepx[rows].  The passes are those listed at the head of od_read.hip from k_od_endpoints on: the kept endpoints sorted and
// made unique (the R regions, ascending as signed 64-bit integers), k_od_edges (rank by binary search, edge h*R + rank(src) -> ((h + 1) % T)*R + rank(dst),
// the layer-0 marks), k_od_sources, the names "<h>-<region id>", and the hand-over to the graph (edges, reserved vertices, dge_graph_set_sources).
// Everything is static, as in seq_tokens.h: each translation unit gets its own copy and the library exports nothing from here.  Outside the build stamp.
#pragma once

#include "seq_tokens.h"

// the ids of the kept flows' endpoints: edge e's at [2e], [2e + 1]
static __global__ void __launch_bounds__(SEQ_BLOCK) k_od_endpoints(const int64_t* src_id, const int64_t* dst_id, const int64_t* keepx, int64_t rows, int64_t* ends) {
    const int64_t r = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (r >= rows || keepx[r + 1] == keepx[r]) return;
    const int64_t e = keepx[r];
    ends[2 * e] = src_id[r]; ends[2 * e + 1] = dst_id[r];
}

struct OdNewFlag { const int64_t* sorted; int64_t n; __device__ int64_t operator()(int64_t i) const { return (i < n && (i == 0 || sorted[i] != sorted[i - 1])) ? 1 : 0; } };

static __global__ void __launch_bounds__(SEQ_BLOCK) k_od_unique(const int64_t* sorted, const int64_t* newx, int64_t n, int64_t* regions) {
    const int64_t i = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (i < n && newx[i + 1] != newx[i]) regions[newx[i]] = sorted[i];
}

static __device__ __forceinline__ int64_t od_rank(const int64_t* regions, int64_t R, int64_t id) {      // id is among the regions
    int64_t lo = 0, hi = R;
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (regions[mid] <= id) lo = mid; else hi = mid; }
    return lo;
}

// kept flow r of slice h -> edge keepx[r]: h*R + rank(src) -> ((h + 1) % T)*R + rank(dst); mark[i] = 1 for every layer-0 vertex i that is an endpoint
static __global__ void __launch_bounds__(SEQ_BLOCK) k_od_edges(const int64_t* src_id, const int64_t* dst_id, const uint64_t* w_bits, const int32_t* slice, const int64_t* keepx,
                                                        int64_t rows, const int64_t* regions, int64_t R, int64_t T, int32_t* coo_src, int32_t* coo_dst, double* coo_w,
                                                        uint8_t* mark) {
    const int64_t r = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (r >= rows || keepx[r + 1] == keepx[r]) return;
    const int64_t e = keepx[r], h = slice[r], h1 = h + 1 == T ? 0 : h + 1;
    const int64_t rs = od_rank(regions, R, src_id[r]), rd = od_rank(regions, R, dst_id[r]);
    coo_src[e] = (int32_t)(h * R + rs);
    coo_dst[e] = (int32_t)(h1 * R + rd);
    coo_w[e] = __longlong_as_double((long long)w_bits[r]);
    if (h == 0) mark[rs] = 1;
    if (h1 == 0) mark[rd] = 1;
}

static __global__ void __launch_bounds__(SEQ_BLOCK) k_od_sources(const int64_t* markx, int64_t R, int32_t* srcv) {
    const int64_t i = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (i < R && markx[i + 1] != markx[i]) srcv[markx[i]] = (int32_t)i;
}

namespace {

// On success g holds the graph, names (may be NULL) the T*Rn vertex names, *n_regions = Rn and *n_sources = S.  On error g and names are as they were.
[[maybe_unused]] int od_commit(SeqRun& R, dge_graph* g, dge_names* names, int64_t rows, int64_t E, int64_t T, const int64_t* src_id, const int64_t* dst_id, const uint64_t* w_bits,
                              const int32_t* slice, const int64_t* keepx, const char* who, int64_t* n_regions_out, int64_t* n_sources_out) {
    // ---- the regions: the kept endpoints' ids, sorted, each once
    int64_t n_regions = 0;
    dge_tmp<int64_t> regions;
    {
        dge_tmp<int64_t> ends, sorted, newx;
        SEQ_TRY(seq_alloc(R, ends, 2 * E, "the endpoints"));
        SEQ_TRY(seq_alloc(R, sorted, 2 * E, "the sorted endpoints"));
        SEQ_TRY(seq_alloc(R, newx, 2 * E + 1, "the regions' numbers"));
        SeqScratch tmp{R, "the sort's scratch", true};
        void* none = nullptr;
        auto tmp_then_ends = [&](size_t bytes, void** p) -> int {       // the sort's input is made once the clock runs
            SEQ_TRY(tmp(bytes, p));
            hipLaunchKernelGGL(k_od_endpoints, dim3(seq_grid(rows)), dim3(SEQ_BLOCK), 0, R.stream, src_id, dst_id, keepx, rows, ends.p);
            return DGE_OK;
        };
        if (E) SEQ_TRY(dge_sort_keys(tmp_then_ends, ends.p, sorted.p, 2 * E, 64, R.stream, false));
        else SEQ_TRY(tmp(0, &none));
        SEQ_TRY(seq_scan(R, rocprim::make_transform_iterator(rocprim::counting_iterator<int64_t>(0), OdNewFlag{sorted.p, 2 * E}), newx.p, 2 * E + 1));
        SEQ_TRY(seq_kernels_end(R));
        SEQ_TRY(seq_read_back(R, &n_regions, newx.p + 2 * E, 8));
        if (T * n_regions > 0x7fffffffLL)
            DGE_FAIL(DGE_ERR_RANGE, "%s: %lld slices of %lld regions are %lld vertices, which do not fit int32 ids", who, (long long)T, (long long)n_regions, (long long)(T * n_regions));
        SEQ_TRY(seq_alloc(R, regions, n_regions, "the regions"));
        SEQ_TRY(seq_kernels_begin(R));
        if (E) hipLaunchKernelGGL(k_od_unique, dim3(seq_grid(2 * E)), dim3(SEQ_BLOCK), 0, R.stream, sorted.p, newx.p, 2 * E, regions.p);
        SEQ_TRY(seq_kernels_end(R));
        seq_release(R, ends, 2 * E); seq_release(R, sorted, 2 * E); seq_release(R, newx, 2 * E + 1); tmp.release();
    }
    const int64_t Rn = n_regions;

    // ---- the edges into the graph's own staging, the layer-0 endpoints
    dge_coo coo;
    dge_tmp<int32_t> srcv;
    dge_tmp<uint8_t> mark;
    dge_tmp<int64_t> markx;
    SEQ_TRY(seq_alloc(R, coo.src, E, "the edges' sources"));
    SEQ_TRY(seq_alloc(R, coo.dst, E, "the edges' destinations"));
    SEQ_TRY(seq_alloc(R, coo.w, E, "the edges' weights"));
    SEQ_TRY(seq_alloc(R, mark, Rn, "the layer-0 vertices"));
    SEQ_TRY(seq_alloc(R, markx, Rn + 1, "the layer-0 vertices' numbers"));
    SEQ_TRY(seq_kernels_begin(R));
    DGE_HIP(hipMemsetAsync(mark.p, 0, (size_t)std::max<int64_t>(Rn, 1), R.stream));
    if (E) hipLaunchKernelGGL(k_od_edges, dim3(seq_grid(rows)), dim3(SEQ_BLOCK), 0, R.stream, src_id, dst_id, w_bits, slice, keepx, rows, regions.p, Rn, T, coo.src.p, coo.dst.p,
                              coo.w.p, mark.p);
    SEQ_TRY(seq_scan(R, rocprim::make_transform_iterator(rocprim::counting_iterator<int64_t>(0), SeqByteFlag{mark.p, Rn}), markx.p, Rn + 1));
    SEQ_TRY(seq_kernels_end(R));
    int64_t S = 0;
    SEQ_TRY(seq_read_back(R, &S, markx.p + Rn, 8));
    SEQ_TRY(seq_alloc(R, srcv, S, "the sources"));
    SEQ_TRY(seq_kernels_begin(R));
    if (Rn) hipLaunchKernelGGL(k_od_sources, dim3(seq_grid(Rn)), dim3(SEQ_BLOCK), 0, R.stream, markx.p, Rn, srcv.p);
    SEQ_TRY(seq_kernels_end(R));
    std::vector<int64_t> host_regions((size_t)Rn);
    std::vector<int32_t> host_srcv((size_t)S);
    if (Rn) SEQ_TRY(seq_read_back(R, host_regions.data(), regions.p, (size_t)Rn * 8));
    if (S) SEQ_TRY(seq_read_back(R, host_srcv.data(), srcv.p, (size_t)S * 4));
    DGE_HIP(hipStreamSynchronize(R.stream));
    DGE_HIP(hipGetLastError());

    // ---- the names "<h>-<region id>" in vertex-id order: the host formats them, R is small against E
    std::vector<int64_t> off;
    std::unique_ptr<char[]> name_blob;
    if (names) {
        std::string all;
        off.reserve((size_t)(T * Rn) + 1);
        char one[48];
        for (int64_t h = 0; h < T; h++)
            for (int64_t i = 0; i < Rn; i++) {
                off.push_back((int64_t)all.size());
                const int len = snprintf(one, sizeof(one), "%lld-%lld", (long long)h, (long long)host_regions[(size_t)i]);
                all.append(one, (size_t)len + 1);
            }
        off.push_back((int64_t)all.size());
        name_blob.reset(new char[all.size() + 1]);
        memcpy(name_blob.get(), all.data(), all.size());
    }

    // ---- the graph takes the edges over, then stands where a host stands after add_edges, reserve_vertices and set_sources
    coo.n = E; coo.cap = std::max<int64_t>(E, 1);
    dge_graph_adopt_coo(g, std::move(coo), (int32_t)(T * Rn));      // (a fresh graph may hold an empty CSR from a read-back: it goes, set_sources builds the real one)
    const int rc = dge_graph_set_sources(g, host_srcv.data(), S, 0);
    if (rc) { dge_graph_reset(g); return rc; }
    // nothing can fail from here on
    g->od_regions = std::move(host_regions);
    if (names && T * Rn > 0) names_append(names, std::move(name_blob), off.data(), T * Rn);
    *n_regions_out = Rn; *n_sources_out = S;
    return DGE_OK;
}

// what both entries check before a device is looked for (the pieces' own arguments are the caller's)
[[maybe_unused]] int od_check(const dge_graph* g, const dge_names* names, const char* who) {
    if (names && !names->ptr.empty()) DGE_FAIL(DGE_ERR_ARG, "%s: names must be empty: it receives the vertex names, it holds %lld", who, (long long)names->ptr.size());
    if (!dge_graph_fresh(g)) DGE_FAIL(DGE_ERR_STATE, "%s: the graph must be fresh: it already holds edges, sources or reserved vertices", who);
    return DGE_OK;
}

}  // namespace
