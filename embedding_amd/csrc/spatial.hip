// spatial.hip — the spatial graph on the device (include/dge.h: dge_regions_centroids, dge_graph_add_spatial, dge_graph_add_spatial_points).
//
// Replaces SpatialGraph.constructGraph_tract / constructGraph_CA (J/SpatialGraph.java:37-88): the centroid of every region (J/Tracts.java:484-497), all R^2
// weights exp(-d * 100), addEdge R^2 times, keepNearestKVertices(10).  Here nothing of size R^2 exists: the weights are formed and the k best of a row are
// selected in one pass.  The arithmetic is that of spatial_weight.h, shared with the host harness.  Outside the build stamp.
//
//   k_sp_centroids     a lane per region walks the region's segments (resident since dge_regions_create: four doubles each, contiguous per region, rings in
//                      order): the chain of sums is sequential by definition.  R is small next to the R^2 of the next kernel.
//   k_sp_topk          a WAVE per row i, SP_ROWS rows per workgroup, so R = 801 rows are 51 264 lanes.  The centroids go through LDS in tiles of SP_TILE
//                      (16 bytes a centroid: one ds_read_b128 per lane, consecutive lanes on consecutive addresses), every tile read by all the workgroup's
//                      waves.  The wave scans the columns j in ascending order, 64 at a time.  Its running best-k under the key (w descending, j ascending)
//                      lives in registers, entry t on lane t (k <= 32): {w, j, dx*dx + dy*dy}.  A column whose squared distance is >= that of the current
//                      k-th entry cannot enter — E never rises with d, sqrt is monotone, and its j is the larger — and needs no E; after the first few
//                      tiles nearly all columns are of that kind.  The others evaluate E on their own lanes and are then inserted one by one in ascending j:
//                      the position is the count of entries with w >= the candidate's (ties go to the entry, whose j is smaller), the lanes behind it
//                      shift up by one.  Among the columns that reach it the insertion decides by the key itself.  What the filter leaves out is right
//                      ONLY BECAUSE E never rises as d grows (and the device sqrt is monotone): that property of the constants in spatial_weight.h is held
//                      by tests/test_spatial_host.py, and a refit of them has to pass that test again before this filter may stay.  The list does not
//                      depend on the chunk of 64 or on the tile
//                      either.  The row's k entries, its outDegree (DoubleStream.sum() over them in order, every lane running the same chain) and its row
//                      pointer leave in the form keepNearestKVertices leaves them.
// Selection is brute force: R^2 squared distances.  A spatial index would be needed to get below that for R in the millions.
//
// No float or double atomics: the two counters are integers.  Coherence: no protocol — every array is written by one kernel and read by later ones on the
// same stream.  Bounds: a wave writes row i < R only; lane t < k writes entry i*k + t of arrays of R*k; tile loads stop at R.
#include <algorithm>

#include "od_commit.h"
#include "spatial_weight.h"

constexpr int SP_TILE = 2048;                    // centroids one LDS tile holds: 32 KiB of the CU's 160
constexpr int SP_ROWS = SEQ_BLOCK / 64;          // rows (waves) of a workgroup
constexpr int32_t SP_MAX_K = 32;

// ------------------------------------------------------------------------------------------ kernels
__global__ void __launch_bounds__(SEQ_BLOCK) k_sp_centroids(const double* __restrict__ seg, const int64_t* __restrict__ seg_first, int64_t R, double* __restrict__ cent,
                                                            uint8_t* __restrict__ ok) {
    const int64_t r = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (r >= R) return;
    const int64_t s0 = seg_first[r];
    double x, y;
    ok[r] = (uint8_t)sw_centroid(seg + 4 * s0, seg_first[r + 1] - s0, &x, &y);
    cent[2 * r] = x; cent[2 * r + 1] = y;
}

__global__ void __launch_bounds__(SEQ_BLOCK) k_sp_topk(const double* __restrict__ cent, int64_t R, int32_t k, double scale, int64_t* __restrict__ row_ptr,
                                                       int32_t* __restrict__ nbr, double* __restrict__ w, double* __restrict__ outdeg, unsigned long long* counters) {
    __shared__ double2 tile[SP_TILE];
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * SP_ROWS + (threadIdx.x >> 6);
    const bool live = i < R;                                                // wave-uniform
    double xi = 0.0, yi = 0.0;
    if (live) { xi = cent[2 * i]; yi = cent[2 * i + 1]; }
    double ew = 0.0, ed2 = 0.0, thr = 0.0;                                  // entry `lane` of the row's list; thr: the k-th entry's squared distance once n == k
    int32_t ej = -1;
    int n = 0;
    unsigned long long evals = 0;
    for (int64_t t0 = 0; t0 < R; t0 += SP_TILE) {
        const int cnt = (int)min((int64_t)SP_TILE, R - t0);
        __syncthreads();                                                    // every wave is done with the tile before
        for (int c = threadIdx.x; c < cnt; c += SEQ_BLOCK) tile[c] = reinterpret_cast<const double2*>(cent)[t0 + c];
        __syncthreads();
        if (!live) continue;
        for (int c0 = 0; c0 < cnt; c0 += 64) {
            const int c = c0 + lane;
            bool cand = false;
            double d2 = 0.0;
            if (c < cnt) {
                const double2 p = tile[c];
                d2 = sw_dist2(xi, yi, p.x, p.y);
                cand = !(n == k && d2 >= thr);
            }
            uint64_t m = __ballot(cand);
            if (!m) continue;
            const double cw = cand ? sw_weight(d2, scale) : 0.0;
            evals += (unsigned long long)__popcll(m);
            while (m) {                                                     // ascending j
                const int s = __ffsll((unsigned long long)m) - 1;
                m &= m - 1;
                const double w_s = __shfl(cw, s), d2_s = __shfl(d2, s);
                const int pos = __popcll(__ballot(lane < n && ew >= w_s));  // entries in front of it: all of w >= its w (their j is smaller)
                if (pos >= k) continue;
                const double uw = __shfl_up(ew, 1), ud2 = __shfl_up(ed2, 1);
                const int32_t uj = __shfl_up(ej, 1);
                if (lane > pos && lane < k) { ew = uw; ed2 = ud2; ej = uj; }
                if (lane == pos) { ew = w_s; ed2 = d2_s; ej = (int32_t)(t0 + c0 + s); }
                if (n < k) n++;
                if (n == k) thr = __shfl(ed2, k - 1);
            }
        }
    }
    if (!live) return;
    // R >= k: the list is full.  Entry t leaves from lane t; the compensated sum is a chain, run by every lane on the same values
    if (lane < k) { nbr[i * k + lane] = ej; w[i * k + lane] = ew; }
    double sum = 0.0, comp = 0.0, simple = 0.0;
    for (int t = 0; t < k; t++) {
        const double x = __shfl(ew, t);
        const double tmp = x - comp;
        const double velvel = sum + tmp;
        comp = (velvel - sum) - tmp;
        sum = velvel;
        simple += x;
    }
    const double tmp = sum + comp;
    const double od = (tmp != tmp && (simple - simple) != 0.0 && simple == simple) ? simple : tmp;      // dge_java8_stream_sum (dge_algos.h)
    const int zeros = __popcll(__ballot(lane < k && ew == 0.0));
    if (lane == 0) {
        outdeg[i] = od;
        row_ptr[i] = i * (int64_t)k;
        if (i == R - 1) row_ptr[R] = R * (int64_t)k;
        atomicAdd(counters, evals);
        if (zeros) atomicAdd(counters + 1, (unsigned long long)zeros);
    }
}

// ------------------------------------------------------------------------------------------ host side
namespace {

// the centroids of rg, on the device and on the host, computed once (under the handle's mutex: a handle may be shared by threads)
int sp_centroids(const dge_regions* rg, const char* who) {
    std::lock_guard<std::mutex> once(rg->cent_mutex);
    if (rg->cent_done) return DGE_OK;
    const int64_t R = rg->R;
    if (R == 0) { rg->cent_done = true; return DGE_OK; }
    SEQ_TRY(dge_require_device(rg->device));
    SeqRun Rn;
    SEQ_TRY(seq_open(Rn, rg->device, who));
    dge_tmp<double> cent;
    dge_tmp<uint8_t> ok;
    SEQ_TRY(seq_alloc(Rn, cent, 2 * R, "the centroids"));
    SEQ_TRY(seq_alloc(Rn, ok, R, "the centroids' flags"));
    SEQ_TRY(seq_kernels_begin(Rn));
    hipLaunchKernelGGL(k_sp_centroids, dim3(seq_grid(R)), dim3(SEQ_BLOCK), 0, Rn.stream, rg->d_seg, rg->d_seg_first, R, cent.p, ok.p);
    SEQ_TRY(seq_kernels_end(Rn));
    DGE_HIP(hipGetLastError());
    std::vector<double> host((size_t)(2 * R));
    std::vector<uint8_t> flags((size_t)R);
    SEQ_TRY(seq_read_back(Rn, host.data(), cent.p, (size_t)(2 * R) * sizeof(double)));
    SEQ_TRY(seq_read_back(Rn, flags.data(), ok.p, (size_t)R));
    for (int64_t r = 0; r < R; r++)
        if (!flags[(size_t)r])
            DGE_FAIL(DGE_ERR_ARG, "%s: region %lld (id %lld) has no centroid: the area sum of its rings is 0, or the centroid is not finite", who, (long long)r,
                     (long long)rg->ids[(size_t)r]);
    rg->d_cent = cent.release(); rg->cent = std::move(host); rg->cent_done = true;
    return DGE_OK;
}

// what both graph entries check before a device is looked for, in this order; g last: a machine without a device has no graph to offer
int sp_check(const dge_graph* g, int32_t k, double scale, const dge_names* names, const char* who) {
    if (k < 1 || k > SP_MAX_K) DGE_FAIL(DGE_ERR_ARG, "%s: k = %d is outside 1 .. %d", who, k, SP_MAX_K);
    if (!(scale > 0.0) || (scale - scale) != 0.0) DGE_FAIL(DGE_ERR_ARG, "%s: scale = %g must be finite and > 0", who, scale);
    if (names && !names->ptr.empty()) DGE_FAIL(DGE_ERR_ARG, "%s: names must be empty: it receives the vertex names, it holds %lld", who, (long long)names->ptr.size());
    if (!g) DGE_FAIL(DGE_ERR_ARG, "%s: null graph", who);
    return od_check(g, names, who);                // fresh, as the .od reader asks
}

// d_cent: R centroids on g's device.  On success g stands where a host stands after add_edges of all R^2 weights, keep_top_k(k) and set_sources(0 .. R-1, 1).
int sp_build(dge_graph* g, const double* d_cent, const int64_t* ids, int64_t R, int32_t k, double scale, dge_names* names, dge_spatial_info* info, const char* who) {
    if (info) *info = dge_spatial_info{};
    if (R > 0 && k > R)
        DGE_FAIL(DGE_ERR_TOPK, "%s: keepNearestKVertices(%d): a vertex has only %lld out-edges (the reference throws IndexOutOfBoundsException)", who, k, (long long)R);
    if (R > 0x7fffffffLL || R * (int64_t)k >= (int64_t)0xFFFFFFFFLL)
        DGE_FAIL(DGE_ERR_RANGE, "%s: %lld regions with %d edges each do not fit the store (int32 vertex ids, fewer than 2^32 edges)", who, (long long)R, k);
    if (R == 0) return dge_graph_set_sources(g, nullptr, 0, 1);            // an empty graph, as the three calls leave it
    DGE_HIP(hipSetDevice(g->device));
    SeqRun Rn;
    SEQ_TRY(seq_open(Rn, g->device, who));
    const int64_t E = R * (int64_t)k;
    dge_csr csr;
    csr.V = (int32_t)R; csr.E = E;
    dge_tmp<unsigned long long> counters;
    SEQ_TRY(seq_alloc(Rn, csr.row_ptr, R + 1, "the row pointers"));
    SEQ_TRY(seq_alloc(Rn, csr.nbr, E, "the edges' destinations"));
    SEQ_TRY(seq_alloc(Rn, csr.w, E, "the edges' weights"));
    SEQ_TRY(seq_alloc(Rn, csr.outdeg, R, "the out-degrees"));
    SEQ_TRY(seq_alloc(Rn, counters, 2, "the counters"));
    DGE_HIP(hipMemsetAsync(counters.p, 0, 2 * sizeof(unsigned long long), Rn.stream));
    SEQ_TRY(seq_kernels_begin(Rn));
    hipLaunchKernelGGL(k_sp_topk, dim3((unsigned)((R + SP_ROWS - 1) / SP_ROWS)), dim3(SEQ_BLOCK), 0, Rn.stream, d_cent, R, k, scale, csr.row_ptr.p, csr.nbr.p, csr.w.p, csr.outdeg.p, counters.p);
    SEQ_TRY(seq_kernels_end(Rn));
    DGE_HIP(hipGetLastError());
    unsigned long long c[2] = {0, 0};
    SEQ_TRY(seq_read_back(Rn, c, counters.p, sizeof(c)));

    // ---- the names: the decimal region ids in vertex order
    std::vector<int64_t> off;
    std::unique_ptr<char[]> name_blob;
    if (names) {
        std::string all;
        off.reserve((size_t)R + 1);
        char one[32];
        for (int64_t r = 0; r < R; r++) {
            off.push_back((int64_t)all.size());
            const int len = snprintf(one, sizeof(one), "%lld", (long long)ids[r]);
            all.append(one, (size_t)len + 1);
        }
        off.push_back((int64_t)all.size());
        name_blob.reset(new char[all.size() + 1]);
        memcpy(name_blob.get(), all.data(), all.size());
    }
    std::vector<int32_t> srcv((size_t)R);
    for (int64_t r = 0; r < R; r++) srcv[(size_t)r] = (int32_t)r;

    // ---- the graph takes the edges over in the state keep_top_k leaves (dge_graph_adopt_pruned), then the sources
    int rc = dge_graph_adopt_pruned(g, std::move(csr));           // (a fresh graph may hold an empty CSR from a read-back: it goes)
    if (!rc) rc = dge_graph_set_sources(g, srcv.data(), R, 1);
    if (rc) { dge_graph_reset(g); return rc; }
    // nothing can fail from here on
    if (names) names_append(names, std::move(name_blob), off.data(), R);
    if (info) { info->regions = R; info->edges = E; info->weights = (int64_t)c[0]; info->zero_weights = (int64_t)c[1]; info->kernel_ms = Rn.kernel_ms; }
    return DGE_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------ entries
extern "C" int dge_regions_centroids(const dge_regions* rg, double* xy, int64_t cap, int64_t* n) {
    const char* who = "dge_regions_centroids";
    if (!rg || !n || cap < 0 || (cap > 0 && !xy)) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    *n = rg->R;
    if (cap < rg->R) DGE_FAIL(DGE_ERR_CAP, "%s: %lld regions exceed cap %lld", who, (long long)rg->R, (long long)cap);
    SEQ_TRY(sp_centroids(rg, who));
    if (rg->R) memcpy(xy, rg->cent.data(), (size_t)(2 * rg->R) * sizeof(double));
    return DGE_OK;
}

extern "C" int dge_graph_add_spatial(dge_graph* g, const dge_regions* rg, int32_t k, double scale, dge_names* names, dge_spatial_info* info) {
    const char* who = "dge_graph_add_spatial";
    SEQ_TRY(sp_check(g, k, scale, names, who));
    if (!rg) DGE_FAIL(DGE_ERR_ARG, "%s: null regions", who);
    if (g->device != rg->device) DGE_FAIL(DGE_ERR_ARG, "%s: the graph is on device %d, the regions on device %d", who, g->device, rg->device);
    SEQ_TRY(sp_centroids(rg, who));
    return sp_build(g, rg->d_cent, rg->ids.data(), rg->R, k, scale, names, info, who);
}

extern "C" int dge_graph_add_spatial_points(dge_graph* g, const int64_t* ids, const double* xy, int64_t R, int32_t k, double scale, dge_names* names, dge_spatial_info* info) {
    const char* who = "dge_graph_add_spatial_points";
    if (R < 0 || (R > 0 && (!ids || !xy))) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    for (int64_t r = 0; r < R; r++)
        if ((xy[2 * r] - xy[2 * r]) != 0.0 || (xy[2 * r + 1] - xy[2 * r + 1]) != 0.0)
            DGE_FAIL(DGE_ERR_ARG, "%s: point %lld (id %lld) is not finite", who, (long long)r, (long long)ids[r]);
    {
        std::vector<int64_t> sorted(ids, ids + R);
        std::sort(sorted.begin(), sorted.end());
        for (int64_t r = 1; r < R; r++)
            if (sorted[(size_t)r] == sorted[(size_t)r - 1]) DGE_FAIL(DGE_ERR_ARG, "%s: region id %lld occurs twice: ids must be distinct", who, (long long)sorted[(size_t)r]);
    }
    SEQ_TRY(sp_check(g, k, scale, names, who));
    if (R > 0 && k > R) return sp_build(g, nullptr, ids, R, k, scale, names, info, who);      // DGE_ERR_TOPK: nothing to upload
    DGE_HIP(hipSetDevice(g->device));
    dge_tmp<double> d_cent;
    SEQ_TRY(d_cent.alloc((size_t)(2 * R)));
    if (R) DGE_HIP(hipMemcpy(d_cent.p, xy, (size_t)(2 * R) * sizeof(double), hipMemcpyHostToDevice));
    return sp_build(g, d_cent.p, ids, R, k, scale, names, info, who);
}
