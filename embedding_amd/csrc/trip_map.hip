// trip_map.hip — trips into regions, regions into flows, flows into the layered graph (include/dge.h: dge_regions_*, dge_flows_*, dge_graph_add_flows).
//
// The stage in front of the .od files: Tracts.mapTripsIntoTracts (J/Tracts.java:71-102) and CommunityAreas.mapTripsIntoCommunities
// (J/CommunityAreas.java:55-103) test every trip's two points with MultiPolygon.contains against every region and count taxiFlows[hour][dst].  Here the
// regions' rings are resident with a uniform cell index, points are located by the exact ray-crossing rule of pip_exact.h, and the flows are a sorted
// table of (hour, s, e) -> count kept on the device.  Outside the build stamp: nothing here is read or written by a training launch.
//
// The index (built once on the host in dge_regions_create; R is hundreds, the points are 1e8): G x G cells over the bounding box of all rings, cell c lists
// the regions whose box meets it, ascending.  pip_cell is the one function that gives a coordinate its cell, for the lists and for the points, and it is
// monotone: a point inside a region's box lies inside that region's cell range.  A listed region is tested only when its box contains the point, so the set
// of side tests — and the counter `exact` — does not depend on G.
//
// Locating a chunk of points:
//   k_trip_keys        the point's cell, or the key behind the last cell when it is outside the domain or the index's box (region -1 at once)
//   radix sort         (cell, point) pairs; k_trip_bounds gives every cell its run by binary search; a scan of ceil(run / 256) numbers the workgroups
//   k_trip_locate      a workgroup = 256 points of ONE cell.  For every listed region some lane needs, the region's segments (four doubles each, contiguous per
//                      region) go through LDS in tiles of TRIP_TILE; every lane runs the same loop over the tile for its own point (all lanes read the same
//                      LDS address: a broadcast), keeping a crossing parity and a boundary flag for the (point, region) at hand.  The loop bounds and the
//                      barriers depend on the cell and the region only, never on a lane.  Results go back to the points' own positions.
// Counters are integers added with atomicAdd after a block reduction: their values do not depend on the order.
//
// Flows of a chunk of trips: both points located, key (hour*R + s)*R + e per mapped trip, radix sort, run lengths by reduce-by-key, then merged with the
// resident table (concatenate, sort pairs, reduce by key).  Counts are int64; nothing is floating point, nothing depends on order.
// Slot edges: every table entry emits its contribution(s) keyed by (slot, rank of ids[s], rank of ids[e]); sort, reduce by key, decode.  DGE_SLOTS_AS_TRACTS
// looks the entry (k, s, e) of the window's first hour up by binary search in the sorted table.
// dge_graph_add_flows hands the slot edges to od_commit.h — the commit path of od_read.hip.
//
// Coherence: no protocol.  Every array is written by one kernel and read by later ones on the same stream.
#include "od_commit.h"
#include "pip_exact.h"
#include "trip_flows.h"                          // the table itself and the passes shared with flow_windows.hip

constexpr int TRIP_TILE = 1024;                  // segments one LDS tile holds: 32 KiB of the CU's 160
constexpr int64_t TRIP_CHUNK = (int64_t)1 << 24; // points (or trips) taken at a time
constexpr int32_t TRIP_MAX_GRID = 4096;

// ------------------------------------------------------------------------------------------ kernels
struct TripIndex { double x0, y0, x1, y1, invx, invy; int32_t G; int32_t has; };

__global__ void __launch_bounds__(SEQ_BLOCK) k_trip_keys(const double* xy, int64_t n, TripIndex ix, uint32_t* key, uint32_t* idx, int32_t* region, unsigned long long* counters) {
    const int64_t i = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    unsigned long long v[1] = {0};
    if (i < n) {
        const double x = xy[2 * i], y = xy[2 * i + 1];
        const bool in = ix.has && pip_in_domain(x) && pip_in_domain(y) && x >= ix.x0 && x <= ix.x1 && y >= ix.y0 && y <= ix.y1;
        const uint32_t cells = (uint32_t)ix.G * (uint32_t)ix.G;
        key[i] = in ? (uint32_t)pip_cell(y, ix.y0, ix.invy, ix.G) * (uint32_t)ix.G + (uint32_t)pip_cell(x, ix.x0, ix.invx, ix.G) : cells;
        idx[i] = (uint32_t)i;
        if (!in) { region[i] = -1; v[0] = 1; }
    }
    const int which[1] = {TC_OUTSIDE};
    trip_count(v, which, counters);
}

// cell_start[c] = the first sorted position whose key is >= c, c = 0 .. cells
__global__ void __launch_bounds__(SEQ_BLOCK) k_trip_bounds(const uint32_t* key, int64_t n, int64_t cells, int64_t* cell_start) {
    const int64_t c = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (c > cells) return;
    cell_start[c] = coo_lower_bound(key, n, (uint32_t)c);
}

struct TripBlocks { const int64_t* cell_start; int64_t cells; __device__ int64_t operator()(int64_t c) const { return c < cells ? (cell_start[c + 1] - cell_start[c] + SEQ_BLOCK - 1) / SEQ_BLOCK : 0; } };

__global__ void __launch_bounds__(SEQ_BLOCK) k_trip_locate(const double* xy, const uint32_t* idx, const int64_t* cell_start, const int64_t* blk_first, int64_t cells,
                                                           const int64_t* cell_first, const int32_t* cand, const double* box, const int64_t* seg_first, const double* seg,
                                                           int32_t* region, unsigned long long* counters) {
    __shared__ double tile[TRIP_TILE * 4];
    __shared__ int64_t s_cell;
    const int64_t b = blockIdx.x;
    if (threadIdx.x == 0) {                      // the last cell whose first workgroup is <= b: the one that owns b (cells without points own none)
        int64_t lo = 0, hi = cells;
        while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (blk_first[mid] <= b) lo = mid; else hi = mid; }
        s_cell = lo;
    }
    __syncthreads();
    const int64_t c = s_cell;
    const int64_t at = cell_start[c] + (b - blk_first[c]) * SEQ_BLOCK + threadIdx.x;
    const bool valid = at < cell_start[c + 1];
    const int64_t i = valid ? (int64_t)idx[at] : 0;
    const double px = valid ? xy[2 * i] : 0.0, py = valid ? xy[2 * i + 1] : 0.0;
    int32_t result = -1;
    int n_interior = 0, any_boundary = 0, in_any = 0;
    unsigned long long exact = 0;
    const int64_t k0 = cell_first[c], k1 = cell_first[c + 1];
    for (int64_t k = k0; k < k1; k++) {
        const int32_t r = cand[k];
        const double* bx = box + 4 * (int64_t)r;
        const int mine = valid && px >= bx[0] && px <= bx[2] && py >= bx[1] && py <= bx[3];
        if (!__syncthreads_or(mine)) continue;   // (a barrier as well: the last tile has been read by every lane)
        pip_state st = {0, 0, 0};
        const int64_t s0 = seg_first[r], s1 = seg_first[r + 1];
        for (int64_t t0 = s0; t0 < s1; t0 += TRIP_TILE) {
            const int cnt = (int)(s1 - t0 < TRIP_TILE ? s1 - t0 : TRIP_TILE);
            if (t0 > s0) __syncthreads();
            for (int q = threadIdx.x; q < cnt * 4; q += SEQ_BLOCK) tile[q] = seg[t0 * 4 + q];
            __syncthreads();
            if (mine)
                for (int j = 0; j < cnt; j++) pip_step(tile[4 * j], tile[4 * j + 1], tile[4 * j + 2], tile[4 * j + 3], px, py, &st);
        }
        if (mine) {
            in_any = 1;
            exact += st.exact;
            if (st.boundary) any_boundary = 1;
            else if (st.parity) { if (result < 0) result = r; n_interior++; }
        }
    }
    if (valid) region[i] = result;
    __syncthreads();
    unsigned long long v[5] = {valid && result >= 0 ? 1ull : 0ull, valid && result < 0 && any_boundary ? 1ull : 0ull, n_interior > 1 ? 1ull : 0ull, valid && !in_any ? 1ull : 0ull, exact};
    const int which[5] = {TC_LOCATED, TC_BOUNDARY, TC_MULTI, TC_OUTSIDE, TC_EXACT};
    trip_count(v, which, counters);
}

// a trip is bad when its hour is outside 0 .. 23 or a coordinate is outside the domain; mapped when both regions are found
__global__ void __launch_bounds__(SEQ_BLOCK) k_flow_keys(const double* sxy, const double* exy, const int32_t* hour, const int32_t* rs, const int32_t* re, int64_t n, uint64_t R,
                                                         uint64_t* key, unsigned long long* counters) {
    const int64_t i = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    unsigned long long v[4] = {0, 0, 0, 0};
    if (i < n) {
        const int32_t h = hour[i];
        const bool bad = h < 0 || h > 23 || !pip_in_domain(sxy[2 * i]) || !pip_in_domain(sxy[2 * i + 1]) || !pip_in_domain(exy[2 * i]) || !pip_in_domain(exy[2 * i + 1]);
        const int32_t s = rs[i], e = re[i];
        uint64_t k = ~0ull;
        if (bad) v[1] = 1;
        else if (s < 0) v[2] = 1;
        else if (e < 0) v[3] = 1;
        else { v[0] = 1; k = ((uint64_t)h * R + (uint64_t)s) * R + (uint64_t)e; }
        key[i] = k;
    }
    const int which[4] = {TC_MAPPED, TC_BAD, TC_NO_START, TC_NO_END};
    trip_count(v, which, counters);
}

// item t = (entry t / step, j = t % step).  DGE_SLOTS_EVEN (step 1): slot hour / width.  DGE_SLOTS_AS_TRACTS: slot k = hour - j, when 0 <= k < T and the table
// holds (k, s, e) — "only destinations seen in hour k itself".  An item that counts nowhere gets the key behind all others.
__global__ void __launch_bounds__(SEQ_BLOCK) k_slot_items(const uint64_t* key, const int64_t* cnt, int64_t n, uint64_t R, int32_t T, int32_t mode, int32_t step, int32_t width,
                                                          const int32_t* idrank, uint64_t* item_key, int64_t* item_w, unsigned long long* counters) {
    const int64_t t = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    unsigned long long v[1] = {0};
    if (t < n * step) {
        const int64_t i = t / step;
        const int32_t j = (int32_t)(t % step);
        const uint64_t kk = key[i], e = kk % R, s = (kk / R) % R;
        const int32_t h = (int32_t)(kk / R / R);
        int32_t slot = mode == DGE_SLOTS_EVEN ? h / width : h - j;
        bool ok = slot >= 0 && slot < T;
        if (ok && j > 0) {
            const uint64_t want = ((uint64_t)slot * R + s) * R + e;
            const int64_t lo = coo_lower_bound(key, n, want);
            ok = lo < n && key[lo] == want;
        }
        item_key[t] = ok ? ((uint64_t)slot * R + (uint64_t)idrank[s]) * R + (uint64_t)idrank[e] : ~0ull;
        item_w[t] = ok ? cnt[i] : 0;
        v[0] = ok ? 1 : 0;
    }
    const int which[1] = {TC_VALID};
    trip_count(v, which, counters);
}

// the slot's edges inside a selection as matrix entries: map[rank] = the compact index of the region of that rank, or -1.  The positions come from a counter:
// the order of the entries is of no account to their reader, which sorts them
__global__ void __launch_bounds__(SEQ_BLOCK) k_slot_coo(const uint64_t* key, const int64_t* w, int64_t n, uint64_t R, int32_t slot, const int32_t* map, int32_t* row, int32_t* col,
                                                        double* val, unsigned long long* count) {
    const int64_t i = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = key[i];
    if ((int32_t)(k / R / R) != slot) return;
    const int32_t a = map[(k / R) % R], b = map[k % R];
    if (a < 0 || b < 0) return;
    const unsigned long long at = atomicAdd(count, 1ULL);
    row[at] = a; col[at] = b; val[at] = (double)w[i];
}

// ------------------------------------------------------------------------------------------ host side
namespace {

template <typename T>
int trip_upload(SeqRun& R, T** dst, const T* src, int64_t n, const char* what) {
    dge_tmp<T> t;
    SEQ_TRY(seq_alloc(R, t, n, what));
    if (n) DGE_HIP(hipMemcpyAsync(t.p, src, (size_t)n * sizeof(T), hipMemcpyHostToDevice, R.stream));
    DGE_HIP(hipStreamSynchronize(R.stream));
    *dst = t.release();
    return DGE_OK;
}

// regions of n <= TRIP_CHUNK points already on the device; the counters (device, TC_N words) are added to
int trip_locate(SeqRun& R, const dge_regions* rg, const double* d_xy, int64_t n, int32_t* d_region, unsigned long long* d_counters) {
    if (n == 0) return DGE_OK;
    const int64_t cells = (int64_t)rg->grid * rg->grid;
    const TripIndex ix = {rg->box[0], rg->box[1], rg->box[2], rg->box[3], rg->invx, rg->invy, rg->grid, rg->R > 0 ? 1 : 0};
    dge_tmp<uint32_t> key, idx, key2, idx2;
    dge_tmp<int64_t> cell_start, blk_first;
    SEQ_TRY(seq_alloc(R, key, n, "the points' cells"));
    SEQ_TRY(seq_alloc(R, idx, n, "the points' numbers"));
    SEQ_TRY(seq_alloc(R, key2, n, "the sorted cells"));
    SEQ_TRY(seq_alloc(R, idx2, n, "the sorted points"));
    SEQ_TRY(seq_alloc(R, cell_start, cells + 1, "the cells' runs"));
    SEQ_TRY(seq_alloc(R, blk_first, cells + 1, "the cells' workgroups"));
    SeqScratch tmp{R, "the sort's scratch", true};
    auto tmp_then_keys = [&](size_t bytes, void** p) -> int {           // the sort's input is made once the clock runs
        SEQ_TRY(tmp(bytes, p));
        hipLaunchKernelGGL(k_trip_keys, dim3(seq_grid(n)), dim3(SEQ_BLOCK), 0, R.stream, d_xy, n, ix, key.p, idx.p, d_region, d_counters);
        return DGE_OK;
    };
    SEQ_TRY(dge_sort_pairs(tmp_then_keys, key.p, key2.p, idx.p, idx2.p, n, dge_bits((uint64_t)cells), R.stream, false));
    hipLaunchKernelGGL(k_trip_bounds, dim3(seq_grid(cells + 1)), dim3(SEQ_BLOCK), 0, R.stream, key2.p, n, cells, cell_start.p);
    SEQ_TRY(seq_scan(R, rocprim::make_transform_iterator(rocprim::counting_iterator<int64_t>(0), TripBlocks{cell_start.p, cells}), blk_first.p, cells + 1));
    SEQ_TRY(seq_kernels_end(R));
    int64_t blocks = 0;
    SEQ_TRY(seq_read_back(R, &blocks, blk_first.p + cells, 8));
    if (blocks > 0) {
        SEQ_TRY(seq_kernels_begin(R));
        hipLaunchKernelGGL(k_trip_locate, dim3((unsigned)blocks), dim3(SEQ_BLOCK), 0, R.stream, d_xy, idx2.p, cell_start.p, blk_first.p, cells, rg->d_cell_first, rg->d_cand, rg->d_box,
                           rg->d_seg_first, rg->d_seg, d_region, d_counters);
        SEQ_TRY(seq_kernels_end(R));
    }
    DGE_HIP(hipGetLastError());
    return DGE_OK;
}

int slot_check(int32_t T, int32_t mode, const char* who) {
    if (mode == DGE_SLOTS_EVEN) { if (T < 1 || T > 24 || 24 % T != 0) DGE_FAIL(DGE_ERR_ARG, "%s: DGE_SLOTS_EVEN needs a T that divides 24, not %d", who, T); }
    else if (mode == DGE_SLOTS_AS_TRACTS) { if (T < 1 || T > 24) DGE_FAIL(DGE_ERR_ARG, "%s: DGE_SLOTS_AS_TRACTS needs 1 <= T <= 24, not %d", who, T); }
    else DGE_FAIL(DGE_ERR_ARG, "%s: mode %d is neither DGE_SLOTS_EVEN nor DGE_SLOTS_AS_TRACTS", who, mode);
    return DGE_OK;
}

// the slot edges on the device, ascending by (slot, src id, dst id): the sorted keys (slot, rank, rank) and their weights
int trip_slot_edges(SeqRun& R, const dge_flows* f, int32_t T, int32_t mode, dge_tmp<uint64_t>& okey, dge_tmp<int64_t>& ow, int64_t* n_out) {
    *n_out = 0;
    const int64_t n = f->n;
    if (n == 0) return DGE_OK;
    const dge_regions* rg = f->regions;
    const int32_t step = mode == DGE_SLOTS_EVEN ? 1 : 24 / T, width = mode == DGE_SLOTS_EVEN ? 24 / T : 1;
    const int64_t items = n * step;
    dge_tmp<uint64_t> ikey, skey;
    dge_tmp<int64_t> iw, sw;
    dge_tmp<unsigned long long> counters;
    SEQ_TRY(seq_alloc(R, ikey, items, "the slot items"));
    SEQ_TRY(seq_alloc(R, iw, items, "the slot items' weights"));
    SEQ_TRY(seq_alloc(R, skey, items, "the sorted slot items"));
    SEQ_TRY(seq_alloc(R, sw, items, "the sorted slot items' weights"));
    SEQ_TRY(seq_alloc(R, counters, TC_N, "the counters"));
    DGE_HIP(hipMemsetAsync(counters.p, 0, TC_N * 8, R.stream));
    SEQ_TRY(seq_kernels_begin(R));
    hipLaunchKernelGGL(k_slot_items, dim3(seq_grid(items)), dim3(SEQ_BLOCK), 0, R.stream, f->d_key, f->d_cnt, n, (uint64_t)rg->R, T, mode, step, width, rg->d_idrank, ikey.p, iw.p, counters.p);
    SEQ_TRY(seq_kernels_end(R));
    SEQ_TRY(trip_sort_pairs(R, ikey.p, skey.p, iw.p, sw.p, items, 64));
    unsigned long long valid = 0;
    SEQ_TRY(seq_read_back(R, &valid, counters.p + TC_VALID, 8));
    return trip_reduce(R, skey.p, sw.p, (int64_t)valid, okey, ow, n_out);
}

void locate_counters(const unsigned long long* c, int64_t points, double ms, dge_locate_info* info) {
    info->points = points; info->located = (int64_t)c[TC_LOCATED]; info->on_boundary = (int64_t)c[TC_BOUNDARY]; info->multi = (int64_t)c[TC_MULTI];
    info->outside = (int64_t)c[TC_OUTSIDE]; info->exact = (int64_t)c[TC_EXACT]; info->kernel_ms = ms;
}

int regions_locate(const dge_regions* rg, const double* xy, int64_t n, int32_t* region, dge_locate_info* info, bool on_device, const char* who) {
    if (!rg || n < 0 || (n > 0 && (!xy || !region))) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    SEQ_TRY(dge_require_device(rg->device));
    if (on_device && n > 0) DGE_HIP(hipDeviceSynchronize());      // the caller's points may still be in flight on a stream of theirs; this call's stream is non-blocking
    SeqRun R;
    SEQ_TRY(seq_open(R, rg->device, who));
    dge_tmp<unsigned long long> counters;
    dge_tmp<double> d_xy;
    dge_tmp<int32_t> d_region;
    SEQ_TRY(seq_alloc(R, counters, TC_N, "the counters"));
    DGE_HIP(hipMemsetAsync(counters.p, 0, TC_N * 8, R.stream));
    if (!on_device) {
        SEQ_TRY(seq_alloc(R, d_xy, 2 * std::min(n, TRIP_CHUNK), "the points"));
        SEQ_TRY(seq_alloc(R, d_region, std::min(n, TRIP_CHUNK), "the points' regions"));
    }
    for (int64_t at = 0; at < n; at += TRIP_CHUNK) {
        const int64_t m = std::min(TRIP_CHUNK, n - at);
        if (on_device) SEQ_TRY(trip_locate(R, rg, xy + 2 * at, m, region + at, counters.p));
        else {
            DGE_HIP(hipMemcpyAsync(d_xy.p, xy + 2 * at, (size_t)m * 16, hipMemcpyHostToDevice, R.stream));
            SEQ_TRY(trip_locate(R, rg, d_xy.p, m, d_region.p, counters.p));
            SEQ_TRY(seq_read_back(R, region + at, d_region.p, (size_t)m * 4));
        }
    }
    unsigned long long c[TC_N];
    SEQ_TRY(seq_read_back(R, c, counters.p, sizeof(c)));
    if (info) locate_counters(c, n, R.kernel_ms, info);
    return DGE_OK;
}

int flows_add(dge_flows* f, const double* sxy, const double* exy, const int32_t* hour, int64_t n, bool on_device, const char* who) {
    if (!f || n < 0 || (n > 0 && (!sxy || !exy || !hour))) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    const dge_regions* rg = f->regions;
    SEQ_TRY(dge_require_device(rg->device));
    if (n == 0) return DGE_OK;
    if (on_device) DGE_HIP(hipDeviceSynchronize());               // the caller's points and hours may still be in flight on a stream of theirs
    SeqRun R;
    SEQ_TRY(seq_open(R, rg->device, who));
    const int64_t cap = std::min(n, TRIP_CHUNK);
    const uint64_t Ru = (uint64_t)std::max<int64_t>(rg->R, 1);
    const int key_bits = 64;                     // (the unmapped trips' key is all ones)
    dge_tmp<unsigned long long> counters;
    dge_tmp<double> d_s, d_e;
    dge_tmp<int32_t> d_h, rs, re;
    dge_tmp<uint64_t> key, skey, tkey;           // tkey / tcnt: the table as it grows in this call
    dge_tmp<int64_t> tcnt;
    int64_t tn = f->n;
    bool own_table = false;
    SEQ_TRY(seq_alloc(R, counters, TC_N, "the counters"));
    DGE_HIP(hipMemsetAsync(counters.p, 0, TC_N * 8, R.stream));
    if (!on_device) {
        SEQ_TRY(seq_alloc(R, d_s, 2 * cap, "the start points"));
        SEQ_TRY(seq_alloc(R, d_e, 2 * cap, "the end points"));
        SEQ_TRY(seq_alloc(R, d_h, cap, "the hours"));
    }
    SEQ_TRY(seq_alloc(R, rs, cap, "the start regions"));
    SEQ_TRY(seq_alloc(R, re, cap, "the end regions"));
    SEQ_TRY(seq_alloc(R, key, cap, "the trips' keys"));
    SEQ_TRY(seq_alloc(R, skey, cap, "the sorted keys"));
    unsigned long long before = 0;
    for (int64_t at = 0; at < n; at += TRIP_CHUNK) {
        const int64_t m = std::min(TRIP_CHUNK, n - at);
        const double *ps = sxy + 2 * at, *pe = exy + 2 * at;
        const int32_t* ph = hour + at;
        if (!on_device) {
            DGE_HIP(hipMemcpyAsync(d_s.p, ps, (size_t)m * 16, hipMemcpyHostToDevice, R.stream));
            DGE_HIP(hipMemcpyAsync(d_e.p, pe, (size_t)m * 16, hipMemcpyHostToDevice, R.stream));
            DGE_HIP(hipMemcpyAsync(d_h.p, ph, (size_t)m * 4, hipMemcpyHostToDevice, R.stream));
            DGE_HIP(hipStreamSynchronize(R.stream));
            ps = d_s.p; pe = d_e.p; ph = d_h.p;
        }
        SEQ_TRY(trip_locate(R, rg, ps, m, rs.p, counters.p));
        SEQ_TRY(trip_locate(R, rg, pe, m, re.p, counters.p));
        SEQ_TRY(seq_kernels_begin(R));
        hipLaunchKernelGGL(k_flow_keys, dim3(seq_grid(m)), dim3(SEQ_BLOCK), 0, R.stream, ps, pe, ph, rs.p, re.p, m, Ru, key.p, counters.p);
        SEQ_TRY(seq_kernels_end(R));
        SEQ_TRY(trip_sort_pairs(R, key.p, skey.p, nullptr, nullptr, m, key_bits));
        unsigned long long mapped = 0;
        SEQ_TRY(seq_read_back(R, &mapped, counters.p + TC_MAPPED, 8));
        const int64_t fresh = (int64_t)(mapped - before);
        before = mapped;
        // ---- the chunk's run lengths, then the merge with the table: concatenate, sort, reduce by key
        dge_tmp<uint64_t> ukey, nkey;
        dge_tmp<int64_t> ucnt, ncnt;
        int64_t u = 0, nn = 0;
        SEQ_TRY(trip_reduce(R, skey.p, nullptr, fresh, ukey, ucnt, &u));
        if (u == 0) continue;
        SEQ_TRY(trip_join(R, own_table ? tkey.p : f->d_key, own_table ? tcnt.p : f->d_cnt, tn, ukey.p, ucnt.p, u, Ru, nkey, ncnt, &nn));
        if (tkey.p) { (void)hipFree(tkey.p); (void)hipFree(tcnt.p); }
        tkey.p = nkey.release(); tcnt.p = ncnt.release(); tn = nn; own_table = true;
    }
    unsigned long long c[TC_N];
    SEQ_TRY(seq_read_back(R, c, counters.p, sizeof(c)));
    // nothing can fail from here on
    if (own_table) {
        dge_dev_free(f->d_key); dge_dev_free(f->d_cnt);
        f->d_key = tkey.release(); f->d_cnt = tcnt.release(); f->n = tn;
    }
    struct dge_flows_info& I = f->info;
    I.trips += n; I.mapped += (int64_t)c[TC_MAPPED]; I.bad += (int64_t)c[TC_BAD]; I.no_start += (int64_t)c[TC_NO_START]; I.no_end += (int64_t)c[TC_NO_END]; I.entries = f->n;
    I.located += (int64_t)c[TC_LOCATED]; I.on_boundary += (int64_t)c[TC_BOUNDARY]; I.multi += (int64_t)c[TC_MULTI]; I.outside += (int64_t)c[TC_OUTSIDE]; I.exact += (int64_t)c[TC_EXACT];
    I.kernel_ms += R.kernel_ms;
    return DGE_OK;
}

void regions_release(dge_regions* rg) { if (rg && rg->refs.fetch_sub(1) == 1) delete rg; }

}  // namespace

// ------------------------------------------------------------------------------------------ entries: regions
extern "C" int dge_regions_create(int device, const int64_t* ids, int64_t R, const int64_t* ring_first, const int64_t* vert_first, const double* xy, int64_t n_rings, int64_t n_verts,
                                  int32_t grid, dge_regions** out) {
    const char* who = "dge_regions_create";
    if (!out || R < 0 || n_rings < 0 || n_verts < 0 || grid < 0 || !ring_first || !vert_first || (R > 0 && !ids) || (n_verts > 0 && !xy))
        DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    if (grid > TRIP_MAX_GRID) DGE_FAIL(DGE_ERR_ARG, "%s: a grid of %d x %d cells is beyond %d x %d", who, grid, grid, TRIP_MAX_GRID, TRIP_MAX_GRID);
    if (R > 0x7fffffffLL) DGE_FAIL(DGE_ERR_ARG, "%s: %lld regions do not fit int32 indices", who, (long long)R);
    if (ring_first[0] != 0 || ring_first[R] != n_rings) DGE_FAIL(DGE_ERR_ARG, "%s: ring_first must run from 0 to n_rings = %lld", who, (long long)n_rings);
    if (vert_first[0] != 0 || vert_first[n_rings] != n_verts) DGE_FAIL(DGE_ERR_ARG, "%s: vert_first must run from 0 to n_verts = %lld", who, (long long)n_verts);
    {
        std::vector<int64_t> sorted(ids, ids + R);
        std::sort(sorted.begin(), sorted.end());
        for (int64_t r = 1; r < R; r++)
            if (sorted[(size_t)r] == sorted[(size_t)r - 1]) DGE_FAIL(DGE_ERR_ARG, "%s: region id %lld occurs twice: ids must be distinct", who, (long long)sorted[(size_t)r]);
    }
    std::unique_ptr<dge_regions> rg(new dge_regions);
    rg->device = device; rg->R = R; rg->n_rings = n_rings;
    rg->ids.assign(ids, ids + R);
    std::vector<double> seg, box((size_t)R * 4);
    std::vector<int64_t> seg_first((size_t)R + 1, 0);
    seg.reserve((size_t)n_verts * 4);
    double gx0 = 0, gy0 = 0, gx1 = 0, gy1 = 0;
    bool any = false;
    for (int64_t r = 0; r < R; r++) {
        if (ring_first[r + 1] < ring_first[r]) DGE_FAIL(DGE_ERR_ARG, "%s: ring_first decreases at region %lld", who, (long long)r);
        double b[4] = {0, 0, 0, 0};
        bool first = true;
        for (int64_t q = ring_first[r]; q < ring_first[r + 1]; q++) {
            const int64_t v0 = vert_first[q], v1 = vert_first[q + 1];
            if (v1 - v0 < 4) DGE_FAIL(DGE_ERR_ARG, "%s: region %lld, ring %lld has %lld vertices: a closed ring has at least 4", who, (long long)r, (long long)q, (long long)(v1 - v0));
            for (int64_t v = v0; v < v1; v++) {
                const double x = xy[2 * v], y = xy[2 * v + 1];
                if (!pip_in_domain(x) || !pip_in_domain(y))
                    DGE_FAIL(DGE_ERR_ARG, "%s: region %lld, ring %lld, vertex %lld is outside the domain (finite; 0 or a magnitude in [2^-450, 2^500])", who, (long long)r, (long long)q, (long long)(v - v0));
                if (first) { b[0] = b[2] = x; b[1] = b[3] = y; first = false; }
                b[0] = std::min(b[0], x); b[2] = std::max(b[2], x); b[1] = std::min(b[1], y); b[3] = std::max(b[3], y);
                if (v + 1 < v1) { seg.push_back(x); seg.push_back(y); seg.push_back(xy[2 * v + 2]); seg.push_back(xy[2 * v + 3]); }
            }
            if (memcmp(xy + 2 * v0, xy + 2 * (v1 - 1), 16) != 0)
                DGE_FAIL(DGE_ERR_ARG, "%s: region %lld, ring %lld is not closed: vertex %lld differs from vertex 0", who, (long long)r, (long long)q, (long long)(v1 - v0 - 1));
        }
        seg_first[(size_t)r + 1] = (int64_t)(seg.size() / 4);
        if (first) { b[0] = b[1] = 1.0; b[2] = b[3] = -1.0; }       // no ring: a box that holds no point
        else {
            if (!any) { gx0 = b[0]; gy0 = b[1]; gx1 = b[2]; gy1 = b[3]; any = true; }
            gx0 = std::min(gx0, b[0]); gy0 = std::min(gy0, b[1]); gx1 = std::max(gx1, b[2]); gy1 = std::max(gy1, b[3]);
        }
        memcpy(&box[(size_t)r * 4], b, sizeof(b));
    }
    rg->n_segs = (int64_t)(seg.size() / 4);
    // ---- the index.  The library's rule for the cell count: about four cells a region, G = 2 ceil(sqrt(R)), between 1 and 1024
    int32_t G = grid;
    if (G == 0) { G = 1; while ((int64_t)G * G < R) G++; G = std::min(std::max(2 * G, 1), 1024); if (R == 0) G = 1; }
    rg->grid = G;
    rg->box[0] = gx0; rg->box[1] = gy0; rg->box[2] = gx1; rg->box[3] = gy1;
    rg->invx = gx1 > gx0 ? (double)G / (gx1 - gx0) : 0.0;
    rg->invy = gy1 > gy0 ? (double)G / (gy1 - gy0) : 0.0;
    const int64_t cells = (int64_t)G * G;
    std::vector<int64_t> cell_first((size_t)cells + 1, 0);
    std::vector<int32_t> cand;
    for (int pass = 0; pass < 2; pass++) {
        for (int64_t r = 0; r < R; r++) {
            const double* b = &box[(size_t)r * 4];
            if (b[0] > b[2]) continue;
            const int32_t cx0 = pip_cell(b[0], gx0, rg->invx, G), cx1 = pip_cell(b[2], gx0, rg->invx, G), cy0 = pip_cell(b[1], gy0, rg->invy, G), cy1 = pip_cell(b[3], gy0, rg->invy, G);
            for (int32_t cy = cy0; cy <= cy1; cy++)
                for (int32_t cx = cx0; cx <= cx1; cx++) {
                    const size_t c = (size_t)cy * (size_t)G + (size_t)cx;
                    if (pass == 0) cell_first[c + 1]++;
                    else cand[(size_t)cell_first[c]++] = (int32_t)r;      // r ascending: every list is
                }
        }
        if (pass == 0) {
            for (int64_t c = 0; c < cells; c++) { rg->max_cand = std::max(rg->max_cand, cell_first[(size_t)c + 1]); cell_first[(size_t)c + 1] += cell_first[(size_t)c]; }
            cand.resize((size_t)cell_first[(size_t)cells]);
        } else {
            for (int64_t c = cells; c > 0; c--) cell_first[(size_t)c] = cell_first[(size_t)c - 1];
            cell_first[0] = 0;
        }
    }
    std::vector<int32_t> order((size_t)R), idrank((size_t)R);
    std::vector<int64_t> id_by_rank((size_t)R);
    for (int64_t r = 0; r < R; r++) order[(size_t)r] = (int32_t)r;
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return ids[a] < ids[b]; });
    for (int64_t k = 0; k < R; k++) { idrank[(size_t)order[(size_t)k]] = (int32_t)k; id_by_rank[(size_t)k] = ids[order[(size_t)k]]; }

    SEQ_TRY(dge_require_device(device));
    SeqRun Rn;
    SEQ_TRY(seq_open(Rn, device, who));
    SEQ_TRY(trip_upload(Rn, &rg->d_seg, seg.data(), (int64_t)seg.size(), "the segments"));
    SEQ_TRY(trip_upload(Rn, &rg->d_seg_first, seg_first.data(), R + 1, "the regions' segments"));
    SEQ_TRY(trip_upload(Rn, &rg->d_box, box.data(), R * 4, "the regions' boxes"));
    SEQ_TRY(trip_upload(Rn, &rg->d_cell_first, cell_first.data(), cells + 1, "the cells"));
    SEQ_TRY(trip_upload(Rn, &rg->d_cand, cand.data(), (int64_t)cand.size(), "the cells' regions"));
    SEQ_TRY(trip_upload(Rn, &rg->d_idrank, idrank.data(), R, "the ids' ranks"));
    SEQ_TRY(trip_upload(Rn, &rg->d_id_by_rank, id_by_rank.data(), R, "the ids"));
    *out = rg.release();
    return DGE_OK;
}

extern "C" int dge_regions_info(const dge_regions* rg, struct dge_regions_info* out) {
    if (!rg || !out) DGE_FAIL(DGE_ERR_ARG, "dge_regions_info: null argument");
    out->regions = rg->R; out->rings = rg->n_rings; out->segments = rg->n_segs; out->max_cell_candidates = rg->max_cand; out->grid = rg->grid; out->tile_segments = TRIP_TILE;
    out->x0 = rg->box[0]; out->y0 = rg->box[1]; out->x1 = rg->box[2]; out->y1 = rg->box[3];
    return DGE_OK;
}

extern "C" int dge_regions_locate(const dge_regions* rg, const double* xy, int64_t n, int32_t* region, dge_locate_info* info) {
    return regions_locate(rg, xy, n, region, info, false, "dge_regions_locate");
}

extern "C" int dge_regions_locate_device(const dge_regions* rg, const double* d_xy, int64_t n, int32_t* d_region, dge_locate_info* info) {
    return regions_locate(rg, d_xy, n, d_region, info, true, "dge_regions_locate_device");
}

extern "C" void dge_regions_free(dge_regions* rg) { regions_release(rg); }

// ------------------------------------------------------------------------------------------ entries: flows
extern "C" int dge_flows_create(const dge_regions* rg, dge_flows** out) {
    if (!rg || !out) DGE_FAIL(DGE_ERR_ARG, "dge_flows_create: null argument");
    if (rg->R > 800000000LL) DGE_FAIL(DGE_ERR_RANGE, "dge_flows_create: the keys (hour, s, e) of %lld regions do not fit 64 bits", (long long)rg->R);
    dge_flows* f = new dge_flows;
    f->regions = const_cast<dge_regions*>(rg);
    f->regions->refs.fetch_add(1);
    *out = f;
    return DGE_OK;
}

extern "C" int dge_flows_add_trips(dge_flows* f, const double* start_xy, const double* end_xy, const int32_t* hour, int64_t n) {
    return flows_add(f, start_xy, end_xy, hour, n, false, "dge_flows_add_trips");
}

extern "C" int dge_flows_add_trips_device(dge_flows* f, const double* d_start_xy, const double* d_end_xy, const int32_t* d_hour, int64_t n) {
    return flows_add(f, d_start_xy, d_end_xy, d_hour, n, true, "dge_flows_add_trips_device");
}

int dge_flows_device(const dge_flows* f) { return f->regions->device; }
int dge_flows_like(const dge_flows* f, dge_flows** out) { return dge_flows_create(f->regions, out); }

// The tables are sorted sets of (key, count): concatenated, sorted and reduced by key they are the table the trips of both give in any order of adding.
int dge_flows_merge(dge_flows* f, const dge_flows* part) {
    const char* who = "dge_flows_merge";
    if (f->regions != part->regions) DGE_FAIL(DGE_ERR_ARG, "%s: the tables are over different regions", who);
    SeqRun R;
    if (part->n > 0) {
        SEQ_TRY(dge_require_device(f->regions->device));
        SEQ_TRY(seq_open(R, f->regions->device, who));
        dge_tmp<uint64_t> nkey;
        dge_tmp<int64_t> ncnt;
        int64_t nn = 0;
        SEQ_TRY(trip_join(R, f->d_key, f->d_cnt, f->n, part->d_key, part->d_cnt, part->n, (uint64_t)std::max<int64_t>(f->regions->R, 1), nkey, ncnt, &nn));
        // nothing can fail from here on
        dge_dev_free(f->d_key); dge_dev_free(f->d_cnt);
        f->d_key = nkey.release(); f->d_cnt = ncnt.release(); f->n = nn;
    }
    struct dge_flows_info& I = f->info;
    const struct dge_flows_info& P = part->info;
    I.trips += P.trips; I.mapped += P.mapped; I.bad += P.bad; I.no_start += P.no_start; I.no_end += P.no_end; I.entries = f->n;
    I.located += P.located; I.on_boundary += P.on_boundary; I.multi += P.multi; I.outside += P.outside; I.exact += P.exact;
    I.kernel_ms += P.kernel_ms + R.kernel_ms;
    return DGE_OK;
}

extern "C" int dge_flows_info(const dge_flows* f, struct dge_flows_info* out) {
    if (!f || !out) DGE_FAIL(DGE_ERR_ARG, "dge_flows_info: null argument");
    *out = f->info;
    out->entries = f->n;
    return DGE_OK;
}

extern "C" int dge_flows_to_host(const dge_flows* f, int32_t* hour, int32_t* src, int32_t* dst, int64_t* count, int64_t cap, int64_t* n) {
    if (!f || !n || cap < 0 || (cap > 0 && (!hour || !src || !dst || !count))) DGE_FAIL(DGE_ERR_ARG, "dge_flows_to_host: null or negative argument");
    *n = f->n;
    if (cap < f->n) DGE_FAIL(DGE_ERR_CAP, "dge_flows_to_host: %lld entries exceed cap %lld", (long long)f->n, (long long)cap);
    if (f->n == 0) return DGE_OK;
    SEQ_TRY(dge_require_device(f->regions->device));
    std::vector<uint64_t> key((size_t)f->n);
    DGE_HIP(hipMemcpy(key.data(), f->d_key, (size_t)f->n * 8, hipMemcpyDeviceToHost));
    DGE_HIP(hipMemcpy(count, f->d_cnt, (size_t)f->n * 8, hipMemcpyDeviceToHost));
    const uint64_t R = (uint64_t)f->regions->R;
    for (int64_t i = 0; i < f->n; i++) { const uint64_t k = key[(size_t)i]; dst[i] = (int32_t)(k % R); src[i] = (int32_t)((k / R) % R); hour[i] = (int32_t)(k / R / R); }
    return DGE_OK;
}

extern "C" int dge_flows_slot_edges(const dge_flows* f, int32_t T, int32_t mode, int32_t* slot, int64_t* src_id, int64_t* dst_id, int64_t* w, int64_t cap, int64_t* n) {
    const char* who = "dge_flows_slot_edges";
    if (!f || !n || cap < 0 || (cap > 0 && (!slot || !src_id || !dst_id || !w))) DGE_FAIL(DGE_ERR_ARG, "%s: null or negative argument", who);
    SEQ_TRY(slot_check(T, mode, who));
    *n = 0;
    if (f->n == 0) return DGE_OK;
    SEQ_TRY(dge_require_device(f->regions->device));
    SeqRun R;
    SEQ_TRY(seq_open(R, f->regions->device, who));
    dge_tmp<uint64_t> okey;
    dge_tmp<int64_t> ow;
    int64_t E = 0;
    SEQ_TRY(trip_slot_edges(R, f, T, mode, okey, ow, &E));
    *n = E;
    if (cap < E) DGE_FAIL(DGE_ERR_CAP, "%s: %lld slot edges exceed cap %lld", who, (long long)E, (long long)cap);
    if (E == 0) return DGE_OK;
    SlotArrays A;
    SEQ_TRY(trip_slot_decode(R, f, okey.p, ow.p, E, A));
    SEQ_TRY(seq_read_back(R, slot, A.slot.p, (size_t)E * 4));
    SEQ_TRY(seq_read_back(R, src_id, A.src_id.p, (size_t)E * 8));
    SEQ_TRY(seq_read_back(R, dst_id, A.dst_id.p, (size_t)E * 8));
    return seq_read_back(R, w, ow.p, (size_t)E * 8);
}

int dge_flows_slot_coo(const dge_flows* f, int32_t T, int32_t mode, int32_t slot, const uint8_t* select, const char* who, dge_tmp<int32_t>& row, dge_tmp<int32_t>& col,
                       dge_tmp<double>& val, int64_t* n_entries, std::vector<int64_t>& regions) {
    *n_entries = 0;
    SEQ_TRY(slot_check(T, mode, who));
    if (slot < 0 || slot >= T) DGE_FAIL(DGE_ERR_ARG, "%s: slot = %d is outside 0 .. %d", who, slot, T - 1);
    const dge_regions* rg = f->regions;
    const int64_t Rn = rg->R;
    regions.clear();
    for (int64_t i = 0; i < Rn; i++) if (!select || select[i]) regions.push_back(i);
    if (regions.empty()) DGE_FAIL(DGE_ERR_ARG, "%s: no region is selected", who);
    if (f->n == 0) DGE_FAIL(DGE_ERR_ARG, "%s: slot %d holds no entry: the table is empty", who, slot);
    SEQ_TRY(dge_require_device(rg->device));
    SeqRun R;
    SEQ_TRY(seq_open(R, rg->device, who));
    // rank of a region's id -> its number among the selected regions
    std::vector<int32_t> idrank((size_t)Rn), map((size_t)Rn, -1);
    SEQ_TRY(seq_read_back(R, idrank.data(), rg->d_idrank, (size_t)Rn * 4));
    for (size_t c = 0; c < regions.size(); c++) map[(size_t)idrank[(size_t)regions[c]]] = (int32_t)c;
    dge_tmp<uint64_t> okey;
    dge_tmp<int64_t> ow;
    dge_tmp<int32_t> d_map;
    dge_tmp<unsigned long long> count;
    int64_t E = 0;
    SEQ_TRY(trip_slot_edges(R, f, T, mode, okey, ow, &E));
    unsigned long long got = 0;
    if (E > 0) {
        SEQ_TRY(seq_alloc(R, d_map, Rn, "the regions' numbers"));
        SEQ_TRY(seq_alloc(R, count, 1, "the number of entries"));
        SEQ_TRY(seq_alloc(R, row, E, "the entries' rows"));
        SEQ_TRY(seq_alloc(R, col, E, "the entries' columns"));
        SEQ_TRY(seq_alloc(R, val, E, "the entries' values"));
        DGE_HIP(hipMemcpyAsync(d_map.p, map.data(), (size_t)Rn * 4, hipMemcpyHostToDevice, R.stream));
        DGE_HIP(hipMemsetAsync(count.p, 0, 8, R.stream));
        SEQ_TRY(seq_kernels_begin(R));
        hipLaunchKernelGGL(k_slot_coo, dim3(seq_grid(E)), dim3(SEQ_BLOCK), 0, R.stream, okey.p, ow.p, E, (uint64_t)std::max<int64_t>(Rn, 1), slot, d_map.p, row.p, col.p, val.p, count.p);
        SEQ_TRY(seq_kernels_end(R));
        SEQ_TRY(seq_read_back(R, &got, count.p, 8));
    }
    if (got == 0) DGE_FAIL(DGE_ERR_ARG, "%s: slot %d holds no entry between the selected regions", who, slot);
    *n_entries = (int64_t)got;
    return DGE_OK;
}

int dge_flows_slot_check(int32_t T, int32_t mode, const char* who) { return slot_check(T, mode, who); }

int dge_flows_slot_keys(const dge_flows* f, int32_t T, int32_t mode, const char* who, dge_tmp<uint64_t>& key, dge_tmp<int64_t>& w, int64_t* n, double* kernel_ms) {
    *n = 0;
    if (f->n == 0) return DGE_OK;
    SeqRun R;
    SEQ_TRY(seq_open(R, f->regions->device, who));
    const int rc = trip_slot_edges(R, f, T, mode, key, w, n);
    *kernel_ms += R.kernel_ms;
    return rc;
}

extern "C" void dge_flows_free(dge_flows* f) {
    if (!f) return;
    dge_dev_free(f->d_key); dge_dev_free(f->d_cnt);
    regions_release(f->regions);
    delete f;
}

extern "C" int dge_graph_add_flows(dge_graph* g, const dge_flows* f, int32_t T, int32_t mode, dge_names* names, dge_od_info* info) {
    const char* who = "dge_graph_add_flows";
    if (!g || !f) DGE_FAIL(DGE_ERR_ARG, "%s: null argument", who);
    SEQ_TRY(slot_check(T, mode, who));
    if (g->device != f->regions->device) DGE_FAIL(DGE_ERR_ARG, "%s: the graph is on device %d, the flows on device %d", who, g->device, f->regions->device);
    SEQ_TRY(od_check(g, names, who));
    SEQ_TRY(dge_require_device(g->device));
    SeqRun R;
    SEQ_TRY(seq_open(R, g->device, who));
    dge_tmp<uint64_t> okey;
    dge_tmp<int64_t> ow;
    int64_t E = 0, Rn = 0, S = 0;
    SEQ_TRY(trip_slot_edges(R, f, T, mode, okey, ow, &E));
    SlotArrays A;
    SEQ_TRY(trip_slot_decode(R, f, okey.p, ow.p, E, A));
    SEQ_TRY(od_commit(R, g, names, E, E, T, A.src_id.p, A.dst_id.p, A.w_bits.p, A.slot.p, A.iota.p, who, &Rn, &S));
    if (info) {
        info->bytes = 0; info->lines = 0; info->flows = E; info->edges = E; info->dropped = 0; info->regions = Rn; info->sources = S; info->host_values = 0; info->slices = T; info->reserved = 0;
        info->read_ms = 0; info->kernel_ms = R.kernel_ms;
    }
    return DGE_OK;
}
