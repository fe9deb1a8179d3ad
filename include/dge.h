/*
 * dge.h — C ABI of libdge.so: the MI355X-native random-walk + SGNS engine.
 *
 * This is the drop-in boundary for the hot path named by BASELINE.json:north_star.  The reference
 * (thekingofkings/embedding) is plain Java with no FFI; the seam is introduced UNDER its public
 * classes.  Each entry point cites the reference interface it replaces, with
 * J/ = embedding/src/main/java/embedding/.  The JNI / ctypes bindings a maintainer adds on the
 * reference side are shown in INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", opaque handles, plain pointers and sizes; every function returns a status
 *     (DGE_OK == 0).  dge_last_error() returns a thread-local message for the last failure.
 *   - No CPU compute path exists in this library: every call needs a visible gfx950 device and fails
 *     with DGE_ERR_DEVICE otherwise.
 *   - Vertex ids are the caller's insertion ordinals (J/LayeredGraph.java:160,166): name <-> id
 *     interning ("h-regionId" strings) stays on the host-language side.
 *   - "host" pointers are ordinary process memory; "d_" pointers are device memory on the handle's
 *     device (e.g. a torch tensor's data_ptr()).  Handles work on their own non-blocking HIP stream: entry points that
 *     READ a caller's device buffer first wait for the device (hipDeviceSynchronize), entry points that WRITE one return
 *     after their stream has drained, so no stream handshake is needed on the caller's side.  (dge_count_tokens, which has no handle with a stream,
 *     does both around a launch on stream 0.)
 *   - Four entries RETURN WITH WORK STILL QUEUED, by design: dge_model_train and dge_model_walk_and_train (on the model's stream; the zero-wait episode of
 *     the block schedule rests on it), dge_model_export/import_partition_async and dge_model_ring_pass (their own sections say what orders a caller's stream).
 *     Later calls on the SAME model are ordered by its stream.  Other handles are ordered through the CORPUS: a dge_walks remembers its last queued use with an
 *     event recorded on the stream that made it, and every other entry that touches the corpus goes behind that event — another model's train,
 *     walk_and_train, eval_links and eval_sgns, dge_sample_walks_into and the .seq writer make their stream wait for it (no host wait is added);
 *     dge_walks_to_host and dge_walks_add_position_prefix wait for it on the host; dge_count_tokens waits for the device.  So a corpus may be read, written
 *     again or re-sampled right behind a queued launch without a handshake.  NOT covered: the raw pointer dge_walks_info hands out (the caller orders its own
 *     reads), and a graph changed (add_edges, build_alias, ..) while a queued dge_model_walk_and_train still reads its tables: read the model's stats, or
 *     synchronise dge_model_stream, first.  dge_walks_free and the other *_free behind a queued launch are safe: hipFree waits for the device.
 *   - dge_graph_set_stream / dge_model_set_stream drain the handle's present stream, then move its work to the caller's; the handle never destroys a stream
 *     it was given, and the rules above hold on it unchanged (a null stream is stream 0).
 *   - Handles are not thread-safe; the reference's walk API is single-threaded
 *     (J/CrossTimeGraph.java:134-140) and the trainer owns its workers (J/DeepWalk.java:75).
 */
#ifndef DGE_H
#define DGE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGE_VERSION 106   /* (still 106: the held-out evaluation entries — dge_model_score_pairs, dge_model_eval_links, dge_model_eval_sgns, struct dge_eval_result — were added without a bump: additions only, no struct changed size)
                             106: dge_selftest_atomics_wave_block; the block kernels' accumulator banks (DGE_TUNE_ACC_ROWS / ACC_DRAIN apply to both tables of a block); k_sgns_train_small and DGE_TUNE_SMALL_ROWS.
                             105: stream-ordered partition copies (dge_model_export/import_partition_async, dge_model_stream), dge_host_sync_count, the lock kernels' watchdog,
                             forced schedules refused where they would diverge or spin (DGE_ERR_ARG), DGE_TUNE_ALLOW_UNSAFE / WATCHDOG_MS / HS_COPIES (additions only) */

enum {
    DGE_OK = 0,
    DGE_ERR_ARG = 1,      /* null / negative / inconsistent argument */
    DGE_ERR_RANGE = 2,    /* vertex id outside the graph */
    DGE_ERR_TOPK = 3,     /* keep_top_k: a vertex has fewer than k edges (Java: IndexOutOfBoundsException) */
    DGE_ERR_CAP = 4,      /* caller buffer too small */
    DGE_ERR_STATE = 5,    /* call order violated (e.g. walks before alias tables) */
    DGE_ERR_DEVICE = 6,   /* no usable gfx950 device / HIP failure */
    DGE_ERR_IO = 7
};

typedef struct dge_graph dge_graph;   /* per-timeslice edge store + alias tables, resident in HBM   */
typedef struct dge_walks dge_walks;   /* walk corpus int32 [n_walks x max_len], pad -1, resident in HBM */
typedef struct dge_model dge_model;   /* vocabulary + syn0/syn1neg tables, resident in HBM           */

const char* dge_last_error(void);
int  dge_version(void);
/* "kernels=<hash> sorted=<hash>": 12 hex digits of the SHA-1 of the stamped sources this library was built from (sgns_kernels.h + dge_algos.h + sgns_plan.h + sgns.hip;
   the same + sgns_sorted.hip).  A source is in the stamp if and only if a change to it can change what a training launch reads or writes per pair: the trainer
   kernels, the schedule, the code that builds what those kernels read (vocabulary order, the unigram table in its block and run forms, Huffman paths, the
   schedule's statistics) and the code that fills the kernels' parameters and launches.  What decides only time (table placement), what runs between launches
   (exchange, read-back, output) and what exists for tests (self-tests, probes) is not.  The committed counter profiles (profiles/traffic.json) carry the stamp
   of the build they were collected with; bench.py quotes a profile's bytes per pair only when the stamp matches the loaded library. */
const char* dge_build_stamp(void);
int  dge_device_count(int* n);

/* ------------------------------------------------------------------------------------------------
 * Edge store — replaces LayeredGraph's HashMap/ArrayList store (J/LayeredGraph.java:142-148).
 * ---------------------------------------------------------------------------------------------- */
/* new LayeredGraph()  J/LayeredGraph.java:150-155.  device >= 0 (no CPU path). */
int  dge_graph_create(dge_graph** out, int device);
void dge_graph_free(dge_graph* g);
/* run this handle's work on an existing hipStream_t (default: a stream the handle owns) */
int  dge_graph_set_stream(dge_graph* g, void* hip_stream);
/* bulk addEdge(fn, tn, weight)  J/LayeredGraph.java:157-174.  Appends in call order; duplicates are
 * kept; per-vertex edge order = insertion order; outDegree = running sum (J/LayeredGraph.java:46-49). */
int  dge_graph_add_edges(dge_graph* g, const int32_t* src, const int32_t* dst, const double* w, int64_t n);
/* same, COO already in device memory (synthetic generators, device-side OD ingest) */
int  dge_graph_add_edges_device(dge_graph* g, const int32_t* d_src, const int32_t* d_dst, const double* d_w, int64_t n);
/* bulk addSourceVertex(vn)  J/LayeredGraph.java:180-189 (after all edges).  stream_sum = 0: sourceWeightSum
 * is the running += of addSourceVertex; 1: DoubleStream.sum() as in J/SpatialGraph.java:56-57,82-83. */
int  dge_graph_set_sources(dge_graph* g, const int32_t* v, int64_t n, int stream_sum);
/* Vertex ids [0, n) exist even when no edge names them (isolated vertices; the unregistered source vertices that
 * addSourceVertex creates for unknown names, J/LayeredGraph.java:182-183).  Before set_sources / build_alias. */
int  dge_graph_reserve_vertices(dge_graph* g, int32_t n);
/* Vertex.outDegree is a PUBLIC FIELD of the reference (J/LayeredGraph.java:35; assigned by J/SpatialGraph.java:33): a host that
 * keeps that field hands over its values (host double[n], n = vertex count) instead of the recomputed running sums.
 * After all edges; adding edges afterwards recomputes the sums. */
int  dge_graph_set_out_degree(dge_graph* g, const double* out_degree, int32_t n);
/* LayeredGraph.sourceWeightSum is a protected field that subclasses assign (J/SpatialGraph.java:57,83): fix it to the
 * host's value.  After dge_graph_set_sources (which recomputes it). */
int  dge_graph_set_source_weight_sum(dge_graph* g, double sum);
/* SpatialGraph.keepNearestKVertices(k)  J/SpatialGraph.java:29-35: stable sort by weight descending,
 * keep the first k, outDegree recomputed.  DGE_ERR_TOPK if some vertex has fewer than k edges. */
int  dge_graph_keep_top_k(dge_graph* g, int32_t k);
/* initiateAliasTables()  J/LayeredGraph.java:195-226 (+ Vertex.initiateAliasTable :54-82).
 * exact_reference_order = 1: the reference's own pairing order (bit-identical prob/alias arrays);
 * 0: Vose O(k) pairing — same sampling distribution, different alias indices (scalable form). */
int  dge_graph_build_alias(dge_graph* g, int exact_reference_order);
int  dge_graph_num_vertices(const dge_graph* g, int32_t* n);
int  dge_graph_num_edges(const dge_graph* g, int64_t* n);
/* Vertex.{probTable,aliasTable,edgesOut,outDegree} read-back for one vertex (J/LayeredGraph.java:31-37);
 * any output pointer may be null.  *k receives the degree even when cap is too small (DGE_ERR_CAP). */
int  dge_graph_get_alias(const dge_graph* g, int32_t v, double* prob, int32_t* alias, int32_t* nbr,
                         double* weight, int32_t cap, int32_t* k, double* out_degree);
/* the same for ALL vertices at once, in CSR order (edges of vertex v at [row_ptr[v], row_ptr[v+1]), insertion order kept):
 * what a host needs to fill every Vertex's probTable/aliasTable after initiateAliasTables(), or to rebuild edgesOut /
 * outDegree after keepNearestKVertices.  Host buffers; any output may be null; row_ptr has cap_vertices + 1 entries. */
int  dge_graph_get_csr(const dge_graph* g, int64_t* row_ptr, int32_t* nbr, double* weight, double* prob, int32_t* alias,
                       double* out_degree, int32_t cap_vertices, int64_t cap_edges);
/* LayeredGraph.{probTable,aliasTable,sourceVertices,sourceWeightSum}  J/LayeredGraph.java:145-148 */
int  dge_graph_get_source_alias(const dge_graph* g, double* prob, int32_t* alias, int32_t* src,
                                int32_t cap, int32_t* k, double* weight_sum);
/* Vertex.sampleNextVertex(double x)  J/LayeredGraph.java:123-132 (test overload); *next = -1 when the
 * vertex has no out-edges.  Runs the device sampler for one explicit x. */
int  dge_graph_sample_next(const dge_graph* g, int32_t v, double x, int32_t* next);
/* ---- .od flow text in (new; additions only, DGE_VERSION unchanged): the files at the front of the pipeline, one "src dst w" line per flow and one file per
 * time slice (written J/Tracts.java:236-264, J/CommunityAreas.java:127-146,171-186), become the layered graph on the device (csrc/od_read.hip).  The rule is
 * that of embedding_amd/io.py: read_od_slices (J/CrossTimeGraph.java:25-52,68-95):
 *   - Piece h of n_slices = T pieces (a file, or a text) is slice h.  A line with a token is a FLOW "src dst w": two region ids and a weight.  A flow with w > 0
 *     is an edge; every other flow — w == 0 (J/CommunityAreas.java:178 writes them), -0, a negative weight — is dropped and counted (info.dropped).
 *   - REGIONS are the distinct region ids that occur in a kept flow of any slice, ascending as signed 64-bit integers: R of them, rank(r) the index of r.
 *   - A kept flow of slice h is the edge  h*R + rank(src)  ->  ((h + 1) % T)*R + rank(dst)  of weight w.  Edges stand in the order of the text, piece after piece,
 *     line after line; duplicates are kept (the per-vertex edge order, and with it the alias tables, follow from that order).  T*R vertices are reserved;
 *     T*R > 2^31 - 1: DGE_ERR_RANGE.  T == 1 gives the static graph of one file (taxi-all.od): its edges stay inside the layer.
 *   - SOURCES: every layer-0 vertex that is an endpoint of some edge, ascending, set as dge_graph_set_sources(.., stream_sum = 0) sets them — a region that
 *     is only a destination of slice T-1 is a source of weight 0.
 *   - The text is BYTES; whitespace, lines, pieces and NUL are what they are to the .seq and .vec readers: whitespace is 0x09-0x0D and 0x20, the last line may
 *     lack its '\n', no token and no line crosses a piece, a line without a token is skipped, a NUL byte is DGE_ERR_IO naming its offset.
 *   - Errors of the text, the first applicable wins: a NUL byte; a RAGGED LINE — a token count that is neither 0 nor 3: DGE_ERR_IO naming the least such
 *     (piece, line), the count found and the count expected; a BAD TOKEN: DGE_ERR_IO naming the least byte offset of one, with its piece, line and column.
 *     An id token is [+-] digits with a value in the int64 range (leading zeros allowed: 007 is region 7).  A weight token is a value token of the .vec grammar
 *     below; its value is the binary64 nearest the exact decimal value, ties to even — what glibc's strtod returns in the "C" locale, for tokens of any length
 *     (csrc/od_parse.h decides every integer of up to 19 digits and most else on the device; the few tokens it hands back are finished by the host with strtod
 *     and counted in info.host_values).  A weight that is not finite — inf, nan, overflow — is a bad token; underflow to 0 is w == 0, so the flow is dropped.
 *   - g must be fresh: one that already holds edges, sources or reserved vertices is DGE_ERR_STATE.  On success g stands where a host stands after
 *     dge_graph_add_edges, dge_graph_reserve_vertices and dge_graph_set_sources; dge_graph_build_alias is next.
 *   - names (may be NULL) must be empty, else DGE_ERR_ARG; it receives the T*R vertex names "<h>-<region id in decimal>" in vertex-id order — what
 *     dge_walks_write_seq and dge_write_vec take.
 *   - Null / negative arguments, n_slices < 1, names not empty: DGE_ERR_ARG before a device is looked for.  A file that is missing or unreadable: DGE_ERR_IO with
 *     its path.  A working set beyond device memory: DGE_ERR_CAP.  On any error g and names are as they were.
 *   - The result is a pure function of the bytes: nothing depends on timing or launch geometry. */
struct dge_names;
typedef struct dge_od_info {
    int64_t bytes;        /* bytes of text taken (the pieces' sizes added up)                            */
    int64_t lines;        /* lines, a last one without '\n' included                                      */
    int64_t flows;        /* lines with a token                                                           */
    int64_t edges;        /* flows kept: w > 0                                                            */
    int64_t dropped;      /* flows - edges: w <= 0                                                        */
    int64_t regions;      /* R                                                                            */
    int64_t sources;      /* layer-0 vertices that are an endpoint of an edge                             */
    int64_t host_values;  /* weight tokens the host finished with strtod                                  */
    int32_t slices;       /* T                                                                            */
    int32_t reserved;
    double  read_ms;      /* bytes to the device (file reads included)                                    */
    double  kernel_ms;    /* the device passes                                                            */
} dge_od_info;            /* 88 bytes */
int  dge_graph_add_od_files(dge_graph* g, const char* const* paths, int32_t n_slices, struct dge_names* names /* may be NULL */, dge_od_info* info /* may be NULL */);
int  dge_graph_add_od_texts(dge_graph* g, const char* const* texts, const int64_t* n_bytes, int32_t n_slices, struct dge_names* names, dge_od_info* info);
/* the R region ids of a graph made by the two entries above, ascending (vertex h*R + i is region regions[i] in slice h); *n = 0 for a graph not made this way;
 * cap too small: DGE_ERR_CAP with *n set.  A host read: no device involved. */
int  dge_graph_regions(const dge_graph* g, int64_t* regions, int64_t cap, int64_t* n);

/* ---- trips into regions, regions into flows (new; additions only, DGE_VERSION unchanged): the stage in front of the .od files — Tracts.mapTripsIntoTracts
 * (J/Tracts.java:71-102) and CommunityAreas.mapTripsIntoCommunities (J/CommunityAreas.java:55-103), which test every trip's pickup and drop-off point with JTS
 * MultiPolygon.contains against every region and count taxiFlows[hour][dst] — on the device (csrc/trip_map.hip, csrc/pip_exact.h).  Arrays in, flows and a
 * graph out: reading shapefiles stays with the host (the trip files themselves: the next section).  The rule; the result is a pure function of the inputs, nothing depends on timing,
 * launch geometry or the index's cell count:
 *   - REGIONS: region r has the id ids[r] (distinct) and the rings ring_first[r] .. ring_first[r+1]-1; ring q has the vertices vert_first[q] .. vert_first[q+1]-1
 *     of xy (binary64, x = longitude, y = latitude, interleaved).  A ring is closed: at least 4 vertices, the last equal to the first bit for bit.  Shells and
 *     holes are not told apart.
 *   - LOCATION of a point p in region r: BOUNDARY when p lies on a segment of a ring of r, its vertices included; INTERIOR when not boundary and the ray from p
 *     towards +x crosses the rings of r an odd number of times, a segment (a, b) being crossed when exactly one of a.y, b.y is > p.y and p lies strictly on the
 *     ray's side of the line through a and b — what JTS's RayCrossingCounter decides, and on a valid MultiPolygon what contains() decides.
 *   - The side test is the sign of (b.x-a.x)(p.y-a.y) - (b.y-a.y)(p.x-a.x) in EXACT arithmetic over the binary64 inputs (a filtered floating-point evaluation,
 *     then error-free transformations: csrc/pip_exact.h).  DOMAIN: every coordinate is finite and either 0 or of magnitude in [2^-450, 2^500].  A ring vertex
 *     outside the domain: DGE_ERR_ARG.  A trip point outside it: its region is -1 and the trip is bad.
 *   - The REGION of a point is the least index r whose location is interior, else -1 (a point on a shared edge of a tiling belongs to no region, as in the
 *     reference).
 *   - FLOWS: trip i has a start point, an end point and an hour.  It is BAD when its hour is outside 0 .. 23 or a coordinate is outside the domain: dropped and
 *     counted.  Otherwise, with s and e the regions of its points, it adds 1 to c(hour, s, e) when both are >= 0.  The table is the triples with c > 0,
 *     ascending by (hour, s, e), counts int64; adding trips in several calls gives the same table, bit for bit, as adding them in one.
 *   - SLOTS, T time slices out of the 24 hours.  DGE_SLOTS_EVEN: T divides 24, hour h belongs to slot h / (24/T); T = 1 is the static graph (taxi-all.od,
 *     J/Tracts.java:251-260).  DGE_SLOTS_AS_TRACTS is Tracts.outputEdgeFile as written (J/Tracts.java:236-249): 1 <= T <= 24, step = 24 / T (integer division),
 *     slot k holds for every (s, e) with c(k, s, e) > 0 the weight c(k, s, e) + .. + c(k+step-1, s, e) — the windows overlap, start at hour k, and only
 *     destinations seen in hour k itself appear.  With T = 24 the modes agree.  A slot edge is (slot, ids[s], ids[e], w), w > 0; slot edges stand ascending by
 *     (slot, src id, dst id).
 *   - dge_graph_add_flows leaves g exactly where dge_graph_add_od_texts leaves it when slice k's text is the lines "%d %d %d\n" % (src id, dst id, w) of slot k
 *     in that order: same fresh-graph and names-empty rules, same statuses, the same commit path (csrc/od_commit.h); info: bytes = lines = 0, flows = edges = the
 *     slot edges, dropped = host_values = 0.  On error g and names are as they were.
 *   - Null / negative arguments, an unclosed or short ring, duplicate ids, a vertex outside the domain (the message names region, ring and vertex), a T the mode
 *     refuses: DGE_ERR_ARG before a device is looked for.  cap too small: DGE_ERR_CAP with *n set.  T*R' > 2^31-1: DGE_ERR_RANGE.  Out of device memory:
 *     DGE_ERR_CAP.  R = 0, n = 0 and an empty table are fine.
 * (dge_regions_info and dge_flows_info name a struct and a function each: write `struct dge_regions_info`, as C requires.) */
typedef struct dge_regions dge_regions;   /* rings + cell index, resident in HBM */
typedef struct dge_flows   dge_flows;     /* sorted (hour, s, e, count) table, resident in HBM; holds a reference to its regions */
enum { DGE_SLOTS_EVEN = 0, DGE_SLOTS_AS_TRACTS = 1 };
struct dge_regions_info {
    int64_t regions;              /* R                                                                  */
    int64_t rings;
    int64_t segments;             /* ring vertices minus rings                                          */
    int64_t max_cell_candidates;  /* the longest list of candidate regions a cell has                   */
    int32_t grid;                 /* the index has grid x grid cells                                    */
    int32_t tile_segments;        /* segments one LDS tile holds                                        */
    double  x0;                   /* the bounding box of all rings: x0 <= x <= x1, y0 <= y <= y1        */
    double  y0;
    double  x1;
    double  y1;
};                                /* 72 bytes */
typedef struct dge_locate_info {
    int64_t points;
    int64_t located;              /* region >= 0                                                        */
    int64_t on_boundary;          /* region -1 and on some ring                                         */
    int64_t multi;                /* interior to more than one region                                   */
    int64_t outside;              /* outside every region's bounding box (out-of-domain points included) */
    int64_t exact;                /* side tests that went past the floating-point filter                */
    double  kernel_ms;
} dge_locate_info;                /* 56 bytes */
struct dge_flows_info {           /* everything accumulates over the calls that added trips             */
    int64_t trips;
    int64_t mapped;               /* both regions found                                                 */
    int64_t bad;                  /* hour outside 0 .. 23 or a coordinate outside the domain            */
    int64_t no_start;             /* not bad, no region for the start point                             */
    int64_t no_end;               /* start found, end not                                               */
    int64_t entries;              /* triples in the table                                               */
    int64_t located;              /* the two points' locate counters, summed                            */
    int64_t on_boundary;
    int64_t multi;
    int64_t outside;
    int64_t exact;
    double  kernel_ms;
};                                /* 96 bytes */
/* replaces the map of Tract(id, MultiPolygon boundary) the constructor fills (J/Tracts.java:26-43); grid 0: the library's rule, n > 0: n x n cells */
int  dge_regions_create(int device, const int64_t* ids, int64_t R, const int64_t* ring_first, const int64_t* vert_first, const double* xy, int64_t n_rings, int64_t n_verts,
                        int32_t grid, dge_regions** out);
int  dge_regions_info(const dge_regions* r, struct dge_regions_info* out);
/* replaces the boundary.contains loop (J/Tracts.java:82-86) for n points; region: host int32[n] */
int  dge_regions_locate(const dge_regions* r, const double* xy, int64_t n, int32_t* region, dge_locate_info* info /* may be NULL */);
int  dge_regions_locate_device(const dge_regions* r, const double* d_xy, int64_t n, int32_t* d_region, dge_locate_info* info /* may be NULL */);
void dge_regions_free(dge_regions* r);
/* replaces Tract.taxiFlows / CommunityArea.taxiFlows and Tracts.mapTripsIntoTracts (J/Tracts.java:71-102), J/CommunityAreas.java:55-103 */
int  dge_flows_create(const dge_regions* r, dge_flows** out);
int  dge_flows_add_trips(dge_flows* f, const double* start_xy, const double* end_xy, const int32_t* hour, int64_t n);              /* host arrays */
int  dge_flows_add_trips_device(dge_flows* f, const double* d_start_xy, const double* d_end_xy, const int32_t* d_hour, int64_t n);
int  dge_flows_info(const dge_flows* f, struct dge_flows_info* out);
/* the table, region INDICES; replaces Tracts.serializeTracts (J/Tracts.java:104) as the way to keep the result */
int  dge_flows_to_host(const dge_flows* f, int32_t* hour, int32_t* src, int32_t* dst, int64_t* count, int64_t cap, int64_t* n);
/* replaces Tracts.outputEdgeFile / outputStaticEdgeFile (J/Tracts.java:236-260): the lines of the T files as arrays */
int  dge_flows_slot_edges(const dge_flows* f, int32_t T, int32_t mode, int32_t* slot, int64_t* src_id, int64_t* dst_id, int64_t* w, int64_t cap, int64_t* n);
void dge_flows_free(dge_flows* f);
/* replaces outputEdgeFile followed by CrossTimeGraph.constructGraphFromOD (J/CrossTimeGraph.java:25-52): no text in between */
int  dge_graph_add_flows(dge_graph* g, const dge_flows* f, int32_t T, int32_t mode, struct dge_names* names /* may be NULL */, dge_od_info* info /* may be NULL */);

/* ---- hour windows of the flow table (new; additions only, DGE_VERSION unchanged): the reads of taxiFlows by hour interval — Tract.getFlowTo(d, lo, hi)
 * (J/Tracts.java:477-482), CommunityArea.getFlowTo(d, lo, hi) (J/CommunityAreas.java:240-245) — and what the reference builds on them: the cross-time graph
 * DeepWalk trains on (CrossTimeGraph.constructGraph_tract, J/CrossTimeGraph.java:25-52), the hand-picked intervals (constructGraph_CA(int[]), :68-95), the
 * brute-force triplet search (Tracts.bruteForceSearchCase, J/Tracts.java:371-415), and the way back into the table (deserialzeTracts, J/Tracts.java:115-125)
 * — on the device (csrc/flow_windows.hip, csrc/flow_rule.h).  Everything is integer arithmetic; the results are pure functions of the table and the arguments,
 * whatever calls built the table, and nothing depends on timing or launch geometry.  The rule:
 *   - An HOUR WINDOW (start, hours) holds the hours start, start+1, .., start+hours-1, each mod 24.  0 <= start <= 23, 0 <= hours <= 24; hours = 0 is an empty
 *     window, not an error.  Tract.getFlowTo(d, lo, hi) is (lo, hi-lo+1) with hi <= 23 (inclusive high, no wrap); CommunityArea.getFlowTo(d, lo, hi) is
 *     (lo, (hi-lo) mod 24) (exclusive high, wrapping).  W(start, hours)[s, e] is the int64 sum of c(h, s, e) over the window's hours.
 *   - The WINDOW EDGES of a list of K windows are the tuples (k, ids[s], ids[e], w) with w = W_k[s, e] > 0, ascending by (k, src id, dst id).  Windows may
 *     overlap, repeat and be empty.  1 <= K; K*R*R must fit 63 bits, and for a graph K*R' <= 2^31-1 as for slots: else DGE_ERR_RANGE.  constructGraph_tract
 *     with numLayer = T is the windows (h, 24/T), h = 0 .. T-1, over ALL destinations; DGE_SLOTS_AS_TRACTS keeps only destinations seen in hour h itself, so
 *     the two differ whenever a pair is silent in hour h and not in the rest of the window.
 *   - dge_flows_add_entries takes host arrays: hour in 0 .. 23, region INDICES in 0 .. R-1, count >= 1, in any order, with repeats, over any number of calls.
 *     The table stands bit for bit where dge_flows_add_trips leaves it on `count` trips per entry; info.trips and info.mapped grow by the counts added, the
 *     other counters do not move.  A bad hour, index or count: DGE_ERR_ARG naming the least offending position.  A key's total above 2^40: DGE_ERR_RANGE.  On
 *     any error the table is as it was.
 *   - dge_graph_add_flow_windows leaves g exactly where dge_graph_add_od_texts leaves it when slice k's text is the lines "%d %d %d\n" % (src id, dst id, w) of
 *     window k's edges in that order: the commit path (csrc/od_commit.h), the fresh-graph and names rules and the statuses of dge_graph_add_flows; info as there,
 *     slices = K.
 *   - The TRIPLET SEARCH.  A rule holds five windows A, B, C, D, E, the minima min_a, min_b (0 .. 2^40) and ratio r (1 .. 65536).  A triplet of pairwise distinct
 *     regions (t1, t2, t3) — residence, office, night life — is kept iff all ten conditions hold (J/Tracts.java:391-400 negated), W[x,y] = W[t_x, t_y]:
 *        1  A[1,2] > min_a        2  B[3,1] > min_b          3  B[2,3] > min_b          4  A[1,2] > r A[2,1]       5  C[1,3] > r D[1,3]
 *        6  C[2,1] > r C[1,2]     7  C[2,3] > r D[2,3]       8  B[3,1] > r E[3,1]       9  B[3,1] > r B[3,2]      10  B[3,1] > r B[1,3]
 *     An absent pair is 0; self flows play no part.  The conditions read THIRTEEN distinct sums; dge_triplet_rule_check takes them in the order
 *        A12, A21, C21, C12, B31, E31, C13, D13, B13, B23, C23, D23, B32
 *     (sums[0] .. sums[12]) and needs no device.  Conditions 1, 4, 6 belong to the pair (t1, t2), 3, 7 to (t2, t3), 2, 5, 8, 10 to (t3, t1); the ninth needs all
 *     three.  The result is the triplets as region IDS, ascending by (id1, id2, id3): the reference's HashMap order is not an order.  dge_triplet_info: the
 *     ordered pairs of distinct regions that pass their pair's conditions, the triangles of three such pairs over pairwise distinct regions before the ninth
 *     condition (candidates), and the triplets.  The default rule holds the reference's constants: A = (7,3), B = (17,7), C = (17,6), D = (7,6), E = (7,7),
 *     min_a = 30, min_b = 70, ratio = 2.
 *   - dge_flows_window_edges and dge_flows_triplets: cap too small is DGE_ERR_CAP with *n set, cap = 0 with null outputs is a size query.  The plain values
 *     are checked first, the handles after: null or negative arguments, a bad window and a bad rule are DGE_ERR_ARG before a device is looked for.  Out of
 *     device memory: DGE_ERR_CAP.  R < 3, an empty table and an empty window are fine. */
typedef struct dge_hour_window { int32_t start; int32_t hours; } dge_hour_window;      /* 8 bytes */
typedef struct dge_triplet_rule {
    dge_hour_window A;            /* morning:            the reference's getFlowTo(.., 7, 9)               */
    dge_hour_window B;            /* evening and night:  (.., 17, 23)                                      */
    dge_hour_window C;            /* evening:            (.., 17, 22)                                      */
    dge_hour_window D;            /* day:                (.., 7, 12)                                       */
    dge_hour_window E;            /* day, an hour more:  (.., 7, 13)                                       */
    int64_t min_a;
    int64_t min_b;
    int32_t ratio;
    int32_t reserved;             /* 0                                                                     */
} dge_triplet_rule;               /* 64 bytes */
typedef struct dge_triplet_info {
    int64_t pairs_12;             /* (t1, t2), t1 != t2, that pass conditions 1, 4, 6                       */
    int64_t pairs_23;             /* (t2, t3) that pass 3, 7                                                */
    int64_t pairs_31;             /* (t3, t1) that pass 2, 5, 8, 10                                         */
    int64_t candidates;           /* triangles of three such pairs, pairwise distinct, before the ninth    */
    int64_t triplets;
    double  kernel_ms;
} dge_triplet_info;               /* 48 bytes */
/* replaces Tracts.deserialzeTracts (J/Tracts.java:115-125): what dge_flows_to_host gave goes back in */
int  dge_flows_add_entries(dge_flows* f, const int32_t* hour, const int32_t* src, const int32_t* dst, const int64_t* count, int64_t n);
/* replaces the getFlowTo(dst, lo, hi) loops over all pairs; k: int32[cap], the others int64[cap] */
int  dge_flows_window_edges(const dge_flows* f, const dge_hour_window* win, int32_t K, int32_t* k, int64_t* src_id, int64_t* dst_id, int64_t* w, int64_t cap, int64_t* n);
/* replaces CrossTimeGraph.constructGraph_tract and constructGraph_CA(int[] timeIntervals) (J/CrossTimeGraph.java:25-52, 68-95) */
int  dge_graph_add_flow_windows(dge_graph* g, const dge_flows* f, const dge_hour_window* win, int32_t K, struct dge_names* names /* may be NULL */, dge_od_info* info /* may be NULL */);
int  dge_triplet_rule_default(dge_triplet_rule* rule);
/* the ten conditions on thirteen given sums: *keep = 1 or 0.  No device, no table */
int  dge_triplet_rule_check(const dge_triplet_rule* rule /* NULL: the default */, const int64_t sums[13], int32_t* keep);
/* replaces Tracts.bruteForceSearchCase (J/Tracts.java:371-415); id1, id2, id3: int64[cap] */
int  dge_flows_triplets(const dge_flows* f, const dge_triplet_rule* rule /* NULL: the default */, int64_t* id1, int64_t* id2, int64_t* id3, int64_t cap, int64_t* n,
                        dge_triplet_info* info /* may be NULL */);

/* ---- flow table out as text (new; additions only, DGE_VERSION unchanged): the files the reference writes from taxiFlows and its later stages open — the
 * .od edge files (Tracts.outputEdgeFile / outputStaticEdgeFile, J/Tracts.java:236-264; CommunityAreas.outputStaticFlowGraph, J/CommunityAreas.java:127-146),
 * the .matrix adjacency files (Tracts.outputAdjacencyMatrix, J/Tracts.java:269-301, comma-separated; CommunityAreas.outputAdjacencyMatrix,
 * J/CommunityAreas.java:148-166, blank-separated), the layered edge text of outputEdgeGraph_crossInterval (J/Tracts.java:314-330) and the in / out traffic
 * time series (Tracts.timeSeries_traffic, J/Tracts.java:187-224) — sized and spelled on the device (csrc/flow_text.hip, csrc/flow_text_plan.h); the host only
 * moves bytes.  Everything is integer arithmetic; every text is a pure function of the table and the arguments, whatever calls built the table, and nothing
 * depends on timing, launch geometry, tile size or slab size.  The rule:
 *   - SLICES.  A dge_flow_slices names S edge sets.  K == 0: the S = T slot-edge sets of dge_flows_slot_edges(T, mode).  K >= 1: the S = K window-edge sets of
 *     dge_flows_window_edges(win, K); T and mode must then be 0.  reserved is 0.  The checks and statuses are those two entries' own.
 *   - DECIMALS.  An integer is written as %lld writes it: a '-' when negative, no '+', no leading zeros.  Region ids are int64 of any sign; weights are
 *     positive int64 (a key holds 2^40 at most, so a sum reaches 24 * 2^40: 14 digits).
 *   - DGE_FLOW_TEXT_OD.  Slice k is one text: the lines "<src id> <dst id> <w>\n" of the slice's edges, ascending by (src id, dst id) — the text the contracts
 *     of dge_graph_add_flows and dge_graph_add_flow_windows describe.  A slice without edges is the empty text.  T = 1, DGE_SLOTS_EVEN gives taxi-all.od.
 *   - DGE_FLOW_TEXT_OD_LAYERED.  ONE text for all S slices: the lines "<k>-<src id> <(k+1) mod S>-<dst id> <w>\n", ascending by (k, src id, dst id).  With
 *     the 24 windows (h, 1) it is taxi-crossInterval.od up to the reference's HashMap order, which is not an order.
 *   - DGE_FLOW_TEXT_MATRIX.  Slice k is one text of n lines: line i holds the n decimals W_k[r_i, r_j], j ascending, 0 for an absent pair, each followed by ONE
 *     byte: sep, or '\n' behind the last.  r_0 .. r_{n-1} are all R regions in ascending id (select == NULL) or the regions with a non-zero select byte (one
 *     byte per region, by region index) in ascending id; entries whose other endpoint is not selected play no part.  sep is ',' (tracts, CA static), ' ' (CA
 *     hourly) or '\t'.  n = 0 gives the empty text.  No header.  Nothing of size n^2 is formed on the device: its memory is bounded by the edges and two slabs.
 *     For the two .od kinds sep must be 0 and select NULL.
 *   - The TIME SERIES.  For the selected regions (as above; the reference's focusKeys) in ascending id and every hour h = 0 .. 23: out[r][h] is the sum of
 *     c(h, r, e) over ALL destinations e; in[r][h] is the sum of c(h, s, r) over the SELECTED sources s, r itself included.  The asymmetry is the
 *     reference's as written (J/Tracts.java:200-206: the flows into a focus tract are looked up in the focus tracts only) and is kept.  The text has two lines
 *     per region: "<id>,<in_0>,..,<in_23>\n" and "<-id>,<out_0>,..,<out_23>\n"; <-id> is the decimal of the negated id, so id 0 gives 0 twice.  A selected id
 *     of -2^63 cannot be negated: DGE_ERR_RANGE naming the region.  Sums are int64 and may be 0.
 *   - NOT CARRIED OVER: CommunityAreas.outputEdgeGraph_LINE (J/CommunityAreas.java:171-186) writes zero-weight lines and stops one column short (j < size): a
 *     quirk with no consumer in either tree.  The three-node .dot case files (J/Tracts.java:127-182) are host work on nine numbers.
 * dge_flow_text_info: edges are the table-derived numbers spelled with their value (.od lines, non-zero matrix entries, the 48 sums of a region's two series
 * lines), zeros the matrix entries written as "0"; over dge_flows_write_text everything is summed over the files.
 * Statuses, those of the .seq writer:
 *   - Null or negative arguments, a bad kind, sep, select, slice, n_paths or slices struct: DGE_ERR_ARG.  Plain values are checked before handles, and all of it
 *     before a device is looked for.
 *   - cap smaller than the text: DGE_ERR_CAP with *n_bytes set and text untouched; text == NULL with cap == 0 is a size query.
 *   - Everything the sizing pass can find is found before a file is created or truncated.  A file is created or truncated, never appended to; files are written
 *     in slice order; an open or write failure is DGE_ERR_IO with the path and the OS error, and the files finished before it stay.
 *   - Out of device memory: DGE_ERR_CAP with the bytes asked for.
 *   - The entries only read the table: after any call dge_flows_to_host and dge_flows_info give what they gave before. */
enum { DGE_FLOW_TEXT_OD = 0, DGE_FLOW_TEXT_OD_LAYERED = 1, DGE_FLOW_TEXT_MATRIX = 2 };
typedef struct dge_flow_slices {
    int32_t T;                    /* K == 0: the slots of dge_flows_slot_edges(T, mode)                     */
    int32_t mode;
    int32_t K;                    /* K >= 1: the windows win[0 .. K) of dge_flows_window_edges; T = mode = 0 */
    int32_t reserved;             /* 0                                                                      */
    const dge_hour_window* win;
} dge_flow_slices;                /* 24 bytes */
typedef struct dge_flow_text_info {
    int64_t bytes;
    int64_t lines;
    int64_t edges;                /* table-derived entries that were spelled with their weight              */
    int64_t zeros;                /* MATRIX: entries written as "0"                                         */
    int32_t slices;               /* texts produced                                                         */
    int32_t reserved;
    double  kernel_ms;            /* as in dge_seq_out_info: the edges' passes, sizing, every slab's emit   */
    double  write_ms;             /* the slab loops: copies to pinned memory and write() / memcpy           */
} dge_flow_text_info;             /* 56 bytes */
/* one text into host memory; slice is ignored (must be 0) for OD_LAYERED.  text == NULL with cap == 0: size query */
int  dge_flows_to_text(const dge_flows* f, const dge_flow_slices* s, int32_t kind, int32_t slice, const uint8_t* select, int32_t sep,
                       char* text, int64_t cap, int64_t* n_bytes /* required */, dge_flow_text_info* info /* may be NULL */);
/* every slice to its own file: n_paths == number of slices (1 for OD_LAYERED); the edges are formed once */
int  dge_flows_write_text(const dge_flows* f, const dge_flow_slices* s, int32_t kind, const uint8_t* select, int32_t sep,
                          const char* const* paths, int32_t n_paths, dge_flow_text_info* info /* may be NULL */);
/* in_flow / out_flow: host int64[cap * 24], region_index int64[cap]; cap too small: DGE_ERR_CAP with *n set; cap == 0 with nulls: size query */
int  dge_flows_time_series(const dge_flows* f, const uint8_t* select, int64_t* in_flow, int64_t* out_flow, int64_t* region_index, int64_t cap, int64_t* n);
int  dge_flows_time_series_text(const dge_flows* f, const uint8_t* select, char* text, int64_t cap, int64_t* n_bytes, dge_flow_text_info* info /* may be NULL */);
int  dge_flows_write_time_series(const dge_flows* f, const uint8_t* select, const char* path, dge_flow_text_info* info /* may be NULL */);

/* ---- .matrix adjacency text in (new; additions only, DGE_VERSION unchanged): the files DGE_FLOW_TEXT_MATRIX writes, and the reference's taxi-h%d.matrix that
 * P/matrixFactorization_tract.py:35 reads with np.loadtxt(delimiter=",") and indexes by f[idx,:][:,idx] (P/flowFeatureGeneration_tract.py:29-40 and
 * P/flowFeatureGeneration_CA.py:30-41 do the same), go back into a flow table on the device (csrc/matrix_read.hip, csrc/matrix_parse.h, csrc/matrix_feed.h).  The
 * text streams through the device in slabs; only the values > 0 leave it, and nothing of size n^2 or one record per value is formed.  A text is BYTES.  The rule:
 *   - PARAMETERS.  sep is ',', ' ' or '\t', the three separators of DGE_FLOW_TEXT_MATRIX.  select is one byte per region index, NULL meaning all R regions, as
 *     in dge_flows_to_text; n is the number of selected regions and r_0 .. r_{n-1} are they in ascending id.
 *   - LINES.  A line ends at '\n'; a '\r' directly before that '\n' belongs to the terminator.  The last line of a piece may lack its terminator; nothing
 *     follows a final terminator.  No line crosses a piece.  A line of zero bytes is skipped: it is counted in info.lines and not in info.rows.  There is no
 *     limit on a line's length.
 *   - VALUES.  A non-empty line is values separated by exactly one sep byte; its VALUE COUNT is its separators + 1.  A value is 1 to 19 decimal digits; leading
 *     zeros are allowed (007 is 7).  No sign, no blank, no fraction, no exponent: Integer.toString of a flow count and the writer's %lld both fall inside this.
 *   - MEANING.  Piece k belongs to hour hour[k] in 0 .. 23; several pieces may share an hour.  Each piece must hold exactly n non-empty lines of exactly n
 *     values.  Value j of non-empty line i, when > 0, adds itself to c(hour[k], r_i, r_j); the diagonal is included; zeros add nothing.
 *   - THE TABLE AFTER A CALL stands bit for bit where dge_flows_add_entries leaves it on the same (hour, region index, region index, value) entries;
 *     info.trips and info.mapped of dge_flows_info grow by the sum of the values, the other counters do not move.
 *   - OFFENCES.  Each has a PLACE, a byte offset inside its piece.  The call reports the offence at the least (piece, offset), and of two at one place the one
 *     listed first here.  The message names the kind, the piece (and its path), the offset, the LINE — 1 + the '\n' bytes of the piece in front of the place,
 *     so empty lines count — and the COLUMN — the sep bytes between the start of that line and the place, so columns count from 0:
 *       "<entry>: <kind> at piece <k>[ (<path>)], offset <o>, line <l>, column <c>[: ..]".
 *        bad byte          anything that is not a digit, sep, '\n', or a '\r' directly followed by '\n'; a NUL is a bad byte.  Place: that byte.  DGE_ERR_IO.
 *        empty value       a sep at the start of a line, or a sep, a terminator or the piece's end directly after a sep.  Place: that byte (of "\r\n" the
 *                          '\r'), or the piece's size at the piece's end.  DGE_ERR_IO.
 *        long value        the 20th consecutive digit.  Place: that digit.  DGE_ERR_IO.  A run of 20 digits or more is no value: it is never "above 2^40".
 *        value above 2^40  a maximal run of 1 .. 19 digits greater than 2^40, whatever stands around it.  Place: its first byte, a leading zero included.
 *                          DGE_ERR_RANGE.
 *        ragged line       a non-empty line whose value count is not n.  Place: its terminator's first byte, or the piece's size.  DGE_ERR_IO, with the
 *                          count found and the count expected.
 *        too many rows     place: the first byte of non-empty line n + 1.  DGE_ERR_IO.
 *        too few rows      place: the piece's size (0 for a piece without a byte).  DGE_ERR_IO.
 *   - OTHER STATUSES.  A key's total above 2^40, or the values adding up beyond 2^62: DGE_ERR_RANGE, as in dge_flows_add_entries.  Null or negative arguments, a
 *     bad sep, a bad hour, n_pieces < 1, a select array when R = 0, non-zero reserved fields and a slab_bytes that is neither 0 nor in 256 .. 16 MiB:
 *     DGE_ERR_ARG; plain values are checked before handles, and all of it before a device is looked for or a file is opened.  A missing or unreadable file:
 *     DGE_ERR_IO with its path.  Out of device memory: DGE_ERR_CAP.  On any error the table is as it was: all pieces are staged and there is one commit at the end.
 *   - PURITY.  The result — table, counters, the offence reported — is a pure function of the bytes, hour, select and sep.  It does not depend on slab_bytes,
 *     the tile size, launch geometry or timing.
 *   - NOT CARRIED OVER: signs, floats (np.savetxt's default %.18e), padding blanks and headers are bad bytes here; the time-series text
 *     (taxi-flow-time-series.txt is 1 602 short lines) is read by dge_counts_add_table_texts (the count tables below), not here.
 * dge_matrix_read_info: lines counts every line, rows the non-empty ones, values = rows * n, entries the values > 0, zeros the others, total the sum of the
 * values; tile_bytes is the text one workgroup takes, slabs the slabs sent; read_ms is the host's reading into pinned memory, kernel_ms the kernels of the slabs
 * and of the commit.  It is filled on success only. */
typedef struct dge_matrix_read_options {
    int32_t sep;                  /* ',', ' ' or '\t'                                                       */
    int32_t reserved;             /* 0                                                                      */
    int64_t slab_bytes;           /* 0: the default, 16 MiB (the most); else 256 at least                   */
} dge_matrix_read_options;        /* 16 bytes */
typedef struct dge_matrix_read_info {
    int64_t bytes;                /* offset 0                                                               */
    int64_t lines;                /* 8                                                                      */
    int64_t rows;                 /* 16                                                                     */
    int64_t values;               /* 24                                                                     */
    int64_t entries;              /* 32: values > 0                                                         */
    int64_t zeros;                /* 40                                                                     */
    int64_t total;                /* 48: the sum of the values                                              */
    int32_t pieces;               /* 56                                                                     */
    int32_t n;                    /* 60                                                                     */
    int32_t tile_bytes;           /* 64: bytes of text one workgroup takes                                  */
    int32_t slabs;                /* 68                                                                     */
    double  read_ms;              /* 72                                                                     */
    double  kernel_ms;            /* 80                                                                     */
} dge_matrix_read_info;           /* 88 bytes */
/* texts[k]: n_bytes[k] bytes, piece k of hour hour[k] */
int  dge_flows_add_matrix_texts(dge_flows* f, const char* const* texts, const int64_t* n_bytes, const int32_t* hour, int32_t n_pieces,
                                const uint8_t* select, const dge_matrix_read_options* opt, dge_matrix_read_info* info /* may be NULL */);
/* the same for files, streamed: the host holds two slabs of a file at a time */
int  dge_flows_add_matrix_files(dge_flows* f, const char* const* paths, const int32_t* hour, int32_t n_pieces,
                                const uint8_t* select, const dge_matrix_read_options* opt, dge_matrix_read_info* info /* may be NULL */);

/* ---- taxi trip text in (new; additions only, DGE_VERSION unchanged): the lines the reference reads in TaxiTrip(String line) and ShortDate
 * (J/TaxiTrip.java:39-78,199-223; the loops J/TaxiTrip.java:123-143 and J/TaxiTripIterator.java:32-62) are parsed on the device (csrc/trip_text.hip, csrc/trip_parse.h)
 * and go into a flow table without per-trip work on the host.  The rule; the result is a pure function of the bytes, the format and the header flag — nothing
 * depends on timing, launch geometry or slab_bytes:
 *   - LINES.  The text is BYTES in pieces (a file, or a text).  A line ends at "\n", "\r\n" or a lone "\r" (BufferedReader.readLine); a last line without a
 *     terminator counts; nothing follows a final terminator.  No line crosses a piece: a "\r" that ends piece A and a "\n" that opens piece B are two terminators,
 *     and B begins with an empty line.  header != 0: the first line of every piece is skipped and counted in header_lines (J/TaxiTrip.java:128); header == 0: it is
 *     parsed like any other (TaxiTripIterator).  No byte is an error, NUL included: text is never refused, lines are good or bad.
 *     DEVIATION: a line longer than 65 535 bytes is status 3 whatever it holds (the reference would parse it).
 *   - SPLIT(s, set) cuts at every byte of set; empty pieces are kept, except that all trailing empty pieces go; an empty s is one empty piece, an s of only
 *     separators is no piece.  SPLIT+ treats a run of separators as one; a leading separator still leaves a leading empty piece.  SPLIT2(s) cuts at the first blank
 *     only: one or two pieces, the second may be empty.  (Java 8 String.split for ",", "\t", "\t+", "[/ :]", "/" and (" ", 2).)
 *   - INT(s, lo, hi): [+-] digits, at least one digit, ASCII digits only, leading zeros allowed, the value in [lo, hi]; else the parse fails.  BYTE is INT with
 *     -128 .. 127, INT32 with the int32 range.
 *   - COORD(s): bytes <= 0x20 go at both ends; then the value grammar of the .od weights above without its inf / nan words; the value is the binary64 nearest the
 *     exact decimal, ties to even (csrc/od_parse.h; the few tokens it hands back are finished by the host with strtod and counted in host_values).  A result that
 *     is not finite fails.  DEVIATION: so do hex floats and the f / d suffixes, which Double.parseDouble takes; NaN and Infinity, which it takes too, fail here —
 *     the flow table is the same either way, because a point that is not finite lies in no region.
 *   - DATE1(s): f = SPLIT(s, "/ :"), at least 5 pieces; BYTE(f0), BYTE(f1), BYTE(f4) must parse; hour = BYTE(f3), as it stands.
 *   - DATE2(date, time): d = SPLIT(date, "/"), at least 2 pieces, BYTE(d0) and BYTE(d1) must parse; t = SPLIT(time, " :"), at least 4 pieces, BYTE(t1) must parse;
 *     h = BYTE(t0); hour = h % 12 + 12 when t3 is exactly "PM", else h % 12 — the remainder truncating, as Java's.
 *   - DGE_TRIPS_TYPE1: p = SPLIT+(line, "\t"), exactly 13 pieces.  DATE1(p7) gives the hour, DATE1(p8) must parse.  A GPS piece g has length >= 2; its first and
 *     last byte go, then q = SPLIT(., ","), at least 2 pieces, y = COORD(q0), x = COORD(q1).  Start point p9, end point p10.  INT32(p2) must parse.
 *   - DGE_TRIPS_TYPE2: p = SPLIT(line, "\t"), exactly 17 pieces.  DATE2(p0, p1) gives the hour, DATE1(p2) must parse.  start = (COORD(p9), COORD(p10)),
 *     end = (COORD(p11), COORD(p12)), each (x, y).  INT32(p15) must parse.
 *   - DGE_TRIPS_TYPE3: p = SPLIT(line, ","), exactly 21 pieces; there is no quoting.  a = SPLIT2(p0), b = SPLIT2(p1), 2 pieces each.  DATE2(a0, a1) gives the hour,
 *     DATE2(b0, b1) must parse.  start = (COORD(p16), COORD(p15)), end = (COORD(p19), COORD(p18)).  INT32(p2) must parse.
 *   - STATUS of a line: 0 ok; 1 the line's piece count is wrong (the reference's badTrip; an empty line is status 1); 2 anything else failed; 3 too long.  An hour
 *     outside 0 .. 23 does not make a line bad: dge_flows drops and counts such trips.
 *   - dge_trips_parse_texts returns one record per non-header line, in text order, in host arrays (start_xy / end_xy: x, y interleaved); a record of status != 0
 *     has hour -1 and zeros.  cap too small: DGE_ERR_CAP with *n_lines set.
 *   - dge_flows_add_trip_texts / _files leave f exactly where dge_flows_add_trips leaves it when given the status-0 records of the same text, bit for bit, the
 *     counters of dge_flows_info included.  The trips gather in a table of their own that is merged into f at the end: on any error f is as it was.  All files are
 *     opened before anything runs; a missing or unreadable file: DGE_ERR_IO with its path.  Out of device memory: DGE_ERR_CAP.
 *   - The text streams through the device in slabs of slab_bytes (0: the library's rule, 16 MiB; else at least 131072; above 2^30 is taken as 2^30): device memory
 *     does not grow with the text.
 *   - Null / negative arguments, an unknown format, slab_bytes in 1 .. 131071: DGE_ERR_ARG before a device is looked for. */
enum { DGE_TRIPS_TYPE1 = 1, DGE_TRIPS_TYPE2 = 2, DGE_TRIPS_TYPE3 = 3 };
struct dge_trip_text_options {
    int32_t format;       /* DGE_TRIPS_TYPE1 .. DGE_TRIPS_TYPE3                                           */
    int32_t header;       /* != 0: the first line of every piece is a header                              */
    int64_t slab_bytes;   /* 0: the library's rule; else >= 131072                                        */
};                        /* 16 bytes */
typedef struct dge_trip_text_info {
    int64_t bytes;        /* bytes of text taken (the pieces' sizes added up)                             */
    int64_t lines;        /* lines, headers and a last one without a terminator included                  */
    int64_t header_lines; /* lines skipped as headers                                                     */
    int64_t ok;           /* records of status 0                                                          */
    int64_t bad_fields;   /* status 1                                                                     */
    int64_t bad_parse;    /* status 2                                                                     */
    int64_t too_long;     /* status 3                                                                     */
    int64_t host_values;  /* coordinates the host finished with strtod                                    */
    int64_t slabs;        /* slabs the text went through the device in                                    */
    double  read_ms;      /* filling the pinned buffers (file reads included)                             */
    double  kernel_ms;    /* the text's device passes (the flow table's are in dge_flows_info)            */
} dge_trip_text_info;     /* 88 bytes */
int  dge_trips_parse_texts(int device, const char* const* texts, const int64_t* n_bytes, int32_t n, const struct dge_trip_text_options* opt, uint8_t* status, int32_t* hour,
                           double* start_xy, double* end_xy, int64_t cap, int64_t* n_lines, dge_trip_text_info* info /* may be NULL */);
/* replace the loops over TaxiTrip lines in front of Tracts.mapTripsIntoTracts (J/TaxiTrip.java:123-143, J/TaxiTripIterator.java:32-62) */
int  dge_flows_add_trip_texts(dge_flows* f, const char* const* texts, const int64_t* n_bytes, int32_t n, const struct dge_trip_text_options* opt, dge_trip_text_info* info /* may be NULL */);
int  dge_flows_add_trip_files(dge_flows* f, const char* const* paths, int32_t n, const struct dge_trip_text_options* opt, dge_trip_text_info* info /* may be NULL */);

/* ---- the spatial graph (new; additions only, DGE_VERSION unchanged): SpatialGraph.constructGraph_tract / constructGraph_CA (J/SpatialGraph.java:37-88) take the
 * centroid of every region's MultiPolygon (J/Tracts.java:484-497), form all R^2 weights exp(-d * 100), call addEdge R^2 times and keep the 10 heaviest edges of every
 * vertex.  Here the centroids, the weights and the selection happen on the device next to the resident rings (csrc/spatial.hip, csrc/spatial_weight.h), fused:
 * nothing of size R^2 ever exists.  The rule; the result is a pure function of the inputs, nothing depends on timing, launch geometry or tile sizes:
 *   - CENTROID of region r: the area-weighted centroid that JTS's Geometry.getCentroid() returns for a MultiPolygon (as recalled: its source was not consulted;
 *     what follows is the rule).  The base point b is the first vertex of the region's first ring.  Over the rings in order and the segments (p, q) of each
 *     ring in order:  a2 = (p.x-b.x)*(q.y-b.y) - (q.x-b.x)*(p.y-b.y);  cx += a2*(b.x+p.x+q.x);  cy += a2*(b.y+p.y+q.y);  A += a2.  The centroid is
 *     (cx/3/A, cy/3/A).  Every operation is a rounded binary64 operation in exactly that order, operands left to right, nothing fused.
 *   - Rings contribute with their own orientation: dge_regions does not tell shells from holes.  With the shapefile convention (shells clockwise, holes
 *     counter-clockwise) this is JTS's sum term for term.  Reversing every ring of a region negates every a2 exactly, and the sign cancels in cx/A: the
 *     centroid is the same point — the same bits where the sums are exact (dyadic coordinates of a few bits); with rounded coordinates the reversed rings are
 *     summed in another order and the result agrees to rounding.
 *   - A == 0 (a region without a ring included) or a centroid that is not finite: DGE_ERR_ARG naming the region.  DEVIATION: JTS falls back to the centroid of
 *     the lines.
 *   - DISTANCE: d(i,j) = sqrt(dx*dx + dy*dy), dx = ci.x - cj.x, dy = ci.y - cj.y (Coordinate.distance); sqrt correctly rounded.  d may be +inf (finite
 *     centroids can overflow dx*dx): the weight is then 0, not an error.
 *   - WEIGHT: w(i,j) = E((-d) * scale); the reference's scale is 100 (J/SpatialGraph.java:46,74).  E is one fixed sequence of rounded binary64 + - * /,
 *     shaped like fdlibm's e_exp (the algorithm java.lang.StrictMath.exp is defined by) and written once in csrc/spatial_weight.h.  For x <= 0:
 *       x < -0x1.74910d52d3051p+9: 0 (E(-inf) = 0; underflow goes to 0);  x >= -0x1p-28: 1 + x (E(-0.0) = E(0) = 1);
 *       x >= -0x1.62e42fefa39efp-2: k = 0, hi = x, lo = 0;  else x > -0x1.0a2b23f3bab73p+0: k = -1, hi = x + ln2HI, lo = -ln2LO;
 *       else k = (int)(invln2*x - 0.5), truncated, hi = x - k*ln2HI, lo = k*ln2LO;
 *       r = hi - lo;  t = r*r;  c = r - t*(P1 + t*(P2 + t*(P3 + t*(P4 + t*P5))));
 *       k == 0: 1 - ((r*c)/(c - 2) - r);  else y = 1 - ((lo - (r*c)/(2 - c)) - hi), scaled by 2^k exactly: y*2^k for k >= -1021, else (y*2^(k+1000))*2^-1000;
 *       ln2HI = 0x1.62e42feep-1, ln2LO = 0x1.a39ef35793c76p-33, invln2 = 0x1.71547652b82fep+0, P1 = 0x1.555555555553ep-3, P2 = -0x1.6c16c16bebd93p-9,
 *       P3 = 0x1.1566aaf25de2cp-14, P4 = -0x1.bbd41c5d26bf1p-20, P5 = 0x1.6376972bea4d0p-25.
 *     E meets what Java asks of Math.exp: within 1 ulp of the true value, and never increasing as d grows (tests/test_spatial_host.py).
 *   - SELECTION: for source i the candidates are j = 0 .. R-1 in region order, i itself included (w = 1).  The edges of vertex i are the first k candidates
 *     under (w descending, j ascending), in that order — what the stable sort and subList(0, k) of keepNearestKVertices leave (J/SpatialGraph.java:29-35) when
 *     addEdge ran in region order.  The order is by w, not by d: two distinct distances that round to one weight are ordered by index.  outDegree is
 *     dge_java8_stream_sum (DoubleStream.sum()) of the k kept weights in that order.  1 <= k <= 32; k > R: DGE_ERR_TOPK, as the reference throws.
 *   - GRAPH: vertex i is region i, in the order of ids; R*k edges; the sources are all vertices in order, set as dge_graph_set_sources(.., stream_sum = 1) sets
 *     them (J/SpatialGraph.java:56-57).  g then stands bit for bit where a host stands after dge_graph_add_edges of all R^2 (i, j, w(i,j)) in row-major order,
 *     dge_graph_keep_top_k(k) and dge_graph_set_sources(0 .. R-1, 1) — the "pruned" state that refuses later dge_graph_add_edges included (for k == R too,
 *     where the three calls would leave a store that still takes edges).  dge_graph_build_alias is next.  R*k must stay below 2^32: DGE_ERR_RANGE.
 *   - g must be fresh (DGE_ERR_STATE).  names (may be NULL) must be empty; it receives the decimal region ids in vertex order (the "j-" position prefix is the
 *     walk writer's: dge_walks_write_seq).  On any error g and names are as they were.
 *   - DGE_ERR_ARG before a device is looked for: null or negative arguments, scale not finite or <= 0, k outside 1 .. 32, duplicate ids, a point that is not
 *     finite, names not empty.  R = 0 is fine and leaves an empty graph.
 *   - Selection is brute force: R^2 squared distances, of which only those that can still enter a row's list get an E (info.weights): a candidate scanned in
 *     ascending j whose dx*dx + dy*dy is >= that of the row's current k-th entry is left out without one.  That is the rule above only because E never rises as
 *     d grows: whoever refits E's constants must pass the monotonicity test (tests/test_spatial_host.py) again, or drop that saving in csrc/spatial.hip.
 *   - A dge_regions may be shared by threads: the first use of its centroids is serialised inside the handle. */
typedef struct dge_spatial_info {
    int64_t regions;      /* R                                                                            */
    int64_t edges;        /* R * k                                                                        */
    int64_t weights;      /* how many times E was evaluated: at most R^2 (a work counter, not part of the rule) */
    int64_t zero_weights; /* kept edges with w == 0                                                       */
    double  kernel_ms;    /* HIP-event time of the fused weight-and-selection kernel                      */
} dge_spatial_info;       /* 40 bytes */
/* the R centroids, x y interleaved, host double[2R]; computed on the device on first use and kept with the handle.  cap (in regions) too small: DGE_ERR_CAP with *n set */
int  dge_regions_centroids(const dge_regions* r, double* xy, int64_t cap, int64_t* n);
/* replaces constructGraph_tract (J/SpatialGraph.java:37-60): from the resident rings to the spatial graph in one call */
int  dge_graph_add_spatial(dge_graph* g, const dge_regions* r, int32_t k, double scale, struct dge_names* names /* may be NULL */, dge_spatial_info* info /* may be NULL */);
/* the same from host arrays of centroids that come from anywhere (community areas, J/SpatialGraph.java:63-88; another tool): ids int64[R], xy double[2R] */
int  dge_graph_add_spatial_points(dge_graph* g, const int64_t* ids, const double* xy, int64_t R, int32_t k, double scale, struct dge_names* names /* may be NULL */,
                                  dge_spatial_info* info /* may be NULL */);

/* ------------------------------------------------------------------------------------------------
 * Walk sampler — replaces sampleVertexSequence() J/LayeredGraph.java:232-252 and the writer loops
 * J/CrossTimeGraph.java:134-140, J/SpatialGraph.java:103-113.
 *   rng_mode 0 ("java-sequential"): one java.util.Random(seed) stream consumed walk after walk, one
 *            nextDouble() per decision — what the reference produces after
 *            `LayeredGraph.rnd = new Random(seed)`.  first_index = draws already consumed.
 *   rng_mode 1 ("strided"): walk i owns draws [i*max_len, (i+1)*max_len) of that same stream.
 *   draws_consumed: mode 0 = draws this call took from the stream (add it to first_index for the next call);
 *            mode 1 = n_walks*max_len, the span of the stream the call owns.
 *            first_index = global index of the first walk (shards / batches).
 *            Both modes give identical walks on graphs where no walk dead-ends.
 * A dead end yields a shorter walk (pad -1), never an error (J/LayeredGraph.java:247-248).
 * max_len is at most DGE_MAX_WALK_LEN: the sampler stages the walks of a block in on-chip memory, and 63 tokens per
 *            walk is what fits.  A longer walk is DGE_ERR_ARG ("walk length N too long (max 63)") from all three entry
 *            points, in both modes, whatever n_walks and first_index are — n_walks == 0 included — and nothing is
 *            launched; dge_sample_walks_into refuses a corpus whose rows are longer (dge_walks_from_host takes any).
 * ---------------------------------------------------------------------------------------------- */
#define DGE_MAX_WALK_LEN 63
int  dge_sample_walks(const dge_graph* g, int64_t n_walks, int32_t max_len, int64_t seed, int rng_mode,
                      int64_t first_index, int32_t* out /* host [n_walks*max_len] */, int64_t* draws_consumed);
int  dge_sample_walks_device(const dge_graph* g, int64_t n_walks, int32_t max_len, int64_t seed, int rng_mode,
                             int64_t first_index, dge_walks** out, int64_t* draws_consumed);
/* re-sample into an existing corpus: rows [row0, row0+n_walks) (strided mode only) */
int  dge_sample_walks_into(const dge_graph* g, dge_walks* w, int64_t row0, int64_t n_walks, int64_t seed,
                           int64_t first_index);
int  dge_walks_from_host(int device, const int32_t* walks, int64_t n_walks, int32_t max_len, dge_walks** out);
/* ---- .seq text in (new; additions only, DGE_VERSION unchanged): the reference hands its walks to the trainer as text, one walk per line, names joined by
 * blanks (written J/CrossTimeGraph.java:136-137, read J/DeepWalk.java:49-56).  The text is tokenised, interned and packed on the device (csrc/seq_ingest.hip).
 *   - The text is BYTES.  A line ends at '\n'; the last line may lack it.  Whitespace is the six bytes 0x09-0x0D and 0x20 (C's isspace in the "C" locale; '\r'
 *     among them, so CRLF files read the same); every other byte, 0x80-0xFF included, is token material; a token is a maximal run of such bytes, of any length.
 *   - A line without a token gives no row; row r is the r-th line that has one; max_len is the largest token count of a line (at least 1); rows are padded with -1.
 *     A text without rows yields what dge_walks_from_host yields for n_walks = 0.
 *   - Several files are taken in the order given; a file whose last byte is not '\n' ends its last line where it ends (tokens never merge across files).
 *   - Ids: the names `names` already holds keep ids 0 .. n-1; a new name gets the next id in the order of its FIRST APPEARANCE in the text, and is appended to
 *     `names`.  intern == 0: nothing is added; a token that is not in `names` becomes -1 in its place (the trainer and the evaluation drop ids < 0 and
 *     left-pack) and is counted in info.unknown.
 *   - A NUL byte in the text: DGE_ERR_IO naming its offset (names are handed out as C strings).  A file that is missing or unreadable: DGE_ERR_IO with its path.
 *     A working set that does not fit in device memory: DGE_ERR_CAP with the bytes asked for.  Null / negative arguments: DGE_ERR_ARG before a device is looked
 *     for.  On any error *out is NULL and `names` is as it was.
 *   - Walks and names are a pure function of the bytes and the prior names: no floating point, nothing that depends on timing or launch geometry.
 * dge_names: interned strings, id = position.  A host object — create / add / count / cstrs need no device. */
typedef struct dge_names dge_names;
int  dge_names_create(dge_names** out);
/* a host that already owns ids (a LayeredGraph's vertex ids) seeds them.  All or nothing: a duplicate (of a held name or within strs), an empty name or one
 * that holds a whitespace byte (it could never be a token): DGE_ERR_ARG, nothing added */
int  dge_names_add(dge_names* n, const char* const* strs, int64_t count);
int  dge_names_count(const dge_names* n, int64_t* count);
/* borrowed, NUL-terminated, dge_names_count entries — what dge_write_vec takes as `names`; valid until the next call that adds names (an ingest with intern != 0 included) */
int  dge_names_cstrs(const dge_names* n, const char* const** strs);
void dge_names_free(dge_names* n);

typedef struct dge_seq_info {
    int64_t bytes;        /* bytes of text taken (the files' sizes added up)                             */
    int64_t lines;        /* lines, a last one without '\n' included                                      */
    int64_t rows;         /* lines with a token = rows of the corpus                                      */
    int64_t tokens;       /* == (ids >= 0 in the corpus) + unknown                                        */
    int64_t unknown;      /* intern == 0: tokens that are not in `names` (-1 in the corpus)               */
    int64_t names_added;
    int32_t max_len;
    int32_t reserved;
    double  read_ms;      /* wall clock spent getting the bytes to the device                             */
    double  kernel_ms;    /* HIP-event time of the ingest kernels                                         */
} dge_seq_info;           /* 72 bytes */

int  dge_walks_from_seq_text(int device, const char* text, int64_t n_bytes, dge_names* names, int intern, dge_walks** out, dge_seq_info* info /* may be NULL */);
int  dge_walks_from_seq_files(int device, const char* const* paths, int32_t n_paths, dge_names* names, int intern, dge_walks** out, dge_seq_info* info /* may be NULL */);
/* ---- .seq text out (new; additions only, DGE_VERSION unchanged): the mirror image of the entries above — rows [row0, row0 + n_rows) of a resident corpus
 * as the text the reference's walk stage writes (J/CrossTimeGraph.java:127-148, J/SpatialGraph.java:91-121), sized and spelled on the device
 * (csrc/seq_write.hip).  The text is this byte string:
 *   - Row r of [row0, row0 + n_rows) gives one line: the tokens of its entries with id >= 0, in column order, joined by ONE blank (0x20), then '\n'.
 *   - Entries < 0 are skipped wherever they stand, not only as trailing pad (what embedding_amd/io.py: write_seq does; on everything the sampler produces
 *     it equals the writer loops of the host mirrors, which stop at the first pad).
 *   - A row without an id >= 0 is a bare '\n'.  The reader above drops such a line: it gives no row.
 *   - The token of id v is the bytes of names[v]; with names == NULL it is the decimal form of v, as in dge_write_vec.
 *   - position_prefix != 0: the token in COLUMN j is preceded by the decimal j and '-' (J/SpatialGraph.java:105-108).  j is the column: a skipped entry does
 *     not renumber the ones behind it.
 *   - No NUL byte, no header.  The text is a pure function of the corpus rows, the names and the flag: no floating point, nothing that depends on timing or
 *     launch geometry.
 * Statuses:
 *   - Null w / n_bytes / path, negative row0 / n_rows / cap, text == NULL with cap > 0, row0 + n_rows beyond the corpus: DGE_ERR_ARG, before a device is
 *     looked for.
 *   - An id >= dge_names_count(names): DGE_ERR_RANGE naming the row, the column and the id — the least (row, column) that holds one.  It is found in the sizing
 *     pass, before anything is written: text is untouched, the file is neither created nor truncated nor appended to.
 *   - dge_walks_to_seq_text: text == NULL with cap == 0 is a size query (DGE_OK, *n_bytes = the text's size).  cap smaller than the text: DGE_ERR_CAP with
 *     *n_bytes set and text untouched.  Otherwise *n_bytes is the size written.
 *   - dge_walks_write_seq: append == 0 creates or truncates the file, append != 0 appends to it (a host that samples in chunks writes chunk after chunk).
 *     Open or write failure: DGE_ERR_IO with the path and the OS error.
 *   - n_rows == 0: DGE_OK, zero bytes; an empty file is created when append == 0.
 * Both entries only read the corpus and the names. */
typedef struct dge_seq_out_info {
    int64_t bytes;        /* bytes of text produced                                                       */
    int64_t lines;        /* == n_rows: every row gives a line                                            */
    int64_t tokens;       /* ids >= 0 written                                                              */
    int64_t empty_lines;  /* rows without an id >= 0 (a bare '\n')                                         */
    double  kernel_ms;    /* HIP-event time of the formatting kernels (sizing, scan, every slab's emit)    */
    double  write_ms;     /* wall clock of getting the bytes off the device and to their place: the slab   */
                          /* loop — copies to pinned memory and write() / memcpy, overlapped with the emit */
} dge_seq_out_info;       /* 48 bytes */

int  dge_walks_to_seq_text(const dge_walks* w, int64_t row0, int64_t n_rows, const dge_names* names, int position_prefix,
                           char* text, int64_t cap, int64_t* n_bytes /* required */, dge_seq_out_info* info /* may be NULL */);
int  dge_walks_write_seq(const dge_walks* w, int64_t row0, int64_t n_rows, const dge_names* names, int position_prefix,
                         const char* path, int append, dge_seq_out_info* info /* may be NULL */);
int  dge_walks_to_host(const dge_walks* w, int32_t* out, int64_t cap_elems);
/* d_ptr: the corpus in device memory, READ-ONLY for the caller: a trainer keeps what it derived from a corpus the library has not
 * written since (vocabulary rows, word offsets) */
int  dge_walks_info(const dge_walks* w, int64_t* n_walks, int32_t* max_len, const int32_t** d_ptr);
/* SpatialGraph's position prefix "j-name" (J/SpatialGraph.java:105-108): token j of each walk becomes
 * j*region_count + id, i.e. lands in layer j of the cross-time id space. */
int  dge_walks_add_position_prefix(dge_walks* w, int32_t region_count);
void dge_walks_free(dge_walks* w);

/* ------------------------------------------------------------------------------------------------
 * SGNS trainer — replaces new Word2Vec.Builder()...build(); w2v.fit()  J/DeepWalk.java:73-79
 * (DL4J-NLP 0.7.2 SkipGram + ND4J AggregateSkipGram; behaviour restated).
 * ---------------------------------------------------------------------------------------------- */
typedef struct dge_train_config {
    int32_t dim;             /* .layerSize(n)          J/DeepWalk.java:62-66,74 */
    int32_t window;          /* .windowSize(n)         J/DeepWalk.java:74 (= LayeredGraph.numLayer) */
    int32_t negative;        /* .negativeSample(5)     J/DeepWalk.java:75 */
    int32_t min_count;       /* .minWordFrequency(2)   J/DeepWalk.java:73 */
    int32_t epochs;          /* .iterations(1) x epochs(1)  J/DeepWalk.java:74 */
    int32_t workers;         /* .workers(8) J/DeepWalk.java:75.  1 = one in-order worker (deterministic);
                                0 = fill the device (Hogwild); n>1 = exactly n concurrent walk workers */
    float   alpha;           /* DL4J default learningRate 0.025 */
    float   min_alpha;       /* DL4J default minLearningRate 1e-4 */
    uint64_t seed;
    int64_t table_size;      /* unigram^0.75 table length; 0 -> 100000000 (word2vec.c) */
    int32_t n_vertices;      /* vertex-id space of the corpus */
    int32_t update_policy;   /* how concurrent workers update the tables (MI355X has 8 L2s that are not coherent):
                                0 = auto: 5 when the vocabulary has >= 131072 rows and its negative-sampling
                                    distribution is flat enough for lock attempts to succeed (expected failure
                                    rate < 0.4) and no single row is busy enough to serialise its pairs behind its lock
                                    (workers x p_row <= 0.5: such rows alone leave the locks, 7); 7 when a head of at most V/4 rows carries
                                    the skew; otherwise (a small vocabulary, a head too large, a block of a schedule of
                                    >= 2 ranks on a flat vocabulary) 8 when the tables are below 4 GiB and a synchronous mini-batch of >= 1e6 items
                                    (5e5 on rows of > 128 floats) keeps the busiest row below 4096 terms; else 2.  A vocabulary whose busiest row
                                    caps the workers below a quarter of the device (48 / its share of the tokens < 4096) runs under 2; the workers of any Hogwild launch are capped so that at most 96 of one row's updates are in flight (profiles/r05_hot_row_inflight.txt).
                                    The constants come from scripts/policy_sweep.py (profiles/r04_policy_sweep.txt);
                                1 = agent-scope row read-modify-write, write-through (last writer of a row wins);
                                2 = agent-scope loads + memory-side float atomics (no update is lost);
                                3 = plain cached accesses (debug only: every XCD trains a private stale copy);
                                5 = every row update under that row's commit lock, 16-byte write-through rows, relaxed
                                    commit (a re-lock can overtake the write-through: measured loss <= 4e-7 of the row
                                    updates at >= 65k rows; fastest);
                                6 = as 5 with strict commit (one returning atomic per stored 128-B line: no update
                                    is ever lost);
                                7 = as 5, but the head of the vocabulary (the rows many workers want at once; how many
                                    is derived from the counts) stays out of the lock protocol and takes atomics as in 2.
                                8 = owner-computes: every (context, target, label) term of a mini-batch becomes an item; items
                                    sorted by target row are applied by the row's owner in order, then sorted by context row and
                                    summed — no locks, no atomics, no lost update; the result is a deterministic function of the
                                    batch whatever the worker count (bit-exact against the oracle at full concurrency).  Within a
                                    mini-batch (~100 items per live row) the other table is read as it stood before the
                                    mini-batch, and the whole mini-batch trains at the learning rate of its first walk.  Tables below 4 GiB, no hierarchical softmax.
                                workers == 1 with policy 0/3/8 is the in-order schedule with plain accesses. */
    int32_t use_hs;          /* .useHierarchicSoftmax(b): 0 = negative sampling only (the north-star path);
                                1 = the hierarchical-softmax term as well, before the negatives of each pair — what
                                DL4J's builder leaves on when J/DeepWalk.java:73-76 does not call it.  Huffman codes over
                                the vocabulary counts (word2vec.c CreateBinaryTree), inner-node table syn1 [V-1 x dim].
                                Policies 0/2/3 only (in-order, or memory-side atomics). */
    int32_t reserved;        /* 0 */
} dge_train_config;

typedef struct dge_train_stats {
    int64_t pairs;           /* (center, context) pairs trained = "edges" of BASELINE.json's metric */
    int64_t words;           /* in-vocabulary tokens consumed */
    double  kernel_ms;       /* HIP-event time of the SGNS kernel launches, summed */
    double  walk_kernel_ms;  /* HIP-event time of the walk kernel launches issued through this model */
    int64_t launches;        /* SGNS kernel launches */
} dge_train_stats;

/* vocabulary pass (DL4J VocabConstructor.buildJointVocabulary): d_counts[v] += occurrences of v.
 * d_counts is device int64[n_vertices]; the caller may all-reduce it across ranks before
 * dge_model_create. */
int  dge_count_tokens(const dge_walks* w, int64_t row0, int64_t n_rows, int32_t n_vertices, int64_t* d_counts);
/* build vocabulary (count >= min_count, ordered by count desc, id asc), unigram table, sigmoid LUT and
 * initial weights (InMemoryLookupTable.resetWeights) */
int  dge_model_create(int device, const dge_train_config* cfg, const int64_t* d_counts, dge_model** out);
int  dge_model_set_stream(dge_model* m, void* hip_stream);
/* one pass of the trainer over corpus rows [row0, row0+n_rows).
 *   walk_index_base : global index of row0 within the epoch (RNG streams are keyed on it)
 *   epoch           : 0-based epoch number
 *   words_before    : in-vocab tokens trained before row0 in this epoch (learning-rate schedule)
 *   words_scale     : 1.0, or the number of ranks when ranks advance through the epoch in parallel */
int  dge_model_train(dge_model* m, const dge_walks* w, int64_t row0, int64_t n_rows, int64_t walk_index_base,
                     int32_t epoch, int64_t words_before, double words_scale, int64_t total_walks_per_epoch);
/* one-shot forms of w2v.fit(): vocabulary + all epochs */
int  dge_train_sgns(int device, const int32_t* walks /* host */, int64_t n_walks, int32_t max_len,
                    const dge_train_config* cfg, dge_model** out);
int  dge_train_sgns_device(const dge_walks* w, const dge_train_config* cfg, dge_model** out);
/* fused step used by bench.py: sample rows [row0,row0+n) of the corpus again from the graph (strided RNG)
 * and train on them, without leaving the device */
int  dge_model_walk_and_train(dge_model* m, const dge_graph* g, dge_walks* w, int64_t row0, int64_t n_rows,
                              int64_t walk_seed, int64_t walk_index_base, int32_t epoch, int64_t words_before,
                              double words_scale, int64_t total_walks_per_epoch);
/* results (w2v.lookupTable): host copies [V x dim], borrowed until the next call on m / dge_model_free */
int  dge_model_vectors(dge_model* m, const float** syn0, const int32_t** vocab_ids, int64_t* V, int32_t* dim);
int  dge_model_syn1neg(dge_model* m, const float** syn1neg);
/* use_hs: inner-node table [max(V-1,0) x dim]; and the Huffman paths of the vocabulary rows in CSR form —
 * offsets[V+1], points (inner-node rows, root first), codes (bit d of codes[r] = branch taken at points[offsets[r]+d]) */
int  dge_model_syn1(dge_model* m, const float** syn1, int64_t* rows);
int  dge_model_huffman(dge_model* m, const int64_t** offsets, const int32_t** points, const uint64_t** codes);
int  dge_model_counts(dge_model* m, const int64_t** counts);
int  dge_model_table(dge_model* m, const int32_t** table, int64_t* table_size);
int  dge_model_stats(const dge_model* m, dge_train_stats* out);
/* Diagnostic: how fast this model's memory answers the four things the lock kernels do to it, measured on the model's stream (tables below
   4 GiB; the rewrite leaves every value as it was; any output may be NULL): GB/s of rows read at random, GB/s (read + written) of rows read and
   stored back write-through, exchanges per second on random lock words, look-ups per second in the unigram table.  Consecutive processes on one box — and two models of one process —
   differ by up to 15 % in training speed with the device's copy rate unchanged (profiles/r02_box_drift.txt); the difference follows the
   allocation and shows here without training anything. */
int  dge_model_row_rates(dge_model* m, double* read_gb_per_s, double* rewrite_gb_per_s, double* lock_exchanges_per_s, double* table_lookups_per_s);
int  dge_model_reset_stats(dge_model* m);
/* Where the tables lie.  Allocations of hundreds of megabytes fall into discrete classes of memory, up to 15 % apart in how fast random rows can be read
   and written back in them (profiles/r03_placement.txt, last block); dge_model_create therefore takes every table of 64 MB ... 2 GiB (syn1neg first) from
   the best of up to 32 candidates — hipMalloc and virtual-memory allocations in turn, all held until the choice — under a 2-ms read-modify-write probe, and
   stops as soon as one candidate is 14 % above the slowest seen.  This reports, for table 0 (syn0), 1 (syn1neg) or 2 (syn1), how many candidates were
   probed and the best (= the one kept) and worst probe rate in GB/s (0 candidates: the table was small or of 2 GiB and more, or the probe could not run). */
int  dge_model_table_placement(const dge_model* m, int32_t table, int32_t* candidates, double* best_gb_per_s, double* worst_gb_per_s);
/* The negative-sampling table's run form.  Rows are ordered by count; the rows of equal count form runs (up to 2 046 of them, counted from the vocabulary's tail; the head rows in front keep the table), the
   slot -> row map of word2vec's unigram^0.75 table is that many straight segments, and the lock kernels compute a negative's row from the run arrays in
   LDS instead of reading the table (5 requests to memory a pair less; profiles/r03_shape_sweep.txt).  dge_model_create compares the closed form with
   the table slot by slot and keeps it only if at most 64 slots differ (those are listed and looked up): the rows drawn are the table's, bit for bit.
   n_runs = 0: this model has no run form (a skewed vocabulary, or too many exceptions). */
int  dge_model_table_runs(const dge_model* m, int32_t* n_runs, int32_t* n_exceptions);
/* Placement search (profiles/r03_placement.txt): which physical memory the allocator handed each of the model's large arrays decides a launch's
   duration by up to 15 %, array by array, under no rule that could be asked for.  Trains rows [row0, row0 + n_rows) of w as a probe; then for
   the negative-sampling table, the lock words, syn1neg and syn0 in turn up to candidates - 1 copies in fresh memory are tried and the faster
   placement kept.  Tables, counters and statistics are saved before and restored after: the model trains exactly as an untuned one.  The arrays are gone
   through in passes until a pass moves nothing (at most six): 2 + 4 (candidates - 1) probe launches per pass, transiently 2 x the tables' memory.  ms_before / ms_after: probe launch before and after (may be NULL). */
int  dge_model_tune_placement(dge_model* m, const dge_walks* w, int64_t row0, int64_t n_rows, int32_t candidates, double* ms_before, double* ms_after,
                              int32_t* arrays_moved);
/* Whether the search has run on this model (the one-shot dge_train_sgns_device runs it only where it can pay: when a tenth of the projected training,
   epochs x walks, exceeds one pass of probes) and its latest report: probe launch before / after (ms), arrays moved. */
int  dge_model_placement_search(const dge_model* m, int32_t* runs, double* ms_before, double* ms_after, int32_t* arrays_moved);
/* what the latest training launch resolved `update_policy` 0 / `workers` 0 to: the policy that ran (0 = in-order plain),
 * the concurrent workers, and for policy 7 the head rows kept out of the lock protocol */
int  dge_model_schedule(const dge_model* m, int32_t* update_policy, int64_t* workers, int32_t* hot_rows);
/* ... and the trainer kernel (name and form) that launch ran, as text: e.g. "k_sgns_train_locked<relaxed>", "k_sgns_train_hsw<negatives under commit locks, 7 waves> (...)",
 * "k_sorted_phase (owner-computes: ...)".  The policy number alone does not say it (hierarchical softmax has three kernels). */
int  dge_model_kernel(const dge_model* m, char* buf, int32_t cap);
/* ... and which pair loop of it: 0 = every pair locks, reads, writes and unlocks its context (syn0) row (every kernel but the next), 1 = the walk-window loop of
 * "k_sgns_train_locked<relaxed>" (csrc/sgns_kernels.h: k_sgns_train_window: the row read unlocked, a walk's syn0 updates parked in LDS and written once at the walk's end); *slots = the
 * walks a workgroup keeps open (0 for loop 0).  The kernel's name does not say it. */
int  dge_model_pair_loop(const dge_model* m, int32_t* loop, int32_t* slots);
/* One block of the multi-GPU schedule under the lock kernels (k_sgns_train_locked<.., PART>), since the last dge_model_reset_stats: pairs that were put back because
 * their context row's lock was taken, lock rounds that left some wanted row unwon, and lock rounds in all — what a block's speed runs against (a block's live rows are
 * V / N per table: locks collide N times as often as on one GPU).  The one-GPU kernels do not count (they have no register to spare). */
int  dge_model_lock_stats(const dge_model* m, int64_t* pairs_put_back, int64_t* rounds_short, int64_t* rounds);
/* Blocking waits the library has made in this process so far — stream / device / event synchronisations and blocking copies, counted at every call site.  An episode
 * of the multi-GPU block schedule makes none once its buffers exist (tests/test_gpu_distributed.py counts them); a global batch makes two (the item store's sizes). */
int  dge_host_sync_count(int64_t* n);
/* ------------------------------------------------------------------------------------------------
 * Held-out evaluation (new; what gensim's compute_loss / DL4J's score listeners give a host): pair scores, link-prediction AUC and
 * the negative-sampling loss, computed on the device from syn0 / syn1neg where they lie (csrc/eval.hip).
 * Common to the three entries: the model is only READ — tables, lock words, counters, dge_train_stats and what dge_model_schedule
 * reports stay as they are, bit for bit, and the trainer's per-call buffers are not used (the next dge_model_train sees the model it left).
 * The kernels run on the model's stream, behind whatever training is queued there; the call returns after the stream has drained.
 * With a partition set (dge_model_set_partition, n_parts > 1) the tables are in pieces: DGE_ERR_STATE.  Null / negative arguments: DGE_ERR_ARG.
 * n = 0 / n_rows = 0: DGE_OK, zero counts, NaN figures.  A hierarchical-softmax model (use_hs) is evaluated on syn0 / syn1neg like any
 * other: the tree term (syn1) is not scored.
 * One dot-product routine serves all three, with an association order fixed by the row width alone: a pair scored through
 * dge_model_score_pairs and the same pair scored inside eval_links / eval_sgns have the same bits.  The negatives are drawn by pure
 * functions of (seed, global row, position) — dge_mix64 is splitmix64, csrc/dge_algos.h — so the counts and the AUC (carried as integer
 * counts of wins and ties) depend on nothing else; the two loss sums are doubles added in an order fixed by the call's arguments
 * (per-workgroup partial sums over statically assigned work, combined by one workgroup in a fixed order; no floating-point atomics):
 * two identical calls return identical bits.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dge_eval_result {
    int64_t pairs;      /* positive scores that entered the figures                         */
    int64_t negatives;  /* negative scores that entered the figures                         */
    int64_t skipped;    /* candidates left out — eval_links: steps with a vertex outside the vocabulary;
                           eval_sgns: drawn negatives equal to the centre (pairs * cfg.negative == negatives + skipped) */
    double  auc;        /* share of (positive, its negative) with pos > neg, ties count 1/2 */
    double  loss;       /* mean over positives of softplus(-pos) + mean over negatives of
                           softplus(neg) for eval_links; see eval_sgns for its own form     */
    double  kernel_ms;  /* HIP-event time of the evaluation kernels                          */
} dge_eval_result;      /* 48 bytes */

/* score[i] = syn0[row(d_ctx[i])] . syn1neg[row(d_tgt[i])] in f32; NaN where either id is < 0,
   >= n_vertices or outside the vocabulary.  Ids are the caller's vertex ids, device int32[n],
   d_score device float[n].  What the trainer calls f for (last_word = ctx, target = tgt). */
int  dge_model_score_pairs(dge_model* m, const int32_t* d_ctx, const int32_t* d_tgt, int64_t n, float* d_score);

/* Link prediction on held-out walk steps — the measure of tests/helpers.py: link_auc.
   For every step (a = walk[g][j], b = walk[g][j+1]), both >= 0, g = global row index row0 + i:
     r   = (b / regions_per_slice) * regions_per_slice + dge_mix64(seed + g * max_len + j) % regions_per_slice      (unsigned 64-bit arithmetic, wrapping)
     pos = score(ctx = b, tgt = a),  neg = score(ctx = r, tgt = a)
   a step whose a, b or r is outside the vocabulary (or r >= n_vertices) is skipped and counted. */
int  dge_model_eval_links(dge_model* m, const dge_walks* w, int64_t row0, int64_t n_rows,
                          int32_t regions_per_slice, uint64_t seed, dge_eval_result* out);

/* The negative-sampling objective on held-out walks, over the pairs the trainer would form
   with a full window: the walk's in-vocabulary tokens left-packed as the trainer packs them
   (ids < 0, >= n_vertices or outside the vocabulary dropped; t_0 .. t_{n-1});
   for every centre i and context c with 0 < |i - c| <= cfg.window:
     pos  = score(ctx = t_c, tgt = t_i)
     for k in 0 .. cfg.negative-1:  slot = dge_mix64(seed + ((g * max_len + i) * max_len + c) * cfg.negative + k) % table_size      (unsigned 64-bit, wrapping)
                                    row  = the model's unigram table at slot (dge_model_table); skipped if row == row(t_i)
                                    neg_k = syn0[row(t_c)] . syn1neg[row]
   loss = ( sum over pairs softplus(-pos) + sum over scored negatives softplus(neg_k) ) / pairs
   — the per-pair objective word2vec minimises; auc as in the struct, over (pos, neg_k).  Walks of up to 12 288 tokens. */
int  dge_model_eval_sgns(dge_model* m, const dge_walks* w, int64_t row0, int64_t n_rows,
                         uint64_t seed, dge_eval_result* out);

/* WordVectorSerializer.writeWordVectors(w2v, path)  J/DeepWalk.java:82: "name v1 .. vD\n" per vocabulary
 * row, no header (header != 0 writes the LINE-style "V D" first line of miscs/taxi_all.txt:1).
 * names[v] is the string of vertex id v; null -> the decimal id. */
int  dge_write_vec(dge_model* m, const char* const* names, const char* path, int header);
void dge_model_free(dge_model* m);

/* ------------------------------------------------------------------------------------------------
 * Multi-GPU block schedule (new; the reference is single-host).  Rows are split by row % n_parts.  With
 * a partition set, dge_model_train / dge_model_walk_and_train only train the pairs whose context row
 * (syn0) lies in ctx_part and whose centre row (syn1neg) lies in tgt_part, and move each drawn negative
 * to the row of tgt_part nearest below it (rows are ordered by count: the frequency rank is kept).  Rank g of
 * N runs episodes e = 0..N-1 with (ctx_part, tgt_part) = (g, (g+e) % N) over the same global batch of
 * walks: the blocks of one episode are row-disjoint, after N episodes every pair was trained once.
 * After an episode a rank hands the syn1neg partition it trained to rank g-1, which trains it next (export -> point-to-point
 * transfer -> import: a ring); syn0 partitions never leave their rank until the final gather.  n_parts <= 1 switches the filter off.
 * Policies under a partition: 0 (auto), 2, 3, 5, 8, and 7 = row locks on syn1neg's tail only, the pair's syn0 row by atomics.  Auto keeps the head / tail
 * split of policy 7 inside a block on skewed vocabularies (the block's own head, derived from the counts with the block's collision rate).
 * With use_hs (policies 0 / 2 / 3): inner-node rows are split by node % n_parts too; a block visits EVERY centre for the inner nodes of its path that lie in
 * tgt_part, the negative-sampling terms of a pair stay with the block of its centre's partition; syn1 partition p travels with syn1neg partition p. */
int  dge_model_set_partition(dge_model* m, int32_t n_parts, int32_t ctx_part, int32_t tgt_part);
/* floats of one packed partition buffer: ceil(V / n_parts) rows x row stride (same for every partition) */
int  dge_model_partition_floats(const dge_model* m, int32_t n_parts, int64_t* n_floats);
/* table: 0 = syn0, 1 = syn1neg, 2 = syn1 (use_hs); d_buf is device memory of dge_model_partition_floats floats */
int  dge_model_export_partition(dge_model* m, int table, int32_t n_parts, int32_t part, float* d_buf);
int  dge_model_import_partition(dge_model* m, int table, int32_t n_parts, int32_t part, const float* d_buf);
/* The same, STREAM-ORDERED: the host never waits.  export: the pack kernel runs on the model's stream and `consumer_stream` (a hipStream_t; NULL = the legacy default
 * stream) is made to wait for it with an event — whatever the caller enqueues there afterwards (ncclSend, a copy) sees the packed buffer.  import: the model's stream
 * is made to wait for everything `producer_stream` holds at the time of the call (the transfer that fills d_buf), then unpacks.  Passing the model's own stream
 * (dge_model_stream) skips the handshake: a host that enqueues its RCCL calls on that stream needs no event at all (dge_model_ring_pass does exactly that).
 * d_buf must stay untouched by the caller until the model's stream has passed the copy. */
int  dge_model_export_partition_async(dge_model* m, int table, int32_t n_parts, int32_t part, float* d_buf, void* consumer_stream);
int  dge_model_import_partition_async(dge_model* m, int table, int32_t n_parts, int32_t part, const float* d_buf, void* producer_stream);
int  dge_model_stream(const dge_model* m, void** hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-GPU exchange at epoch boundaries (new; the reference is single-host).  Each rank trains its
 * walk shard from a common snapshot; delta = current - snapshot is summed across ranks (RCCL
 * all-reduce on the caller's communicator, e.g. torch.distributed) and applied with a scale.
 * ---------------------------------------------------------------------------------------------- */
int  dge_model_sync_size(const dge_model* m, int64_t* n_floats);          /* 2 * V * row_stride */
int  dge_model_snapshot(dge_model* m);                                     /* snapshot = current (start of a shard) */
int  dge_model_export_delta(dge_model* m, float* d_buf);                  /* d_buf = current - snapshot */
int  dge_model_import_delta(dge_model* m, const float* d_buf, float scale); /* current = snapshot + scale*d_buf; re-snapshot */

/* The same exchange with RCCL called by the library itself (hosts without torch.distributed, e.g. the JNI form):
 * rank 0 obtains an id, the host application hands it to the other ranks (any channel: file, socket, MPI), every rank
 * creates its communicator, then dge_model_allreduce_deltas replaces the export/all-reduce/import triple.
 * librccl is loaded lazily (dlopen) on the first of these calls. */
typedef struct dge_comm dge_comm;
typedef struct dge_unique_id { char bytes[128]; } dge_unique_id;          /* = ncclUniqueId */
int  dge_comm_unique_id(dge_unique_id* out);
int  dge_comm_create(dge_comm** out, const dge_unique_id* id, int rank, int nranks, int device);
void dge_comm_free(dge_comm* c);
int  dge_model_allreduce_deltas(dge_model* m, dge_comm* c);
/* block schedule with RCCL called from the library (N = nranks).  dge_model_ring_pass: after episode `episode` rank g hands the
 * syn1neg partition it just trained, (g + episode) % N, to rank g-1 and takes (g + 1 + episode) % N — the one it trains next — from
 * rank g+1 (ncclSend / ncclRecv; with use_hs the syn1 partition of the same number in the same transfer).  dge_model_gather_table: every rank publishes partition `rank` of `table` (0 = syn0, 1 = syn1neg, 2 = syn1)
 * and takes the others (all-gather): the end of training.  NOT YET RUN ON MORE THAN ONE GPU (README.md: verification status). */
int  dge_model_ring_pass(dge_model* m, dge_comm* c, int32_t episode);
int  dge_model_gather_table(dge_model* m, dge_comm* c, int table);

/* ------------------------------------------------------------------------------------------------
 * Quality metric ("next" row of the scope table): pairwiseEstimator of P/embeddingEvaluation_tract.py:169-196 — for every
 * row of features [n x dim] the k other rows nearest in cosine distance (1 - cos; a zero vector is at distance 2 from
 * everything), ascending, smaller index first among equals.  Exact-f32 MFMA tiles fused with the top-k selection.
 * dim <= 256, k <= 64.  Host buffers.  Slots beyond n-1 neighbours hold -1 / 3.0.
 * RULE: a row with a non-finite entry (NaN, +-infinity) counts as a zero vector, as the reference's NaN -> 2 puts it at distance 2 from
 * everything.  Every other non-zero row, of any float32 magnitude (all-subnormal entries included), is scaled to a unit row: x * (1 / |x|)
 * formed in binary64 and rounded once.
 * ---------------------------------------------------------------------------------------------- */
int  dge_knn_cosine(int device, const float* features, int32_t n, int32_t dim, int32_t k, int32_t* out_idx, float* out_dist,
                    double* ms_kernel);
/* ndcg_atK of P/embeddingEvaluation_tract.py:249-260 wholly on the device: the k nearest neighbours of every region in `features`
 * [n x dim] are scored with relevance 1 - (cosine distance in gnd_features [n x gnd_dim]), DCG = sum_i relv_i / log2(i + 1), normalised
 * by the DCG of the ground features' own k nearest; *ndcg = mean over the n regions (rows of the two arrays are the same regions).
 * RULE: a region whose ideal DCG is exactly 0 (e.g. every one of its k nearest ground neighbours orthogonal to it) contributes 0 to the
 * mean, where the reference would divide by zero.  Zero and non-finite rows, of either array, are zero vectors as above. */
int  dge_ndcg_at_k(int device, const float* features, int32_t dim, const float* gnd_features, int32_t gnd_dim, int32_t n, int32_t k,
                   double* ndcg, double* ms_kernels);

/* ------------------------------------------------------------------------------------------------
 * .vec text in (new; additions only, DGE_VERSION unchanged): the file dge_write_vec / WordVectorSerializer.writeWordVectors leaves (J/DeepWalk.java:82) and
 * the reference's evaluators load (P/embeddingEvaluation_tract.py:113-117,139-166), read on the device into resident float32 rows aligned by name
 * (csrc/vec_read.hip; the decimal conversion: csrc/vec_parse.h).
 *   - The text is BYTES.  A line ends at '\n'; the last line may lack it.  Whitespace is the six bytes 0x09-0x0D and 0x20 (C's isspace in the "C" locale; '\r'
 *     among them, so CRLF files read the same); every other byte, 0x80-0xFF included, is token material; a token is a maximal run of such bytes, of any length.
 *     A line without a token is skipped (trailing blanks on a line, as in miscs/taxi_all.txt, change nothing).  A NUL byte: DGE_ERR_IO naming its offset.
 *   - Rows.  Every other line is a row: its first token is the row's name, the rest are its values.  The first row fixes dim = tokens - 1 >= 1; a row with another
 *     token count: DGE_ERR_IO naming the least such line, with the count found and the count expected.
 *   - header == 0: there is no header line.  header != 0: the first line with a token of EVERY piece (file, or the text) must be two unsigned decimal integers
 *     "V D" (miscs/taxi_all.txt:1); after reading, V must equal that piece's row count and D must equal dim, else DGE_ERR_IO carrying both numbers.  A piece
 *     without a token has no such line and passes.  A text without any row has dim = the first header's D (0 with header == 0).
 *   - Several files are taken in the order given; a file whose last byte is not '\n' ends its last line where it ends (no token and no line crosses a file);
 *     all files share one dim; with header != 0 each carries its own header.
 *   - A value token is  [+-] digits [. digits] [(e|E) [+-] digits]  with at least one digit in front of the exponent (".5" and "5." are values, "." is not), or
 *     inf / infinity / nan with an optional sign in any letter case.  Anything else — hex floats, nan(...), "1e", a trailing letter — is DGE_ERR_IO naming the
 *     least byte offset of such a token, with its piece, line and column.  The value is the binary32 NEAREST THE EXACT DECIMAL VALUE, TIES TO EVEN; overflow
 *     gives +-inf, underflow goes through the denormals to +-0 with the sign kept ("-0" is 0x80000000), nan is a quiet NaN with the token's sign: what glibc's
 *     strtof returns in the "C" locale, for tokens of any length (800 digits, 0e999999, 1e-9999).  Not what a reader that goes through a double returns.
 *   - Names and alignment (the .seq reader's rule, applied to rows).  The names `names` already holds keep ids 0 .. n-1.  intern != 0: a new name gets the next id
 *     in the order of its first appearance and is appended.  intern == 0: a row whose name is unknown is dropped and counted (info.dropped); its values are
 *     still checked.  The result has dge_names_count(names) rows AFTER the call; row i is the vector of names[i], present[i] says whether the text held it;
 *     absent rows are all-zero and counted (info.missing).  A name on two rows, in any piece: DGE_ERR_IO naming the second occurrence (the least such line).
 *   - A text with several kinds of error reports the first of: NUL, malformed header, ragged row, bad value, duplicate name, header counts.  A file that is
 *     missing or unreadable: DGE_ERR_IO with its path.  A working set beyond device memory: DGE_ERR_CAP.  Null / negative arguments: DGE_ERR_ARG before a device
 *     is looked for.  On any error *out is NULL and `names` is as it was.
 *   - The result is a pure function of the bytes, the prior names and the flags.  No floating-point operation decides a bit of it; nothing depends on timing or
 *     launch geometry.  Value tokens the device routine hands back (more than 19 significant digits with a non-zero tail, or a power of ten outside its
 *     128-bit range — never a token of <= 19 digits with |value| in [1e-10, 1e10]) are finished by the host with strtof and counted in info.host_values;
 *     both paths give the correctly rounded value, so a result never depends on which took a token.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dge_vectors dge_vectors;      /* resident float32 [rows x dim], row-major, + one present byte per row */
typedef struct dge_vec_info {
    int64_t bytes;         /* bytes of text taken (the files' sizes added up)                              */
    int64_t lines;         /* lines, a last one without '\n' included                                      */
    int64_t rows;          /* rows read: lines with a token that are no header line, dropped ones included */
    int64_t values;        /* rows * dim                                                                   */
    int64_t dropped;       /* intern == 0: rows whose name is not in `names`                               */
    int64_t missing;       /* rows of the result the text did not hold (present == 0, all-zero)            */
    int64_t names_added;
    int64_t host_values;   /* value tokens finished by the host path (rows that are kept only)             */
    int32_t dim;
    int32_t reserved;
    double  read_ms;       /* wall clock spent getting the bytes to the device                             */
    double  kernel_ms;     /* HIP-event time of the kernels                                                */
} dge_vec_info;            /* 88 bytes */

int  dge_vectors_from_vec_text (int device, const char* text, int64_t n_bytes, int header, dge_names* names, int intern, dge_vectors** out, dge_vec_info* info /* may be NULL */);
int  dge_vectors_from_vec_files(int device, const char* const* paths, int32_t n_paths, int header, dge_names* names, int intern, dge_vectors** out, dge_vec_info* info /* may be NULL */);
/* rows: host float32 [n_rows x dim]; present: host, one byte a row (non-zero = present), NULL = every row */
int  dge_vectors_from_host(int device, const float* rows, int64_t n_rows, int32_t dim, const uint8_t* present /* NULL: all */, dge_vectors** out);
/* d_ptr / d_present: device memory, READ-ONLY for the caller; any output may be NULL */
int  dge_vectors_info(const dge_vectors* v, int64_t* rows, int32_t* dim, const float** d_ptr, const uint8_t** d_present);
/* out: host [rows x dim], cap_elems floats (smaller: DGE_ERR_CAP), or NULL: the rows are not copied and only present is filled; present: host [rows] */
int  dge_vectors_to_host(const dge_vectors* v, float* out /* may be NULL */, uint8_t* present /* may be NULL */, int64_t cap_elems);
void dge_vectors_free(dge_vectors* v);

/* syn0 row of every vocabulary word whose vertex id is a present row of v := that row (continuing from published vectors).  v's dim must equal the model's
 * (DGE_ERR_ARG); other rows, syn1neg and the counters stay untouched; *rows_set (may be NULL) = how many rows were set.  Ordered on the model's stream, behind
 * whatever training is queued there; returns after the stream has drained.  With a partition set: DGE_ERR_STATE. */
int  dge_model_load_vectors(dge_model* m, const dge_vectors* v, int64_t* rows_set);

/* the two quality entries above on resident rows: the same kernels, no host round trip of the features */
int  dge_knn_cosine_vectors(const dge_vectors* v, int32_t k, int32_t* out_idx, float* out_dist, double* ms_kernel);           /* absent rows are zero vectors, whatever they hold */
int  dge_ndcg_at_k_vectors(const dge_vectors* f, const dge_vectors* gnd, int32_t k, double* ndcg, double* ms_kernels);         /* equal row counts, every row present in both: else DGE_ERR_ARG */

/* ------------------------------------------------------------------------------------------------
 * k-means and clustering accuracy (new; additions only, DGE_VERSION unchanged): the reference's second figure of merit, clusteringAccuracy
 * (P/embeddingEvaluation_tract.py:539-571, driven by evaluate_by_clustering, :574-631): k-means on the embedding's rows, the contingency table against ground
 * labels, a greedy map of clusters to labels, the share of regions that land on their label.  The reference takes scikit-learn's KMeans, which draws its own
 * random numbers: two of its runs do not agree.  Here k-means is a RULE (csrc/kmeans.hip; the per-element pieces: csrc/kmeans_rule.h); the result is a pure
 * function of the rows, k, the seed, n_init and max_iter.  Nothing depends on timing, launch geometry or tile sizes: every sum that decides anything is an
 * integer sum or a binary64 sum in an order fixed below.  tests/kmeans_ref.py is this text in Python.
 *   - INPUTS.  Resident float32 rows [rows x dim] with one present byte per row, and an optional host array `select`, one byte per row (NULL: every present
 *     row).  The SELECTED rows are the present rows with a non-zero select byte, in ascending row order; n is their count and "row i" below is the i-th of
 *     them.  Limits: 1 <= k <= 64, 1 <= dim <= 256, k <= n <= 2^31 - 1, n_init >= 1, max_iter >= 1; anything outside: DGE_ERR_ARG with the reason.  A value
 *     that is not finite in a selected row: DGE_ERR_ARG naming the least such row (by its number among all rows); rows that are not selected are never
 *     read.  Null arguments and the limits on k, n_init, max_iter and dim: DGE_ERR_ARG before a device is looked for.  On any error the outputs are untouched.
 *   - DISTANCE.  d(i, c) is a binary64 accumulator that starts at +0.0; for j = 0 .. dim-1 ascending: t = (double)x[i][j] - (double)centre[c][j] (one rounded
 *     subtraction), acc = fma(t, t, acc) (one rounding).  The label of a row is the LEAST c with minimal d.
 *   - FIXED-POINT ROW SUMS.  M = max |x| over the selected rows; e is the integer with M = m * 2^e, 0.5 <= m < 1 (e = 0 if M = 0); b is the bit length of n;
 *     s = 62 - b - e, which may be negative; q[i][j] = (double)x[i][j] * 2^s (exact) rounded to the nearest integer, ties to even.  S[c][j] is the int64 sum
 *     of q over the members of c: |q| < 2^(62-b) and n < 2^b, so it cannot overflow, and being an integer sum it is the same in any order.
 *   - CENTRE UPDATE.  centre[c][j] = (float) ldexp((double)S[c][j] / (double)count[c], -s): int64 to binary64 rounded to nearest even, one division, an exact
 *     scaling, one rounding to binary32.  A centre without a member keeps its position; info.empty counts those of the final state.
 *   - BLOCKED SUM.  Every binary64 sum over rows has this one shape: the selected rows, in order, are cut into blocks of 256; each block's values are added
 *     sequentially from +0.0; the block sums are added sequentially, from +0.0, in block order.  It is used for the inertia and for the seeding totals.
 *   - SEEDING (k-means++), once per restart r = 0 .. n_init-1.  dge_mix64 is the splitmix64 of csrc/dge_algos.h; the arithmetic is unsigned 64-bit and wraps.
 *     Centre 0 is row dge_mix64(seed + r*k) % n.  dmin[i] is the least d of row i to the centres chosen so far.  For c = 1 .. k-1:
 *     u = (dge_mix64(seed + r*k + c) >> 11) * 2^-53;  target = u * total, total being the blocked sum of dmin.  Walk the block sums in order, from +0.0, to
 *     the first block after which the running total exceeds target; then, starting again from the total in front of that block, add that block's dmin row by
 *     row: the pick is the first row after which this running sum exceeds target (should rounding let none of the block's rows do so, its last row).  If no
 *     block exceeds the target (total = 0, or u * total rounding to total), the pick is the row with the greatest dmin, the least row among equals.
 *     Caller-supplied initial centres (host [k x dim]) replace seeding; n_init is then taken as 1.
 *   - ITERATION.  Assign labels and count the labels that changed (the first pass counts every row).  If none changed, stop; otherwise update the centres and
 *     repeat, for at most max_iter assignment passes: after the max_iter-th pass the centres are not updated again.
 *   - A RESTART gives the labels and d of its last assignment pass, the centres that pass used, and its inertia, the blocked sum of d(i, label_i).
 *   - THE BEST RESTART is that of least inertia, the lower restart number among equals.  Its labels go to the host as int32[rows] (all rows; a row that is not
 *     selected gets -1), its centres as float[k x dim].
 *   - ACCURACY (dge_cluster_accuracy; clusteringAccuracy, :544-571).  labels[n_rows] and gnd[n_rows] hold values in [0, k) or -1 (anything else: DGE_ERR_ARG
 *     naming the row).  cnt[a][g] counts the rows where labels = a and gnd = g, both >= 0.  Clusters are visited by row total of cnt, descending, the LARGER
 *     index first among equal totals; for each cluster the ground labels by cnt[a][.], descending, the larger label first among equals; the cluster maps to
 *     the first label not yet taken.  (That tie order is numpy's argsort(..)[::-1] under a stable sort, which is what numpy uses at these sizes.)
 *     accuracy = sum of cnt[a][map[a]] / (number of rows with gnd >= 0): the denominator counts labelled regions the embedding lacks, as len(gndTid) does in
 *     the reference.  A zero denominator gives NaN and DGE_OK.  A host computation: no device involved.
 *   - NOT the reference's KMeans: no tol stop, no relocation of empty clusters, no greedy multi-trial seeding.  For the reference's per-slice loop a host passes
 *     `select` masks built from the "h-rid" names.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dge_kmeans_cfg {
    int32_t  k;
    int32_t  n_init;       /* restarts (taken as 1 with initial centres)                                   */
    int32_t  max_iter;     /* assignment passes of one restart, at most                                    */
    int32_t  reserved;
    uint64_t seed;
} dge_kmeans_cfg;          /* 24 bytes */
typedef struct dge_kmeans_info {
    int64_t rows;              /* n: the selected rows                                                     */
    int32_t best_restart;
    int32_t iterations;        /* assignment passes of the best restart                                    */
    int64_t total_iterations;  /* assignment passes of all restarts                                        */
    int32_t scale_bits;        /* s                                                                        */
    int32_t empty;             /* centres of the best restart without a member in its last pass            */
    double  inertia;
    double  kernel_ms;         /* HIP-event time from the first kernel of the call to its last             */
} dge_kmeans_info;             /* 48 bytes */
/* labels: host int32[rows]; centres: host float[k x dim]; select, init_centres and info may be NULL */
int  dge_kmeans_vectors(const dge_vectors* v, const uint8_t* select, const dge_kmeans_cfg* cfg, const float* init_centres, int32_t* labels, float* centres, dge_kmeans_info* info);
/* the same on host rows float32 [n_rows x dim], every row present (through dge_vectors_from_host) */
int  dge_kmeans(int device, const float* features, int64_t n_rows, int32_t dim, const uint8_t* select, const dge_kmeans_cfg* cfg, const float* init_centres, int32_t* labels,
                float* centres, dge_kmeans_info* info);
/* cnt: host int64[k x k], may be NULL; map: host int32[k], may be NULL */
int  dge_cluster_accuracy(const int32_t* labels, const int32_t* gnd, int64_t n_rows, int32_t k, int64_t* cnt, int32_t* map, double* accuracy);

/* ------------------------------------------------------------------------------------------------
 * NMF of a sparse matrix (new; additions only, DGE_VERSION unchanged): the "MF" column of the reference's figures (P/embeddingEvaluation_tract.py:318-342,604).
 * The reference writes R x R text matrices (Tracts.outputAdjacencyMatrix, J/Tracts.java:269-301), reads them back with np.loadtxt and factors them with
 * nimfa.Nmf(rank=10, max_iter=30, update="divergence") (P/matrixFactorization_tract.py:26-45; P/flowFeatureGeneration_tract.py:29-40 takes the Euclidean update
 * and 100 iterations); a region's feature is concat(W, H^T).  nimfa draws its own random numbers: two of its runs do not agree.  Here NMF is a RULE
 * (csrc/nmf.hip; the per-element pieces: csrc/nmf_rule.h): W and H are a pure function of the entries, the shape, rank, max_iter, update and the seed (or the
 * initial factors).  Nothing depends on timing, launch geometry or the order of the input entries, and nothing of size n x m is ever formed.  Everything is
 * binary64; fma(a, b, c) is a * b + c with ONE rounding; every other operation rounds once.  tests/nmf_ref.py is this text in Python.
 *   - INPUT.  A matrix V [n x m] as n_entries entries (row, col, val).  An entry outside the matrix: DGE_ERR_ARG naming the least such input index.  A value
 *     that is not finite: DGE_ERR_ARG naming the least such input index; then a value < 0: DGE_ERR_ARG likewise.  A value == 0 is dropped and counted in
 *     info.zeros.  A second kept entry with the (row, col) of another: DGE_ERR_ARG naming the least input index that is not the first of its (row, col).  The
 *     KEPT entries are held twice: by row with the columns ascending, by column with the rows ascending; "entry e" is one of them.  Limits: 1 <= rank <= 32,
 *     1 <= n, m <= 2^31 - 1, 1 <= n_entries <= 2^31 - 1 with at least one kept, 1 <= max_iter <= 10000, update 0 (divergence) or 1 (euclidean).  Null
 *     arguments, limit violations and bad initial factors: DGE_ERR_ARG before a device is looked for.  On any error the outputs are untouched.
 *   - INIT.  vmax = the greatest kept value.  u(t) = (dge_mix64(seed + t) >> 11) * 2^-53 (dge_mix64: the splitmix64 of csrc/dge_algos.h; unsigned 64-bit
 *     arithmetic, wrapping).  W[i][r] = u(i*rank + r) * vmax;  H[r][j] = u(n*rank + r*m + j) * vmax.  Caller-supplied W and H (host doubles, both or neither,
 *     every value finite and >= 0) replace this.
 *   - FLOOR.  EPS = 2^-52; a value of W or H below EPS becomes EPS: after INIT (supplied factors included) and after every update.  This is nimfa's
 *     adjustment step AS RECALLED — nimfa is not at hand where this was written, so the constant and the place are not verified against it.
 *   - SEGMENT SUM of a list of products a_t * b_t, t = 0 .. c-1.  16 partials p[0 .. 15] start at +0.0; product t goes to partial t mod 16, in ascending t:
 *     p[l] = fma(a_t, b_t, p[l]).  Then for s = 8, 4, 2, 1 and every l < s: p[l] = p[l] + p[l+s].  The sum is p[0]; an empty list gives +0.0.  (16 lanes are
 *     one DPP row: the fold is four row shifts.)
 *   - BLOCKED SUM of a list of values: k-means' shape exactly — blocks of 256 added sequentially from +0.0, the block sums added sequentially from +0.0.
 *   - P[e], for entry e = (i, j): acc = +0.0; for r ascending: acc = fma(W[i][r], H[r][j], acc).
 *   - DIVERGENCE iteration (nimfa update="divergence": Lee and Seung's rule for the Kullback-Leibler divergence).
 *       1. Q[e] = V[e] / P[e].                 2. N[r][j] = SEGMENT SUM over column j's entries (rows ascending) of W[i][r] * Q[e].
 *       3. d[r] = BLOCKED SUM over i of W[i][r].                 4. H[r][j] = FLOOR(H[r][j] * (N[r][j] / d[r])): one division, then one multiplication.
 *       5. P and Q again, with the new H.       6. N'[i][r] = SEGMENT SUM over row i's entries (columns ascending) of Q[e] * H[r][j].
 *       7. d'[r] = BLOCKED SUM over j of H[r][j].                8. W[i][r] = FLOOR(W[i][r] * (N'[i][r] / d'[r])).
 *   - EUCLIDEAN iteration (nimfa's default update).
 *       1. A[r][j] = SEGMENT SUM over column j's entries of W[i][r] * V[e].      2. G[r][s] = BLOCKED SUM over i of the rounded product W[i][r] * W[i][s].
 *       3. B[r][j]: acc = +0.0; for s ascending: acc = fma(G[r][s], H[s][j], acc) — every B from the OLD H.       4. H[r][j] = FLOOR(H[r][j] * (A[r][j] / B[r][j])).
 *       5. with the new H: A'[i][r] = SEGMENT SUM over row i's entries of V[e] * H[r][j].      6. G'[r][s] = BLOCKED SUM over j of the rounded product H[r][j] * H[s][j].
 *       7. B'[i][r]: acc = +0.0; for s ascending: acc = fma(W[i][s], G'[s][r], acc) — every B' from the OLD W.    8. W[i][r] = FLOOR(W[i][r] * (A'[i][r] / B'[i][r])).
 *   - STOP.  Exactly max_iter iterations.  (The reference's objective="conn", conn_change=50 cannot stop before its max_iter=30 either.)
 *   - NOT nimfa: the random numbers are this rule's own, there is no connectivity test and there are no multiple runs.
 *   - OBJECTIVE (info.objective), of the final factors; OUTSIDE the exact rule, because the device's log is not libm's.  Divergence: the sum over the entries of
 *     V log(V / P) - V, plus the sum over r of cw[r] * ch[r] (cw, ch: the blocked column sums of W and row sums of H) — the generalised Kullback-Leibler
 *     divergence of V from W H.  Euclidean: the sum over the entries of (V - P)^2 - P^2, plus the sum over r, s of G[r][s] * G'[r][s] — the squared Frobenius
 *     distance.  tests hold it to (entries + rank^2 + 8) * 2^-50 * (the sum of the absolute values of those terms).
 *   - dge_nmf_flows replaces outputAdjacencyMatrix + loadtxt + the idx sub-matrix (P/matrixFactorization_tract.py:32-38): its entries are exactly the edges
 *     dge_flows_slot_edges(f, T, mode, ..) gives for `slot`, V[index(src)][index(dst)] = w, restricted to the regions with a non-zero select byte ([R], NULL:
 *     all) and re-indexed in ascending region index; n = m = the number of selected regions, region_index[n] (may be NULL) lists them.  The matrix is built on
 *     the device from the resident table.  No selected region, or no entry of the slot between them: DGE_ERR_ARG.  dge_nmf_flows(f, 1, mode, 0, ..) factors
 *     taxi-all.matrix.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dge_nmf_cfg {
    int32_t  rank;
    int32_t  max_iter;     /* iterations: exactly this many                                                */
    int32_t  update;       /* 0 divergence, 1 euclidean                                                    */
    int32_t  reserved;
    uint64_t seed;
} dge_nmf_cfg;             /* 24 bytes */
typedef struct dge_nmf_info {
    int64_t rows;              /* n                                                                        */
    int64_t cols;              /* m                                                                        */
    int64_t entries;           /* kept                                                                     */
    int64_t zeros;             /* dropped                                                                  */
    int32_t iterations;
    int32_t reserved;
    double  vmax;
    double  objective;
    double  kernel_ms;         /* HIP-event time from the first kernel of the call to its last             */
} dge_nmf_info;                /* 64 bytes */
/* row, col, val: host arrays of n_entries; W: host double[n x rank]; H: host double[rank x m]; init_W, init_H (both or neither) and info may be NULL */
int  dge_nmf_coo(int device, const int32_t* row, const int32_t* col, const double* val, int64_t n_entries, int64_t n, int64_t m, const dge_nmf_cfg* cfg, const double* init_W,
                 const double* init_H, double* W, double* H, dge_nmf_info* info);
/* W: host double[n x rank], H: host double[rank x n] and region_index: host int64[n], n = the selected regions (at most the table's regions) */
int  dge_nmf_flows(const dge_flows* f, int32_t T, int32_t mode, int32_t slot, const uint8_t* select, const dge_nmf_cfg* cfg, double* W, double* H, int64_t* region_index,
                   dge_nmf_info* info);

/* ------------------------------------------------------------------------------------------------
 * LINE on a weighted directed graph (new; additions only, DGE_VERSION unchanged): the "LINE" column of the reference's figures
 * (P/embeddingEvaluation_tract.py:318-342,364; P/flowFeatureGeneration_tract.py:54-73,100; regression-eval.sh:14-27; J/Tracts.java:335).  The reference shells
 * out to a third-party LINE/linux/train-CA.sh that is in neither tree; that tool draws from rand() and races its threads, so two of its runs disagree.  Here LINE
 * is a RULE (csrc/line.hip; the per-element pieces: csrc/line_rule.h): X and Y are a pure function of the entries, n, the configuration and the seed (or the
 * initial tables).  Nothing depends on timing, launch geometry or the order of the input entries.  LINE's source is not at hand where this was written: where
 * the text says "LINE's", it is LINE AS RECALLED and not verified against it.  Everything real is binary64; every operation rounds once, in the order written;
 * fma(a, b, c) is a * b + c with ONE rounding and appears only where written.  dge_mix64 is the splitmix64 of csrc/dge_algos.h; index arithmetic is unsigned
 * 64-bit and wraps.  tests/line_ref.py is this text in Python.
 *   - INPUT.  A directed weighted graph on n vertices as n_entries entries (src, dst, w).  An entry outside [0, n): DGE_ERR_ARG naming the least such input
 *     index.  A w that is not finite, negative or not an integer value: DGE_ERR_ARG naming the least such input index.  w >= 2^31: DGE_ERR_ARG.  w == 0 is
 *     dropped and counted in info.zeros.  A second kept entry with the (src, dst) of another: DGE_ERR_ARG naming the least input index that is not the first of
 *     its pair.  The KEPT entries are sorted by (src, dst) ascending; "edge e" is the e-th of them.  Self loops are kept.  Limits: 1 <= n <= 2^22,
 *     1 <= n_entries <= 2^31 - 1 with at least one kept, total weight W < 2^40, 1 <= dim <= 256, 0 <= negative (K) <= 32, order 1 or 2, 1 <= batch <= 65536,
 *     1 <= samples <= 2^40, 0 < rho0 <= 1.  Null arguments and limit violations: DGE_ERR_ARG before a device is looked for.  On any error the outputs are
 *     untouched.
 *   - STATE.  Two int64 tables PX[n][dim] (vertex) and PY[n][dim] (context).  The value of a cell is (double)P * 2^-32, exact while |P| < 2^40.
 *   - INIT.  seed2 = dge_mix64(seed ^ 0x4C494E45);  u(t) = (dge_mix64(seed2 + t) >> 11) * 2^-53;  PX[v][j] = rint(((u(v*dim + j) - 0.5) / dim) * 2^32) — LINE's
 *     (rand()/RAND_MAX - 0.5)/dim;  PY = 0.  Caller-supplied host doubles replace this: init_X alone, or init_X and init_Y; every value finite with |x| < 256;
 *     they are quantised the same way, rint(x * 2^32).  rint rounds to nearest, ties to even.
 *   - EDGE TABLE.  C[e] = the inclusive int64 prefix sum of the weights in edge order, W = C[last].  For a draw r the edge is the least e with C[e] > r mod W.
 *   - NEGATIVE TABLE.  d[v] = the int64 sum of the weights of the edges with src == v (LINE's degree: sources only);  p[v] = sqrt((double)d[v] *
 *     sqrt((double)d[v])) (d^0.75 as two correctly rounded roots and one product);  nw[v] = (int64)(p[v] * 1024.0), truncated;  NC[v] = the inclusive prefix sum
 *     of nw, N = NC[n-1].  For a draw r the negative is the least v with NC[v] > r mod N.  A vertex without an out-edge is never a negative; a negative that
 *     equals the sample's source or target is trained like any other, as in LINE.
 *   - SIGMOID TABLE.  1000 doubles built on the host with E = sw_exp_neg of csrc/spatial_weight.h:  x_k = (k * 12.0) / 1000.0 - 6.0;  x_k >= 0: T[k] = 1.0 /
 *     (1.0 + E(-x_k)), else T[k] = E(x_k) / (1.0 + E(x_k)).  sig(f) = 1.0 if f > 6.0; 0.0 if f < -6.0; else T[min(999, (int)(((f + 6.0) * 1000.0) / 12.0))].
 *   - DOT.  dot(a, b) over dim values is the SEGMENT SUM of the NMF rule above: 16 partials from +0.0, product j into partial j mod 16 by fma in ascending j,
 *     folded 8, 4, 2, 1.
 *   - SAMPLES.  Sample s = 0 .. samples-1: the edge by dge_mix64(seed + 64*s), giving (u, v); negative d = 1 .. K by dge_mix64(seed + 64*s + d).  Target
 *     t_0 = v has label 1; the targets t_d, d >= 1, are the negatives, label 0.
 *   - BATCHES.  Batch b holds the samples [b*batch, min((b+1)*batch, samples)).  rho_b = rho0 * (1.0 - (double)(b*batch) / (double)(samples + 1)); below
 *     rho0 * 0.0001 it is rho0 * 0.0001.  All reads of a batch see the tables as they stood at its start (a synchronous mini-batch).  For every sample and every
 *     d:  A = the value row PX[u];  Bt = the value row PX[t_d] (order 1) or PY[t_d] (order 2);  g = (label - sig(dot(A, Bt))) * rho_b;  for every j the
 *     target's delta cell takes rint((g * A[j]) * 2^32) and u's delta cell in PX takes rint((g * Bt[j]) * 2^32).  The target's deltas go to PX for order 1, to
 *     PY for order 2.  All adds are int64 adds; at the end of the batch P += delta for both tables.
 *   - BOUND.  The greatest |value| of the state must stay below 256: then a term is below 2^40, a cell takes fewer than 2 * 65536 * 33 terms a batch, and nothing
 *     overflows.  If the tables after some batch hold a cell with |P| >= 2^40 the call fails with DGE_ERR_ARG naming the least such batch; the outputs are
 *     untouched.  (The apply pass folds the batch number into a device word by an integer minimum; the host reads it once, at the end.)
 *   - OUTPUTS.  X: host double[n x dim].  Y: host double[n x dim], may be NULL; order 1 leaves it all zero.  touched: host uint8[n], may be NULL: 1 where the
 *     vertex is an endpoint of a kept edge.  info.max_abs is the greatest |value| of both tables at the end.
 *   - NOT LINE: its own random numbers; mini-batches instead of racing threads; rho stepped per batch, not per 10 000 samples; fixed-point tables; inverse-CDF
 *     tables instead of alias tables and a 1e8-slot table.
 *   - dge_line_flows takes its edges and the re-indexing exactly as dge_nmf_flows takes them: the edges dge_flows_slot_edges(f, T, mode, ..) gives for `slot`,
 *     restricted to the regions with a non-zero select byte ([R], NULL: all) and re-indexed in ascending region index; n = the number of selected regions,
 *     region_index[n] (may be NULL) lists them.  The graph is built on the device from the resident table.  dge_line_flows(f, 1, mode, 0, ..) trains on
 *     taxi-all.od.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dge_line_cfg {
    int32_t  dim;
    int32_t  order;        /* 1 or 2                                                                       */
    int32_t  negative;     /* K                                                                            */
    int32_t  batch;
    int64_t  samples;
    double   rho0;
    uint64_t seed;
} dge_line_cfg;            /* 40 bytes */
typedef struct dge_line_info {
    int64_t vertices;          /* n                                                                        */
    int64_t entries;           /* kept                                                                     */
    int64_t zeros;             /* dropped                                                                  */
    int64_t batches;
    int64_t samples;
    int64_t total_weight;      /* W                                                                        */
    int64_t neg_total;         /* N                                                                        */
    double  max_abs;
    double  kernel_ms;         /* HIP-event time from the first kernel of the call to its last             */
} dge_line_info;               /* 72 bytes */
/* src, dst, w: host arrays of n_entries; X: host double[n x dim]; init_X, init_Y (only with init_X), Y, touched and info may be NULL */
int  dge_line_coo(int device, const int32_t* src, const int32_t* dst, const double* w, int64_t n_entries, int64_t n, const dge_line_cfg* cfg, const double* init_X,
                  const double* init_Y, double* X, double* Y, uint8_t* touched, dge_line_info* info);
/* X, Y: host double[n x dim], touched: host uint8[n] and region_index: host int64[n], n = the selected regions (at most the table's regions) */
int  dge_line_flows(const dge_flows* f, int32_t T, int32_t mode, int32_t slot, const uint8_t* select, const dge_line_cfg* cfg, double* X, double* Y, uint8_t* touched,
                    int64_t* region_index, dge_line_info* info);

/* ------------------------------------------------------------------------------------------------
 * Decision-tree classification accuracy (new; additions only, DGE_VERSION unchanged): the reference's third figure of merit, evalute_by_binary_classification
 * (P/embeddingEvaluation_tract.py:201-232; labels by generatePOIlabel_helper, :34-47) and P/binaryClassification_CA.py:33-58: for every label, slice and method
 * cross_val_score(tree.DecisionTreeClassifier(), features, L, cv=10).  scikit-learn's tree breaks equal splits by a random permutation of the features: two of
 * its runs do not agree.  Here a binary CART classifier and its F-fold cross-validated accuracy are a RULE (csrc/tree.hip; the per-element pieces and the one
 * comparator: csrc/tree_rule.h); the result is a pure function of the used rows AS A SET, their labels, the fold numbers and the three limits.  Nothing depends
 * on the order of the rows, launch geometry, concurrency or timing: every comparison that chooses a split is made on integers.  tests/tree_ref.py is this text
 * in Python.
 *   - ROWS.  Resident float32 rows [rows x dim], 1 <= dim <= 4096, one present byte per row, and a host label y[i] in {0, 1} per row.  A row is USED if it is
 *     present and, where a `select` mask is given, selected (non-zero byte); in a cross-validation, if it is present and its fold is not -1.  Values compare as
 *     numbers: -0.0 equals +0.0.  A value that is not finite in a used row: DGE_ERR_ARG naming the least (row, column); a label other than 0 or 1 on a used
 *     row: DGE_ERR_ARG naming the row; rows that are not used may hold anything.  At most 2^20 rows may train one tree, more is DGE_ERR_RANGE: the bound makes
 *     the cross products below fit 128 bits.
 *   - A NODE holds a set of training rows: n of them, p with label 1, at depth d (the root: depth 0).  It is a LEAF if p == 0, or p == n, or
 *     n < min_samples_split, or max_depth > 0 and d == max_depth, or it has no valid candidate.  A split that gains nothing is still taken (scikit-learn with
 *     min_impurity_decrease = 0 does the same).
 *   - CANDIDATES.  For feature f, every pair of consecutive distinct values a < b among the node's rows: the rows with value <= a go left, nL of them, pL with
 *     label 1; nR = n - nL, pR = p - pL.  A candidate is valid if nL >= min_samples_leaf and nR >= min_samples_leaf.
 *   - SCORE.  S = (pL^2 + qL^2) / nL + (pR^2 + qR^2) / nR with q = n - p on each side (the greatest S is the least weighted Gini impurity).  The greatest S
 *     wins.  Scores are compared exactly, as rationals: N = (pL^2 + qL^2) nR + (pR^2 + qR^2) nL, Dn = nL nR, and N1 Dn2 against N2 Dn1 in 128-bit integers
 *     (N <= 2^58, Dn <= 2^38).  Among equal scores the least feature index wins, then the least a.  That order is total: any reduction tree gives the same winner.
 *   - THRESHOLD.  m = RN(RN((double)a + (double)b) * 0.5), the only floating-point operations of the rule.  At prediction x goes left iff (double)x <= m.
 *     a <= m < b always holds, so training and prediction send every row the same way: 2a <= RN(a + b) <= 2b because rounding is monotone and 2a, 2b are
 *     binary64 values; halving is exact (a non-zero sum of two float32 values is no binary64 subnormal); and m = b would need b - a <= half a binary64 ulp of
 *     2b, while two distinct float32 values are a float32 step apart.
 *   - LEAF VOTE.  1 iff 2p > n; a tie gives 0.
 *   - NODE NUMBERS.  The root is node 0.  The levels are processed in turn and a level's nodes in the order of their numbers; a node that splits receives the
 *     next two numbers, left then right: right = left + 1.  The tree is five arrays of n_nodes: feature int32 (-1 in a leaf), threshold double (0 in a leaf),
 *     left int32 (-1 in a leaf), count int64 (n), pos int64 (p).
 *   - CROSS-VALIDATION.  fold[i] in -1 .. F-1, 1 <= F <= 64 (anything else: DGE_ERR_ARG); -1 takes the row out.  Tree t trains on the used rows with fold != t
 *     and is tested on the used rows with fold == t: correct[t] of tested[t] rows get their label, and n_nodes[t], depth[t] describe the tree.  A fold without
 *     training rows: DGE_ERR_ARG naming it.  A fold without test rows reports 0 of 0.  The folds are the caller's; embedding_amd.evaluate.stratified_folds is the
 *     rule the Python view offers (the j-th used row of its class, in row order, gets fold j mod F).
 *   - NOT scikit-learn: ties are broken by the rule above, not by a random order of the features; binary labels only; no sample weights; the folds are a rule
 *     of our own, not StratifiedKFold's.  (scikit-learn also thresholds at the float32 midpoint where ours is the binary64 one; both lie in [a, b).)
 *   - Null and negative arguments and limits outside max_depth >= 0, min_samples_split >= 2, min_samples_leaf >= 1: DGE_ERR_ARG before a device is looked for.
 *     Device memory that does not suffice: DGE_ERR_CAP.  The trees of a cross-validation grow together where the device's free memory holds their lists
 *     (about 23 bytes x dim x rows a tree), else in batches, one after another (DGE_TUNE_TREE_BATCH sets the batch by hand); the result is the same.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dge_tree_cfg {
    int32_t max_depth;           /* 0 = no limit                                                             */
    int32_t min_samples_split;   /* default 2                                                                */
    int32_t min_samples_leaf;    /* default 1                                                                */
    int32_t reserved;
} dge_tree_cfg;                  /* 16 bytes */
typedef struct dge_tree_info {
    int64_t rows;              /* the used rows                                                            */
    int64_t n_nodes;           /* of all trees of the call                                                 */
    int32_t depth;             /* the deepest tree's                                                       */
    int32_t levels;            /* level passes, summed over the batches                                    */
    int32_t trees;
    int32_t batches;           /* 1: all trees grew together                                               */
    double  kernel_ms;         /* HIP-event time from the first kernel of the call to its last             */
} dge_tree_info;               /* 40 bytes */
/* y: host uint8[rows]; select, cfg (NULL: the defaults) and info may be NULL; the five arrays: host, `cap` entries each.  A tree of more than cap nodes:
   DGE_ERR_CAP with info->n_nodes set (2 x used rows - 1 always suffices) */
int  dge_tree_fit_vectors(const dge_vectors* v, const uint8_t* y, const uint8_t* select, const dge_tree_cfg* cfg, int64_t cap, int32_t* feature, double* threshold,
                          int32_t* left, int64_t* count, int64_t* pos, dge_tree_info* info);
/* out_labels: host uint8[rows], the leaf vote of every present row, 255 on an absent one.  A malformed tree — an inner node whose feature is outside the rows'
   columns or whose children are not behind it and inside the tree — is DGE_ERR_ARG; nothing is read out of bounds */
int  dge_tree_predict_vectors(const dge_vectors* v, int64_t n_nodes, const int32_t* feature, const double* threshold, const int32_t* left, const int64_t* count,
                              const int64_t* pos, uint8_t* out_labels);
/* y: host uint8[rows], fold: host int32[rows]; correct, tested: host int64[n_folds]; n_nodes, depth: host int32[n_folds], may be NULL, as cfg and info */
int  dge_tree_cv_vectors(const dge_vectors* v, const uint8_t* y, const int32_t* fold, int32_t n_folds, const dge_tree_cfg* cfg, int64_t* correct, int64_t* tested,
                         int32_t* n_nodes, int32_t* depth, dge_tree_info* info);
/* the same on host rows float32 [n_rows x dim], every row present (through dge_vectors_from_host) */
int  dge_tree_fit(int device, const float* features, int64_t n_rows, int32_t dim, const uint8_t* y, const uint8_t* select, const dge_tree_cfg* cfg, int64_t cap,
                  int32_t* feature, double* threshold, int32_t* left, int64_t* count, int64_t* pos, dge_tree_info* info);
int  dge_tree_cv(int device, const float* features, int64_t n_rows, int32_t dim, const uint8_t* y, const int32_t* fold, int32_t n_folds, const dge_tree_cfg* cfg,
                 int64_t* correct, int64_t* tested, int32_t* n_nodes, int32_t* depth, dge_tree_info* info);

/* ------------------------------------------------------------------------------------------------
 * Leave-one-out ridge regression (new; additions only, DGE_VERSION unchanged): the reference's fourth figure of merit, the regression error that closes
 * regression-eval.sh (:43-49): P/tf_linear_regression.py:61-83 leaves one region out, fits a linear model with an L2 penalty on the rest, predicts the region
 * left out and prints np.mean(mae) and np.mean(mae) / mean(target).  The reference's fit is 10 steps of TensorFlow's FTRL from TensorFlow's initialisation: not
 * a converged fit, and not reproducible by the reference itself.  Here it is a RULE (csrc/ridge.hip; the per-element pieces and a one-thread host solver:
 * csrc/ridge_rule.h): ridge regression solved in closed form, the left-out errors from the leverage identity e_i = r_i / (1 - h_i) instead of n refits.  The
 * result is a pure function of the used rows in row order, the targets and the penalties, bit for bit, whatever the launch geometry, the chunk size or the
 * schedule of the factorisation: only rounded + * / and fma take part, each element's chain in the order fixed below.  tests/ridge_ref.py is this text in Python.
 *   - INPUTS.  Resident float32 rows [rows x dim] with one present byte per row, 1 <= dim <= 256; an optional host array `select`, one byte per row (NULL: every
 *     present row); host targets y, binary64 [rows x n_targets] row-major, 1 <= n_targets <= 64; host lambda[n_lambda], binary64, each finite and >= 0,
 *     1 <= n_lambda <= 64.  The USED rows are the present rows with a non-zero select byte, in ascending row order; n is their count, 2 <= n <= 2^31 - 1, and
 *     "row i" below is the i-th of them.  Anything outside the limits: DGE_ERR_ARG with the reason.  A feature or a target that is not finite in a used row:
 *     DGE_ERR_ARG naming the least such row (by its number among all rows); rows that are not used are never read, neither their features nor their targets.
 *     Null arguments and the limits on dim, n_targets, n_lambda and lambda: DGE_ERR_ARG before a device is looked for.  On any error the outputs are untouched.
 *   - DESIGN ROW.  P = dim + 1; z[i][0] = 1.0, z[i][j] = (double)x[i][j-1].
 *   - MOMENTS, in the blocked order of k-means: the used rows, in order, are cut into blocks of 256.  For 0 <= a <= b < P a block's partial of G[a][b] starts at
 *     +0.0 and adds z[i][a] * z[i][b] row by row — the product of two float32 values is exact in binary64, so a step is one rounding — and the block partials
 *     are added, from +0.0, in block order.  c[t][a] has the same shape with acc = fma(z[i][a], y[i][t], acc).  ysum[t] is the blocked sum of y[i][t] (c[t][0]
 *     holds the same bits).
 *   - SYSTEM.  For each lambda: A = G (symmetric) with lambda added once, one rounded addition, to every A[j][j], j >= 1.  The intercept is not penalised.
 *   - FACTORISATION.  A = L D L' with L unit lower triangular, no pivoting, no square root.  For j ascending: acc = A[j][j]; for k = 0 .. j-1 ascending:
 *     t = L[j][k] * d[k] (rounded), acc = fma(-L[j][k], t, acc); d[j] = acc.  For every i > j: acc = A[i][j], the same chain with fma(-L[i][k], L[j][k] * d[k], acc),
 *     then L[i][j] = acc / d[j], one division.  Every element's chain runs over k ascending, so any column-parallel schedule gives the same bits.  A d[j] that
 *     is not > 0 — what lambda = 0 gives on collinear columns — refuses the call: DGE_ERR_ARG naming j and the index of the lambda.
 *   - COEFFICIENTS, per lambda l and target t.  w[j] starts at c[t][j]; forward: w[j] = fma(-L[j][k], w[k], w[j]) for k = 0 .. j-1 ascending; then one division
 *     w[j] = w[j] / d[j]; backward: w[j] = fma(-L[k][j], w[k], w[j]) for k = P-1 .. j+1 descending.  beta[l][t][0 .. P) = w, the intercept first.
 *   - LEVERAGE, per lambda and row.  u = L^-1 z[i]: u[j] starts at z[i][j], then u[j] = fma(-L[j][k], u[k], u[j]) for k ascending.  inv[j] = 1.0 / d[j], computed
 *     once.  h[i] = the chain acc = fma(u[j], u[j] * inv[j], acc) (the inner product rounded), j ascending from +0.0.
 *   - LEFT-OUT ERROR, per lambda, target and row.  p = beta[0], then p = fma(z[i][j], beta[j], p) for j = 1 .. P-1 ascending; r = y[i][t] - p; g = 1.0 - h[i].  A g
 *     that is not > 0 (a row nothing else can predict) refuses the call: DGE_ERR_ARG naming the row (among all rows) and the index of the lambda.  Otherwise
 *     e = r / g, and the left-out prediction is y[i][t] - e.
 *   - REFUSALS IN ORDER.  Every factorisation comes before the first leverage: a pivot's refusal goes before a leverage's; among pivots the least lambda index
 *     and its first j; among leverages the least lambda index and its least row.
 *   - FIGURES.  mae[l][t] = the blocked sum of |e| divided by (double)n; mre[l][t] = mae[l][t] / (ysum[t] / (double)n), the reference's second printed number;
 *     it is +-inf or NaN where the targets' mean is 0.
 *   - PREDICTION (dge_ridge_predict_vectors): for every present row of any resident rows of the same dim, the p chain above; NaN on an absent row, which is not
 *     read.  For a fit on one select mask applied to the other rows.
 *   - NOT TensorFlow's FTRL regressor.  NOT a standardising pipeline: the columns are taken as they are, and a host that wants them scaled scales them.  NOT
 *     order-free: it is a function of the used rows in row order, as k-means is.  No search for lambda, no k-fold, no wide-and-deep model
 *     (P/tf_hybrid_regression.py); the target tables are read by the count tables' reader (dge_counts_*) where they are delimited text.
 *   - Device memory for the moments' block partials is bounded by a chunk of blocks (64; the knob DGE_TUNE_RIDGE_CHUNK sets it by hand), not by n; the result
 *     is the same for every chunk size.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dge_ridge_info {
    int64_t rows;              /* n: the used rows                                                         */
    int64_t blocks;            /* blocks of 256 used rows                                                  */
    int64_t chunks;            /* chunks of blocks the moments were taken in                               */
    double  min_pivot;         /* the least d[j] of all factorisations                                     */
    double  max_leverage;      /* the greatest h[i] of all lambdas                                         */
    double  kernel_ms;         /* HIP-event time from the first kernel of the call to its last             */
} dge_ridge_info;              /* 48 bytes */
/* y: host binary64 [rows x n_targets]; mae, mre: host binary64 [n_lambda x n_targets]; beta: host [n_lambda x n_targets x (dim + 1)]; loo_pred: host
   [n_lambda x n_targets x rows], NaN on rows that are not used; select, beta, loo_pred and info may be NULL */
int  dge_ridge_loo_vectors(const dge_vectors* v, const double* y, int32_t n_targets, const uint8_t* select, const double* lambda, int32_t n_lambda, double* mae, double* mre,
                           double* beta, double* loo_pred, dge_ridge_info* info);
/* the same on host rows float32 [n_rows x dim], every row present (through dge_vectors_from_host); fewer than 2 used rows and a target that is not finite are
   refused before a device is looked for */
int  dge_ridge_loo(int device, const float* features, int64_t n_rows, int32_t dim, const double* y, int32_t n_targets, const uint8_t* select, const double* lambda,
                   int32_t n_lambda, double* mae, double* mre, double* beta, double* loo_pred, dge_ridge_info* info);
/* beta: host binary64 [n_models x (dim + 1)], 1 <= n_models <= 4096; out: host binary64 [n_models x rows] */
int  dge_ridge_predict_vectors(const dge_vectors* v, const double* beta, int32_t n_models, double* out);

/* ------------------------------------------------------------------------------------------------
 * SVM classification accuracy (new; additions only, DGE_VERSION unchanged): the SVM line of the reference's classification table,
 * P/binaryClassification_CA.py:33-58 — for every label cross_val_score(svm.SVC(), F, l[k], cv=10) (:38,55-57) beside the tree's.  libsvm's result depends on its
 * kernel cache, its shrinking heuristic and the platform's exp.  Here an RBF C-SVC solved by sequential minimal optimisation, its decision function and its
 * F-fold cross-validated accuracy for many label columns at once are a RULE (csrc/svm.hip; the per-element pieces and a one-thread host solver:
 * csrc/svm_rule.h): a pure function of the used rows in row order, the labels, the folds and the configuration, bit for bit, whatever the launch geometry,
 * the place of the solver's state or the length of a launch.  Only rounded + - * / and fma take part, each element's chain in the order fixed below; RN(.)
 * marks one rounding to binary64.  tests/svm_ref.py is this text in Python.
 *   - INPUTS.  Resident float32 rows [rows x dim], 1 <= dim <= 4096, one present byte per row; host labels y, uint8 [n_labels x rows] in {0, 1},
 *     1 <= n_labels <= 64.  A row is USED if it is present and, where a `select` mask is given, selected; in a cross-validation, if it is present and its fold
 *     is not -1.  n is the number of used rows, taken in ascending row order, 2 <= n <= 65 536: fewer is DGE_ERR_ARG, more is DGE_ERR_RANGE (the kernel matrix
 *     is held whole, there is no row cache).  A value that is not finite in a used row: DGE_ERR_ARG naming the least (row, column); a label other than 0 or 1
 *     on a used row: DGE_ERR_ARG naming it.  Rows that are not used are never read.  s_t = +1 for label 1, -1 for label 0.
 *   - CONFIGURATION, struct dge_svm_cfg (NULL: the defaults): C > 0 and finite (1); gamma > 0 and finite (1.0 / dim, scikit-learn's gamma='auto' of 2017);
 *     eps > 0 (1e-3); max_iter >= 0 (10 000 000); state: 0 = the library chooses, 1 = the solver's state in LDS, 2 = in global memory (1 on more than 3 584
 *     used rows: DGE_ERR_ARG with that bound); launch_iters >= 0: iterations per kernel launch, 0 = the library's default (1 024; at most 65 536 are run in
 *     one launch whatever the value).  No kernel of the solver loops unbounded.  state and launch_iters change no bit of any result.  Anything outside these
 *     limits: DGE_ERR_ARG before a device is looked for.
 *   - KERNEL MATRIX.  d2(i, j) is k-means' distance chain: t = (double)x_i[c] - (double)x_j[c], acc = fma(t, t, acc), c ascending from +0.0.
 *     K(i, j) = E(-(gamma * d2)): one rounded product, an exact negation, and E the exponential of the spatial graph's weight (csrc/spatial_weight.h).  K is
 *     symmetric bit for bit (t only changes sign) and K(i, i) = 1.  It is computed once per call for all used rows, 8 n^2 bytes, and shared by every problem
 *     of the call; device memory that does not hold it: DGE_ERR_CAP.
 *   - ONE PROBLEM = a set of training rows (a subset of the used rows, ascending) and one label column.  State: alpha_t = 0, G_t = -1 for every training
 *     row.  v_t = -s_t * G_t (exact).  I_up = {s_t = +1 and alpha_t < C} u {s_t = -1 and alpha_t > 0}; I_low = {s_t = +1 and alpha_t > 0} u {s_t = -1 and
 *     alpha_t < C}.  "At a bound" always means alpha == 0 or alpha == C exactly.  Iteration k = 0, 1, ...:
 *       1. m = max v_t over I_up, attained at i = the least such row; M = min v_t over I_low.
 *       2. If either set is empty, or RN(m - M) < eps: stop, converged = 1.  Else if k == max_iter: stop, converged = 0.
 *       3. For every t in I_low with v_t < m: b_t = RN(m - v_t); a_t = RN(2.0 - 2.0 * K(i, t)), replaced by 0x1p-40 where it is not > 0;
 *          score_t = RN(RN(b_t * b_t) / a_t).  j = the row of the greatest score, the least row among equals.  Both selections are exact comparisons under
 *          a total order: any reduction tree gives the same i, j.
 *       4. delta = RN(b_j / a_j); lim_i = (s_i > 0 ? RN(C - alpha_i) : alpha_i); lim_j = (s_j > 0 ? alpha_j : RN(C - alpha_j)); delta = min(delta, lim_i, lim_j).
 *       5. alpha_i' = its bound (C if s_i > 0, else 0) when delta == lim_i, otherwise RN(alpha_i + s_i * delta) clamped into [0, C]; alpha_j' = its bound
 *          (0 if s_j > 0, else C) when delta == lim_j, otherwise RN(alpha_j - s_j * delta) clamped.
 *       6. D_i = RN(alpha_i' - alpha_i), D_j likewise; for every training row t: G_t = fma(s_t s_j K(t, j), D_j, fma(s_t s_i K(t, i), D_i, G_t)); the sign
 *          flips are exact.  Each element's chain is fixed, so any geometry gives the same bits.
 *     After the loop: bias = RN(RN(m + M) * 0.5) from the last m, M; where one set was empty, the other value twice.  iterations = the updates made.  A
 *     one-class training set: alpha = 0, iterations = 0, converged = 1, bias = +1 (all labels 1) or -1 (what the loop gives by itself).  An empty training
 *     set: DGE_ERR_ARG naming the fold.
 *   - DECISION.  The SUPPORT rows are the training rows with alpha > 0, in ascending row order; coef_u = s_u * alpha_u.  For a row x the terms
 *     RN(coef_u * K(x_u, x)) over the support rows are added in k-means' blocked order: blocks of 256 support rows are each summed from +0.0 in order, and the
 *     block sums are added, from +0.0, in block order.  f(x) = RN(bias + sum); the label is 1 iff f(x) > 0.  It depends on the support rows and their
 *     coefficients only: a stand-alone decision call on the coef a fit returned gives the bits the cross-validation used.
 *   - CROSS-VALIDATION.  fold[i] in -1 .. F-1, 1 <= F <= 64, as dge_tree_cv*.  Problem (l, f) trains label column l on the used rows with fold != f and is
 *     tested on those with fold == f; the call runs all n_labels x F problems, one workgroup each, in one grid.  A fold without test rows reports 0 of 0.
 *   - NOT libsvm: no shrinking, no cache, an exponential of its own; the bias is the midpoint of the final gap, not an average over the free rows; ties are
 *     decided by row; the folds are the caller's (embedding_amd.evaluate.stratified_folds is the rule the Python view offers), not StratifiedKFold's.  RBF
 *     only.  Binary labels.  No probabilities.  No class weights.  No search over C or gamma.
 *   - Null and negative arguments: DGE_ERR_ARG naming the entry and "null", before a device is looked for.  On any error the outputs are untouched.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dge_svm_cfg {
    double  C;                 /* > 0, finite; default 1                                                   */
    double  gamma;             /* > 0, finite; default 1.0 / dim                                           */
    double  eps;               /* > 0; default 1e-3                                                        */
    int64_t max_iter;          /* >= 0; default 10 000 000                                                 */
    int32_t state;             /* 0 = the library chooses, 1 = LDS, 2 = global memory                      */
    int32_t launch_iters;      /* iterations per kernel launch, 0 = the library's default                  */
} dge_svm_cfg;                 /* 40 bytes */
typedef struct dge_svm_info {
    int64_t rows;              /* n: the used rows                                                         */
    int64_t problems;          /* n_labels, or n_labels x n_folds                                          */
    int64_t iterations;        /* summed over the problems                                                 */
    int64_t max_iterations;    /* the longest problem's                                                    */
    int64_t not_converged;     /* problems that stopped at max_iter                                        */
    int64_t support;           /* support rows, summed over the problems                                   */
    int64_t kernel_bytes;      /* 8 n^2                                                                    */
    int64_t launches;          /* of the solver                                                            */
    double  kernel_ms;         /* HIP-event time from the kernel matrix to the call's last kernel (the     */
                               /* check of the values runs before it, ahead of the large allocations)      */
} dge_svm_info;                /* 72 bytes */
/* One model per label column on all used rows.  y: host uint8 [n_labels x rows]; coef: host binary64 [n_labels x rows], s * alpha, 0 on used rows that are not
   support, NaN on rows not used; bias: host binary64 [n_labels]; iterations: host int64 [n_labels], converged: host int32 [n_labels]; select, cfg, iterations,
   converged and info may be NULL */
int  dge_svm_fit_vectors(const dge_vectors* v, const uint8_t* y, int32_t n_labels, const uint8_t* select, const dge_svm_cfg* cfg, double* coef, double* bias,
                         int64_t* iterations, int32_t* converged, dge_svm_info* info);
/* f(x) of n_models models for every row of x (which may be sv itself; same dim, same device).  coef: host binary64 [n_models x rows(sv)] — rows of sv with
   coef 0 or NaN are not support and are not read, a coefficient on an absent row is DGE_ERR_ARG; bias: host [n_models], 1 <= n_models <= 4096;
   out: host binary64 [n_models x rows(x)], NaN on absent rows of x.  The values of sv and x are taken as they are */
int  dge_svm_decision_vectors(const dge_vectors* sv, const double* coef, const double* bias, int32_t n_models, double gamma, const dge_vectors* x, double* out);
/* fold: host int32 [rows]; correct, iterations, support: host int64 [n_labels x n_folds], converged: host int32 [n_labels x n_folds]; tested: host int64
   [n_folds]; decision: host binary64 [n_labels x rows], the held-out f(x) of every used row, NaN elsewhere.  cfg, iterations, support, converged, decision and
   info may be NULL */
int  dge_svm_cv_vectors(const dge_vectors* v, const uint8_t* y, int32_t n_labels, const int32_t* fold, int32_t n_folds, const dge_svm_cfg* cfg, int64_t* correct,
                        int64_t* tested, int64_t* iterations, int64_t* support, int32_t* converged, double* decision, dge_svm_info* info);
/* the same on host rows float32 [n_rows x dim], every row present (through dge_vectors_from_host); x_features NULL: the rows of sv themselves,
   and n_x is not looked at */
int  dge_svm_fit(int device, const float* features, int64_t n_rows, int32_t dim, const uint8_t* y, int32_t n_labels, const uint8_t* select, const dge_svm_cfg* cfg,
                 double* coef, double* bias, int64_t* iterations, int32_t* converged, dge_svm_info* info);
int  dge_svm_decision(int device, const float* sv_features, int64_t n_sv, int32_t dim, const double* coef, const double* bias, int32_t n_models, double gamma,
                      const float* x_features, int64_t n_x, double* out);
int  dge_svm_cv(int device, const float* features, int64_t n_rows, int32_t dim, const uint8_t* y, int32_t n_labels, const int32_t* fold, int32_t n_folds,
                const dge_svm_cfg* cfg, int64_t* correct, int64_t* tested, int64_t* iterations, int64_t* support, int32_t* converged, double* decision, dge_svm_info* info);

/* ------------------------------------------------------------------------------------------------
 * Per-slice pairwise evaluation (new; additions only, DGE_VERSION unchanged): evalute_by_pairwise_similarity of P/embeddingEvaluation_tract.py:285-367, the
 * figure behind python/ndcg.pickle — nDCG@k of a method's neighbour lists under the POI ground truth for every slice and every k of the figure at once,
 * precision@k against the ground's nearest rel_m (precision_atK, :236-246) and coverage (:326-331), from resident rows (csrc/pairwise.hip; the per-element
 * pieces: csrc/pairwise_rule.h).  The reference takes scipy's cosine and numpy's sums; here the figure is a RULE, restated by the kernels and by
 * tests/pairwise_ref.py, and the result is a pure function of the inputs.
 *
 * Inputs: ground rows gnd [n x g] float32, one row a region, g <= 256; feature rows f [V x D], D <= 256; row_of [n_sets x n] int64, the feature row of region i
 * in set s, or -1; test [n] bytes or NULL; ks [n_k], strictly ascending, 1 <= k <= 128, n_k <= 16, kmax the last; rel_m (0: no precision, else 1 .. n - 1).
 *  1. MEMBERS.  Region i is a member of set s iff row_of[s][i] >= 0 and that row is present in f.  A set is scored over its members with test non-zero (NULL:
 *     all members).  coverage = members / n.
 *  2. GROUND DISTANCE.  Every value is widened to binary64.  ss[a] is the chain acc = acc + x_j * x_j and dot(a, b) the chain acc = acc + x_aj * x_bj, j
 *     ascending from 0 (the product of two widened float32 is exact, so a fused multiply-add gives the same bits).  Row a is a ZERO VECTOR iff it is absent or
 *     ss[a] is not in (0, +inf) — a NaN or an infinity anywhere in the row makes it one.  dist(a, b) = 2 if either is a zero vector, else
 *     1 - dot / sqrt(ss[a] * ss[b]): one rounded multiply, one rounded sqrt, one rounded divide, one rounded subtract.  It is symmetric bit for bit.
 *  3. GROUND ORDER of region r: the keys (dist(r, c), c) over ALL c != r in 0 .. n-1, members or not; the distance ascends, then the region number (Python's
 *     stable sort over rids, :99, NaN -> 2, :96-97).  The ideal list is the kmax least keys; rank(r, j) = the number of c != r with key(r, c) < key(r, j).
 *  4. DISCOUNTS.  disc[i] = 1 / log2(i + 2), i = 0 .. kmax-1, taken by the host with the C library's log2 and one division, then uploaded.
 *  5. ESTIMATED LISTS.  The members' feature rows of set s are stacked in region order; the list of a member is exactly what dge_knn_cosine gives for that
 *     stack with k = kmax, mapped back to region numbers (the stacking is monotone, so ties go to the smaller region number).  A set with fewer than kmax + 1
 *     members: DGE_ERR_ARG naming the least such set and its member count (the reference raises there).
 *  6. SCORES of a tested region r in set s.  dcg is the chain acc = acc + (1 - dist(r, nb_i)) * disc[i], i ascending: a rounded subtract, a rounded multiply, a
 *     rounded add, no fma; its value after i = k-1 is dcg_k, so every k comes from one chain.  ideal_k[r] is the same chain over the ideal list.
 *     ratio = ideal_k != 0 ? dcg_k / ideal_k : 0 (a zero-vector ground row has every relevance -1 and so ratio 1, as in the reference).
 *     hits_k = the number of i < k with rank(r, nb_i) < rel_m.
 *  7. MEANS.  ndcg[s][k] = the plain ascending sum of ratio over the tested regions in region order, taken on the host, divided by their count.
 *     precision[s][k] = sum(hits_k) / (k * tested), the product an integer.  (The reference divides by the number of ALL regions, :241; `tested` is returned so
 *     that a caller can rescale.)  A set with no tested region reports 0 and tested = 0.
 *  8. ERRORS.  DGE_ERR_ARG for: a row_of entry outside [-1, V) (naming the set and the region); a feature row named twice within a set; n - 1 < kmax; ks not
 *     strictly ascending; f and gnd on different devices; nulls and limits.  All of these are looked at before a device is looked for.  The presence of a
 *     row, the one check that needs device data, comes after: a row_of entry that names an absent row makes no member, and a set left short is refused (5).
 *  9. PURITY.  The result is a pure function of the two tables, row_of, test, ks and rel_m; it does not depend on launch geometry or on how the sets are
 *     spread over calls.
 * Outputs: ndcg, precision [n_sets x n_k] (precision NULL iff rel_m == 0); members, tested [n_sets]; ratio binary64 and hits int32 [n_sets x n_k x n], 0 where
 * the region is not tested; lists int32 [n_sets x n x kmax], region numbers, -1 rows for non-members; ideal [n_k x n].  The last four and info may be NULL.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dge_pairwise_info {
    int64_t regions;         /* n                                                                  */
    int64_t members;         /* over all sets                                                      */
    int64_t tested;          /* over all sets                                                      */
    int64_t threshold_keys;  /* slots of a region's sorted neighbour keys in the rank pass (0: rel_m == 0) */
    double  knn_ms;          /* HIP-event time of the strip kernels                                */
    double  ground_ms;       /* of the ground side: norms, ideal pass, rank pass (none: rel_m == 0) */
    double  score_ms;
} dge_pairwise_info;         /* 56 bytes */
int  dge_pairwise_eval_vectors(const dge_vectors* f, const dge_vectors* gnd, const int64_t* row_of, int32_t n_sets /* <= 64 */, const uint8_t* test,
                               const int32_t* ks, int32_t n_k, int32_t rel_m, double* ndcg, double* precision, int64_t* members, int64_t* tested,
                               double* ratio, int32_t* hits, int32_t* lists, double* ideal, dge_pairwise_info* info);
/* the ground's own m <= 128 nearest by steps 2 and 3 (generatePairWiseGT's lists as far as a list goes; beyond 128 the rank of step 3 answers membership):
   idx int32, dist binary64, host [n x m]; n - 1 < m: DGE_ERR_ARG */
int  dge_pairwise_ground_vectors(const dge_vectors* gnd, int32_t m, int32_t* idx, double* dist);

/* ------------------------------------------------------------------------------------------------
 * Ablation / test knobs of the trainer (process-wide relaxed atomics; nothing in a normal run sets them).  value < 0 puts
 * a knob back to the library's own rule.
 * ---------------------------------------------------------------------------------------------- */
enum {
    DGE_TUNE_HOT_ROWS = 0,        /* update_policy 7: head rows [0, value) stay out of the lock protocol instead of the count-derived head */
    DGE_TUNE_HS_DRAIN = 1,        /* hierarchical softmax: additions between drains of an LDS accumulator (default 64) */
    DGE_TUNE_FORCE_SEGMENTS = 2,  /* > 0: address the tables through per-segment descriptors as tables of >= 4 GiB are (parity tests) */
    DGE_TUNE_SEGMENT_SHIFT = 3,   /* rows per descriptor segment = 2^value (with FORCE_SEGMENTS: many segments on a small table) */
    DGE_TUNE_SORTED_CHUNK = 4,    /* update_policy 8: items per work unit (default 128); a row's item list longer than what is left of a unit is split */
    DGE_TUNE_SORTED_WALKS = 5,    /* update_policy 8: walks per synchronous mini-batch (default: as many as the item buffers hold) */
    DGE_TUNE_WORKERS = 6,         /* workers = 0 (fill the device): this many concurrent walks instead of the count the library derives */
    DGE_TUNE_STATIC_WALKS = 7,    /* > 0: the lock kernels' worker w trains walks w, w + workers, ... instead of taking them from a launch-wide counter */
    DGE_TUNE_HS_COLD = 8,         /* hierarchical softmax under atomics: inner nodes [0, value) take plain read-modify-write (default: those on < 2e-5 of the paths — derived from the COUNTS the model was created with: they must describe the corpus that is trained, or updates of nodes that are busier than their count says are lost; 0 = every node by atomics) */
    DGE_TUNE_HS_WAVE = 9,         /* hierarchical softmax under atomics: 0 = the workers issue their atomics themselves, 1 = through the workgroup's atomics wave (default: the wave from 65 536 rows on) */
    DGE_TUNE_ACC_ROWS = 10,       /* update_policy 7: the hottest rows [0, value) add their syn1neg updates up in LDS (one set of atomics per DGE_TUNE_ACC_DRAIN updates; the kernel caps the value at what its LDS holds, 8 .. 16); one GPU: default 0 = none (measured: 2-4 %, and from 16 updates a flush on it shifts the trained scores).
                                     One block of the multi-GPU schedule (v106): the partition's hottest `value` rows of BOTH tables (a bank each; slot = the row's rank inside the partition); default 16 where the busiest row's chain of atomics is long against the block, else 0; 0 = off, > 0 = on whatever the chain */
    DGE_TUNE_ACC_DRAIN = 11,      /* updates of such a row between two flushes (one GPU: default 16; a block: default 2048 / workgroups of the launch = 4 — 16 diverges there, measured) */
    DGE_TUNE_TABLE_RUNS = 12,     /* the negative-sampling table's run form (dge_model_table_runs): 0 = not built / not used (the lock kernels read the table), N > 0 = built from at most N runs of the vocabulary's tail (tests: the head rows in front stay on the table); default: up to 2 046 runs */
    DGE_TUNE_BLOCK_SYN0_FREE = 13, /* block schedule, mixed lock kernel: 1 = the pair's syn0 row is never locked (agent-scope read, atomics), 0 = it is locked unless it is a head row; default: the library's rule */
    DGE_TUNE_HS_CENTRE = 14,      /* hierarchical softmax under atomics: 0 = pair by pair (k_sgns_train), 1 = a wave per centre wherever it applies (rows of up to 128 floats, walks of up to 64 tokens; k_sgns_train_hsw); 2 = that kernel with the pair's negatives and the centre's gathered syn1neg update under the rows' commit locks instead of atomics, 3 = the same in workgroups of seven training waves (one a compute unit) that share their LDS accumulators; default: a wave per centre from 65 536 vocabulary rows on — form 3 where update_policy 0 would pick the commit locks for the negative-sampling kernels, form 1 elsewhere */
    DGE_TUNE_HS_HOT_KB = 15,      /* k_sgns_train_hsw: > 0 = keep the inner nodes next to the root in that many KB of LDS accumulators per workgroup (drained every DGE_TUNE_HS_DRAIN additions; round 4's first form: faster by a tenth, staler) instead of the default, the busiest nodes in copies (nothing parked; the root's number of copies: DGE_TUNE_HS_COPIES).  Capped at 100 (seven-wave workgroups) / 30 (three-wave) */
    DGE_TUNE_ALLOW_UNSAFE = 16,   /* > 0: a FORCED update_policy runs even where the library would refuse it (8 on a vocabulary whose busiest row would take > 8192 terms of one mini-batch; 5 / 6 where workers x the busiest row's share > 2) — tests of the watchdog, reproductions of the failure */
    DGE_TUNE_WATCHDOG_MS = 17,    /* the lock kernels' watchdog: a worker still waiting for a row lock after this many milliseconds of the launch gives up (dge_model_stats then returns DGE_ERR_STATE); 0 = no watchdog; default: 5 s + 100 x the launch's bytes at the 8 TB/s roofline */
    DGE_TUNE_HS_COPIES = 18,      /* k_sgns_train_hsw, copies form: the root's number of copies (a node's copies = ceil(its share of the paths x value), at most 16); default 16 */
    DGE_TUNE_SMALL_ROWS = 19,     /* rows of 17 .. 32 floats under the atomics policy: 1 = k_sgns_train_small (32 lanes a worker, a row = one request), 0 = k_sgns_train's 16-lane groups; default: the small-row kernel wherever it applies (v106) */
    DGE_TUNE_TREE_BATCH = 20,     /* dge_tree_cv*: at most this many trees grow together (1: one after another); default: as many as half the free device memory holds */
    DGE_TUNE_RIDGE_CHUNK = 21,    /* dge_ridge_loo*: blocks of 256 used rows whose partial moments are held at once (default 64); the result is the same for every value */
    DGE_TUNE_COUNT = 22
};
int  dge_set_tuning(int32_t knob, int64_t value);
int  dge_get_tuning(int32_t knob, int64_t* value);   /* -1 = the library's own rule */

/* ------------------------------------------------------------------------------------------------
 * Count tables (new; additions only, DGE_VERSION unchanged): the ground-truth tables the evaluators are scored against — a resident int64 table c[R][C] over a
 * dge_regions handle, filled from delimited text, from points and from entries, merged along a region map and handed on as dge_vectors
 * (csrc/table_read.hip, csrc/table_parse.h).  The reference builds them line by line on the host: getLEHDfeatures_helper
 * (P/embeddingEvaluation_tract.py:512-536), generateLEHD_ac_clusteringLabel (:473-509), generateCrimeClusteringlabel (:435-449),
 * generateTweetsClusteringlabel (:398-407), get_CAfeatures_from_tractFeatures (P/embeddingCaseStudy_CA.py:56-74), Tweets.mapTweetsIntoTracts
 * (J/Tweets.java:43-88) and the read of taxi-flow-time-series.txt (P/caseStudy.py:44-48).  Each ends in row / row.sum() and KMeans: dge_counts_vectors and
 * dge_kmeans_vectors.  Pickles and shapefiles stay with the host, which puts what it unpickled in through dge_counts_add_entries.  The rule:
 *   - THE TABLE.  R is the regions' count; ROW i belongs to the region with the i-th least id (with ids given ascending, as Regions.from_ids usually gets
 *     them, that is the region index).  1 <= C <= 1024.  Everything that fills the table is 64-bit integer addition: the table is a pure function of the
 *     multiset of contributions — not of slab_bytes, launch geometry or timing.  A call stages its contributions and commits once: a call that would leave a
 *     cell above 2^62, or whose own values add up to more than 2^62, is DGE_ERR_RANGE, and on ANY refusal the table is as it was.
 *   - dge_counts_add_entries: host arrays row[], col[], value[] of n entries in any order, with repeats; 0 <= row < R, 0 <= col < C, 0 <= value <= 2^40, else
 *     DGE_ERR_ARG naming the least offending position.  The independent way in, and the way back for what dge_counts_to_host gave.
 *   - dge_counts_add_points: point i (x, y) is located by dge_regions_locate's rule — one region or none — and adds 1 to c[row of that region][col[i]].  Points
 *     in no region are counted in *dropped.  Tweets.mapTweetsIntoTracts counts a point once for EVERY tract whose boundary contains it; this counts it once
 *     (interior to several regions is no region, as in dge_regions_locate).  The hour column, time.substring(8, 10), is the host's to compute.
 *   - dge_counts_merge: a NEW table over `groups` with c's C whose row g is the sum of the rows i of c with group_of[i] == g; group_of[i] is a row of the new
 *     table or -1, which drops row i; anything else is DGE_ERR_ARG.  A sum above 2^62: DGE_ERR_RANGE.  The two region handles lie on one device.
 *   - dge_counts_vectors: columns [col_lo, col_lo + n_cols) as float32 rows.  s_i is the exact sum of row i's selected columns (above 2^63 - 1:
 *     DGE_ERR_RANGE).  normalise != 0: (float)((double)c / (double)s_i), each conversion and the division rounded to nearest even; a row with s_i == 0 is all
 *     +0.0f.  normalise == 0: (float)c.  DGE_COUNTS_PRESENT_ALL marks every row present — POI and LEHD-od keep their zero rows (:411-432, :453-469);
 *     DGE_COUNTS_PRESENT_NONZERO marks the rows with s_i != 0 — LEHD-ac and the CA merge drop the others (:498-505).  The crime file's float total column
 *     is not read anywhere: normalise divides by the row's own sum.
 *   - THE TEXT READER (dge_counts_add_table_texts / _files).  A text is BYTES, in pieces; no line crosses a piece.
 *       LINES end at "\n", "\r\n" or a lone "\r" (the trip reader's rule and its feeder, csrc/seq_pieces.h).  The first skip_lines lines of every piece are
 *         headers: counted in info.skipped and not looked at.  Lines of zero bytes are counted in info.empty and skipped.  A piece's last line may lack its
 *         terminator.  A line of more than 65 536 bytes is the offence "long line"; nothing else of it is looked at.
 *       FIELDS are cut at every sep byte (',', ' ' or a tab); there is no quoting.  Field numbers count from 0.  Only the key field and the value fields are
 *         looked at; every other field's bytes pass unread but for the search for sep.
 *       The KEY is bytes [key_lo, key_hi) of field key_field, clipped to the field's end; key_hi == 0 means to the field's end.  A leading '-' is the offence
 *         "key sign" when neg_col_offset is -1; else the key is the digits behind it and the line's values land at column neg_col_offset instead of
 *         col_offset ("id,in_0..in_23" / "-id,out_0..out_23" of the time-series text).  What remains is 1 .. 18 decimal digits.
 *       VALUES are fields col_lo .. col_lo + n_cols - 1; value j adds itself to column col_offset + j (or neg_col_offset + j) of the row whose region id is the
 *         key.  A value is 1 .. 19 decimal digits, at most 2^40; leading zeros are allowed.  No sign, no blank, no fraction.
 *       FOREIGN KEYS.  A key that is no region's id skips the line and is counted in info.foreign — the reference's `if tid in keys`.  Such a line is still
 *         checked for offences, so the verdict does not depend on the region set.
 *       OFFENCES.  Each has a PLACE, a byte offset in its piece.  The call reports the one at the least (piece, offset), and of two at one place the one listed
 *         first here.  The message names kind, piece (and path), offset, LINE — 1 + the lines of the piece in front — and FIELD — the sep bytes between the
 *         line's start and the place:  "<entry>: <kind> at piece <k>[ (<path>)], offset <o>, line <l>, field <f>".
 *           short line         fewer fields than the key and the values need.  Place: the line's end (its terminator's first byte, or the piece's size).
 *           short key          the key field is shorter than key_lo + 1 bytes.  Place: the field's first byte.
 *           bad key            no digit, a byte that is no digit, or a 19th digit.  Place: that byte, or where the first digit is missing.
 *           key sign           place: the '-'.
 *           empty value        place: the field's place (the sep or terminator that follows at once).
 *           bad value byte     place: the field's first byte that is no digit, when it comes before a 20th digit.
 *           long value         the 20th digit of a field.  Place: that digit.  Such a field is never "above 2^40".
 *           value above 2^40   1 .. 19 digits greater than 2^40.  Place: the field's first byte.  DGE_ERR_RANGE; every other offence is DGE_ERR_IO.
 *           long line          place: the line's first byte.
 *         The offence reported does not depend on slab_bytes.
 *       OTHER STATUSES.  Null or negative arguments, a bad sep, key_hi neither 0 nor above key_lo, key_lo or key_hi above 65 536, n_cols outside 1 .. 1024, a key field among the value fields, columns outside the table, neg_col_offset < -1,
 *         non-zero reserved fields, n_pieces < 1 and a slab_bytes that is neither 0 nor at least 131 072 (the trip reader's range; above 1 GiB is 1 GiB):
 *         DGE_ERR_ARG; plain values are checked before handles, and all of it before a device is looked for or a file is opened.  A missing file: DGE_ERR_IO
 *         with its path.  Device memory: DGE_ERR_CAP.
 * dge_table_read_info, filled on success only: lines counts every line, skipped the headers, empty the empty ones, rows the lines that reached the table,
 * foreign those with a foreign key; values = rows * n_cols, total their sum; read_ms is the host's reading into pinned memory, kernel_ms the slabs' kernels. */
typedef struct dge_counts dge_counts;     /* int64 [R x C], resident in HBM; holds a reference to its regions */
enum { DGE_COUNTS_PRESENT_ALL = 0, DGE_COUNTS_PRESENT_NONZERO = 1 };
struct dge_counts_info {
    int64_t regions;              /* R                                                                      */
    int64_t cols;                 /* C                                                                      */
    int64_t nonzero;              /* cells != 0                                                             */
    int64_t total;                /* the sum of all cells; INT64_MAX when it does not fit                   */
};                                /* 32 bytes */
typedef struct dge_table_read_options {
    int32_t sep;                  /* offset 0: ',', ' ' or '\t'                                             */
    int32_t skip_lines;           /* 4: header lines of every piece                                         */
    int32_t key_field;            /* 8                                                                      */
    int32_t key_lo;               /* 12                                                                     */
    int32_t key_hi;               /* 16: 0 = to the field's end                                             */
    int32_t col_lo;               /* 20: the first value field                                              */
    int32_t n_cols;               /* 24                                                                     */
    int32_t col_offset;           /* 28: value j lands in column col_offset + j                             */
    int32_t neg_col_offset;       /* 32: -1 = a '-' in front of the key is an offence                       */
    int32_t reserved;             /* 36: 0                                                                  */
    int64_t slab_bytes;           /* 40: 0 = the default, 16 MiB                                            */
    int64_t reserved2;            /* 48: 0                                                                  */
} dge_table_read_options;         /* 56 bytes */
typedef struct dge_table_read_info {
    int64_t bytes;                /* offset 0                                                               */
    int64_t lines;                /* 8                                                                      */
    int64_t skipped;              /* 16                                                                     */
    int64_t empty;                /* 24                                                                     */
    int64_t rows;                 /* 32                                                                     */
    int64_t foreign;              /* 40                                                                     */
    int64_t values;               /* 48                                                                     */
    int64_t total;                /* 56                                                                     */
    int32_t pieces;               /* 64                                                                     */
    int32_t slabs;                /* 68                                                                     */
    double  read_ms;              /* 72                                                                     */
    double  kernel_ms;            /* 80                                                                     */
} dge_table_read_info;            /* 88 bytes */
/* what the per-tract rows of the reference's label builders are kept in: replaces the dict of numpy rows of getLEHDfeatures_helper (:519-523) */
int  dge_counts_create(const dge_regions* regions, int32_t n_cols, dge_counts** out);
void dge_counts_destroy(dge_counts* c);
int  dge_counts_info(const dge_counts* c, struct dge_counts_info* out);
int  dge_counts_to_host(const dge_counts* c, int64_t* out /* R x C */);
/* replaces pickle.load of a ready table (generatePOIClusteringlabel, :411-432): the host hands its cells over */
int  dge_counts_add_entries(dge_counts* c, const int32_t* row, const int32_t* col, const int64_t* value, int64_t n);
/* replace the line loops of getLEHDfeatures_helper (:512-536), generateCrimeClusteringlabel (:435-449), generateTweetsClusteringlabel (:398-407) and the
   read of taxi-flow-time-series.txt (P/caseStudy.py:44-48) */
int  dge_counts_add_table_texts(dge_counts* c, const char* const* texts, const int64_t* n_bytes, int32_t n_pieces, const dge_table_read_options* opt,
                                dge_table_read_info* info /* may be NULL */);
int  dge_counts_add_table_files(dge_counts* c, const char* const* paths, int32_t n_pieces, const dge_table_read_options* opt, dge_table_read_info* info /* may be NULL */);
/* replaces Tweets.mapTweetsIntoTracts (J/Tweets.java:43-88); xy: host float64 [n x 2], col: host int32 [n] */
int  dge_counts_add_points(dge_counts* c, const double* xy, const int32_t* col, int64_t n, int64_t* dropped /* may be NULL */);
/* replaces get_CAfeatures_from_tractFeatures (P/embeddingCaseStudy_CA.py:56-74); group_of: host int32 [R] */
int  dge_counts_merge(const dge_counts* c, const dge_regions* groups, const int32_t* group_of, dge_counts** out);
/* replaces row / row.sum() (:505, :531) in front of KMeans */
int  dge_counts_vectors(const dge_counts* c, int32_t col_lo, int32_t n_cols, int32_t normalise, int32_t present_mode, struct dge_vectors** out);

/* ------------------------------------------------------------------------------------------------
 * Device self-test of the commit-lock protocol of update_policy 5 (new; no reference counterpart): n_workers groups
 * each do `iters` rounds of "lock 5 pseudo-random rows of an n_rows x 128 table, add 1.0 to every element, unlock".
 * Returns the number of row increments performed and the largest |element - increments of its row| (0 when no
 * update was lost).
 * ---------------------------------------------------------------------------------------------- */
int  dge_selftest_locked_rows(int device, int32_t n_rows, int64_t n_workers, int32_t iters, uint64_t seed,
                              int32_t commit /* 0 relaxed (policy 5), 1 strict (policy 6), 2 agent release fence */,
                              int64_t* total_increments, double* max_abs_error);
/* The atomics wave of the mixed kernels in isolation, LDS accumulators of the n_acc hottest rows included: `blocks` workgroups x 12 workers x `iters`
   messages of 5 rows each, half of them among the 8 hottest; every element of a row must end at the number of times the row was posted. */
int  dge_selftest_atomics_wave(int device, int32_t n_rows, int32_t n_acc, int32_t drain, int32_t blocks, int32_t iters, uint64_t seed,
                               int64_t* total_updates, double* max_abs_error);
/* the same with the rows of ONE BLOCK of a div-rank schedule (v106): messages alternate between the two tables' accumulator banks, a row's slot is its rank
   inside its partition (row / div); div = 1 is the call above */
int  dge_selftest_atomics_wave_block(int device, int32_t n_rows, int32_t n_acc, int32_t drain, int32_t div, int32_t blocks, int32_t iters, uint64_t seed,
                                     int64_t* total_updates, double* max_abs_error);
/* the LDS combining of the hierarchical-softmax updates near the root (hot_add) in isolation: n_workers workers add 1.0
 * to skewed pseudo-random rows `iters` times with the given drain period; max_abs_error = worst |row element - additions
 * that row received| (0 when no addition is lost or doubled). */
/* host code only: the vector file's number formatter (csrc/fmt_g9.h: printf's "%.9g" by integer arithmetic) against snprintf on n pseudo-random floats;
 * *fast_path = how many took the formatter (the rest are outside its range and go through std::to_chars in dge_write_vec), *mismatches must come back 0 */
int  dge_selftest_fmt_g9(int64_t n, uint64_t seed, int64_t* fast_path, int64_t* mismatches);
int  dge_selftest_hot_add(int device, int32_t n_hot, int64_t n_workers, int32_t iters, int32_t drain, uint64_t seed,
                          int64_t* total_additions, double* max_abs_error);
/* the .seq ingest's tokeniser and name table on `text` (no prior names), with the token hash cut to hash_bits (1 .. 64) bits and the table started at
 * initial_slots slots — few bits make distinct strings share a hash (byte comparison, probing), few slots make the table grow and the pass be redone.
 * ids int32[*n_tokens]: the first-appearance id of every token in text order; *n_names: distinct tokens.  cap < *n_tokens: DGE_ERR_CAP with both counts set. */
int  dge_selftest_seq_intern(int device, const char* text, int64_t n_bytes, int32_t hash_bits, int64_t initial_slots, int32_t* ids, int64_t cap, int64_t* n_tokens,
                             int64_t* n_names);

#ifdef __cplusplus
}
#endif
#endif
