// sgns_exchange.hip — what ranks hand each other between training launches (libdge.so, gfx950): the block schedule's partition copies, the delta
// exchange of the data-parallel form, and the same two with RCCL called from the library.  Outside the build stamp (dge_build_stamp, include/dge.h);
// which block a launch trains is set by dge_model_set_partition (sgns.hip), which the plan reads.
#include <dlfcn.h>
#include <string.h>
#include <rccl/rccl.h>      // types and enum values only (ncclComm_t, ncclUniqueId, ncclFloat32, ncclSum, ncclResult_t): no RCCL symbol is linked

#include "dge_internal.h"
#include "sgns_model.h"

// ------------------------------------------------------------------------------------------ multi-GPU block schedule
// N ranks, rows split by row % N.  In episode e rank g trains the block (contexts in partition g, centres and negatives
// in partition (g+e) % N) of the SAME global batch of walks: the N blocks of an episode touch disjoint rows of both
// tables, after N episodes every pair has been trained exactly once, and nothing is ever averaged or summed — the
// result is the single-GPU result with the pairs in another order.  syn0 partition g never leaves rank g during
// training; after each episode the ranks exchange the syn1neg partitions they just trained (an all-gather of packed rows).
__global__ void k_partition_pack(const float* __restrict__ table, float* __restrict__ buf, int64_t V, int32_t stride, int32_t n, int32_t part, int64_t rows_padded) {
    const int64_t total = rows_padded * stride;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / stride * n + part;
        buf[i] = r < V ? table[r * stride + i % stride] : 0.f;
    }
}
__global__ void k_partition_unpack(float* __restrict__ table, const float* __restrict__ buf, int64_t V, int32_t stride, int32_t n, int32_t part, int64_t rows_padded) {
    const int64_t total = rows_padded * stride;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / stride * n + part;
        if (r < V) table[r * stride + i % stride] = buf[i];
    }
}

extern "C" int dge_model_partition_floats(const dge_model* m, int32_t n_parts, int64_t* n_floats) {
    if (!m || !n_floats || n_parts <= 0) DGE_FAIL(DGE_ERR_ARG, "dge_model_partition_floats: bad argument");
    *n_floats = (m->V + n_parts - 1) / n_parts * (int64_t)m->stride;
    return DGE_OK;
}

// `peer`: the caller's stream the buffer is produced / consumed on.  DGE_STREAM_BLOCKING (the synchronous entry points): a reader of a caller's buffer first waits for
// the whole device, a writer returns after the model's stream has drained.  Otherwise the copy is STREAM-ORDERED and the host never waits: an import makes the
// model's stream wait for what `peer` holds at the time of the call (an event), an export makes `peer` wait for the pack kernel.
#define DGE_STREAM_BLOCKING ((hipStream_t)(intptr_t)-1)
static int partition_copy(dge_model* m, int table, int32_t n_parts, int32_t part, float* d_buf, bool pack, hipStream_t peer) {
    if (!m || !d_buf || n_parts <= 0 || part < 0 || part >= n_parts || table < 0 || table > 2) DGE_FAIL(DGE_ERR_ARG, "dge_model_%s_partition: bad argument", pack ? "export" : "import");
    if (table == 2 && !m->d_syn1) DGE_FAIL(DGE_ERR_STATE, "dge_model_%s_partition: table 2 (syn1) exists with use_hs only", pack ? "export" : "import");
    DGE_HIP(hipSetDevice(m->device));
    const bool blocking = peer == DGE_STREAM_BLOCKING;
    const bool handshake = !blocking && peer != m->stream;
    if (handshake && !m->ev_peer) DGE_HIP(hipEventCreateWithFlags(&m->ev_peer, hipEventDisableTiming));
    if (!pack) {
        if (blocking) DGE_HIP(hipDeviceSynchronize());          // d_buf comes from the caller's collective, on the caller's stream
        else if (handshake) { DGE_HIP(hipEventRecord(m->ev_peer, peer)); DGE_HIP(hipStreamWaitEvent(m->stream, m->ev_peer, 0)); }
    }
    float* tab = table == 0 ? m->d_syn0 : (table == 1 ? m->d_syn1neg : m->d_syn1);
    const int64_t rows = (m->V + n_parts - 1) / n_parts;
    if (rows > 0) {
        if (pack) hipLaunchKernelGGL(k_partition_pack, dim3(2048), dim3(256), 0, m->stream, tab, d_buf, m->V, m->stride, n_parts, part, rows);
        else hipLaunchKernelGGL(k_partition_unpack, dim3(2048), dim3(256), 0, m->stream, tab, d_buf, m->V, m->stride, n_parts, part, rows);
    }
    DGE_HIP(hipGetLastError());
    if (blocking) DGE_HIP(hipStreamSynchronize(m->stream));
    else if (handshake && pack) { DGE_HIP(hipEventRecord(m->ev_peer, m->stream)); DGE_HIP(hipStreamWaitEvent(peer, m->ev_peer, 0)); }
    return DGE_OK;
}
extern "C" int dge_model_export_partition(dge_model* m, int table, int32_t n_parts, int32_t part, float* d_buf) { return partition_copy(m, table, n_parts, part, d_buf, true, DGE_STREAM_BLOCKING); }
extern "C" int dge_model_import_partition(dge_model* m, int table, int32_t n_parts, int32_t part, const float* d_buf) { return partition_copy(m, table, n_parts, part, const_cast<float*>(d_buf), false, DGE_STREAM_BLOCKING); }
extern "C" int dge_model_export_partition_async(dge_model* m, int table, int32_t n_parts, int32_t part, float* d_buf, void* consumer_stream) {
    return partition_copy(m, table, n_parts, part, d_buf, true, (hipStream_t)consumer_stream);
}
extern "C" int dge_model_import_partition_async(dge_model* m, int table, int32_t n_parts, int32_t part, const float* d_buf, void* producer_stream) {
    return partition_copy(m, table, n_parts, part, const_cast<float*>(d_buf), false, (hipStream_t)producer_stream);
}
extern "C" int dge_model_stream(const dge_model* m, void** hip_stream) {
    if (!m || !hip_stream) DGE_FAIL(DGE_ERR_ARG, "dge_model_stream: null argument");
    *hip_stream = (void*)m->stream;
    return DGE_OK;
}

// ------------------------------------------------------------------------------------------ multi-GPU exchange
extern "C" int dge_model_sync_size(const dge_model* m, int64_t* n_floats) {
    if (!m || !n_floats) DGE_FAIL(DGE_ERR_ARG, "dge_model_sync_size: null argument");
    *n_floats = (m->d_syn1 ? 3 : 2) * m->V * (int64_t)m->stride;
    return DGE_OK;
}

__global__ void k_delta_export(const float* __restrict__ cur, const float* __restrict__ snap, float* __restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = cur[i] - snap[i];
}
__global__ void k_delta_import(float* __restrict__ cur, float* __restrict__ snap, const float* __restrict__ in, float scale, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float v = fmaf(scale, in[i], snap[i]);
        cur[i] = v; snap[i] = v;
    }
}

extern "C" int dge_model_snapshot(dge_model* m) {
    if (!m) DGE_FAIL(DGE_ERR_ARG, "dge_model_snapshot: null model");
    DGE_HIP(hipSetDevice(m->device));
    size_t tab = (size_t)m->V * (size_t)m->stride;
    if (!m->d_snap) { int rc = dge_dev_alloc(&m->d_snap, (m->d_syn1 ? 3 : 2) * tab + 64); if (rc) return rc; }
    DGE_HIP(hipMemcpyAsync(m->d_snap, m->d_syn0, tab * sizeof(float), hipMemcpyDeviceToDevice, m->stream));
    DGE_HIP(hipMemcpyAsync(m->d_snap + tab, m->d_syn1neg, tab * sizeof(float), hipMemcpyDeviceToDevice, m->stream));
    if (m->d_syn1) DGE_HIP(hipMemcpyAsync(m->d_snap + 2 * tab, m->d_syn1, tab * sizeof(float), hipMemcpyDeviceToDevice, m->stream));
    DGE_HIP(hipStreamSynchronize(m->stream));
    return DGE_OK;
}

extern "C" int dge_model_export_delta(dge_model* m, float* d_buf) {
    if (!m || !d_buf) DGE_FAIL(DGE_ERR_ARG, "dge_model_export_delta: null argument");
    if (!m->d_snap) DGE_FAIL(DGE_ERR_STATE, "dge_model_export_delta: call dge_model_snapshot before training the shard");
    DGE_HIP(hipSetDevice(m->device));
    int64_t tab = m->V * (int64_t)m->stride;
    if (tab) {
        hipLaunchKernelGGL(k_delta_export, dim3(2048), dim3(256), 0, m->stream, m->d_syn0, m->d_snap, d_buf, tab);
        hipLaunchKernelGGL(k_delta_export, dim3(2048), dim3(256), 0, m->stream, m->d_syn1neg, m->d_snap + tab, d_buf + tab, tab);
        if (m->d_syn1) hipLaunchKernelGGL(k_delta_export, dim3(2048), dim3(256), 0, m->stream, m->d_syn1, m->d_snap + 2 * tab, d_buf + 2 * tab, tab);
    }
    DGE_HIP(hipStreamSynchronize(m->stream));
    DGE_HIP(hipGetLastError());
    return DGE_OK;
}

extern "C" int dge_model_import_delta(dge_model* m, const float* d_buf, float scale) {
    if (!m || !d_buf) DGE_FAIL(DGE_ERR_ARG, "dge_model_import_delta: null argument");
    if (!m->d_snap) DGE_FAIL(DGE_ERR_STATE, "dge_model_import_delta: no snapshot");
    DGE_HIP(hipSetDevice(m->device));
    DGE_HIP(hipDeviceSynchronize());      // d_buf comes from the caller's collective, on the caller's stream
    int64_t tab = m->V * (int64_t)m->stride;
    if (tab) {
        hipLaunchKernelGGL(k_delta_import, dim3(2048), dim3(256), 0, m->stream, m->d_syn0, m->d_snap, d_buf, scale, tab);
        hipLaunchKernelGGL(k_delta_import, dim3(2048), dim3(256), 0, m->stream, m->d_syn1neg, m->d_snap + tab, d_buf + tab, scale, tab);
        if (m->d_syn1) hipLaunchKernelGGL(k_delta_import, dim3(2048), dim3(256), 0, m->stream, m->d_syn1, m->d_snap + 2 * tab, d_buf + 2 * tab, scale, tab);
    }
    DGE_HIP(hipStreamSynchronize(m->stream));
    DGE_HIP(hipGetLastError());
    return DGE_OK;
}

// ------------------------------------------------------------------------------------------ native RCCL exchange
// For hosts without torch.distributed (the Java/JNI form): the same delta exchange with RCCL called directly.  librccl
// is dlopen()ed on first use, so a process that already carries a RCCL (PyTorch bundles one) is never handed a second
// copy at load time.
static_assert(sizeof(dge_unique_id) == sizeof(ncclUniqueId), "include/dge.h: dge_unique_id must be the size of ncclUniqueId");
struct dge_comm {
    ncclComm_t nccl = nullptr;
    int rank = 0, nranks = 1, device = 0;
    float* d_buf = nullptr; int64_t buf_floats = 0;
};
namespace {
// the entry points are looked up with dlsym at first use; their prototypes are the header's own (decltype), so a change of rccl.h shows at compile time
struct RcclApi {
    void* lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
};
RcclApi g_rccl;
int rccl_load() {
    if (g_rccl.lib) return DGE_OK;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    for (const char* n : names) { h = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (h) break; }
    if (!h) DGE_FAIL(DGE_ERR_DEVICE, "cannot load librccl: %s", dlerror());
    g_rccl.GetUniqueId = (decltype(&ncclGetUniqueId))dlsym(h, "ncclGetUniqueId");
    g_rccl.CommInitRank = (decltype(&ncclCommInitRank))dlsym(h, "ncclCommInitRank");
    g_rccl.AllReduce = (decltype(&ncclAllReduce))dlsym(h, "ncclAllReduce");
    g_rccl.AllGather = (decltype(&ncclAllGather))dlsym(h, "ncclAllGather");
    g_rccl.Send = (decltype(&ncclSend))dlsym(h, "ncclSend");
    g_rccl.Recv = (decltype(&ncclRecv))dlsym(h, "ncclRecv");
    g_rccl.GroupStart = (decltype(&ncclGroupStart))dlsym(h, "ncclGroupStart");
    g_rccl.GroupEnd = (decltype(&ncclGroupEnd))dlsym(h, "ncclGroupEnd");
    g_rccl.CommDestroy = (decltype(&ncclCommDestroy))dlsym(h, "ncclCommDestroy");
    g_rccl.GetErrorString = (decltype(&ncclGetErrorString))dlsym(h, "ncclGetErrorString");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce || !g_rccl.AllGather || !g_rccl.CommDestroy || !g_rccl.Send || !g_rccl.Recv ||
        !g_rccl.GroupStart || !g_rccl.GroupEnd) DGE_FAIL(DGE_ERR_DEVICE, "librccl lacks an expected symbol");
    g_rccl.lib = h;
    return DGE_OK;
}
int rccl_fail(int rc, const char* what) {
    DGE_FAIL(DGE_ERR_DEVICE, "RCCL %s failed: %s", what, g_rccl.GetErrorString ? g_rccl.GetErrorString((ncclResult_t)rc) : "?");
}
}  // namespace

extern "C" int dge_comm_unique_id(dge_unique_id* out) {
    if (!out) DGE_FAIL(DGE_ERR_ARG, "dge_comm_unique_id: null output");
    int rc = rccl_load();
    if (rc) return rc;
    int n = g_rccl.GetUniqueId(reinterpret_cast<ncclUniqueId*>(out));
    return n ? rccl_fail(n, "ncclGetUniqueId") : DGE_OK;
}

extern "C" int dge_comm_create(dge_comm** out, const dge_unique_id* id, int rank, int nranks, int device) {
    if (!out || !id || nranks <= 0 || rank < 0 || rank >= nranks) DGE_FAIL(DGE_ERR_ARG, "dge_comm_create: bad argument");
    *out = nullptr;
    int rc = dge_require_device(device);
    if (rc) return rc;
    if ((rc = rccl_load())) return rc;
    dge_comm* c = new dge_comm();
    c->rank = rank; c->nranks = nranks; c->device = device;
    ncclUniqueId nid; memcpy(&nid, id, sizeof(nid));
    int n = g_rccl.CommInitRank(&c->nccl, nranks, nid, rank);
    if (n) { delete c; return rccl_fail(n, "ncclCommInitRank"); }
    *out = c;
    return DGE_OK;
}

extern "C" void dge_comm_free(dge_comm* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->nccl && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->nccl);
    dge_dev_free(c->d_buf);
    delete c;
}

// delta = tables - snapshot; all-reduce(sum) over the communicator; tables = snapshot + delta_sum / nranks; re-snapshot
extern "C" int dge_model_allreduce_deltas(dge_model* m, dge_comm* c) {
    if (!m || !c) DGE_FAIL(DGE_ERR_ARG, "dge_model_allreduce_deltas: null argument");
    if (c->device != m->device) DGE_FAIL(DGE_ERR_ARG, "dge_model_allreduce_deltas: communicator and model live on different devices");
    DGE_HIP(hipSetDevice(m->device));
    int64_t nfl = 0;
    int rc = dge_model_sync_size(m, &nfl);
    if (rc) return rc;
    if (c->buf_floats < nfl) { dge_dev_free(c->d_buf); c->d_buf = nullptr; if ((rc = dge_dev_alloc(&c->d_buf, (size_t)nfl + 64))) return rc; c->buf_floats = nfl; }
    if ((rc = dge_model_export_delta(m, c->d_buf))) return rc;
    int n = g_rccl.AllReduce(c->d_buf, c->d_buf, (size_t)nfl, ncclFloat32, ncclSum, c->nccl, m->stream);
    if (n) return rccl_fail(n, "ncclAllReduce");
    DGE_HIP(hipStreamSynchronize(m->stream));
    return dge_model_import_delta(m, c->d_buf, 1.0f / (float)c->nranks);
}

// block schedule with RCCL called from the library.  dge_model_ring_pass: after episode `episode` rank g hands the syn1neg partition
// it just trained, (g + episode) % N, to rank g-1 and takes partition (g + 1 + episode) % N — the one it trains next — from rank
// g+1 (ncclSend/ncclRecv in one group).  dge_model_gather_table: every rank publishes partition `rank` of `table` and takes the
// others (all-gather): the end of training, or a checkpoint.
static int comm_buffers(dge_model* m, dge_comm* c, int64_t need) {
    if (c->buf_floats >= need) return DGE_OK;
    dge_dev_free(c->d_buf); c->d_buf = nullptr; c->buf_floats = 0;
    int rc = dge_dev_alloc(&c->d_buf, (size_t)need + 64);
    if (rc) return rc;
    c->buf_floats = need;
    return DGE_OK;
}

extern "C" int dge_model_ring_pass(dge_model* m, dge_comm* c, int32_t episode) {
    if (!m || !c || episode < 0) DGE_FAIL(DGE_ERR_ARG, "dge_model_ring_pass: bad argument");
    if (c->device != m->device) DGE_FAIL(DGE_ERR_ARG, "dge_model_ring_pass: communicator and model live on different devices");
    if (c->nranks == 1) return DGE_OK;
    DGE_HIP(hipSetDevice(m->device));
    int64_t pf = 0;
    int rc = dge_model_partition_floats(m, c->nranks, &pf);
    if (rc) return rc;
    const int n_tab = m->d_syn1 ? 2 : 1;                   // with the hierarchical softmax the syn1 partition of the same number travels along
    if ((rc = comm_buffers(m, c, 2 * pf * n_tab))) return rc;
    float* mine = c->d_buf; float* next = c->d_buf + pf * n_tab;
    // everything below is enqueued on the model's stream — pack, ncclSend / ncclRecv, unpack — and the host never waits: the next episode's launches queue up behind
    for (int t = 0; t < n_tab; t++)
        if ((rc = partition_copy(m, 1 + t, c->nranks, (c->rank + episode) % c->nranks, mine + t * pf, true, m->stream))) return rc;
    const int dst = (c->rank + c->nranks - 1) % c->nranks, src = (c->rank + 1) % c->nranks;
    int n = g_rccl.GroupStart();
    if (!n) n = g_rccl.Send(mine, (size_t)(pf * n_tab), ncclFloat32, dst, c->nccl, m->stream);
    if (!n) n = g_rccl.Recv(next, (size_t)(pf * n_tab), ncclFloat32, src, c->nccl, m->stream);
    const int n2 = g_rccl.GroupEnd();
    if (n || n2) return rccl_fail(n ? n : n2, "ncclSend/ncclRecv");
    for (int t = 0; t < n_tab; t++)
        if ((rc = partition_copy(m, 1 + t, c->nranks, (c->rank + 1 + episode) % c->nranks, next + t * pf, false, m->stream))) return rc;
    return DGE_OK;
}

extern "C" int dge_model_gather_table(dge_model* m, dge_comm* c, int table) {
    if (!m || !c || table < 0 || table > 2 || (table == 2 && !m->d_syn1)) DGE_FAIL(DGE_ERR_ARG, "dge_model_gather_table: bad argument");
    if (c->device != m->device) DGE_FAIL(DGE_ERR_ARG, "dge_model_gather_table: communicator and model live on different devices");
    DGE_HIP(hipSetDevice(m->device));
    int64_t pf = 0;
    int rc = dge_model_partition_floats(m, c->nranks, &pf);
    if (rc) return rc;
    if ((rc = comm_buffers(m, c, pf * ((int64_t)c->nranks + 1)))) return rc;
    float* mine = c->d_buf; float* all = c->d_buf + pf;
    if ((rc = partition_copy(m, table, c->nranks, c->rank, mine, true, m->stream))) return rc;
    int n = g_rccl.AllGather(mine, all, (size_t)pf, ncclFloat32, c->nccl, m->stream);
    if (n) return rccl_fail(n, "ncclAllGather");
    for (int r = 0; r < c->nranks; r++)
        if (r != c->rank && (rc = partition_copy(m, table, c->nranks, r, all + (int64_t)r * pf, false, m->stream))) return rc;
    DGE_HIP(hipStreamSynchronize(m->stream));              // (end of training: the caller reads the tables next)
    return DGE_OK;
}
