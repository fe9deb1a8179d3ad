// coo_entries.h — the intake of sparse entries (a, b, value) that nmf.hip and line.hip share: every entry is checked, the zeros are dropped, the kept entries are
// sorted by (a, b) and no (a, b) may come twice.  A module gives the two ranges, a classifier of values and says whether it wants the greatest kept value; it
// words the messages itself.  Outside the build stamp, like its two readers.
#pragma once
#include <string.h>

#include "dge_device.h"

#define COO_NONE (~0ULL)
// the counters of the scan (COO_SPARE: a word of all ones that the intake leaves to the module); as a fault: COO_ZEROS = nothing is left after the zeros,
// COO_MANY = more kept entries than the module takes
enum { COO_RANGE = 0, COO_KIND1, COO_KIND2, COO_DUP, COO_ZEROS, COO_VMAX, COO_SPARE, COO_N, COO_KEEP = COO_N, COO_MANY };

// every input entry: its checks (the least input index of each kind of fault), the zeros, with VMAX the greatest kept value (the bits of non-negative doubles
// order as unsigned integers), and its sort key a * nb + b — a dropped entry sorts behind all kept ones.
// Classify::kind(v) is COO_KEEP, COO_ZEROS, COO_KIND1 or COO_KIND2.
template <typename Classify, bool VMAX>
__global__ void __launch_bounds__(256) k_coo_scan(const int32_t* __restrict__ a, const int32_t* __restrict__ b, const double* __restrict__ val, int64_t ne, int64_t na, int64_t nb,
                                                  uint64_t* __restrict__ key, int64_t* __restrict__ idx, unsigned long long* __restrict__ c) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ne) return;
    const double v = val[e];
    const int64_t i = a[e], j = b[e];
    uint64_t k = COO_NONE;
    if (i < 0 || i >= na || j < 0 || j >= nb) atomicMin(c + COO_RANGE, (unsigned long long)e);
    else {
        const int kind = Classify::kind(v);
        if (kind == COO_KIND1 || kind == COO_KIND2) atomicMin(c + kind, (unsigned long long)e);
        else if (kind == COO_ZEROS) atomicAdd(c + COO_ZEROS, 1ULL);
        else {
            k = (uint64_t)i * (uint64_t)nb + (uint64_t)j;
            if (VMAX) atomicMax(c + COO_VMAX, (unsigned long long)__double_as_longlong(v));
        }
    }
    key[e] = k;
    idx[e] = e;
}

// the sort is stable: among equal keys the input indices ascend, so every entry that equals the one in front of it is a second occurrence
// (a template only so that the header may be included where the kernel is not launched)
template <typename I>
__global__ void __launch_bounds__(256) k_coo_dups(const uint64_t* __restrict__ key, const I* __restrict__ idx, int64_t kept, unsigned long long* __restrict__ c) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < 1 || p >= kept) return;
    if (key[p] == key[p - 1]) atomicMin(c + COO_DUP, (unsigned long long)idx[p]);
}

// the first of the n ascending keys that is at least `want` (n: none is)
template <typename K>
__device__ __forceinline__ int64_t coo_lower_bound(const K* __restrict__ key, int64_t n, K want) {
    int64_t lo = 0, hi = n;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (key[mid] < want) lo = mid + 1; else hi = mid; }
    return lo;
}

struct coo_entries {
    dge_tmp<uint64_t> skey, key;        // skey [ne]: the keys ascending, the kept entries, then the dropped ones
    dge_tmp<int64_t> sidx, idx;         // sidx [ne]: the input index of each
    dge_tmp<unsigned long long> d_c;    // the counters.  They and the unsorted key, idx stay until the call ends: a free inside it would wait for the device
    int64_t kept = 0, zeros = 0;
    double vmax = 0.0;
    int fault = COO_KEEP;               // COO_KEEP: none; else the kind, and for a kind that names an entry its input index
    int64_t at = 0;
};

// the intake of ne >= 1 device entries.  The faults in the order they are looked for: out of range, value kind 1, value kind 2, nothing left, more than max_kept,
// (the sort,) a repeat; within a kind the least input index.  A fault returns DGE_OK with E.fault set: the caller words it.
template <typename Classify, bool VMAX>
int coo_intake(const int32_t* d_a, const int32_t* d_b, const double* d_val, int64_t ne, int64_t na, int64_t nb, int64_t max_kept, coo_entries& E) {
    int rc;
    if ((rc = E.d_c.alloc(COO_N)) || (rc = E.key.alloc((size_t)ne)) || (rc = E.skey.alloc((size_t)ne)) || (rc = E.idx.alloc((size_t)ne)) || (rc = E.sidx.alloc((size_t)ne))) return rc;
    unsigned long long* d_c = E.d_c.p;
    unsigned long long c[COO_N] = {COO_NONE, COO_NONE, COO_NONE, COO_NONE, 0, 0, COO_NONE};
    DGE_HIP(hipMemcpy(d_c, c, sizeof c, hipMemcpyHostToDevice));
    hipLaunchKernelGGL((k_coo_scan<Classify, VMAX>), dim3(dge_grid(ne)), dim3(256), 0, 0, d_a, d_b, d_val, ne, na, nb, E.key.p, E.idx.p, d_c);
    DGE_HIP(hipGetLastError());
    DGE_HIP(hipMemcpy(c, d_c, sizeof c, hipMemcpyDeviceToHost));
    for (int kind : {COO_RANGE, COO_KIND1, COO_KIND2})
        if (c[kind] != COO_NONE) { E.fault = kind; E.at = (int64_t)c[kind]; return DGE_OK; }
    E.zeros = (int64_t)c[COO_ZEROS]; E.kept = ne - E.zeros;
    memcpy(&E.vmax, &c[COO_VMAX], sizeof E.vmax);
    if (E.kept < 1) { E.fault = COO_ZEROS; return DGE_OK; }
    if (E.kept > max_kept) { E.fault = COO_MANY; return DGE_OK; }
    if ((rc = dge_sort_pairs(dge_scratch(), (const uint64_t*)E.key.p, E.skey.p, (const int64_t*)E.idx.p, E.sidx.p, ne, 64, 0, true))) return rc;
    hipLaunchKernelGGL(k_coo_dups<int64_t>, dim3(dge_grid(E.kept)), dim3(256), 0, 0, E.skey.p, E.sidx.p, E.kept, d_c);
    DGE_HIP(hipGetLastError());
    DGE_HIP(hipMemcpy(c, d_c, sizeof c, hipMemcpyDeviceToHost));
    if (c[COO_DUP] != COO_NONE) { E.fault = COO_DUP; E.at = (int64_t)c[COO_DUP]; }
    return DGE_OK;
}

// the caller's three host arrays of ne entries onto the device
static inline int coo_upload(const int32_t* a, const int32_t* b, const double* val, int64_t ne, dge_tmp<int32_t>& d_a, dge_tmp<int32_t>& d_b, dge_tmp<double>& d_val) {
    int rc;
    if ((rc = d_a.alloc((size_t)ne)) || (rc = d_b.alloc((size_t)ne)) || (rc = d_val.alloc((size_t)ne))) return rc;
    DGE_HIP(hipMemcpy(d_a.p, a, (size_t)ne * sizeof(int32_t), hipMemcpyHostToDevice));
    DGE_HIP(hipMemcpy(d_b.p, b, (size_t)ne * sizeof(int32_t), hipMemcpyHostToDevice));
    DGE_HIP(hipMemcpy(d_val.p, val, (size_t)ne * sizeof(double), hipMemcpyHostToDevice));
    return DGE_OK;
}
