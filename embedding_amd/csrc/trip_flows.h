// trip_flows.h — the resident flow table and the passes over it that trip_map.hip (trips in, slots out), flow_windows.hip (entries in, hour windows and
// triplets out) and matrix_read.hip (.matrix text in) share: the table's layout, the counters' block reduction, sort / reduce-by-key under a run's accounting,
// the join of a table with more (key, count) pairs, the commit of such pairs into a table (trip_commit_entries: what dge_flows_add_entries ends with), and
// the decode of sorted (slice, rank, rank) keys into the arrays od_commit.h takes.  Everything is static, as in od_commit.h: each
// translation unit gets its own copy and the library exports nothing from here.  Outside the build stamp.
#pragma once
#include <algorithm>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/iterator/constant_iterator.hpp>

#include "coo_entries.h"
#include "od_commit.h"

enum { TC_LOCATED = 0, TC_BOUNDARY, TC_MULTI, TC_OUTSIDE, TC_EXACT, TC_MAPPED, TC_BAD, TC_NO_START, TC_NO_END, TC_VALID, TC_N };

struct dge_flows {
    dge_regions* regions = nullptr;
    uint64_t* d_key = nullptr;                   // ascending: (hour * R + s) * R + e
    int64_t* d_cnt = nullptr;
    int64_t n = 0;
    struct dge_flows_info info = {};
};

template <int N>
__device__ __forceinline__ void trip_count(unsigned long long (&v)[N], const int (&which)[N], unsigned long long* counters) {
    typedef hipcub::BlockReduce<unsigned long long, SEQ_BLOCK> Reduce;
    __shared__ typename Reduce::TempStorage tmp;
    for (int k = 0; k < N; k++) {
        const unsigned long long sum = Reduce(tmp).Sum(v[k]);
        if (threadIdx.x == 0 && sum) atomicAdd(counters + which[k], sum);
        __syncthreads();
    }
}

static __global__ void __launch_bounds__(SEQ_BLOCK) k_slot_decode(const uint64_t* key, const int64_t* w, int64_t n, uint64_t R, const int64_t* id_by_rank, int32_t* slot, int64_t* src_id,
                                                                  int64_t* dst_id, uint64_t* w_bits, int64_t* iota) {
    const int64_t i = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (i == 0) iota[n] = n;
    if (i >= n) return;
    const uint64_t k = key[i];
    slot[i] = (int32_t)(k / R / R);
    src_id[i] = id_by_rank[(k / R) % R];
    dst_id[i] = id_by_rank[k % R];
    w_bits[i] = (uint64_t)__double_as_longlong((double)w[i]);     // round to nearest even: the binary64 nearest the decimal, as the .od reader gives
    iota[i] = i;
}

// is any count above the limit?
static __global__ void __launch_bounds__(SEQ_BLOCK) k_win_over(const int64_t* cnt, int64_t n, int64_t limit, unsigned long long* over) {
    const int64_t i = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    unsigned long long v[1] = {i < n && cnt[i] > limit ? 1ull : 0ull};
    const int which[1] = {0};
    trip_count(v, which, over);
}

namespace {

// keys ascending with duplicates, vals: -> distinct keys with summed values.  vals == nullptr: every value is 1.  The outputs are allocated here.
int trip_reduce(SeqRun& R, const uint64_t* keys, const int64_t* vals, int64_t n, dge_tmp<uint64_t>& ukey, dge_tmp<int64_t>& usum, int64_t* n_out) {
    *n_out = 0;
    SEQ_TRY(seq_alloc(R, ukey, n, "the distinct keys"));
    SEQ_TRY(seq_alloc(R, usum, n, "the summed counts"));
    if (n == 0) return DGE_OK;
    dge_tmp<int64_t> count;
    SEQ_TRY(seq_alloc(R, count, 1, "the number of keys"));
    SeqScratch tmp{R, "the reduction's scratch", true};
    auto reduce = [&](auto values) {
        return dge_two_pass(tmp, [&](void* t, size_t& bytes) {
            return rocprim::reduce_by_key(t, bytes, keys, values, (size_t)n, ukey.p, usum.p, count.p, rocprim::plus<int64_t>(), rocprim::equal_to<uint64_t>(), R.stream);
        }, R.stream, false);
    };
    SEQ_TRY(vals ? reduce(vals) : reduce(rocprim::constant_iterator<int64_t>(1)));
    SEQ_TRY(seq_kernels_end(R));
    return seq_read_back(R, n_out, count.p, 8);
}

int trip_sort_pairs(SeqRun& R, const uint64_t* k_in, uint64_t* k_out, const int64_t* v_in, int64_t* v_out, int64_t n, int end_bit) {
    if (n == 0) return DGE_OK;
    SeqScratch tmp{R, "the sort's scratch", true};
    SEQ_TRY(v_in ? dge_sort_pairs(tmp, k_in, k_out, v_in, v_out, n, end_bit, R.stream, false) : dge_sort_keys(tmp, k_in, k_out, n, end_bit, R.stream, false));
    return seq_kernels_end(R);
}

// The tables are sorted sets of (key, count): a table of tn entries and u more pairs (device arrays, u >= 1), concatenated, sorted and reduced by key, are the
// table the trips of both give in any order of adding.  Ru: the regions, 1 at least.  When this returns the stream has drained.
int trip_join(SeqRun& R, const uint64_t* old_key, const int64_t* old_cnt, int64_t tn, const uint64_t* add_key, const int64_t* add_cnt, int64_t u, uint64_t Ru, dge_tmp<uint64_t>& nkey,
              dge_tmp<int64_t>& ncnt, int64_t* nn) {
    dge_tmp<uint64_t> ckey, cskey;
    dge_tmp<int64_t> ccnt, cscnt;
    SEQ_TRY(seq_alloc(R, ckey, tn + u, "the joined tables"));
    SEQ_TRY(seq_alloc(R, ccnt, tn + u, "the joined tables' counts"));
    SEQ_TRY(seq_alloc(R, cskey, tn + u, "the joined tables, sorted"));
    SEQ_TRY(seq_alloc(R, cscnt, tn + u, "the joined tables' counts, sorted"));
    if (tn) {
        DGE_HIP(hipMemcpyAsync(ckey.p, old_key, (size_t)tn * 8, hipMemcpyDeviceToDevice, R.stream));
        DGE_HIP(hipMemcpyAsync(ccnt.p, old_cnt, (size_t)tn * 8, hipMemcpyDeviceToDevice, R.stream));
    }
    DGE_HIP(hipMemcpyAsync(ckey.p + tn, add_key, (size_t)u * 8, hipMemcpyDeviceToDevice, R.stream));
    DGE_HIP(hipMemcpyAsync(ccnt.p + tn, add_cnt, (size_t)u * 8, hipMemcpyDeviceToDevice, R.stream));
    SEQ_TRY(trip_sort_pairs(R, ckey.p, cskey.p, ccnt.p, cscnt.p, tn + u, dge_bits(24 * Ru * Ru)));
    SEQ_TRY(trip_reduce(R, cskey.p, cscnt.p, tn + u, nkey, ncnt, nn));
    DGE_HIP(hipStreamSynchronize(R.stream));
    return DGE_OK;
}

// u >= 1 checked (key, count) pairs on the device into f, under one commit: the join, the test of every key's total against limit, the swap and the counters.
// added: the sum of the counts.  On any error f is as it was.  dge_flows_add_entries (flow_windows.hip) and the .matrix reader (matrix_read.hip) end here.
[[maybe_unused]] int trip_commit_entries(SeqRun& R, dge_flows* f, const uint64_t* add_key, const int64_t* add_cnt, int64_t u, int64_t added, int64_t limit, const char* who) {
    const uint64_t Ru = (uint64_t)std::max<int64_t>(f->regions->R, 1);
    dge_tmp<uint64_t> nkey;
    dge_tmp<int64_t> ncnt;
    dge_tmp<unsigned long long> over_at;
    int64_t nn = 0;
    SEQ_TRY(seq_alloc(R, over_at, 1, "the counters"));
    DGE_HIP(hipMemsetAsync(over_at.p, 0, 8, R.stream));
    SEQ_TRY(trip_join(R, f->d_key, f->d_cnt, f->n, add_key, add_cnt, u, Ru, nkey, ncnt, &nn));
    SEQ_TRY(seq_kernels_begin(R));
    hipLaunchKernelGGL(k_win_over, dim3(seq_grid(nn)), dim3(SEQ_BLOCK), 0, R.stream, ncnt.p, nn, limit, over_at.p);
    SEQ_TRY(seq_kernels_end(R));
    unsigned long long over = 0;
    SEQ_TRY(seq_read_back(R, &over, over_at.p, 8));
    DGE_HIP(hipGetLastError());
    if (over) DGE_FAIL(DGE_ERR_RANGE, "%s: %llu keys would hold a total above 2^40", who, over);
    // nothing can fail from here on
    dge_dev_free(f->d_key); dge_dev_free(f->d_cnt);
    f->d_key = nkey.release(); f->d_cnt = ncnt.release(); f->n = nn;
    f->info.trips += added; f->info.mapped += added; f->info.entries = nn; f->info.kernel_ms += R.kernel_ms;
    return DGE_OK;
}

struct SlotArrays { dge_tmp<int32_t> slot; dge_tmp<int64_t> src_id, dst_id, iota; dge_tmp<uint64_t> w_bits; };

// sorted keys (slice, rank of src id, rank of dst id) with their weights -> the arrays od_commit takes and the caller's read-back gives
[[maybe_unused]] int trip_slot_decode(SeqRun& R, const dge_flows* f, const uint64_t* okey, const int64_t* ow, int64_t n, SlotArrays& A) {
    SEQ_TRY(seq_alloc(R, A.slot, n, "the edges' slots"));
    SEQ_TRY(seq_alloc(R, A.src_id, n, "the edges' sources"));
    SEQ_TRY(seq_alloc(R, A.dst_id, n, "the edges' destinations"));
    SEQ_TRY(seq_alloc(R, A.w_bits, n, "the edges' weights"));
    SEQ_TRY(seq_alloc(R, A.iota, n + 1, "the edges' numbers"));
    SEQ_TRY(seq_kernels_begin(R));
    hipLaunchKernelGGL(k_slot_decode, dim3(seq_grid(n + 1)), dim3(SEQ_BLOCK), 0, R.stream, okey, ow, n, (uint64_t)std::max<int64_t>(f->regions->R, 1), f->regions->d_id_by_rank, A.slot.p, A.src_id.p,
                       A.dst_id.p, A.w_bits.p, A.iota.p);
    return seq_kernels_end(R);
}

}  // namespace
