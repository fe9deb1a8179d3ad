// text_out_pump.h — how a text that was sized and is spelled on the device leaves it: the host half shared by the .seq writer (seq_write.hip) and the flow-table
// text writer (flow_text.hip).  The text leaves in slabs of SEQ_OUT_SLAB output bytes (seq_out_plan.h).  The device holds two slab buffers, the host two pinned
// ones; slab s + 1 is formatted while slab s is copied out and slab s - 1 goes to write() or to the caller's memory.  Nothing is staged through pageable memory.
// Everything is static, as in od_commit.h: each translation unit gets its own copy and the library exports nothing from here.  Outside the build stamp.
#pragma once
#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <unistd.h>

#include "dge_device.h"
#include "seq_out_plan.h"

namespace {

#define TXO_TRY(expr) do { int rc__ = (expr); if (rc__) return rc__; } while (0)

// where the text goes: the caller's memory or a file
struct TextSink {
    const char* who;
    char* text = nullptr; int64_t cap = 0;       // text leg
    const char* path = nullptr; int append = 0;  // file leg
    int fd = -1;
    int64_t at = 0;
    ~TextSink() { if (fd >= 0) close(fd); }
    // *done = 1: nothing more to do (a size query)
    int begin(int64_t total, int64_t* n_bytes, int* done) {
        *done = 0;
        if (n_bytes) *n_bytes = total;
        if (path) {
            fd = open(path, O_WRONLY | O_CREAT | O_CLOEXEC | (append ? O_APPEND : O_TRUNC), 0666);
            if (fd < 0) DGE_FAIL(DGE_ERR_IO, "%s: cannot open %s: %s", who, path, strerror(errno));
            return DGE_OK;
        }
        if (!text) { *done = 1; return DGE_OK; }                  // cap == 0: a size query
        if (total > cap) DGE_FAIL(DGE_ERR_CAP, "%s: text holds %lld of %lld bytes", who, (long long)cap, (long long)total);
        return DGE_OK;
    }
    int put(const uint8_t* p, int64_t n) {
        if (!path) { memcpy(text + at, p, (size_t)n); at += n; return DGE_OK; }
        for (int64_t done = 0; done < n;) {
            const ssize_t r = write(fd, p + done, (size_t)(n - done));
            if (r < 0 && errno == EINTR) continue;
            if (r <= 0) DGE_FAIL(DGE_ERR_IO, "%s: cannot write %s: %s after %lld bytes", who, path, r < 0 ? strerror(errno) : "nothing was taken", (long long)(at + done));
            done += (int64_t)r;
        }
        at += n;
        return DGE_OK;
    }
    int end() {
        if (fd >= 0) {
            const int rc = close(fd);
            fd = -1;
            if (rc != 0) DGE_FAIL(DGE_ERR_IO, "%s: cannot close %s: %s", who, path, strerror(errno));
        }
        return DGE_OK;
    }
};

// the two streams, the events and the four slab buffers of one call; a call that writes several texts runs them through one pump
struct TextPump {
    hipStream_t ks = nullptr, cs = nullptr;                       // kernels; copies to the host
    hipEvent_t ka[2] = {nullptr, nullptr}, kb[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
    uint8_t* pin[2] = {nullptr, nullptr};
    dge_tmp<uint8_t> text;                                        // the two device slab buffers, back to back
    int64_t buf = 0;                                              // bytes of one of them
    double kernel_ms = 0;
    bool drained = false;                                         // nothing was queued since the last drain(): the host waits are counted, none is made twice
    TextPump() = default;
    TextPump(const TextPump&) = delete;
    TextPump& operator=(const TextPump&) = delete;
    void drain() {
        if (cs) (void)hipStreamSynchronize(cs);
        if (ks) (void)hipStreamSynchronize(ks);
        drained = true;
    }
    ~TextPump() {
        if (!drained) drain();
        for (int i = 0; i < 2; i++) {
            if (pin[i]) (void)hipHostFree(pin[i]);
            if (ka[i]) (void)hipEventDestroy(ka[i]);
            if (kb[i]) (void)hipEventDestroy(kb[i]);
            if (copied[i]) (void)hipEventDestroy(copied[i]);
        }
        if (cs) (void)hipStreamDestroy(cs);
        if (ks) (void)hipStreamDestroy(ks);
    }
    int open() {
        DGE_HIP(hipStreamCreateWithFlags(&ks, hipStreamNonBlocking));
        DGE_HIP(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
        for (int i = 0; i < 2; i++) {
            DGE_HIP(hipEventCreate(&ka[i]));
            DGE_HIP(hipEventCreate(&kb[i]));
            DGE_HIP(hipEventCreateWithFlags(&copied[i], hipEventDisableTiming));
        }
        return DGE_OK;
    }
    // the event time between ka[b] and kb[b], both reached, into kernel_ms
    int add_kernel_ms(int b) {
        float ms = 0.f;
        DGE_HIP(hipEventElapsedTime(&ms, ka[b], kb[b]));
        kernel_ms += ms;
        return DGE_OK;
    }
    // the buffers a text of `total` > 0 bytes needs; they only grow.  cap_who: out of device memory is that caller's DGE_ERR_CAP (null: a device error)
    int reserve(int64_t total, const char* cap_who) {
        const int64_t want = seq_out_buffer_bytes(total);
        const int pins = seq_out_slab_count(total) < 2 ? 1 : 2;
        if (want > buf) {
            if (buf) drain();                                     // (a first allocation has no tenant to wait for)
            for (int i = 0; i < 2; i++) if (pin[i]) { (void)hipHostFree(pin[i]); pin[i] = nullptr; }
            buf = 0;
            TXO_TRY(cap_who ? dge_alloc_for(text, (size_t)(2 * want), cap_who) : text.alloc((size_t)(2 * want)));
            buf = want;
        }
        for (int i = 0; i < pins; i++) if (!pin[i]) DGE_HIP(hipHostMalloc((void**)&pin[i], (size_t)buf, hipHostMallocDefault));
        return DGE_OK;
    }
    // the slab loop.  emit(s0, s1, out) queues on ks what spells bytes [s0, s1) of the text into out (out[0] is byte s0; s0 is a multiple of the tile)
    template <typename Emit>
    int run(int64_t total, TextSink& sink, const char* cap_who, Emit&& emit) {
        const int64_t S = seq_out_slab_count(total);
        if (S == 0) return DGE_OK;
        TXO_TRY(reserve(total, cap_who));
        drained = false;
        for (int64_t i = 0; i <= S; i++) {
            if (i < S) {
                const int b = (int)(i & 1);
                const int64_t s0 = seq_out_slab_begin(i), s1 = seq_out_slab_end(total, i);
                if (i >= 2) DGE_HIP(hipStreamWaitEvent(ks, copied[b], 0));            // the device buffer's last tenant has left
                DGE_HIP(hipEventRecord(ka[b], ks));
                TXO_TRY(emit(s0, s1, text.p + (int64_t)b * buf));
                DGE_HIP(hipGetLastError());
                DGE_HIP(hipEventRecord(kb[b], ks));
                DGE_HIP(hipStreamWaitEvent(cs, kb[b], 0));
                DGE_HIP(hipMemcpyAsync(pin[b], text.p + (int64_t)b * buf, (size_t)(s1 - s0), hipMemcpyDeviceToHost, cs));      // (the host is done with pin[b]: slab i - 2 went out below)
                DGE_HIP(hipEventRecord(copied[b], cs));
            }
            if (i >= 1) {
                const int p = (int)((i - 1) & 1);
                DGE_HIP(hipEventSynchronize(copied[p]));
                TXO_TRY(add_kernel_ms(p));
                TXO_TRY(sink.put(pin[p], seq_out_slab_end(total, i - 1) - seq_out_slab_begin(i - 1)));
            }
        }
        return DGE_OK;
    }
};

}  // namespace
