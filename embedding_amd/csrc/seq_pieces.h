// seq_pieces.h — the host side of the text readers' intake, free of HIP so that tests/native/seq_pieces_harness.cpp builds it with g++: the caller's files and
// texts as PIECES, the one step that reads a piece's next bytes, and the two producers on top of it — the joiner of seq_tokens.h's one buffer (.seq, .vec,
// .od) and the slab feeder of trip_text.hip.  This is all the code of the readers that deals with the file system, short reads and the "\r" / "\n" cut across
// slab boundaries.  Everything is static; nothing here touches a device.
#pragma once
#include <errno.h>
#include <fcntl.h>
#include <stdint.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/dge.h"
#include "seq_plan.h"
#include "trip_parse.h"

#ifndef DGE_FAIL      // dge_internal.h, or a host harness with a dge_set_error of its own, may stand in front
void dge_set_error(const char* fmt, ...);
#define DGE_FAIL(code, ...) do { dge_set_error(__VA_ARGS__); return (code); } while (0)
#endif

namespace {

// a file (path, fd) or a text of the caller's (mem); size bytes either way
struct SeqPiece { const char* path = nullptr; const uint8_t* mem = nullptr; int fd = -1; int64_t size = 0; };

inline void seq_close_pieces(std::vector<SeqPiece>& pieces) {
    for (SeqPiece& p : pieces) if (p.fd >= 0) { close(p.fd); p.fd = -1; }
}

// The checks stand apart from the appending because an entry refuses a bad text or path among its argument checks, before it looks for a device.
inline int seq_check_texts(const char* const* texts, const int64_t* n_bytes, int32_t n, const char* who) {
    for (int32_t k = 0; k < n; k++)
        if (n_bytes[k] < 0 || (n_bytes[k] > 0 && !texts[k])) DGE_FAIL(DGE_ERR_ARG, "%s: text %d is null or of negative size", who, k);
    return DGE_OK;
}
inline int seq_check_paths(const char* const* paths, int32_t n, const char* who) {
    for (int32_t k = 0; k < n; k++) if (!paths[k]) DGE_FAIL(DGE_ERR_ARG, "%s: path %d is null", who, k);
    return DGE_OK;
}

inline int seq_add_texts(std::vector<SeqPiece>& pieces, const char* const* texts, const int64_t* n_bytes, int32_t n, const char* who) {
    if (int rc = seq_check_texts(texts, n_bytes, n, who)) return rc;
    for (int32_t k = 0; k < n; k++) {
        SeqPiece p; p.mem = reinterpret_cast<const uint8_t*>(texts[k]); p.size = n_bytes[k];
        pieces.push_back(p);
    }
    return DGE_OK;
}

// every file is opened before anything runs; whoever owns the vector closes them (seq_close_pieces), after a failure too
inline int seq_add_files(std::vector<SeqPiece>& pieces, const char* const* paths, int32_t n, const char* who) {
    if (int rc = seq_check_paths(paths, n, who)) return rc;
    for (int32_t k = 0; k < n; k++) {
        SeqPiece p; p.path = paths[k];
        p.fd = open(paths[k], O_RDONLY | O_CLOEXEC);
        if (p.fd < 0) DGE_FAIL(DGE_ERR_IO, "cannot open %s: %s", paths[k], strerror(errno));
        pieces.push_back(p);                       // (before the fstat: a failure still closes it)
        struct stat st;
        if (fstat(p.fd, &st) != 0 || !S_ISREG(st.st_mode)) DGE_FAIL(DGE_ERR_IO, "cannot read %s: not a regular file", paths[k]);
        pieces.back().size = (int64_t)st.st_size;
    }
    return DGE_OK;
}

// up to cap bytes of the piece from offset at (a file is read in sequence: at is where its descriptor stands); *got >= 1 bytes on success, at < p.size, cap >= 1
inline int seq_piece_read(const SeqPiece& p, int64_t at, uint8_t* dst, int64_t cap, int64_t* got) {
    const int64_t m = std::min<int64_t>(cap, p.size - at);
    if (p.mem) { memcpy(dst, p.mem + at, (size_t)m); *got = m; return DGE_OK; }
    ssize_t r;
    do r = read(p.fd, dst, (size_t)m); while (r < 0 && errno == EINTR);
    if (r <= 0) DGE_FAIL(DGE_ERR_IO, "cannot read %s: %s after %lld of %lld bytes", p.path, r < 0 ? strerror(errno) : "the file ends", (long long)at, (long long)p.size);
    *got = (int64_t)r;
    return DGE_OK;
}

// The joined stream — prior names, then every piece with its pad byte — produced front to back (seq_plan.h: seq_layout).
struct SeqJoiner {
    std::vector<SeqPiece>& pieces; const std::string& prefix;
    int64_t in_prefix = 0; size_t k = 0; int64_t at = 0; uint8_t last = '\n';
    int fill(uint8_t* dst, int64_t cap, int64_t* got) {
        int64_t n = 0;
        while (n < cap) {
            if (in_prefix < (int64_t)prefix.size()) {
                const int64_t m = std::min<int64_t>(cap - n, (int64_t)prefix.size() - in_prefix);
                memcpy(dst + n, prefix.data() + in_prefix, (size_t)m);
                in_prefix += m; n += m;
                continue;
            }
            if (k >= pieces.size()) break;
            const SeqPiece& p = pieces[k];
            if (at < p.size) {
                int64_t m = 0;
                if (int rc = seq_piece_read(p, at, dst + n, cap - n, &m)) return rc;
                last = dst[n + m - 1];
                at += m; n += m;
                continue;
            }
            dst[n++] = seq_pad_byte(p.size, last);
            k++; at = 0; last = '\n';
        }
        *got = n;
        return DGE_OK;
    }
};

inline int64_t trip_last_terminator(const uint8_t* b, int64_t n) {
    const uint8_t* nl = n ? static_cast<const uint8_t*>(memrchr(b, '\n', (size_t)n)) : nullptr;
    const int64_t a = nl ? nl - b : -1;
    const uint8_t* cr = n - a - 1 > 0 ? static_cast<const uint8_t*>(memrchr(b + a + 1, '\r', (size_t)(n - a - 1))) : nullptr;
    return cr ? cr - b : a;
}

// the pieces' bytes, cut into slabs of whole lines (the head of trip_text.hip states what a slab is).
// A reader that reports byte offsets (TabReader::fill of the counts reader) reads k, at, n_tail, opens and pending_cr after next() to place a slab in its
// piece: `at - n_tail` is the offset behind the bytes sent or dropped so far, `opens` after a call says the slab was its piece's last.  Keep those meanings,
// or change fill() with them; it refuses with DGE_ERR_STATE when they no longer add up.
struct TripFeeder {
    std::vector<SeqPiece>& pieces;
    int64_t S;
    size_t k = 0;
    int64_t at = 0;                   // bytes of piece k taken
    bool opens = true;                // the next slab is the first of piece k
    bool pending_cr = false;          // the last byte sent was a "\r" that ended a buffer: a "\n" that follows is its other half
    std::vector<uint8_t> tail, skip;
    int64_t n_tail = 0;

    int read_some(uint8_t* dst, int64_t cap, int64_t* got) {
        const SeqPiece& p = pieces[k];
        *got = 0;
        while (*got == 0 && at < p.size && cap > 0) {
            int64_t m = 0;
            if (int rc = seq_piece_read(p, at, dst, cap, &m)) return rc;
            at += m;
            if (pending_cr) {
                pending_cr = false;
                if (dst[0] == '\n') { m--; memmove(dst, dst + 1, (size_t)m); }
            }
            *got = m;
        }
        return DGE_OK;
    }

    // an over-long line's rest: bytes up to and with the next terminator are dropped, what follows it becomes the tail
    int skip_line() {
        if (skip.empty()) skip.resize((size_t)std::min<int64_t>(S, (int64_t)1 << 20));          // what follows the terminator becomes the tail: no more than a tail's room
        for (;;) {
            int64_t got = 0;
            if (int rc = read_some(skip.data(), (int64_t)skip.size(), &got)) return rc;
            if (got == 0) return DGE_OK;
            int64_t p = 0;
            while (p < got && skip[(size_t)p] != '\n' && skip[(size_t)p] != '\r') p++;
            if (p == got) continue;
            if (skip[(size_t)p] == '\r') {
                if (p + 1 < got) { if (skip[(size_t)p + 1] == '\n') p++; }
                else pending_cr = true;
            }
            n_tail = got - p - 1;
            memcpy(tail.data(), skip.data() + p + 1, (size_t)n_tail);
            return DGE_OK;
        }
    }

    // the next slab into buf (S bytes): *n = 0 when the text is through.  *first: the slab opens its piece.  *open_end: its last line has no terminator.
    int next(uint8_t* buf, int64_t* n_out, bool* first, bool* open_end) {
        *n_out = 0;
        if (tail.empty()) tail.resize((size_t)S);
        while (k < pieces.size()) {
            int64_t n = n_tail;
            if (n) memcpy(buf, tail.data(), (size_t)n);
            n_tail = 0;
            for (;;) {
                int64_t got = 0;
                if (int rc = read_some(buf + n, S - n, &got)) return rc;
                if (got == 0) break;
                n += got;
            }
            const bool at_end = at >= pieces[k].size;
            int64_t send = n;
            if (!at_end) {                                   // the buffer is full and the piece goes on
                const int64_t t = trip_last_terminator(buf, n);
                if (t < 0) {
                    send = TRIP_MAX_LINE + 2;
                    buf[TRIP_MAX_LINE + 1] = '\n';
                    if (int rc = skip_line()) return rc;
                } else {
                    send = t + 1;
                    n_tail = n - send;
                    memcpy(tail.data(), buf + send, (size_t)n_tail);
                    if (n_tail == 0 && buf[t] == '\r') pending_cr = true;
                }
            }
            const bool was_first = opens;
            opens = false;
            if (at >= pieces[k].size && n_tail == 0) { k++; at = 0; opens = true; pending_cr = false; }
            if (send == 0) continue;                         // an empty piece, or one whose rest was the "\n" of a "\r\n"
            *n_out = send; *first = was_first;
            *open_end = buf[send - 1] != '\n' && buf[send - 1] != '\r';
            return DGE_OK;
        }
        return DGE_OK;
    }
};

}  // namespace
