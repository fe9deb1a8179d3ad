// matrix_parse_harness.cpp — embedding_amd/csrc/matrix_parse.h and matrix_feed.h on the host, as a program of its own (tests/test_matrix_host.py builds it with
// g++, plain and under the sanitizers; scripts/matrix_read_rate.py times its `rate` mode).  Modes:
//   ops <seed>                      the lane summary and the segmented operator on random byte triples: associativity, and against a byte-by-byte loop
//   read <file> <sep> <n> <slab>    the file as one piece through MatrixFeeder at that slab size: "offence <kind> <offset> <line> <column>" or the entries
//   sweep <file> <sep> <n>          the same at EVERY slab size from MAT_SLAB_MIN to the file's length: the result must be the same every time
//   rate <file> <sep> <n>           one pass at the default slab size, timed: entries, checksum, milliseconds
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <random>

static char g_msg[1024];
void dge_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
}

#include "../../embedding_amd/csrc/matrix_feed.h"

namespace {

struct Entry { int64_t out, row, col; uint64_t v; };
struct Keep {
    std::vector<Entry> e;
    void entry(int64_t out, int64_t row, int64_t col, uint64_t v) { e.push_back({out, row, col, v}); }
};
struct Hash {                                 // the checksum of (row, column, value) in text order, without keeping them
    uint64_t h = 1469598103934665603ULL; int64_t count = 0;
    void entry(int64_t, int64_t row, int64_t col, uint64_t v) {
        for (uint64_t x : {(uint64_t)row, (uint64_t)col, v}) { h ^= x; h *= 1099511628211ULL; }
        count++;
    }
};

struct Result { MatState st; int64_t lines = 0, rows = 0, where_nl = 0, where_cols = 0; int32_t slabs = 0; };

template <typename Sink>
int read_all(std::vector<SeqPiece>& pieces, uint32_t sep, int64_t nsel, int64_t S, Sink& sink, Result& r) {
    MatrixFeeder feed{pieces, S, sep};
    std::vector<uint8_t> buf((size_t)mat_frame_bytes(S));
    r.st = MatState{};
    r.st.offence = MAT_NO_OFFENCE;
    for (;;) {
        int64_t n = 0, base = 0; int32_t piece = 0; bool first = false, last = false;
        if (int rc = feed.next(buf.data(), &n, &piece, &base, &first, &last)) return rc;
        if (n == 0) return DGE_OK;
        const MatSlab slab = {buf.data() + MAT_LEAD, n, base, nsel, last ? 1 : 0};
        const MatState before = r.st;
        mat_host_slab(slab, first ? 1 : 0, sep, r.st, sink);
        r.slabs++;
        if (r.st.offence != MAT_NO_OFFENCE) {
            r.where_nl = first ? 0 : before.nl; r.where_cols = first ? 0 : before.cols;
            mat_where(slab.text, 0, (int64_t)(r.st.offence >> 3) - base, sep, &r.where_nl, &r.where_cols);
            return DGE_OK;
        }
        if (last) { r.lines += r.st.nl + (slab.text[n - 1] != '\n'); r.rows += r.st.rows; }
    }
}

std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> v;
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    uint8_t b[65536];
    size_t got;
    while ((got = fread(b, 1, sizeof(b), f)) > 0) v.insert(v.end(), b, b + got);
    fclose(f);
    return v;
}

std::vector<SeqPiece> one_piece(const std::vector<uint8_t>& text) {
    SeqPiece p; p.mem = text.data(); p.size = (int64_t)text.size();
    return {p};
}

void print(const Keep& k, const Result& r) {
    if (r.st.offence != MAT_NO_OFFENCE) {
        printf("offence %d %lld %lld %lld\n", (int)(r.st.offence & 7), (long long)(r.st.offence >> 3), (long long)r.where_nl + 1, (long long)r.where_cols);
        return;
    }
    printf("ok %lld %lld %lld %llu %llu\n", (long long)r.lines, (long long)r.rows, (long long)r.st.out, (unsigned long long)r.st.sum_hi, (unsigned long long)r.st.sum_lo);
    for (const Entry& e : k.e) printf("%lld %lld %llu\n", (long long)e.row, (long long)e.col, (unsigned long long)e.v);
}

bool same(const Keep& a, const Result& ra, const Keep& b, const Result& rb) {
    if (ra.st.offence != rb.st.offence) return false;
    if (ra.st.offence != MAT_NO_OFFENCE) return ra.where_nl == rb.where_nl && ra.where_cols == rb.where_cols;
    if (ra.lines != rb.lines || ra.rows != rb.rows || ra.st.out != rb.st.out || ra.st.sum_hi != rb.st.sum_hi || ra.st.sum_lo != rb.st.sum_lo || a.e.size() != b.e.size()) return false;
    for (size_t i = 0; i < a.e.size(); i++)
        if (a.e[i].out != (int64_t)i || a.e[i].out != b.e[i].out || a.e[i].row != b.e[i].row || a.e[i].col != b.e[i].col || a.e[i].v != b.e[i].v) return false;
    return true;
}

// the summary of bytes [32, 32 + len) of t (the lane before them is t[0 .. 32), the byte behind them t[32 + len]), one byte at a time
MatSum slow_summary(const uint8_t* t, int len, uint32_t sep) {
    MatSum s = {0, 0, 0, 0};
    for (int i = 32; i < 32 + len; i++) {
        const uint8_t c = t[i];
        const bool term_first = (c == '\r' && t[i + 1] == '\n') || (c == '\n' && t[i - 1] != '\r');
        if (t[i - 1] == '\n' && !term_first) s.rows++;
        if (c == '\n') { s.nl++; s.cols = 0; }
        if (c == sep) s.cols++;
        if (c >= '0' && c <= '9' && !(t[i + 1] >= '0' && t[i + 1] <= '9')) {
            bool nz = false;
            for (int k = i; k >= 0 && t[k] >= '0' && t[k] <= '9'; k--) nz = nz || t[k] != '0';
            if (nz) s.emits++;
        }
    }
    return s;
}

bool eq(const MatSum& a, const MatSum& b) { return a.nl == b.nl && a.cols == b.cols && a.rows == b.rows && a.emits == b.emits; }

int ops(uint64_t seed) {
    std::mt19937_64 rng(seed);
    const char alphabet[] = "0000011234567890,,,,\n\n\r x";
    const uint32_t sep = ',';
    long checked = 0;
    for (int round = 0; round < 20000; round++) {
        uint8_t t[32 + 96 + 33] = {0};
        const int density = (int)(rng() % 4);
        for (int i = 31; i < 32 + 96 + 1; i++) t[i] = density == 0 ? (uint8_t)"0,"[rng() % 2] : (uint8_t)alphabet[rng() % (sizeof(alphabet) - 1)];
        for (int i = 32; i < 32 + 96; i++) if (t[i] == '\r' && rng() % 2) t[i + 1] = '\n';
        // digit runs that reach back from a lane into the one before, but no further: the reader's slabs and the 19-digit rule see to that
        const int valid3 = 1 + (int)(rng() % 32);
        MatSum s[3];
        MatRaw prev = mat_raw_bytes(t, sep);
        bool long_run = false;
        for (int l = 0; l < 3; l++) {
            const MatRaw cur = mat_raw_bytes(t + 32 + 32 * l, sep);
            const MatLane L = mat_lane(cur, prev, t[64 + 32 * l], l == 2 ? valid3 : 32);
            long_run = long_run || L.lng;
            s[l] = mat_summary(L);
            const MatSum slow = slow_summary(t + 32 * l, l == 2 ? valid3 : 32, sep);
            if (!L.lng && !eq(s[l], slow)) { printf("lane %d of round %d: summary (%d %d %d %d), byte by byte (%d %d %d %d)\n", l, round, s[l].nl, s[l].cols, s[l].rows, s[l].emits, slow.nl, slow.cols, slow.rows, slow.emits); return 1; }
            prev = cur;
        }
        const MatSum left = mat_combine(mat_combine(s[0], s[1]), s[2]), right = mat_combine(s[0], mat_combine(s[1], s[2]));
        if (!eq(left, right)) { printf("round %d: the operator is not associative\n", round); return 1; }
        if (!long_run) {
            MatSum whole = {0, 0, 0, 0};
            for (int l = 0; l < 3; l++) whole = mat_combine(whole, slow_summary(t + 32 * l, l == 2 ? valid3 : 32, sep));
            MatSum direct = slow_summary(t, 64 + valid3, sep);
            // slow_summary's cols is "since the last line end" only inside its own bytes: the same as the operator's
            if (!eq(left, whole) || !eq(left, direct)) { printf("round %d: three lanes combined differ from one pass\n", round); return 1; }
        }
        const MatSum id = {0, 0, 0, 0};
        if (!eq(mat_combine(id, s[0]), s[0]) || !eq(mat_combine(s[0], id), s[0])) { printf("round %d: (0, 0, 0, 0) is no identity\n", round); return 1; }
        checked++;
    }
    printf("ok %ld\n", checked);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 3 && !strcmp(argv[1], "ops")) return ops(strtoull(argv[2], nullptr, 10));
    if (argc < 5) { fprintf(stderr, "usage: see the head of the source\n"); return 2; }
    const std::vector<uint8_t> text = slurp(argv[2]);
    const uint32_t sep = (uint32_t)atoi(argv[3]);
    const int64_t nsel = atoll(argv[4]);
    std::vector<SeqPiece> pieces = one_piece(text);
    if (!strcmp(argv[1], "read") && argc >= 6) {
        Keep k; Result r;
        if (read_all(pieces, sep, nsel, atoll(argv[5]), k, r)) { fprintf(stderr, "%s\n", g_msg); return 1; }
        print(k, r);
        return 0;
    }
    if (!strcmp(argv[1], "sweep")) {
        Keep k0; Result r0;
        if (read_all(pieces, sep, nsel, MAT_SLAB_MAX, k0, r0)) return 1;
        long sizes = 0;
        for (int64_t S = MAT_SLAB_MIN; S <= (int64_t)text.size(); S++, sizes++) {
            Keep k; Result r;
            if (read_all(pieces, sep, nsel, S, k, r)) return 1;
            if (!same(k0, r0, k, r)) { printf("slab size %lld gives another result\n", (long long)S); return 1; }
        }
        printf("sizes %ld\n", sizes);
        print(k0, r0);
        return 0;
    }
    if (!strcmp(argv[1], "rate")) {
        Hash h; Result r;
        const auto t0 = std::chrono::steady_clock::now();
        if (read_all(pieces, sep, nsel, MAT_SLAB_MAX, h, r)) return 1;
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("entries %lld checksum %llu offence %d ms %.3f\n", (long long)h.count, (unsigned long long)h.h, r.st.offence == MAT_NO_OFFENCE ? 0 : (int)(r.st.offence & 7), ms);
        return 0;
    }
    fprintf(stderr, "unknown mode %s\n", argv[1]);
    return 2;
}
