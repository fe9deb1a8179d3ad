// seq_pieces_harness.cpp — embedding_amd/csrc/seq_pieces.h on the host: the pieces, the one read step, the joiner and the slab feeder, with a dge_set_error of
// its own that keeps the message.  Built by tests/test_seq_pieces_host.py as a shared object (ctypes) and, with -DHARNESS_MAIN, as a stand-alone program whose
// main runs the same cases under the sanitizers.
#include <stdarg.h>
#include <stdio.h>

static char g_msg[1024];
void dge_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
}

#include "../../embedding_amd/csrc/seq_pieces.h"

namespace {
struct Pieces {      // the owner: closes the descriptors as SeqRun does
    std::vector<SeqPiece> v;
    ~Pieces() { seq_close_pieces(v); }
};
int add(Pieces& P, const char* const* items, const int64_t* n_bytes, int32_t n, int as_files) {
    return as_files ? seq_add_files(P.v, items, n, "who") : seq_add_texts(P.v, items, n_bytes, n, "who");
}
}  // namespace

extern "C" {

const char* harness_message() { return g_msg; }

// -> the return code; sizes[k]: what the piece list holds afterwards (n_pieces of them)
int harness_add(const char* const* items, const int64_t* n_bytes, int32_t n, int as_files, int64_t* sizes, int32_t* n_pieces) {
    g_msg[0] = 0;
    Pieces P;
    const int rc = add(P, items, n_bytes, n, as_files);
    *n_pieces = (int32_t)P.v.size();
    for (size_t k = 0; k < P.v.size(); k++) sizes[k] = P.v[k].size;
    return rc;
}

// the joined stream through fill calls of capacity cap.  truncate_to >= 0: file 0 is cut to that size between the fstat and the first read
int harness_join(const char* prefix, int64_t n_prefix, const char* const* items, const int64_t* n_bytes, int32_t n, int as_files, int64_t cap, int64_t truncate_to, uint8_t* out,
                 int64_t out_cap, int64_t* n_out) {
    g_msg[0] = 0;
    *n_out = 0;
    Pieces P;
    if (int rc = add(P, items, n_bytes, n, as_files)) return rc;
    if (truncate_to >= 0 && truncate(items[0], (off_t)truncate_to) != 0) return -1;
    const std::string pre(prefix, (size_t)n_prefix);
    SeqJoiner join{P.v, pre};
    std::vector<uint8_t> buf((size_t)cap);
    for (;;) {
        int64_t got = 0;
        if (int rc = join.fill(buf.data(), cap, &got)) return rc;
        if (got == 0) return DGE_OK;
        if (*n_out + got > out_cap) return -2;
        memcpy(out + *n_out, buf.data(), (size_t)got);
        *n_out += got;
    }
}

// the slabs of S bytes, one after the other in out; slab s: slab_n[s] bytes, flags[2s] = first, flags[2s + 1] = open_end
int harness_feed(const char* const* items, const int64_t* n_bytes, int32_t n, int as_files, int64_t S, uint8_t* out, int64_t out_cap, int64_t* slab_n, uint8_t* flags,
                 int64_t max_slabs, int64_t* n_slabs) {
    g_msg[0] = 0;
    *n_slabs = 0;
    Pieces P;
    if (int rc = add(P, items, n_bytes, n, as_files)) return rc;
    TripFeeder feed{P.v, S};
    std::vector<uint8_t> buf((size_t)S);
    int64_t at = 0;
    for (;;) {
        int64_t got = 0;
        bool first = false, open_end = false;
        if (int rc = feed.next(buf.data(), &got, &first, &open_end)) return rc;
        if (got == 0) return DGE_OK;
        if (*n_slabs >= max_slabs || at + got > out_cap) return -2;
        memcpy(out + at, buf.data(), (size_t)got);
        at += got;
        slab_n[*n_slabs] = got; flags[2 * *n_slabs] = first; flags[2 * *n_slabs + 1] = open_end;
        ++*n_slabs;
    }
}

}  // extern "C"

#ifdef HARNESS_MAIN
#include <stdlib.h>

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s [%s]\n", __LINE__, #c, g_msg); wrong++; } } while (0)

static int open_descriptors() {
    int n = 0;
    for (int fd = 0; fd < 1024; fd++) if (fcntl(fd, F_GETFD) != -1) n++;
    return n;
}

// argv[1]: a directory to write in.  The cases of tests/test_seq_pieces_host.py, against expectations written out here
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    int wrong = 0;
    const std::string dir = argv[1], fa = dir + "/a.txt", fb = dir + "/b.txt", missing = dir + "/missing";
    const std::string A = "one two\nthree", B = "four\n";
    { FILE* f = fopen(fa.c_str(), "wb"); fwrite(A.data(), 1, A.size(), f); fclose(f); f = fopen(fb.c_str(), "wb"); fwrite(B.data(), 1, B.size(), f); fclose(f); }
    const int fds = open_descriptors();
    int64_t sizes[8]; int32_t np = 0;
    // files: good, missing, a directory, a null path in the middle
    { const char* p[] = {fa.c_str(), fb.c_str()}; CHECK(harness_add(p, nullptr, 2, 1, sizes, &np) == DGE_OK && np == 2 && sizes[0] == 13 && sizes[1] == 5); }
    { const char* p[] = {fa.c_str(), missing.c_str()}; CHECK(harness_add(p, nullptr, 2, 1, sizes, &np) == DGE_ERR_IO && std::string(g_msg).find("cannot open " + missing + ": ") == 0); }
    { const char* p[] = {fa.c_str(), dir.c_str()}; CHECK(harness_add(p, nullptr, 2, 1, sizes, &np) == DGE_ERR_IO && g_msg == "cannot read " + dir + ": not a regular file"); }
    { const char* p[] = {fa.c_str(), nullptr, fb.c_str()}; CHECK(harness_add(p, nullptr, 3, 1, sizes, &np) == DGE_ERR_ARG && g_msg == std::string("who: path 1 is null") && np == 0); }
    // texts: a negative size, null with a positive size
    { const char* t[] = {A.data(), B.data()}; const int64_t nb[] = {13, -1}; CHECK(harness_add(t, nb, 2, 0, sizes, &np) == DGE_ERR_ARG && g_msg == std::string("who: text 1 is null or of negative size")); }
    { const char* t[] = {nullptr, B.data()}; const int64_t nb[] = {3, 5}; CHECK(harness_add(t, nb, 2, 0, sizes, &np) == DGE_ERR_ARG && g_msg == std::string("who: text 0 is null or of negative size")); }
    { const char* t[] = {nullptr, B.data()}; const int64_t nb[] = {0, 5}; CHECK(harness_add(t, nb, 2, 0, sizes, &np) == DGE_OK && np == 2); }
    // the joiner: prefix, pieces, pads — through every capacity, from files and from texts
    const std::string want = "p q\n" + A + "\n" + " " + B + " ";
    for (int as_files = 0; as_files < 2; as_files++)
        for (int64_t cap : {1, 7, 4096}) {
            const char* t[] = {A.data(), "", B.data()}; const int64_t nb[] = {13, 0, 5};
            const std::string fe = dir + "/empty.txt";
            { FILE* f = fopen(fe.c_str(), "wb"); fclose(f); }
            const char* p[] = {fa.c_str(), fe.c_str(), fb.c_str()};
            uint8_t out[64]; int64_t n = 0;
            CHECK(harness_join("p q\n", 4, as_files ? p : t, nb, 3, as_files, cap, -1, out, 64, &n) == DGE_OK);
            CHECK(std::string((const char*)out, (size_t)n) == want);
        }
    // a file cut short between the fstat and the read
    { const char* p[] = {fa.c_str()}; uint8_t out[64]; int64_t n = 0;
      CHECK(harness_join("", 0, p, nullptr, 1, 1, 4, 6, out, 64, &n) == DGE_ERR_IO && g_msg == "cannot read " + fa + ": the file ends after 6 of 13 bytes"); }
    // the feeder, S = 131072: a "\r\n" across the read boundary, a piece that ends in "\r" before one that starts with "\n", an empty piece, lines no slab holds
    {
        const int64_t S = 131072;
        std::string x((size_t)S - 1, 'x'); x += "\r\nabc\r"; for (size_t i = 1000; i < x.size() - 8; i += 1000) x[i] = '\n';
        std::string y = "\ndef\n" + std::string(200000, 'w') + "\r\nghi\r" + std::string(400000, 'v') + "\rjk";
        const char* t[] = {x.data(), "", y.data()}; const int64_t nb[] = {(int64_t)x.size(), 0, (int64_t)y.size()};
        std::vector<uint8_t> out(x.size() + y.size());
        int64_t slab_n[16], ns = 0; uint8_t flags[32];
        CHECK(harness_feed(t, nb, 3, 0, S, out.data(), (int64_t)out.size(), slab_n, flags, 16, &ns) == DGE_OK);
        std::string got((const char*)out.data(), (size_t)[&] { int64_t s = 0; for (int64_t i = 0; i < ns; i++) s += slab_n[i]; return s; }());
        std::string expect = x; expect.erase((size_t)S, 1);                                             // the "\n" half of the split "\r\n"
        expect += "\ndef\n" + std::string(65536, 'w') + "\nghi\r" + std::string(65536, 'v') + "\njk";
        CHECK(got == expect);
        CHECK(ns >= 4 && flags[0] == 1 && flags[2] == 0 && flags[2 * (ns - 1) + 1] == 1 && slab_n[0] == S);
    }
    CHECK(open_descriptors() == fds);
    printf("wrong %d\n", wrong);
    return wrong ? 1 : 0;
}
#endif
