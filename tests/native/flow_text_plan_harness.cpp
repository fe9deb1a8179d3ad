// Host build of the flow-table text writer's arithmetic (embedding_amd/csrc/flow_text_plan.h) for tests/test_flow_text_host.py:
//   flow_text_plan_harness decimal V...    "length spelling" of every V as the header sizes and spells it
//   flow_text_plan_harness rows SEED       random sparse matrices of n = 1 .. 300 columns, weights of 1 .. 15 digits: every byte offset -> (column, character)
//                                          against the rows spelled out with snprintf; the cursor that walks the text; the column starts and row lengths
//   flow_text_plan_harness far             row starts above 2^32 on synthetic prefix arrays
// A check that fails prints what it found and the program ends with status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../embedding_amd/csrc/flow_text_plan.h"

static uint64_t g_state = 1;
static uint64_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return g_state; }

#define CHECK(cond, ...) do { if (!(cond)) { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

static int rows(uint64_t seed) {
    g_state = seed * 2654435761u + 88172645463325252ull;
    const uint8_t seps[3] = {',', ' ', '\t'};
    int64_t bytes = 0;
    for (int64_t n = 1; n <= 300; n++) {
        const uint8_t sep = seps[n % 3];
        const int density = (int)(rnd() % 5);                         // 0: all zero, .. 4: nearly full
        std::vector<int32_t> col;
        std::vector<int64_t> w, P(1, 0), rowb(1, 0);
        std::string text;
        std::vector<int64_t> col_of;                                  // the column of every byte of the text
        const int64_t n_rows = n < 6 ? n : 6;                         // the writer's matrices are square; the arithmetic does not ask for it
        for (int64_t i = 0; i < n_rows; i++) {
            for (int64_t c = 0; c < n; c++) {
                int64_t v = 0;
                const bool edge = c == 0 || c == n - 1 ? rnd() % 2 == 0 : (int)(rnd() % 8) < 2 * density;
                if (edge && density) {
                    const int digits = 1 + (int)(rnd() % 15);
                    uint64_t lo = 1;
                    for (int k = 1; k < digits; k++) lo *= 10;
                    v = (int64_t)(lo + rnd() % (9 * lo));
                    col.push_back((int32_t)c); w.push_back(v); P.push_back(P.back() + digits - 1);
                }
                char buf[32];
                const int len = std::snprintf(buf, sizeof buf, "%lld", (long long)v);
                text.append(buf, (size_t)len);
                text.push_back(c == n - 1 ? '\n' : (char)sep);
                col_of.insert(col_of.end(), (size_t)len + 1, c);
            }
            rowb.push_back((int64_t)col.size());
        }
        if (col.empty()) { col.push_back(0); w.push_back(0); }        // (never read: the arrays only must not be null)
        // lengths and column starts
        int64_t at = 0;
        for (int64_t i = 0; i < n_rows; i++) {
            CHECK(ftp_row_start(n, P.data(), rowb.data(), i) == at, "n %lld: row %lld starts at %lld, not %lld", (long long)n, (long long)i, (long long)ftp_row_start(n, P.data(), rowb.data(), i), (long long)at);
            const int64_t len = ftp_row_len(n, P.data(), rowb[i], rowb[i + 1]);
            int64_t want = 0;
            for (int64_t c = 0; c <= n; c++) {
                if (c < n) while (col_of[(size_t)(at + want)] != c) want++;
                else want = len;
                CHECK(ftp_col_start(col.data(), P.data(), rowb[i], rowb[i + 1], c) == want, "n %lld row %lld: column %lld does not start at %lld", (long long)n, (long long)i, (long long)c, (long long)want);
            }
            at += len;
        }
        CHECK(at == (int64_t)text.size(), "n %lld: the rows hold %lld bytes, the text %lld", (long long)n, (long long)at, (long long)text.size());
        // every byte by itself
        for (int64_t t = 0; t < at; t++) {
            ftp_cursor c;
            ftp_seek(c, n_rows, n, col.data(), P.data(), rowb.data(), t);
            int64_t column = -1;
            const uint8_t ch = ftp_row_char(col.data(), P.data(), w.data(), n, sep, c.b, c.j, c.q, &column);
            CHECK(ch == (uint8_t)text[(size_t)t] && column == col_of[(size_t)t], "n %lld: byte %lld is '%c' in column %lld, found '%c' in column %lld", (long long)n, (long long)t, text[(size_t)t],
                  (long long)col_of[(size_t)t], ch, (long long)column);
        }
        // the walk, from a few starts
        for (int64_t start : {(int64_t)0, at / 3, at - 1}) {
            ftp_cursor c;
            ftp_seek(c, n_rows, n, col.data(), P.data(), rowb.data(), start);
            for (int64_t t = start; t < at; t++) {
                const uint8_t ch = ftp_next(c, n_rows, n, col.data(), P.data(), w.data(), rowb.data(), sep);
                CHECK(ch == (uint8_t)text[(size_t)t], "n %lld: the walk from %lld gives '%c' at %lld, not '%c'", (long long)n, (long long)start, ch, (long long)t, text[(size_t)t]);
            }
            CHECK(c.row == n_rows && c.q == 0, "n %lld: the walk ends in row %lld at %lld", (long long)n, (long long)c.row, (long long)c.q);
        }
        bytes += at;
    }
    std::printf("ok %lld\n", (long long)bytes);
    return 0;
}

static int far() {
    // n rows of n columns with one 15-digit entry each, in column i % n: only the prefix arrays exist, as on the device
    const int64_t n = 50000;
    std::vector<int64_t> P((size_t)n + 1), rowb((size_t)n + 1);
    std::vector<int32_t> col((size_t)n);
    for (int64_t i = 0; i <= n; i++) { P[(size_t)i] = 14 * i; rowb[(size_t)i] = i; }
    for (int64_t i = 0; i < n; i++) col[(size_t)i] = (int32_t)((i * 7919) % n);
    const int64_t row_bytes = 2 * n + 14, total = ftp_row_start(n, P.data(), rowb.data(), n);
    CHECK(total == row_bytes * n && total > ((int64_t)1 << 32), "the text holds %lld bytes", (long long)total);
    int64_t above = 0;
    for (int64_t i = 0; i < n; i += (i > 42940 && i < 42960) ? 1 : 97) {          // 2^32 / row_bytes = 42943.7: every row around it
        const int64_t s = i * row_bytes;
        for (int64_t t : {s, s + 1, s + row_bytes - 1}) {
            ftp_cursor c;
            ftp_seek(c, n, n, col.data(), P.data(), rowb.data(), t);
            CHECK(c.row == i && c.q == t - s && c.b == i && c.e == i + 1, "byte %lld lies in row %lld at %lld, found row %lld at %lld", (long long)t, (long long)i, (long long)(t - s), (long long)c.row, (long long)c.q);
            const int64_t es = 2 * (int64_t)col[(size_t)i];
            CHECK(c.j == (c.q >= es ? i : i - 1), "byte %lld: entry %lld", (long long)t, (long long)c.j);
            if (t > ((int64_t)1 << 32)) above++;
        }
        if (i > 0) CHECK(ftp_find_row(n, n, P.data(), rowb.data(), s - 1) == i - 1, "byte %lld lies in row %lld", (long long)(s - 1), (long long)(i - 1));
    }
    // the byte at 2^32 itself and its neighbours
    for (int64_t t = ((int64_t)1 << 32) - 2; t <= ((int64_t)1 << 32) + 2; t++) CHECK(ftp_find_row(n, n, P.data(), rowb.data(), t) == t / row_bytes, "byte %lld", (long long)t);
    CHECK(above > 0, "no offset above 2^32 was tried");
    std::printf("ok %lld\n", (long long)above);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::cerr << "usage: flow_text_plan_harness decimal V... | rows SEED | far\n"; return 2; }
    const std::string mode = argv[1];
    if (mode == "decimal") {
        for (int i = 2; i < argc; i++) {
            const int64_t v = (int64_t)std::strtoll(argv[i], nullptr, 10);
            const int len = ftp_len(v);
            std::string s;
            for (int q = 0; q < len; q++) s.push_back((char)ftp_char(v, q));
            std::printf("%d %s\n", len, s.c_str());
        }
        return 0;
    }
    if (mode == "rows" && argc >= 3) return rows((uint64_t)std::strtoull(argv[2], nullptr, 10));
    if (mode == "far") return far();
    return 2;
}
