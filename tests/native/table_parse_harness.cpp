// table_parse_harness.cpp — embedding_amd/csrc/table_parse.h built for the host, driven over a whole text by a one-thread loop: what
// tests/test_counts_host.py compares with tests/counts_ref.py, plain and under -fsanitize=address,undefined, and what scripts/counts_rate.py times against the
// device.  The line cutting here ("\n", "\r\n", a lone "\r") is the harness's own; on the device it is k_tab_count / k_tab_emit.
//
//   table_parse_harness read|time <text> <ids> <table cols> <sep> <skip_lines> <key_field> <key_lo> <key_hi> <col_lo> <n_cols> <col_offset> <neg_col_offset>
//     read:  "offence <kind> <offset> <line> <field>", or "ok <lines> <skipped> <empty> <rows> <foreign> <total>" and a line "<row> <col> <value>" per cell != 0
//     time:  "ok .." and "time <ms> checksum <sum of (cell index + 1) * value mod 2^64>"
// Every line is copied into a buffer of exactly its size first, so that the sanitizer sees a read past a line's end.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "../../embedding_amd/csrc/table_parse.h"

static std::vector<uint8_t> slurp(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    std::vector<uint8_t> b;
    uint8_t chunk[65536];
    size_t n;
    while ((n = fread(chunk, 1, sizeof(chunk), f)) > 0) b.insert(b.end(), chunk, chunk + n);
    fclose(f);
    return b;
}

int main(int argc, char** argv) {
    if (argc != 14 || (strcmp(argv[1], "read") != 0 && strcmp(argv[1], "time") != 0)) { fprintf(stderr, "usage: see the head of table_parse_harness.cpp\n"); return 2; }
    const bool timing = strcmp(argv[1], "time") == 0;
    const std::vector<uint8_t> text = slurp(argv[2]);
    std::vector<uint8_t> id_text = slurp(argv[3]);
    id_text.push_back(0);                              // strtoll stops there
    std::vector<int64_t> ids;
    for (char* p = (char*)id_text.data(), *end = p + id_text.size() - 1; p < end;) {
        char* q = nullptr;
        const long long v = strtoll(p, &q, 10);
        if (q == p) break;
        ids.push_back(v);
        p = q;
    }
    std::sort(ids.begin(), ids.end());
    const int32_t C = atoi(argv[4]), skip_lines = atoi(argv[6]), col_offset = atoi(argv[12]), neg_col_offset = atoi(argv[13]);
    const tab_rule rule = {atoi(argv[5]), atoi(argv[7]), atoi(argv[8]), atoi(argv[9]), atoi(argv[10]), atoi(argv[11]), neg_col_offset >= 0 ? 1 : 0};
    std::vector<uint64_t> table(ids.size() * (size_t)C, 0);
    long long lines = 0, skipped = 0, empty = 0, rows = 0, foreign = 0;
    unsigned long long total = 0;
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t n = (int64_t)text.size();
    std::vector<uint8_t> exact;
    for (int64_t at = 0; at < n;) {
        int64_t e = at;
        while (e < n && text[(size_t)e] != '\n' && text[(size_t)e] != '\r') e++;
        const int64_t next = e < n ? (text[(size_t)e] == '\r' && e + 1 < n && text[(size_t)e + 1] == '\n' ? e + 2 : e + 1) : n;
        const int64_t len = e - at;
        lines++;
        if (lines <= skip_lines) skipped++;
        else if (len == 0) empty++;
        else {
            const uint8_t* s = text.data() + at;
            if (!timing) { exact.assign(s, s + len); exact.shrink_to_fit(); s = exact.data(); }
            tab_line L;
            tab_parse_line(s, (int32_t)std::min<int64_t>(len, TAB_MAX_LINE + 1), rule, &L);      // (a longer line is refused by its length alone)
            if (L.offence != TAB_NO_OFFENCE) {
                const int64_t off = (int64_t)(L.offence >> 4);
                long long field = 0;
                for (int64_t q = 0; q < off; q++) field += s[q] == (uint8_t)rule.sep;
                printf("offence %d %lld %lld %lld\n", (int)(L.offence & 15), (long long)(at + off), lines, field);
                return 0;
            }
            const auto it = std::lower_bound(ids.begin(), ids.end(), L.key);
            if (it == ids.end() || *it != L.key) foreign++;
            else {
                rows++;
                uint64_t* row = &table[(size_t)(it - ids.begin()) * (size_t)C + (size_t)(L.neg ? neg_col_offset : col_offset)];
                int32_t p = L.val_at;
                for (int32_t j = 0; j < rule.n_cols; j++) { const uint64_t v = tab_next_value(s, (int32_t)len, rule.sep, &p); row[j] += v; total += v; }
            }
        }
        at = next;
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("ok %lld %lld %lld %lld %lld %llu\n", lines, skipped, empty, rows, foreign, total);
    if (timing) {
        uint64_t sum = 0;
        for (size_t i = 0; i < table.size(); i++) sum += (uint64_t)(i + 1) * table[i];
        printf("time %.3f checksum %llu\n", ms, (unsigned long long)sum);
    } else
        for (size_t i = 0; i < table.size(); i++)
            if (table[i]) printf("%zu %zu %llu\n", i / (size_t)C, i % (size_t)C, (unsigned long long)table[i]);
    return 0;
}
