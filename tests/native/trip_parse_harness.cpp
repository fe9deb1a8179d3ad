// Host build of embedding_amd/csrc/trip_parse.h — what every lane of k_trip_parse (trip_text.hip) runs on its line — for tests/test_trip_parse_host.py, which
// compares it record by record with tests/trip_text_ref.py.  As a shared library it parses the lines it is handed; as a program (it has a main) it reads a file,
// cuts it into lines by the rule of include/dge.h, parses every line out of a heap copy of exactly the line's size — so that the address sanitizer sees every
// read past a line's end — and prints the counts:   trip_parse_harness FILE FORMAT [HEADER]
// scripts/trip_text_rate.py times the same program as the host path a caller has without the device reader.
#include <stdio.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "../../embedding_amd/csrc/trip_parse.h"

// line i = text[off[i] .. off[i + 1]); xy: 4 words a line; host: coordinates finished with strtod
extern "C" void harness_trip_parse(const uint8_t* text, const int64_t* off, int64_t n, int format, uint8_t* status, int32_t* hour, uint64_t* xy, int32_t* host) {
    locale_t c_locale = newlocale(LC_ALL_MASK, "C", (locale_t)0);
    for (int64_t i = 0; i < n; i++) {
        trip_rec r;
        trip_parse_line(text + off[i], off[i + 1] - off[i], format, &r);
        host[i] = trip_finish_host(text + off[i], &r, c_locale);
        status[i] = (uint8_t)r.status; hour[i] = r.hour;
        memcpy(xy + 4 * i, r.xy, 32);
    }
    freelocale(c_locale);
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s FILE FORMAT [HEADER]\n", argv[0]); return 2; }
    const int format = atoi(argv[2]), header = argc > 3 ? atoi(argv[3]) : 0;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint8_t> text;
    std::vector<uint8_t> chunk((size_t)1 << 20);
    for (size_t got; (got = fread(chunk.data(), 1, chunk.size(), f)) > 0;) text.insert(text.end(), chunk.begin(), chunk.begin() + (long)got);
    fclose(f);
    locale_t c_locale = newlocale(LC_ALL_MASK, "C", (locale_t)0);
    long long lines = 0, count[4] = {0, 0, 0, 0}, host = 0, hours = 0;
    uint64_t sum = 0;
    const size_t n = text.size();
    size_t start = 0;
    auto take = [&](size_t a, size_t b) {
        if (lines++ == 0 && header) return;
        uint8_t* line = new uint8_t[b - a ? b - a : 1];
        memcpy(line, text.data() + a, b - a);
        trip_rec r;
        trip_parse_line(line, (int64_t)(b - a), format, &r);
        host += trip_finish_host(line, &r, c_locale);
        delete[] line;
        count[r.status]++;
        if (r.status == TRIP_OK) { hours += r.hour; sum += r.xy[0] ^ r.xy[1] ^ r.xy[2] ^ r.xy[3]; }
    };
    for (size_t i = 0; i < n;) {
        const uint8_t c = text[i];
        if (c == '\n' || c == '\r') {
            take(start, i);
            i++;
            if (c == '\r' && i < n && text[i] == '\n') i++;
            start = i;
        } else i++;
    }
    if (start < n) take(start, n);
    freelocale(c_locale);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("bytes %zu lines %lld ok %lld bad_fields %lld bad_parse %lld too_long %lld host_values %lld hours %lld xor %016llx ms %.3f\n", n, lines, count[0], count[1], count[2], count[3],
           host, hours, (unsigned long long)sum, ms);
    return 0;
}
