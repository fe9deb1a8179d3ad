// Host build of embedding_amd/csrc/od_parse.h (the per-lane routines of k_od_parse, od_read.hip) for tests/test_od_parse_host.py and
// tests/test_gpu_od_read.py, compared bit for bit with libc's strtod and strtoll in the "C" locale:
//   g++ -O2 -shared -fPIC -std=c++17 -o libod_parse_harness.so od_parse_harness.cpp          the entries below, called through ctypes
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -o od_parse_harness od_parse_harness.cpp && ./od_parse_harness [n_random [seed]]
//                                                                                             the same checks as a stand-alone program; exit 0 = all equal
// tokens come as one blob, token k at blob + off[k] with off[k + 1] - off[k] bytes (no separators).
#include <errno.h>
#include <locale.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../embedding_amd/csrc/od_parse.h"

extern "C" void harness_od_parse_f64(const uint8_t* blob, const int64_t* off, int64_t n, uint64_t* bits, uint8_t* status) {
    for (int64_t k = 0; k < n; k++) {
        uint64_t b = 0;
        status[k] = (uint8_t)od_parse_f64(blob + off[k], off[k + 1] - off[k], &b);
        bits[k] = b;
    }
}

extern "C" void harness_od_parse_id(const uint8_t* blob, const int64_t* off, int64_t n, int64_t* value, uint8_t* ok) {
    for (int64_t k = 0; k < n; k++) {
        int64_t v = 0;
        ok[k] = od_parse_id(blob + off[k], off[k + 1] - off[k], &v) ? 1 : 0;
        value[k] = v;
    }
}

namespace {

struct Rng {      // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    uint64_t below(uint64_t n) { return next() % n; }
};

struct Tally { int64_t tokens = 0, host = 0, integers = 0, integers_host = 0, wrong = 0; };

// what a well-formed weight token must give: strtod's bits (a NaN by NaN-ness and sign), or "the host's"
void check_weight(const std::string& t, bool integer19, Tally& tally) {
    uint64_t got = 0;
    const int rc = od_parse_f64(reinterpret_cast<const uint8_t*>(t.data()), (int64_t)t.size(), &got);
    char* end = nullptr;
    const double d = strtod(t.c_str(), &end);
    uint64_t want;
    memcpy(&want, &d, 8);
    tally.tokens++;
    tally.integers += integer19;
    bool ok = true;
    if (rc == VEC_PARSE_BAD || *end) ok = false;
    else if (rc == VEC_PARSE_HOST) { tally.host++; tally.integers_host += integer19; }
    else {
        const bool nan_w = (want & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull, nan_g = (got & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull;
        ok = nan_w || nan_g ? (nan_w && nan_g && (want >> 63) == (got >> 63)) : want == got;
    }
    if (!ok) { if (tally.wrong++ < 10) fprintf(stderr, "weight %.60s: rc %d, got %016llx, strtod %016llx\n", t.c_str(), rc, (unsigned long long)got, (unsigned long long)want); }
}

void check_bad_weight(const std::string& t, Tally& tally) {
    uint64_t got = 0;
    tally.tokens++;
    if (od_parse_f64(reinterpret_cast<const uint8_t*>(t.data()), (int64_t)t.size(), &got) != VEC_PARSE_BAD) { if (tally.wrong++ < 10) fprintf(stderr, "weight %s: not refused\n", t.c_str()); }
}

// an id token: strtoll's value when the token is [+-] digits in range, refused otherwise
void check_id(const std::string& t, Tally& tally) {
    int64_t got = 0;
    const bool mine = od_parse_id(reinterpret_cast<const uint8_t*>(t.data()), (int64_t)t.size(), &got);
    size_t i = (!t.empty() && (t[0] == '+' || t[0] == '-')) ? 1 : 0;
    bool form = i < t.size();
    for (size_t j = i; j < t.size(); j++) form = form && t[j] >= '0' && t[j] <= '9';
    errno = 0;
    char* end = nullptr;
    const long long want = strtoll(t.c_str(), &end, 10);
    const bool theirs = form && errno == 0 && !*end;
    tally.tokens++;
    if (mine != theirs || (mine && got != (int64_t)want)) { if (tally.wrong++ < 10) fprintf(stderr, "id %.60s: %d %lld, strtoll %d %lld\n", t.c_str(), mine, (long long)got, theirs, want); }
}

std::string digits(Rng& r, int n, bool first_nonzero) {
    std::string s;
    for (int i = 0; i < n; i++) s.push_back((char)('0' + (i == 0 && first_nonzero ? 1 + r.below(9) : r.below(10))));
    return s;
}

}  // namespace

// counts[0..4] = tokens, tokens handed to the host, integers of up to 19 digits among them, of those handed to the host, mismatches.  Returns the mismatches.
extern "C" int64_t harness_od_selfcheck(int64_t n_random, uint64_t seed, int64_t* counts) {
    setlocale(LC_ALL, "C");
    Tally w, id;
    // ---- the fixed list
    const char* good[] = {"9007199254740993", "9007199254740995", "9007199254740992", "9007199254740994", "9007199254740997", "18014398509481985", "18014398509481986",
                          "1.7976931348623157e308", "1.7976931348623158e308", "1.7976931348623159e308", "1e309", "1e308", "179769313486231580793728971405303415079934132710037826936173778980444968292764750946649017977587207096330286416692887910946555547851940402630657488671505820681908902000708383676273854845817711531764475730270069855571366959622842914819860834936475292719074168444365510704342711559699508093042880177904174497791",
                          "179769313486231580793728971405303415079934132710037826936173778980444968292764750946649017977587207096330286416692887910946555547851940402630657488671505820681908902000708383676273854845817711531764475730270069855571366959622842914819860834936475292719074168444365510704342711559699508093042880177904174497792",
                          "4.9406564584124654e-324", "2e-324", "1e-400", "2.4703282292062327e-324", "2.4703282292062328e-324", "2.5e-324", "1e-323", "1e-324", "9.9e-324", "2.2250738585072014e-308", "2.2250738585072011e-308",
                          "2.225073858507201136057409796709131975934819546351645648023426109724822222021076945516529523908135087914149158913039621106870086438694594645527657207407820621743379988141063267329253552286881372149012981122451451889849057222307285255133155755015914397476397983411801999323962548289017107081850690630666655994938275772572015763062690663332647565300009245888316433037779791869612049497390377829704905051080609940730262937128958950003583799967207254304360284078895771796150945516748243471030702609144621572289880258182545180325707018860872113128079512233426288368622321503775666622503982534335974568884423900265498198385487948292206894721689831099698365846814022854243330660339850886445804001034933970427567186443383770486037861622771738545623065874679014086723327636718751234567890123456789012345678901234567890e-308",
                          "-0", "0", "+0.0", "-0e10", "5.", ".5", "+1", "1E5", "000.0001", "0e999999", "-0e-999999", "1e-9999", "1e9999", "3", "3.0", "2.5e1", "1e-3", "12345678901234567", "1234567890123456789012345",
                          "9999999999999999999", "1000000000000000000", "0.1", "0.3", "1e22", "1e23", "8.5e22", "123456789012345678e-54", "1e-54", "1e-55", "9999999999999999999e27", "1e28",
                          "inf", "-Infinity", "+INF", "nan", "-NaN", "0.500000000000000166533453693773481063544750213623046875", "1.00000000000000011102230246251565404236316680908203125",
                          "1.00000000000000011102230246251565404236316680908203124", "1.00000000000000011102230246251565404236316680908203126", "007", "7.0", "+7"};
    for (const char* t : good) check_weight(t, false, w);
    const char* bad[] = {"1e", ".", "0x10", "nan(1)", "0x1p3", "1e+", "+", "-", "", "1.0f", "1,5", "--1", "e5", ".e5", "1..2", "infinit", "nanx", "12a", "1_000", "1d5"};
    for (const char* t : bad) check_bad_weight(t, w);
    for (int k = 0; k < 4; k++) {                       // 800-digit tokens
        std::string t(800, (char)('1' + 2 * k));
        check_weight(t, false, w);
        check_weight("0." + t, false, w);
        check_weight("1." + t + "e-3", false, w);
        check_weight(t + "e-780", false, w);
        check_weight(t + "e-1100", false, w);
        check_id(t, id);
    }
    const char* ids[] = {"9223372036854775807", "9223372036854775808", "-9223372036854775808", "-9223372036854775809", "+9223372036854775807", "+9223372036854775808",
                         "0009223372036854775807", "00000000000000000000000000000007", "18446744073709551616", "18446744073709551623", "99999999999999999999", "+7", "007", "7", "-7", "0", "-0", "+0",
                         "7.0", "7.", "7e0", "", "+", "-", "+-7", "7a", "a7", "0x7", " 7", "7 ", "1099511627776", "-10100", "980100"};
    for (const char* t : ids) check_id(t, id);
    // ---- seeded random tokens: integers of 1 to 19 digits, decimals, exponents
    Rng r{seed};
    const char* signs[] = {"", "", "", "-", "+"};
    for (int64_t i = 0; i < n_random; i++) {
        const int kind = (int)r.below(4);
        const int nd = 1 + (int)r.below(19);
        std::string t = signs[r.below(5)];
        if (kind <= 1) {                                 // an integer of nd digits (leading zeros now and then)
            if (r.below(16) == 0) t += "00";
            t += digits(r, nd, true);
            check_weight(t, true, w);
            if (r.below(4) == 0) check_id(t, id);
        } else if (kind == 2) {                          // the point somewhere among the digits
            const std::string d = digits(r, nd, false);
            const size_t at = (size_t)r.below((uint64_t)nd + 1);
            t += d.substr(0, at) + "." + d.substr(at);
            check_weight(t, false, w);
        } else {                                         // digits and an exponent over the whole range of the format and beyond
            t += digits(r, nd, true);
            if (r.below(2)) t.insert(t.size() - (size_t)r.below((uint64_t)nd), ".");
            t += r.below(2) ? "e" : "E";
            t += std::to_string((int)r.below(700) - 350);
            check_weight(t, false, w);
        }
    }
    for (int i = 0; i < 20000; i++) {                    // ids around the ends of the range
        std::string t = r.below(2) ? "-" : "";
        t += std::to_string(9223372036854775807ull - 1000 + r.below(2000));
        check_id(t, id);
    }
    if (w.integers_host) { fprintf(stderr, "%lld integers of up to 19 digits were handed to the host\n", (long long)w.integers_host); w.wrong += w.integers_host; }
    if (counts) { counts[0] = w.tokens + id.tokens; counts[1] = w.host; counts[2] = w.integers; counts[3] = w.integers_host; counts[4] = w.wrong + id.wrong; }
    return w.wrong + id.wrong;
}

int main(int argc, char** argv) {
    const int64_t n = argc > 1 ? atoll(argv[1]) : 1000000;
    const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 20251018ull;
    int64_t c[5] = {0, 0, 0, 0, 0};
    const int64_t wrong = harness_od_selfcheck(n, seed, c);
    printf("tokens %lld host %lld integers %lld integers_host %lld wrong %lld\n", (long long)c[0], (long long)c[1], (long long)c[2], (long long)c[3], (long long)c[4]);
    return wrong ? 1 : 0;
}
