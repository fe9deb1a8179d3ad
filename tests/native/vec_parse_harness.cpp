// Host build of embedding_amd/csrc/vec_parse.h (the per-lane routine of k_vec_parse, vec_read.hip) for tests/test_vec_parse_host.py:
//   g++ -O2 -shared -fPIC -std=c++17 -o libvec_parse_harness.so vec_parse_harness.cpp
// tokens come as one blob, token k at blob + off[k] with off[k + 1] - off[k] bytes (no separators).
#include "../../embedding_amd/csrc/vec_parse.h"

extern "C" void harness_vec_parse(const uint8_t* blob, const int64_t* off, int64_t n, uint32_t* bits, uint8_t* status) {
    for (int64_t k = 0; k < n; k++) {
        uint32_t b = 0;
        status[k] = (uint8_t)vec_parse_f32(blob + off[k], off[k + 1] - off[k], &b);
        bits[k] = b;
    }
}
