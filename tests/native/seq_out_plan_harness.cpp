// Host build of embedding_amd/csrc/seq_out_plan.h (the .seq writer's planning: tile and slab sizes, the slabs of a text, decimals without floating point)
// for tests/test_seq_write_abi.py, the way seq_plan_harness.cpp serves seq_plan.h.
//   seq_out_plan_harness sizes           tile, slab: what tests/test_gpu_seq_write.py aims its line lengths at
//   seq_out_plan_harness slabs TOTAL     the bytes of one device buffer, then "begin end tiles" of every slab, one per line
//   seq_out_plan_harness decimal V...    digits and spelling of every V
#include <cstdlib>
#include <iostream>
#include <string>

#include "../../embedding_amd/csrc/seq_out_plan.h"

int main(int argc, char** argv) {
    if (argc < 2) { std::cerr << "usage: seq_out_plan_harness sizes | slabs TOTAL | decimal V...\n"; return 2; }
    const std::string cmd = argv[1];
    if (cmd == "sizes") {
        std::cout << SEQ_OUT_TILE << " " << SEQ_OUT_SLAB << "\n";
        return 0;
    }
    if (cmd == "slabs" && argc == 3) {
        const int64_t total = std::atoll(argv[2]);
        std::cout << seq_out_buffer_bytes(total) << "\n";
        for (int64_t s = 0; s < seq_out_slab_count(total); s++) {
            const int64_t b = seq_out_slab_begin(s), e = seq_out_slab_end(total, s);
            std::cout << b << " " << e << " " << seq_out_tiles(e - b) << "\n";
        }
        return 0;
    }
    if (cmd == "decimal" && argc >= 3) {
        for (int i = 2; i < argc; i++) {
            const uint32_t v = (uint32_t)std::strtoul(argv[i], nullptr, 10);
            const int nd = seq_out_digits(v);
            std::cout << nd << " ";
            for (int q = 0; q < nd; q++) std::cout << (char)seq_out_digit(v, nd, q);
            std::cout << "\n";
        }
        return 0;
    }
    std::cerr << "bad arguments\n";
    return 2;
}
