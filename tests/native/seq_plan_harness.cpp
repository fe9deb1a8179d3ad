// Host build of embedding_amd/csrc/seq_plan.h (the .seq ingest's planning: whitespace class, buffer layout, pad bytes, name-table growth) for
// tests/test_seq_abi.py, the way plan_harness.cpp serves sgns_plan.h.
//   seq_plan_harness space                    the 256 bytes' whitespace class, one digit each
//   seq_plan_harness layout PREFIX SIZE...    offsets, used, padded, text_bytes
//   seq_plan_harness join OUT NAME... -- FILE...   the buffer the kernels would read — every NAME on a line of its own, then every FILE with its pad byte,
//                                                  blanks up to `padded` — written to OUT
//   seq_plan_harness slots TOKENS INITIAL     the table sizes tried, first to last
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>

#include "../../embedding_amd/csrc/seq_plan.h"

int main(int argc, char** argv) {
    if (argc < 2) { std::cerr << "usage: seq_plan_harness space | layout | join | slots\n"; return 2; }
    const std::string cmd = argv[1];
    if (cmd == "space") {
        for (int c = 0; c < 256; c++) std::cout << (seq_is_space((uint32_t)c) ? '1' : '0');
        std::cout << "\n";
        return 0;
    }
    if (cmd == "layout" && argc >= 3) {
        std::vector<int64_t> sizes;
        for (int i = 3; i < argc; i++) sizes.push_back(std::atoll(argv[i]));
        seq_layout L;
        if (!seq_plan_layout(std::atoll(argv[2]), sizes.data(), (int64_t)sizes.size(), &L)) { std::cout << "refused\n"; return 0; }
        for (int64_t o : L.offset) std::cout << o << " ";
        std::cout << "| " << L.used << " " << L.padded << " " << L.text_bytes << "\n";
        return 0;
    }
    if (cmd == "join" && argc >= 3) {
        std::string prefix;
        int i = 3;
        for (; i < argc && std::strcmp(argv[i], "--") != 0; i++) { prefix += argv[i]; prefix += '\n'; }
        std::vector<std::string> data;
        for (i++; i < argc; i++) {
            std::ifstream in(argv[i], std::ios::binary);
            if (!in) { std::cerr << "cannot open " << argv[i] << "\n"; return 2; }
            data.emplace_back(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
        }
        std::vector<int64_t> sizes;
        for (const std::string& d : data) sizes.push_back((int64_t)d.size());
        seq_layout L;
        if (!seq_plan_layout((int64_t)prefix.size(), sizes.data(), (int64_t)sizes.size(), &L)) return 3;
        std::string buf((size_t)L.padded, ' ');
        buf.replace(0, prefix.size(), prefix);
        for (size_t k = 0; k < data.size(); k++) {
            buf.replace((size_t)L.offset[k], data[k].size(), data[k]);
            buf[(size_t)L.offset[k] + data[k].size()] = (char)seq_pad_byte(sizes[k], data[k].empty() ? 0 : (uint8_t)data[k].back());
        }
        std::ofstream out(argv[2], std::ios::binary);
        out.write(buf.data(), (std::streamsize)buf.size());
        std::cout << L.used << " " << L.padded << " " << L.text_bytes << "\n";
        return 0;
    }
    if (cmd == "slots" && argc == 4) {
        const int64_t tokens = std::atoll(argv[2]);
        int64_t s = seq_slots_first(tokens, std::atoll(argv[3]));
        std::cout << s;
        while (s < seq_slots_cap(tokens)) { s = seq_slots_next(s, tokens); std::cout << " " << s; }
        std::cout << "\n";
        return 0;
    }
    std::cerr << "bad arguments\n";
    return 2;
}
