// DeepWalk::learnEmbedding reads its .seq files through the device ingest (dge_walks_from_seq_files) and trains where the corpus lies; this program holds it to
// what the host reader gave: readSentencesHost + dge_train_sgns + dge_write_vec on the same two files at workers = 1 must write the same .vec bytes, and the
// held-out figures must be the same in every integer and in the bits of auc and loss.  Needs a GPU: built and run by tests/test_gpu_host_mirror_seq.py.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <random>

#include "../../embedding_amd/host/embedding_host.hpp"
using namespace embedding;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static std::string slurp(const std::string& p) {
    std::ifstream in(p, std::ios::binary);
    return std::string(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
}

// what learnEmbedding did before the ingest existed, member for member
static dge_train_stats learnEmbeddingHost(const std::vector<std::string>& seqFiles, const std::string& outVec, int layerSize, int device, int workers, uint64_t seed,
                                          const std::vector<std::string>& heldOutFiles, dge_eval_result* heldOut) {
    std::unordered_map<std::string, int> ids;
    std::vector<std::string> names;
    std::vector<int32_t> walks;
    size_t maxLen = 1;
    const size_t nRows = DeepWalk::readSentencesHost(seqFiles, true, ids, names, walks, maxLen);
    dge_train_config cfg{};
    cfg.dim = layerSize; cfg.window = LayeredGraph::numLayer; cfg.negative = 5; cfg.min_count = 2; cfg.epochs = 1; cfg.workers = workers;
    cfg.alpha = 0.025f; cfg.min_alpha = 1e-4f; cfg.seed = seed; cfg.table_size = 0;
    cfg.n_vertices = (int32_t)std::max<size_t>(names.size(), 1);
    cfg.use_hs = DeepWalk::useHierarchicSoftmax ? 1 : 0;
    dge_model* m = nullptr;
    dge_check(dge_train_sgns(device, walks.data(), (int64_t)nRows, (int32_t)maxLen, &cfg, &m));
    std::vector<const char*> cn(names.size());
    for (size_t i = 0; i < names.size(); i++) cn[i] = names[i].c_str();
    dge_check(dge_write_vec(m, cn.data(), outVec.c_str(), 0));
    dge_train_stats st{};
    dge_check(dge_model_stats(m, &st));
    if (heldOut) {
        std::vector<int32_t> held;
        size_t heldLen = 1;
        const size_t nHeld = DeepWalk::readSentencesHost(heldOutFiles, false, ids, names, held, heldLen);
        dge_walks* hw = nullptr;
        dge_check(dge_walks_from_host(device, held.data(), (int64_t)nHeld, (int32_t)heldLen, &hw));
        *heldOut = DeepWalk::evalSgns(m, hw);
        dge_walks_free(hw);
    }
    dge_model_free(m);
    return st;
}

int main(int argc, char** argv) {
    const std::string tmp = argc > 1 ? argv[1] : "/tmp";
    const int T = 6, R = 40;
    LayeredGraph::numLayer = T;
    std::mt19937_64 rng(2017);
    auto walk = [&](int firstRegion, int regions) {
        std::string line;
        int r = firstRegion + (int)(rng() % (uint64_t)regions);
        for (int h = 0; h < T; h++) {
            if (h) line += ' ';
            line += std::to_string(h) + "-" + std::to_string(17031000 + r);
            r = firstRegion + (r - firstRegion + 1 + (int)(rng() % 3)) % regions;
        }
        return line;
    };
    const std::string a = tmp + "/train-a.seq", b = tmp + "/train-b.seq", held = tmp + "/held.seq", held2 = tmp + "/held-2.seq";
    {   // two training files: the first ends without a newline, the second has CRLF lines, blank lines and ragged blanks
        std::ofstream fa(a, std::ios::binary), fb(b, std::ios::binary), fh(held, std::ios::binary), fh2(held2, std::ios::binary);
        for (int i = 0; i < 3000; i++) fa << walk(0, R) << (i < 2999 ? "\n" : "");
        for (int i = 0; i < 2000; i++) fb << (i % 7 == 0 ? "  " : "") << walk(0, R) << (i % 5 == 0 ? " \t\r\n" : "\n") << (i % 11 == 0 ? "\n \n" : "");
        fb << "0-17031000 1-17031001\n";                                 // a short line
        for (int i = 0; i < 500; i++) fh << walk(0, R + 10) << "\n";      // regions R .. R+9 never trained on: unknown names, -1 in place
        for (int i = 0; i < 100; i++) fh2 << walk(0, R) << (i < 99 ? "\r\n" : "");
    }
    for (int hs = 0; hs < 2; hs++) {
        DeepWalk::useHierarchicSoftmax = hs != 0;
        const std::string v1 = tmp + "/ingest" + std::to_string(hs) + ".vec", v2 = tmp + "/host" + std::to_string(hs) + ".vec";
        dge_eval_result r1{}, r2{};
        const dge_train_stats s1 = DeepWalk::learnEmbedding({a, b}, v1, 20, 0, 1, 1, {held, held2}, &r1);
        const dge_train_stats s2 = learnEmbeddingHost({a, b}, v2, 20, 0, 1, 1, {held, held2}, &r2);
        CHECK(s1.pairs == s2.pairs && s1.words == s2.words && s1.pairs > 0);
        const std::string b1 = slurp(v1), b2 = slurp(v2);
        CHECK(!b1.empty() && b1 == b2);                                    // same ids, same model, same bytes
        CHECK(r1.pairs == r2.pairs && r1.negatives == r2.negatives && r1.skipped == r2.skipped && r1.pairs > 0);
        CHECK(std::memcmp(&r1.auc, &r2.auc, sizeof(double)) == 0 && std::memcmp(&r1.loss, &r2.loss, sizeof(double)) == 0);
        std::printf("hs=%d pairs=%lld vec=%zu bytes held-out pairs=%lld auc=%.6f loss=%.6f\n", hs, (long long)s1.pairs, b1.size(), (long long)r1.pairs, r1.auc, r1.loss);
    }
    {   // the readers agree on the corpus itself, unknown names in place included
        std::unordered_map<std::string, int> ids; std::vector<std::string> names; std::vector<int32_t> w, hw; size_t L = 1, hL = 1;
        const size_t n = DeepWalk::readSentencesHost({a, b}, true, ids, names, w, L);
        const size_t hn = DeepWalk::readSentencesHost({held, held2}, false, ids, names, hw, hL);
        dge_names* nm = nullptr;
        dge_check(dge_names_create(&nm));
        dge_seq_info info{}, hinfo{};
        dge_walks* dw = DeepWalk::readSentences({a, b}, true, nm, 0, &info);
        dge_walks* dh = DeepWalk::readSentences({held, held2}, false, nm, 0, &hinfo);
        std::vector<int32_t> g((size_t)info.rows * info.max_len), hg((size_t)hinfo.rows * hinfo.max_len);
        dge_check(dge_walks_to_host(dw, g.data(), (int64_t)g.size()));
        dge_check(dge_walks_to_host(dh, hg.data(), (int64_t)hg.size()));
        CHECK((size_t)info.rows == n && (size_t)info.max_len == L && g == w);
        CHECK((size_t)hinfo.rows == hn && (size_t)hinfo.max_len == hL && hg == hw && hinfo.unknown > 0 && hinfo.names_added == 0);
        int64_t cnt = 0; const char* const* cs = nullptr;
        dge_check(dge_names_count(nm, &cnt)); dge_check(dge_names_cstrs(nm, &cs));
        CHECK((size_t)cnt == names.size());
        for (int64_t i = 0; i < cnt; i++) CHECK(names[(size_t)i] == cs[i]);
        dge_walks_free(dw); dge_walks_free(dh); dge_names_free(nm);
    }
    {   // a missing file is the library's DGE_ERR_IO with the path, as an exception
        bool threw = false;
        try { DeepWalk::learnEmbedding({a, tmp + "/no-such.seq"}, tmp + "/x.vec", 20, 0, 1); } catch (const std::runtime_error& e) { threw = std::string(e.what()).find("no-such.seq") != std::string::npos; }
        CHECK(threw);
    }
    std::printf("HOST SEQ OK\n");
    return 0;
}
