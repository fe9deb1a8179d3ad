// The C++ mirror's held-out figure: DeepWalk::learnEmbedding(..., heldOutFiles, &result) trains on one .seq file and evaluates the trained model on
// another before it is freed (embedding_amd/host/embedding_host.hpp: evalSgns over dge_model_eval_sgns).  Run by tests/test_gpu_eval.py.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>

#include "../../embedding_amd/host/embedding_host.hpp"

using namespace embedding;

// sentences that walk a ring of `n` names in steps of 1 or 2: neighbours on the ring co-occur, nothing else does
static void write_seq(const std::string& path, int sentences, int n, unsigned seed, bool with_unknown) {
    std::ofstream out(path);
    unsigned s = seed;
    for (int i = 0; i < sentences; i++) {
        s = s * 1664525u + 1013904223u;
        int v = (int)((s >> 8) % (unsigned)n);
        for (int j = 0; j < 8; j++) {
            out << (j ? " " : "") << "0-" << v;
            s = s * 1664525u + 1013904223u;
            v = (v + 1 + (int)((s >> 16) & 1u)) % n;
        }
        if (with_unknown && i % 7 == 0) out << " never-seen-" << i;
        out << "\n";
    }
}

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : ".";
    write_seq(dir + "/train.seq", 6000, 50, 1u, false);
    write_seq(dir + "/held.seq", 500, 50, 77u, true);
    LayeredGraph::numLayer = 4;
    DeepWalk::useHierarchicSoftmax = false;
    dge_eval_result r{};
    const dge_train_stats st = DeepWalk::learnEmbedding({dir + "/train.seq"}, dir + "/out.vec", 20, 0, 0, 1, {dir + "/held.seq"}, &r);
    std::printf("trained %lld pairs; held-out: %lld pairs, %lld negatives, %lld skipped, loss %.4f, auc %.4f\n", (long long)st.pairs, (long long)r.pairs,
                (long long)r.negatives, (long long)r.skipped, r.loss, r.auc);
    // 500 sentences of 8 known names, window 4: 2 * (7 + 6 + 5 + 4) = 44 pairs each; the unknown names are dropped
    if (r.pairs != 500 * 44 || r.negatives + r.skipped != 5 * r.pairs) { std::printf("FAIL: counts\n"); return 1; }
    // an untrained model scores 0 everywhere: loss 6 ln 2, auc 1/2
    if (!(r.loss < 6.0 * std::log(2.0)) || !(r.auc > 0.5)) { std::printf("FAIL: the trained model is no better than an untrained one\n"); return 1; }
    std::printf("HOST EVAL OK\n");
    return 0;
}
