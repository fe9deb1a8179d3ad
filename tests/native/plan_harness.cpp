// Test-only host build of embedding_amd/csrc/sgns_plan.h: runs schedule_stats + plan_train over a list of cases and prints one JSON line per
// case, so that tests/test_train_plan.py can check the launch schedule against tests/golden/train_plans.json without a GPU.
//
//   plan_harness CASES
//   CASES: text, one record a line —
//     vocab <name> <path>        counts of a vocabulary (int64, little-endian, descending)
//     case <id> <vocab> <dim> <use_hs> <update_policy> <workers> <part_n> <L> <n_rows> <window> <negative> <n_runs> <n_knobs> [<knob> <value>]...
#include "../../embedding_amd/csrc/dge_algos.h"
#include "../../embedding_amd/csrc/sgns_plan.h"

#include <fstream>
#include <iostream>
#include <map>
#include <sstream>

struct Vocab {
    std::vector<int64_t> counts;
    ScheduleStats stats;
    BlockHeadMemo memo;       // one per vocabulary, as one per model
};

static const char* form_name(TrainForm f) {
    switch (f) {
        case TrainForm::Sorted: return "sorted";
        case TrainForm::InOrder: return "in_order";
        case TrainForm::RowRmw: return "row_rmw";
        case TrainForm::Atomics: return "atomics";
        case TrainForm::SmallRows: return "small_rows";
        case TrainForm::Locked: return "locked";
        default: return "hs_centre";
    }
}

static std::string quoted(const std::string& s) {
    std::string o = "\"";
    for (char c : s) {
        if (c == '"' || c == '\\') o += '\\';
        o += c;
    }
    return o + "\"";
}

int main(int argc, char** argv) {
    if (argc != 2) { std::cerr << "usage: plan_harness CASES\n"; return 2; }
    std::ifstream in(argv[1]);
    std::map<std::string, Vocab> vocabs;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string kind;
        if (!(ls >> kind)) continue;
        if (kind == "vocab") {
            std::string name, path;
            ls >> name >> path;
            std::ifstream f(path, std::ios::binary | std::ios::ate);
            Vocab& v = vocabs[name];
            v.counts.resize((size_t)f.tellg() / sizeof(int64_t));
            f.seekg(0);
            f.read((char*)v.counts.data(), (std::streamsize)(v.counts.size() * sizeof(int64_t)));
            const int64_t V = (int64_t)v.counts.size();
            v.stats = schedule_stats(v.counts.data(), V, 0, 0, 256);
            std::vector<int64_t> off, node_w; std::vector<int32_t> points; std::vector<uint64_t> codes;
            dge_huffman_paths(v.counts.data(), V, off, points, codes, &node_w);
            schedule_stats_hs(v.stats, node_w);
            continue;
        }
        std::string id, vname;
        dge_train_config cfg{};
        int32_t part_n, L, n_runs, n_knobs;
        int64_t n_rows;
        ls >> id >> vname >> cfg.dim >> cfg.use_hs >> cfg.update_policy >> cfg.workers >> part_n >> L >> n_rows >> cfg.window >> cfg.negative >> n_runs >> n_knobs;
        int64_t knob[DGE_TUNE_COUNT];
        for (int k = 0; k < DGE_TUNE_COUNT; k++) knob[k] = -1;
        for (int k = 0; k < n_knobs; k++) { int i; int64_t val; ls >> i >> val; knob[i] = val; }
        Vocab& v = vocabs.at(vname);
        ScheduleStats s = v.stats;
        s.D = cfg.dim; s.stride = (cfg.dim + 63) / 64 * 64;
        TrainPlan P;
        const int rc = plan_train(cfg, s, v.counts.data(), part_n, n_rows, L, knob, v.memo, &P);
        std::ostringstream o;
        o << "{\"id\": " << quoted(id) << ", \"rc\": " << rc;
        if (rc) o << ", \"error\": " << quoted(P.error);
        else {
            o << ", \"form\": \"" << form_name(P.form) << "\", \"hs\": " << P.hs << ", \"part\": " << P.part << ", \"strict\": " << P.strict << ", \"hotmix\": " << P.hotmix
              << ", \"wdog\": " << P.wdog << ", \"nlock\": " << P.nlock << ", \"head\": " << P.head << ", \"waves\": " << P.waves << ", \"big\": " << P.big
              << ", \"workers\": " << P.workers << ", \"blocks\": " << P.blocks << ", \"threads\": " << P.threads << ", \"shmem\": " << P.shmem
              << ", \"hot_rows\": " << P.hot_rows << ", \"acc_rows\": " << P.acc_rows << ", \"acc_drain\": " << P.acc_drain << ", \"syn0_free\": " << P.syn0_free
              << ", \"hs_hot0\": " << P.hs_hot0 << ", \"hs_n_hot\": " << P.hs_n_hot << ", \"hs_drain\": " << P.hs_drain << ", \"hs_cold\": " << P.hs_cold
              << ", \"hs_wave\": " << P.hs_wave << ", \"hs_rep0\": " << P.hs_rep0 << ", \"hs_rep_n\": " << P.hs_rep_n << ", \"hs_rep_thr\": [";
            for (int k = 0; k < HS_REP; k++) o << (k ? ", " : "") << P.hs_rep_thr[k];
            o << "], \"wd_ticks\": " << P.wd_ticks << ", \"n_runs\": " << ((knob[DGE_TUNE_TABLE_RUNS] == 0 || P.runs_off) ? 0 : n_runs)
              << ", \"walk_counter\": " << P.walk_counter << ", \"policy\": " << P.reported_policy() << ", \"kernel\": " << quoted(P.kernel_name());
        }
        std::cout << o.str() << "}\n";
    }
    return 0;
}
