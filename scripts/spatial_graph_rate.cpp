// One leg of scripts/spatial_graph_rate.py: wall time from R centroids in host memory to a graph ready for dge_graph_build_alias.
//   old   a one-thread double loop shaped like J/SpatialGraph.java:43-49 fills the R x R matrix with the rule's weight (csrc/spatial_weight.h), then
//         dge_graph_add_edges of the R^2 edges, dge_graph_keep_top_k(k), dge_graph_set_sources(0 .. R-1, 1) — the path before dge_graph_add_spatial_points;
//   new   dge_graph_add_spatial_points.
// usage: spatial_graph_rate <old|new> R k runs   -> one line: seconds of every run after a warm-up.  Build with -ffp-contract=off.
// A size the path cannot hold — a DGE error such as DGE_ERR_CAP, or host memory for the matrix — is a line "FAILED <what> rc <n>: ..." and exit status 1, nothing
// else: the script takes only that as "cannot hold" and stops at any other status.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../embedding_amd/csrc/spatial_weight.h"
#include "../include/dge.h"

// exit status 1 only for a size that does not fit (DGE_ERR_CAP, or the device allocator out of memory); any other error is status 3
static int fail(const char* what, int rc) {
    const bool no_room = rc == DGE_ERR_CAP || strstr(dge_last_error(), "hipErrorOutOfMemory") != nullptr;
    std::printf("\n%s %s rc %d: %s\n", no_room ? "FAILED" : "ERROR", what, rc, dge_last_error());
    return no_room ? 1 : 3;
}

static int run(int argc, char** argv) {
    if (argc < 5) return 2;
    const bool old_path = !strcmp(argv[1], "old");
    const int64_t R = atoll(argv[2]);
    const int k = atoi(argv[3]), runs = atoi(argv[4]);
    std::vector<int64_t> ids((size_t)R);
    std::vector<double> xy((size_t)(2 * R));
    uint64_t s = 20261018;
    auto next = [&]() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(s >> 11) * 0x1.0p-53; };
    for (int64_t r = 0; r < R; r++) { ids[(size_t)r] = 17031000000LL + r; xy[(size_t)(2 * r)] = -87.9 + 0.4 * next(); xy[(size_t)(2 * r + 1)] = 41.6 + 0.4 * next(); }
    std::printf("%s R %lld k %d seconds", argv[1], (long long)R, k);
    for (int run = 0; run <= runs; run++) {
        dge_graph* g = nullptr;
        int rc = dge_graph_create(&g, 0);
        if (rc) return fail("dge_graph_create", rc);
        dge_spatial_info info{};
        const auto t0 = std::chrono::steady_clock::now();
        if (old_path) {
            std::vector<int32_t> src((size_t)(R * R)), dst((size_t)(R * R));
            std::vector<double> w((size_t)(R * R));
            for (int64_t i = 0; i < R; i++)
                for (int64_t j = 0; j < R; j++) {
                    const size_t e = (size_t)(i * R + j);
                    src[e] = (int32_t)i; dst[e] = (int32_t)j;
                    w[e] = sw_weight(sw_dist2(xy[(size_t)(2 * i)], xy[(size_t)(2 * i + 1)], xy[(size_t)(2 * j)], xy[(size_t)(2 * j + 1)]), 100.0);
                }
            std::vector<int32_t> sv((size_t)R);
            for (int64_t i = 0; i < R; i++) sv[(size_t)i] = (int32_t)i;
            if ((rc = dge_graph_add_edges(g, src.data(), dst.data(), w.data(), R * R))) return fail("dge_graph_add_edges", rc);
            if ((rc = dge_graph_keep_top_k(g, k))) return fail("dge_graph_keep_top_k", rc);
            if ((rc = dge_graph_set_sources(g, sv.data(), R, 1))) return fail("dge_graph_set_sources", rc);
        } else if ((rc = dge_graph_add_spatial_points(g, ids.data(), xy.data(), R, k, 100.0, nullptr, &info))) return fail("dge_graph_add_spatial_points", rc);
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        dge_graph_free(g);
        if (run) std::printf(" %.6f", sec);
        if (run == runs && !old_path) std::printf(" kernel_ms %.3f weights %lld", info.kernel_ms, (long long)info.weights);
    }
    std::printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    try { return run(argc, argv); }
    catch (const std::bad_alloc&) { std::printf("\nFAILED host memory rc %d: the R x R matrix does not fit in host memory\n", DGE_ERR_CAP); return 1; }
}
