// SpatialGraph::constructGraph of the C++ host mirror (embedding_amd/host/embedding_host.hpp) in its two forms on a 12-region fixture: the n x n weight matrix
// (filled here with the rule's own weight, csrc/spatial_weight.h; k = 10 as the reference's) and the centroids handed to the device
// (dge_graph_add_spatial_points).  Prints edgesOut, outDegree and sourceWeightSum of both as hex floats; tests/test_gpu_spatial.py compares the two listings.
// Needs a GPU.  Build with -ffp-contract=off.
#include <cstdio>

#include "../../embedding_amd/csrc/spatial_weight.h"
#include "../../embedding_amd/host/embedding_host.hpp"
using namespace embedding;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static void print(SpatialGraph& g, const std::vector<std::string>& names) {
    for (const std::string& n : names) {
        const LayeredGraph::Vertex* v = g.allVertices.at(n);
        std::printf("%s od %a:", v->name.c_str(), v->outDegree);
        for (const LayeredGraph::Edge& e : v->edgesOut) std::printf(" %s %a", e.to->name.c_str(), e.weight);
        std::printf("\n");
    }
    std::printf("sourceWeightSum %a sources %zu\n", g.sourceWeightSum, g.sourceVertices.size());
}

int main() {
    const int n = 12;
    std::vector<int64_t> ids;
    std::vector<double> xy;
    std::vector<std::string> names;
    for (int i = 0; i < n; i++) {                         // a 4 x 3 block of tract-sized cells, two of them on one spot
        ids.push_back(17031000100LL + 7 * i);
        names.push_back(std::to_string(ids.back()));
        xy.push_back(-87.7 + 0.011 * (i % 4) + 0.0003 * i);
        xy.push_back(41.8 + 0.013 * (i / 4));
    }
    xy[2 * 9] = xy[2 * 3]; xy[2 * 9 + 1] = xy[2 * 3 + 1];
    std::vector<double> W((size_t)n * n);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) W[(size_t)i * n + j] = sw_weight(sw_dist2(xy[2 * i], xy[2 * i + 1], xy[2 * j], xy[2 * j + 1]), 100.0);
    SpatialGraph a, b;
    SpatialGraph::constructGraph(a, names, W);
    SpatialGraph::constructGraph(b, ids, xy);
    std::printf("== matrix overload\n");
    print(a, names);
    std::printf("== points overload\n");
    print(b, names);
    CHECK(a.sourceWeightSum == b.sourceWeightSum && b.sourceVertices.size() == (size_t)n && b.allVertices.size() == (size_t)n);
    for (int i = 0; i < n; i++) {
        const LayeredGraph::Vertex *va = a.allVertices.at(names[i]), *vb = b.allVertices.at(names[i]);
        CHECK(va->id == vb->id && vb->id == i && va->outDegree == vb->outDegree && va->edgesOut.size() == 10 && vb->edgesOut.size() == 10);
        CHECK(va->probTable == vb->probTable && va->aliasTable == vb->aliasTable);
        for (int e = 0; e < 10; e++) CHECK(va->edgesOut[e].to->name == vb->edgesOut[e].to->name && va->edgesOut[e].weight == vb->edgesOut[e].weight);
    }
    CHECK(a.probTable == b.probTable && a.aliasTable == b.aliasTable);
    LayeredGraph::rnd = Random(42);
    const std::vector<int32_t> wa = a.sampleVertexSequences(200);
    LayeredGraph::rnd = Random(42);
    CHECK(wa == b.sampleVertexSequences(200));
    SpatialGraph c;
    bool threw = false;
    try { SpatialGraph::constructGraph(c, ids, xy, 13); } catch (const std::out_of_range&) { threw = true; }
    CHECK(threw);
    std::printf("HOST SPATIAL OK\n");
    return 0;
}
