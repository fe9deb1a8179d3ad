// CrossTimeGraph::outputSampleSequence and SpatialGraph::outputSampleSequence format their lines on the device (dge_sample_walks_device + dge_walks_write_seq,
// chunk after chunk); this program holds them to the host loop they replaced, restated below: from the same seed the file's bytes and the position of
// LayeredGraph::rnd afterwards must be the same.  numSamples crosses the writer's chunk of 2^18 walks once.  Needs a GPU: built and run by
// tests/test_gpu_host_mirror_seq_write.py.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iterator>

#include "../../embedding_amd/host/embedding_host.hpp"
using namespace embedding;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static std::string slurp(const std::string& p) {
    std::ifstream in(p, std::ios::binary);
    return std::string(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
}

// the writer loop as the mirror ran it on the host: walks to the host chunk by chunk, a std::string per line, an ofstream
static void writeSeqHost(LayeredGraph& g, const std::string& path, int64_t n, bool positionPrefix) {
    std::ofstream out(path);
    if (!out) throw std::runtime_error("cannot open " + path);
    const int L = LayeredGraph::numLayer;
    const int64_t chunk = 1 << 18;
    for (int64_t done = 0; done < n; done += chunk) {
        int64_t m = std::min(chunk, n - done);
        std::vector<int32_t> w = g.sampleVertexSequences(m);
        std::string line;
        for (int64_t i = 0; i < m; i++) {
            line.clear();
            for (int j = 0; j < L && w[(size_t)i * L + j] >= 0; j++) {
                if (j) line += ' ';
                if (positionPrefix) { line += std::to_string(j); line += '-'; }
                line += g.nameOfDeviceId(w[(size_t)i * L + j]);
            }
            line += '\n';
            out << line;
        }
    }
}

int main(int argc, char** argv) {
    const std::string tmp = argc > 1 ? argv[1] : ".";
    const int64_t N = ((int64_t)1 << 18) + 1500;
    {   // cross-time: 4 slices x 7 regions; region 103 of slice 2 has no out-flow, so the walks that reach it end there (a short line)
        CrossTimeGraph::numLayer = 4; CrossTimeGraph::numSamples = N;
        std::vector<Flow> flows; std::vector<int> regions;
        for (int r = 0; r < 7; r++) regions.push_back(100 + r);
        for (int h = 0; h < 4; h++)
            for (int s = 0; s < 7; s++)
                for (int d = 0; d < 7; d++)
                    if (!(h == 2 && s == 3)) flows.push_back({h, 100 + s, 100 + d, (double)(1 + (s * 7 + d * 3 + h) % 5)});
        CrossTimeGraph g;
        CrossTimeGraph::constructGraph(g, flows, regions);
        LayeredGraph::rnd = Random(2017);
        CrossTimeGraph::outputSampleSequence(g, tmp + "/device-crosstime.seq");
        const int64_t draws = LayeredGraph::rnd.draws();
        LayeredGraph::rnd = Random(2017);
        writeSeqHost(g, tmp + "/host-crosstime.seq", N, false);
        CHECK(LayeredGraph::rnd.draws() == draws && draws < N * 4 && draws > N * 3);       // the same stream position; some walks were short
        const std::string a = slurp(tmp + "/device-crosstime.seq"), b = slurp(tmp + "/host-crosstime.seq");
        CHECK(!a.empty() && a == b);
        CHECK((int64_t)std::count(a.begin(), a.end(), '\n') == N);
        // a second file over the first: truncated, not appended to
        CrossTimeGraph::numSamples = 10;
        LayeredGraph::rnd = Random(2017);
        CrossTimeGraph::outputSampleSequence(g, tmp + "/device-crosstime.seq");
        const std::string c = slurp(tmp + "/device-crosstime.seq");
        CHECK(std::count(c.begin(), c.end(), '\n') == 10 && a.compare(0, c.size(), c) == 0);
        CrossTimeGraph::numSamples = 0;
        CrossTimeGraph::outputSampleSequence(g, tmp + "/device-crosstime.seq");
        CHECK(slurp(tmp + "/device-crosstime.seq").empty());
    }
    {   // spatial: the "j-" prefix, top-10 prune
        SpatialGraph::numLayer = 3; SpatialGraph::numSamples = N;
        std::vector<std::string> names; std::vector<double> wt;
        const int n = 12;
        for (int i = 0; i < n; i++) names.push_back(std::to_string(100 + i));
        for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) wt.push_back(std::exp(-100.0 * std::fabs(i - j) * 0.004));
        SpatialGraph g;
        SpatialGraph::constructGraph(g, names, wt);
        LayeredGraph::rnd = Random(7);
        SpatialGraph::outputSampleSequence(g, tmp + "/device-spatial.seq");
        const int64_t draws = LayeredGraph::rnd.draws();
        LayeredGraph::rnd = Random(7);
        writeSeqHost(g, tmp + "/host-spatial.seq", N, true);
        CHECK(LayeredGraph::rnd.draws() == draws && draws == N * 3);
        const std::string a = slurp(tmp + "/device-spatial.seq"), b = slurp(tmp + "/host-spatial.seq");
        CHECK(!a.empty() && a == b && a.compare(0, 2, "0-") == 0);
    }
    std::printf("HOST SEQ WRITE OK\n");
    return 0;
}
