"""How long the held-out evaluation takes next to the training launch it reads behind (profiles/eval_rate.txt is this script's output).

On bench.py's cfg3 shape (WORKLOADS["cfg3"]: the graph, the epoch corpus, the vocabulary, the launch of epoch/10 walks), tables trained for one launch first:
  * dge_model_eval_sgns over the rows of one training launch, and the training launch over the same rows, in the same process — each the median of five after
    one warm-up, HIP-event time of the kernels.  The evaluation scores every pair of the FULL window, the trainer the pairs of its randomly reduced windows:
    the pairs differ, so the time per pair is printed as well;
  * dge_model_eval_links over 20 000 held-out walks next to tests/helpers.py: link_auc_device (host wall time around a device synchronisation).
Run from the repository root:  python scripts/eval_rate.py [--scale S]"""
import argparse
import importlib.util
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="scale the region count (quick checks)")
    args = ap.parse_args()
    import numpy as np
    import torch
    import embedding_amd as E
    from embedding_amd import synth
    import helpers
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
    wl = dict(bench.WORKLOADS["cfg3"])
    R, T, L, D, K = max(16, int(wl["R"] * args.scale)), wl["T"], wl["L"], wl["dim"], wl["negative"]
    NV = R * T
    dev = "cuda:0"
    G = synth.flow_graph_torch(R, T, wl["mean_degree"], dev, dst=wl.get("dst", "uniform"))
    g = E.DeviceGraph(0); g.add_edges_device(G["src"], G["dst"], G["w"]); g.set_sources(G["sources"]); del G
    g.build_alias(exact=False)
    epoch_walks = wl["walks_per_vertex"] * NV
    B = max(1, epoch_walks // 10)
    corpus = g.sample_walks_device(epoch_walks, L, seed=20171106, rng_mode=1, first_index=0)
    held = g.sample_walks_device(20_000, L, seed=99, rng_mode=1)
    counts = torch.zeros(NV, dtype=torch.int64, device=dev); corpus.count_tokens(NV, counts)
    m = E.SgnsModel.create(E.make_config(D, L, NV, negative=K, min_count=2, epochs=1000, workers=0, seed=1), counts, 0)
    print("cfg3 shape: %d vertices, D = %d, K = %d, L = W = %d; a launch = %d walks; build %s" % (NV, D, K, L, B, E.lib.dge_build_stamp().decode()))

    def train_ms():
        m.reset_stats()
        m.train(corpus, 0, B, walk_index_base=0, epoch=0, words_before=0, words_scale=1.0, total_walks=epoch_walks)
        s = m.stats()
        return s["kernel_ms"], s["pairs"]

    train_ms()                                                       # the tables are trained for one launch (and the work buffers exist)
    tr = [train_ms() for _ in range(6)][1:]
    ev = [m.eval_sgns(corpus, seed=3, row0=0, n_rows=B) for _ in range(6)][1:]
    t_ms = statistics.median(x[0] for x in tr); t_pairs = tr[0][1]
    e_ms = statistics.median(x["kernel_ms"] for x in ev); e_pairs = ev[0]["pairs"]
    print("training launch  (%s): median %.2f ms of %s, %d pairs, %.3f ns a pair" % (m.kernel(), t_ms, ["%.2f" % x[0] for x in tr], t_pairs, 1e6 * t_ms / t_pairs))
    print("dge_model_eval_sgns, same rows: median %.2f ms of %s, %d pairs (full window), %.3f ns a pair; loss %.4f auc %.4f"
          % (e_ms, ["%.2f" % x["kernel_ms"] for x in ev], e_pairs, 1e6 * e_ms / e_pairs, ev[0]["loss"], ev[0]["auc"]))
    print("evaluation / training: %.2f x in time, %.2f x in time per pair; %.0f GB/s of rows at 4 D (K + 2) bytes a pair" % (e_ms / t_ms, (e_ms / e_pairs) / (t_ms / t_pairs), 4.0 * D * (K + 2) * e_pairs / (e_ms * 1e6)))

    _, vid = m.vectors()
    tw = torch.from_numpy(held.to_host().astype(np.int64)).to(dev)
    lk = [m.eval_links(held, R, seed=3) for _ in range(6)][1:]
    wall = []
    for _ in range(6):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        auc_t, loss_t = helpers.link_auc_device(m, vid, tw, R, NV, seed=3)
        torch.cuda.synchronize(); wall.append(1e3 * (time.perf_counter() - t0))
    wall_e = []
    for _ in range(6):
        t0 = time.perf_counter(); m.eval_links(held, R, seed=3); wall_e.append(1e3 * (time.perf_counter() - t0))
    print("dge_model_eval_links, 20 000 held-out walks: %d steps, kernels median %.3f ms, the call %.3f ms of host wall time; auc %.4f loss %.4f"
          % (lk[0]["pairs"], statistics.median(x["kernel_ms"] for x in lk), statistics.median(wall_e[1:]), lk[0]["auc"], lk[0]["loss"]))
    print("helpers.link_auc_device, same walks: %.1f ms of host wall time (median of five); auc %.4f loss %.4f" % (statistics.median(wall[1:]), auc_t, loss_t))


if __name__ == "__main__":
    main()
