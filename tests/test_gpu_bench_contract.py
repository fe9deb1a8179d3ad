"""GPU: bench.py keeps its output contract — one JSON line on stdout with the metric and the roofline object, and with --full the CPU
baseline — checked on the small 'tiny' workload (the default workload is BASELINE.json's cfg3)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_emits_one_json_line_with_the_contract_fields():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "tiny", "--steps", "2", "--warmup", "1", "--cpu-seconds", "1",
                          "--full"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["metric"] == "SGNS training edges/sec" and d["unit"] == "edges/s" and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert d["value"] > 0 and "workload" in d["config"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["box_copy_GBps"] > 0 and r["row_read_GBps"] > 0 and r["row_rewrite_GBps"] > 0
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["value"] > 0 and c["cores"] >= 1 and c["unit"] == "edges/s" and c["sample"]


def test_plain_run_times_the_steps_and_dumps_the_last_steps_outputs(tmp_path, dge):
    """A plain run (no --full) prints the headline line without the figures that take runs of their own; --dump-outputs writes what the last
    timed step computed reproducibly as float .npy files within 64 MB, and a second run with the same arguments writes the same arrays bit for
    bit.  'tiny' trains under owner-computes (update_policy 8, a fixed order of the updates): the tables are written.  Under a Hogwild schedule
    (--policy 2: memory-side atomics, the order of a shared row's updates differs from run to run) they are not; the walks and the trainer's
    pair and word counts are, and they equal the owner-computes runs' (neither depends on the schedule).  The dumped walks are those of the LAST
    timed step: their indices lie in its batch, and the graph built here independently samples the same walks at those indices."""
    import numpy as np
    import torch
    from bench import WORKLOADS
    from embedding_amd import synth
    steps, warmup = 3, 1
    dumps = []
    for k, extra in enumerate(([], [], ["--policy", "2"])):
        d_out = tmp_path / ("run%d" % k)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "tiny", "--steps", str(steps), "--warmup", str(warmup),
                              "--dump-outputs", str(d_out)] + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.strip()]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert d["metric"] == "SGNS training edges/sec" and d["unit"] == "edges/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["steps"] == steps and d["warmup"] == warmup and d["value"] > 0 and d["ms_per_step"] > 0
        assert abs(d["config"]["pairs_per_step_per_gpu"] * steps / (d["ms_per_step"] * steps * 1e-3) - d["value"]) < 1e-6 * d["value"]
        assert "cpu_baseline" not in d and "box_copy_GBps" not in d["roofline"] and "row_read_GBps" not in d["roofline"]
        policy = d["roofline"]["schedule"]["update_policy"]
        assert policy == (2 if extra else 8), d["roofline"]["schedule"]
        files = sorted(p.name for p in d_out.iterdir())
        always = ["train_counts.npy", "walk_index.npy", "walks.npy"]
        assert files == (always if extra else sorted(always + ["syn0.npy", "syn1neg.npy", "vocab_ids.npy"])), files
        arrs = {f[:-4]: np.load(d_out / f) for f in files}
        assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
        assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
        B, L, D = d["config"]["walks_per_step_per_gpu"], d["config"]["walk_len"], d["config"]["dim"]
        assert arrs["walks"].shape == (min(B, 16384), L) and (arrs["walks"] >= -1).all() and (arrs["walks"] < d["config"]["vertices"]).all()
        assert arrs["train_counts"][0] == d["config"]["pairs_per_step_per_gpu"] * steps and arrs["train_counts"][1] > 0
        if not extra:
            n = len(arrs["vocab_ids"])
            assert n > 0 and arrs["syn0"].shape == (n, D) and arrs["syn1neg"].shape == (n, D)
            assert np.isfinite(arrs["syn0"]).all() and np.isfinite(arrs["syn1neg"]).all() and np.abs(arrs["syn1neg"]).max() > 0
        dumps.append(arrs)
    assert sorted(dumps[0]) == sorted(dumps[1]) and all(np.array_equal(dumps[0][k], dumps[1][k]) for k in dumps[0])
    for k in ("walks", "walk_index", "train_counts"):
        assert np.array_equal(dumps[0][k], dumps[2][k]), k
    # the last timed step's batch (one GPU: step i trains rows [i B, (i + 1) B) of the epoch's walks while they fit)
    wl = WORKLOADS["tiny"]
    epoch = wl["walks_per_vertex"] * wl["R"] * wl["T"]
    idx = dumps[0]["walk_index"].astype(np.int64)
    row0 = ((warmup + steps - 1) * B) % max(epoch - B + 1, 1)
    assert (idx >= row0).all() and (idx < row0 + B).all() and len(np.unique(idx)) == len(idx)
    G = synth.flow_graph_torch(wl["R"], wl["T"], wl["mean_degree"], "cuda:0")
    g = dge.DeviceGraph(0)
    g.add_edges_device(G["src"], G["dst"], G["w"]); g.set_sources(G["sources"]); g.build_alias(exact=False)
    del G
    torch.cuda.empty_cache()
    lo = int(idx.min())
    again = g.sample_walks(int(idx.max()) - lo + 1, L, seed=20171106, rng_mode=1, first_index=lo)       # bench.py's WALK_SEED
    assert np.array_equal(again[idx - lo].astype(np.float64), dumps[0]["walks"])


def test_bench_two_ranks_on_one_gpu():
    """`bench.py --gpus 2` with no torchrun environment starts its two ranks itself; over gloo they share this box's one card and run the
    block schedule for real (RCCL needs one GPU per rank: that run is the driver's).  n_gpus must equal --gpus."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--workload", "tiny", "--steps", "2", "--warmup", "1"],
                         capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and "cpu_baseline" not in d
    assert "block schedule x2" in d["config"]["parallelism"]
    # N ranks step in the global batch the product trains with — a tenth of the epoch whatever N (fit_distributed's; the schedule keeps the one-GPU embedding only in
    # batches of at most a fifth of it) — so the total work of a step is fixed: "strong"; the round-1..4 step (N x a tenth of the epoch) is behind --weak-batch
    c = d["config"]
    assert d["scaling"] == "strong" and abs(c["batch_fraction_of_epoch"] - 0.1) < 0.01 and c["global_batch_walks"] == 2 * c["walks_per_step_per_gpu"], c
