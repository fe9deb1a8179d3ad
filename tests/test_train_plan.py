"""CPU: the trainer's launch schedule (embedding_amd/csrc/sgns_plan.h: schedule_stats + plan_train, host build in tests/native/plan_harness.cpp)
against tests/golden/train_plans.json — for every case the kernel form and its template flags, the geometry, every TrainParams field the rules
set, the reported policy, the kernel name and the refusals.

The table was recorded from the rules as they stood before they moved into sgns_plan.h (the policy-code form of train_rows), with one intended
difference: a case marked "small_row_cap" is a row width of 17 .. 32 floats on >= 4 096 rows whose launch runs the 16-lane kernel (walks of more
than 64 tokens, a policy other than 2, or tables addressed by segments); its worker cap is the 1.5 workers a row measured for that kernel, no longer
the one a row of k_sgns_train_small."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "train_plans.json")
# a plan's fields as TrainPlan starts them: the golden table lists, per case, only the fields that differ from these
PLAN_DEFAULTS = {"hs": 0, "part": 0, "strict": 0, "hotmix": 0, "wdog": 0, "nlock": 0, "head": 0, "waves": 0, "big": 0, "shmem": 0, "hot_rows": 0,
                 "acc_rows": 0, "acc_drain": 16, "syn0_free": 0, "hs_hot0": 0x7FFFFFFF, "hs_n_hot": 0, "hs_drain": 1, "hs_cold": 0, "hs_wave": 0,
                 "hs_rep0": 0x7FFFFFFF, "hs_rep_n": 0, "hs_rep_thr": [0x7FFFFFFF] * 16, "wd_ticks": 0, "walk_counter": 0}


def make_counts(spec):
    """A vocabulary's counts (descending, int64) from a few parameters — the shapes the rules tell apart."""
    kind, V = spec["kind"], spec["V"]
    r = np.arange(1, V + 1, dtype=np.float64)
    if kind == "flat":
        c = np.full(V, spec["count"], np.int64)
    elif kind == "power":            # rank^-a popularity over a floor of 2
        c = np.floor(spec["scale"] * r ** -spec["a"]).astype(np.int64) + 2
    elif kind == "hot_row":          # a flat vocabulary and ONE row with `share` of all tokens
        c = np.full(V, spec["count"], np.int64)
        c[0] = int(spec["share"] * spec["count"] * V)
    elif kind == "tract":            # the reference's 801 x 8 tract graph: counts 8 .. 40, mildly skewed
        c = (8 + np.floor(32 * r ** -0.3)).astype(np.int64)
    else:
        raise ValueError(kind)
    return np.sort(c)[::-1].copy()


@pytest.fixture(scope="module")
def plan_harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan_harness")
    exe = str(d / "plan_harness")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "native", "plan_harness.cpp")])
    return exe, d


def run_cases(exe, d, vocabs, cases):
    lines = []
    for name, spec in vocabs.items():
        path = str(d / ("%s.i64" % name))
        make_counts(spec).astype("<i8").tofile(path)
        lines.append("vocab %s %s" % (name, path))
    for i, c in enumerate(cases):
        knobs = c["knobs"]
        lines.append("case %d %s %d %d %d %d %d %d %d %d %d %d %d %s" % (
            i, c["vocab"], c["dim"], c["hs"], c["policy"], c["workers"], c["part_n"], c["L"], c["n_rows"], c["window"], c["negative"],
            c["n_runs"], len(knobs), " ".join("%s %s" % kv for kv in sorted((int(k), int(v)) for k, v in knobs.items()))))
    path = d / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], check=True, capture_output=True, text=True).stdout
    return [r for r in map(json.loads, out.splitlines())]


def test_plans_match_golden(plan_harness):
    g = json.load(open(GOLDEN))
    got = run_cases(*plan_harness, g["vocabs"], g["cases"])
    assert [r.pop("id") for r in got] == [str(i) for i in range(len(g["cases"]))]
    bad = []
    for i, (c, r) in enumerate(zip(g["cases"], got)):
        want = c["expect"] if c["expect"]["rc"] else dict(PLAN_DEFAULTS, **c["expect"])
        if r != want:
            bad.append((i, {k: (want.get(k), r.get(k)) for k in set(want) | set(r) if want.get(k) != r.get(k)}))
    assert not bad, bad[:5]


def test_golden_covers_every_form_and_refusal():
    g = json.load(open(GOLDEN))
    ex = [c["expect"] for c in g["cases"]]
    assert all(set(e) <= set(PLAN_DEFAULTS) | {"rc", "error", "form", "workers", "blocks", "threads", "n_runs", "policy", "kernel"} for e in ex)
    assert {e["form"] for e in ex if e["rc"] == 0} == {"sorted", "in_order", "row_rmw", "atomics", "small_rows", "locked", "hs_centre"}
    assert {e["policy"] for e in ex if e["rc"] == 0} == {0, 1, 2, 5, 6, 7, 8}
    errors = " ".join(e["error"] for e in ex if e["rc"])
    for what in ("update_policy 8 does not carry", "update_policy 8 (owner-computes) on this vocabulary", "(commit locks on every row)",
                 "walks of up to 64 tokens", "the block schedule runs under"):
        assert what in errors, what
    assert any(c.get("small_row_cap") for c in g["cases"])
