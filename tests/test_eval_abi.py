"""CPU: the held-out evaluation entries (dge_model_score_pairs, dge_model_eval_links, dge_model_eval_sgns) are part of the C ABI — declared, exported,
bound — were added without moving the version or the trainer's build stamp, and refuse a null model before they look for a device."""
import ctypes as C
import hashlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "embedding_amd", "csrc")
ENTRIES = ("dge_model_score_pairs", "dge_model_eval_links", "dge_model_eval_sgns")


def test_the_three_entries_are_declared_exported_and_bound(dge):
    h = open(os.path.join(ROOT, "include", "dge.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    declared = set(re.findall(r"\b(dge_[a-z0-9_]+)\s*\(", h))
    raw = C.CDLL(dge.LIB_PATH)
    from embedding_amd._native import SIGNATURES
    for name in ENTRIES:
        assert name in declared, "%s is not declared in include/dge.h" % name
        assert hasattr(raw, name), "libdge.so does not export %s" % name
        assert name in SIGNATURES
    assert re.search(r"\bdge_eval_result\b", h)


def test_result_layout_and_version(dge):
    from embedding_amd._native import EvalResult
    assert C.sizeof(EvalResult) == 48
    assert [f[0] for f in EvalResult._fields_] == ["pairs", "negatives", "skipped", "auc", "loss", "kernel_ms"]
    assert EvalResult.auc.offset == 24 and EvalResult.kernel_ms.offset == 40
    assert dge.lib.dge_version() == 106            # additions only: no bump


def test_a_null_model_is_an_argument_error_without_a_device(dge):
    from embedding_amd._native import EvalResult
    lib = dge.lib
    r = EvalResult()
    calls = {
        "dge_model_score_pairs": lambda: lib.dge_model_score_pairs(None, None, None, 0, None),
        "dge_model_eval_links": lambda: lib.dge_model_eval_links(None, None, 0, 0, 4, 3, C.byref(r)),
        "dge_model_eval_sgns": lambda: lib.dge_model_eval_sgns(None, None, 0, 0, 3, C.byref(r)),
    }
    for name, call in calls.items():
        assert call() == 1, name                   # DGE_ERR_ARG
        msg = (lib.dge_last_error() or b"").decode()
        assert name in msg and "null" in msg, msg


def test_the_build_stamp_is_the_hash_of_the_stamped_sources(dge):
    """embedding_amd/csrc/Makefile: KHASH = sha1(sgns_kernels.h dge_algos.h sgns_plan.h sgns.hip)[:12], SHASH the same behind sgns_sorted.hip.  The
    evaluation lives in a translation unit of its own: the stamp the counter profiles (profiles/traffic.json) are keyed on is still that hash."""
    def sha(names):
        return hashlib.sha1(b"".join(open(os.path.join(CSRC, n), "rb").read() for n in names)).hexdigest()[:12]
    k = ["sgns_kernels.h", "dge_algos.h", "sgns_plan.h", "sgns.hip"]
    want = "kernels=%s sorted=%s" % (sha(k), sha(["sgns_sorted.hip"] + k))
    got = dge.lib.dge_build_stamp().decode()
    print("build stamp:", got)
    assert got == want
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "cat sgns_kernels.h dge_algos.h sgns_plan.h sgns.hip |" in mk and "cat sgns_sorted.hip sgns_kernels.h dge_algos.h sgns_plan.h sgns.hip |" in mk
    hash_lines = "".join(l for l in mk.splitlines() if "HASH" in l)
    assert "eval.o" in mk and "eval" not in hash_lines
    # what only decides time, runs between launches or exists for tests is built into the library and stays out of the stamp
    objs = next(l for l in mk.splitlines() if l.startswith("OBJS")).split()
    for unit in ("sgns_place", "sgns_io", "sgns_exchange", "sgns_selftest"):
        assert os.path.exists(os.path.join(CSRC, unit + ".hip")), unit
        assert unit + ".o" in objs, unit
        assert unit not in hash_lines, unit
    # ... and only sgns.o is compiled with the stamp's flags
    recipes = [l for l in mk.splitlines() if l.startswith("\t") and "$(STAMP_FLAGS)" in l]
    assert len(recipes) == 1 and "-c sgns.hip " in recipes[0], recipes
