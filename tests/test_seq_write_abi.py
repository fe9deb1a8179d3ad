"""CPU: the .seq writer's entries (dge_walks_to_seq_text, dge_walks_write_seq) are part of the C ABI — declared, exported, bound — were added without
moving the version or the trainer's build stamp, refuse null and negative arguments before they look for a device and before they touch the path, and
cut the text into slabs by rules (embedding_amd/csrc/seq_out_plan.h) that a host build can check."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "embedding_amd", "csrc")
ENTRIES = ("dge_walks_to_seq_text", "dge_walks_write_seq")


def test_the_entries_are_declared_exported_and_bound(dge):
    h = open(os.path.join(ROOT, "include", "dge.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    declared = set(re.findall(r"\b(dge_[a-z0-9_]+)\s*\(", h))
    raw = C.CDLL(dge.LIB_PATH)
    from embedding_amd._native import SIGNATURES
    for name in ENTRIES:
        assert name in declared, "%s is not declared in include/dge.h" % name
        assert hasattr(raw, name), "libdge.so does not export %s" % name
        assert name in SIGNATURES
    assert re.search(r"\bdge_seq_out_info\b", h)
    assert dge.lib.dge_version() == 106            # additions only: no bump
    assert callable(dge.WalkCorpus.write_seq) and callable(dge.WalkCorpus.to_seq_bytes)


def test_info_layout(dge):
    from embedding_amd._native import SeqOutInfo
    assert C.sizeof(SeqOutInfo) == 48
    assert [f[0] for f in SeqOutInfo._fields_] == ["bytes", "lines", "tokens", "empty_lines", "kernel_ms", "write_ms"]
    assert [getattr(SeqOutInfo, f[0]).offset for f in SeqOutInfo._fields_] == [0, 8, 16, 24, 32, 40]
    assert [f[1] for f in SeqOutInfo._fields_] == [C.c_int64] * 4 + [C.c_double] * 2


def test_seq_write_is_built_into_the_library_and_stays_out_of_the_stamp():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = next(l for l in mk.splitlines() if l.startswith("OBJS")).split()
    assert "seq_write.o" in objs and os.path.exists(os.path.join(CSRC, "seq_write.hip"))
    hash_lines = "".join(l for l in mk.splitlines() if "HASH" in l)
    assert "seq_write" not in hash_lines and "seq_out_plan" not in hash_lines
    assert [l for l in mk.splitlines() if l.startswith("\t") and "seq_write" in l] == []      # the generic rule builds it


def test_null_and_negative_arguments_are_argument_errors_without_a_device(dge, tmp_path):
    """Every form is decided by the arguments alone: status 1 with or without a GPU, the entry's name and "null" in the message, no file at the path.  The
    corpus handle of the negative forms is 64 zero bytes — a corpus of no rows if a check ever got as far as reading it."""
    from embedding_amd._native import SeqOutInfo
    lib = dge.lib
    w = C.create_string_buffer(64)
    info = SeqOutInfo(); n = C.c_int64(-7)
    text = C.create_string_buffer(b"\xAA" * 16, 16)
    path = os.fsencode(str(tmp_path / "never.seq"))
    calls = {
        "dge_walks_to_seq_text": [lambda: lib.dge_walks_to_seq_text(None, 0, 0, None, 0, text, 16, C.byref(n), C.byref(info)),
                                  lambda: lib.dge_walks_to_seq_text(w, 0, 0, None, 0, text, 16, None, C.byref(info)),
                                  lambda: lib.dge_walks_to_seq_text(w, 0, 0, None, 0, None, 16, C.byref(n), C.byref(info)),
                                  lambda: lib.dge_walks_to_seq_text(w, -1, 0, None, 0, text, 16, C.byref(n), C.byref(info)),
                                  lambda: lib.dge_walks_to_seq_text(w, 0, -1, None, 0, text, 16, C.byref(n), C.byref(info)),
                                  lambda: lib.dge_walks_to_seq_text(w, 0, 0, None, 0, text, -1, C.byref(n), C.byref(info))],
        "dge_walks_write_seq": [lambda: lib.dge_walks_write_seq(None, 0, 0, None, 0, path, 0, C.byref(info)),
                                lambda: lib.dge_walks_write_seq(w, 0, 0, None, 0, None, 0, C.byref(info)),
                                lambda: lib.dge_walks_write_seq(w, -1, 0, None, 0, path, 0, C.byref(info)),
                                lambda: lib.dge_walks_write_seq(w, 0, -1, None, 1, path, 0, C.byref(info))],
    }
    for name, forms in calls.items():
        for k, call in enumerate(forms):
            assert call() == 1, (name, k)              # DGE_ERR_ARG
            msg = (lib.dge_last_error() or b"").decode()
            assert name in msg and "null" in msg, msg
    assert not os.path.exists(path) and text.raw == b"\xAA" * 16 and n.value == -7
    # rows beyond the corpus: the argument and the handle decide it, no device is asked
    for call in (lambda: lib.dge_walks_to_seq_text(w, 0, 1, None, 0, text, 16, C.byref(n), None), lambda: lib.dge_walks_write_seq(w, 1, 0, None, 0, path, 0, None)):
        assert call() == 1 and "corpus" in lib.dge_last_error().decode()
    assert not os.path.exists(path) and text.raw == b"\xAA" * 16


# ---------------------------------------------------------------------------------------------- the planning header, built for the host
@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("seq_out_plan_harness")
    exe = str(d / "seq_out_plan_harness")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "native", "seq_out_plan_harness.cpp")])

    def run(*args):
        return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout.strip()
    return run


def test_slabs_tile_the_text_exactly_and_stay_within_the_bound(plan):
    tile, slab = map(int, plan("sizes").split())
    assert tile % 16 == 0 and tile > 0 and slab % tile == 0
    for total in (0, 1, 15, 16, 17, tile - 1, tile, tile + 1, slab - 1, slab, slab + 1, 2 * slab, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1):
        lines = plan("slabs", total).splitlines()
        buf = int(lines[0])
        slabs = [tuple(map(int, l.split())) for l in lines[1:]]
        assert buf % tile == 0 and 0 < buf <= slab                       # one device buffer; two of them whatever the total
        assert len(slabs) == -(-total // slab)
        at = 0
        for b, e, tiles in slabs:
            assert b == at and b % 16 == 0 and b % tile == 0 and b < e <= total
            assert e - b <= buf and tiles * tile <= buf and (tiles - 1) * tile < e - b <= tiles * tile
            assert e % 16 == 0 or e == total                              # only the text's end may be unaligned
            at = e
        assert at == total


def test_decimals_are_sized_by_comparison_and_spelled_digit_by_digit(plan):
    vals = [0, 9, 10, 99, 100, 999, 1000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999, 100000000, 999999999, 1000000000, 2147483647]
    out = plan("decimal", *vals).splitlines()
    assert out == ["%d %d" % (len(str(v)), v) for v in vals]
