"""CPU: the .seq ingest entries (dge_names_*, dge_walks_from_seq_text / _files, dge_selftest_seq_intern) are part of the C ABI — declared, exported,
bound — were added without moving the version or the trainer's build stamp, refuse null arguments before they look for a device, keep names as a host
object that needs none, and plan their buffer by rules (embedding_amd/csrc/seq_plan.h) that a host build can check."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "embedding_amd", "csrc")
ENTRIES = ("dge_names_create", "dge_names_add", "dge_names_count", "dge_names_cstrs", "dge_names_free", "dge_walks_from_seq_text",
           "dge_walks_from_seq_files", "dge_selftest_seq_intern")
WS = bytes([9, 10, 11, 12, 13, 32])


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
    assert re.search(r"\bdge_seq_info\b", h) and re.search(r"\bdge_names\b", h)
    assert dge.lib.dge_version() == 106            # additions only: no bump


def test_info_layout(dge):
    from embedding_amd._native import SeqInfo
    assert C.sizeof(SeqInfo) == 72
    assert [f[0] for f in SeqInfo._fields_] == ["bytes", "lines", "rows", "tokens", "unknown", "names_added", "max_len", "reserved", "read_ms", "kernel_ms"]
    assert [getattr(SeqInfo, f[0]).offset for f in SeqInfo._fields_] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 64]


def test_null_arguments_are_argument_errors_without_a_device(dge):
    from embedding_amd._native import SeqInfo
    lib = dge.lib
    names = dge.Names()
    out = C.c_void_p(0); info = SeqInfo(); n = C.c_int64(0)
    ids = (C.c_int32 * 4)()
    path = (C.c_char_p * 1)(b"/nonexistent.seq")
    calls = {
        "dge_walks_from_seq_text": [lambda: lib.dge_walks_from_seq_text(0, b"a b\n", 4, None, 1, C.byref(out), C.byref(info)),
                                    lambda: lib.dge_walks_from_seq_text(0, b"a b\n", 4, names._h, 1, None, C.byref(info)),
                                    lambda: lib.dge_walks_from_seq_text(0, None, 4, names._h, 1, C.byref(out), C.byref(info)),
                                    lambda: lib.dge_walks_from_seq_text(0, b"a b\n", -1, names._h, 1, C.byref(out), C.byref(info))],
        "dge_walks_from_seq_files": [lambda: lib.dge_walks_from_seq_files(0, path, 1, None, 1, C.byref(out), C.byref(info)),
                                     lambda: lib.dge_walks_from_seq_files(0, path, 1, names._h, 1, None, C.byref(info)),
                                     lambda: lib.dge_walks_from_seq_files(0, None, 1, names._h, 1, C.byref(out), C.byref(info)),
                                     lambda: lib.dge_walks_from_seq_files(0, path, -1, names._h, 1, C.byref(out), C.byref(info))],
        "dge_selftest_seq_intern": [lambda: lib.dge_selftest_seq_intern(0, None, 4, 4, 16, ids, 4, C.byref(n), C.byref(n)),
                                    lambda: lib.dge_selftest_seq_intern(0, b"a b\n", 4, 4, 16, ids, 4, None, C.byref(n)),
                                    lambda: lib.dge_selftest_seq_intern(0, b"a b\n", 4, 0, 16, ids, 4, C.byref(n), C.byref(n)),
                                    lambda: lib.dge_selftest_seq_intern(0, b"a b\n", 4, 4, 16, None, 4, C.byref(n), C.byref(n))],
        "dge_names_create": [lambda: lib.dge_names_create(None)],
        "dge_names_add": [lambda: lib.dge_names_add(None, None, 0), lambda: lib.dge_names_add(names._h, None, 2)],
        "dge_names_count": [lambda: lib.dge_names_count(None, C.byref(n)), lambda: lib.dge_names_count(names._h, None)],
        "dge_names_cstrs": [lambda: lib.dge_names_cstrs(None, C.byref(out)), lambda: lib.dge_names_cstrs(names._h, None)],
    }
    for name, forms in calls.items():
        for k, call in enumerate(forms):
            assert call() == 1, (name, k)              # DGE_ERR_ARG, on a machine with or without a GPU
            msg = (lib.dge_last_error() or b"").decode()
            assert name in msg and "null" in msg, msg
    assert len(names) == 0 and not out.value
    lib.dge_names_free(None)                           # like free(NULL)


def test_names_round_trip_on_the_host(dge):
    """dge_names is a host object: strings go in and come back by id without a device; a duplicate — of a held name or inside the call —, an empty name
    and a name that holds whitespace are refused, and a refused call adds nothing."""
    first = ["0-17031", "1-17031", "hé-x", "a" * 5000]
    names = dge.Names(first)
    assert len(names) == 4 and list(names) == first and names[2] == "hé-x" and names[-1] == "a" * 5000
    names.add([b"\x85\xa0\xff", "z"])
    assert names.as_bytes() == [s.encode() for s in first] + [b"\x85\xa0\xff", b"z"]
    for bad in (["q", "0-17031"], ["q", "r", "q"], ["q", ""], ["q", "two words"], ["q", "tab\tbed"], ["q", "line\n"]):
        with pytest.raises(dge.DgeError) as ei:
            names.add(bad)
        assert ei.value.code == 1 and "dge_names_add" in str(ei.value)
        assert len(names) == 6
    names.add(["q"])
    assert len(names) == 7 and names[6] == "q"
    big = dge.Names(["n%d" % i for i in range(20000)])
    assert len(big) == 20000 and big[19999] == "n19999" and list(big)[12345] == "n12345"
    assert len(dge.Names()) == 0 and list(dge.Names()) == []


def test_seq_ingest_is_built_into_the_library_and_stays_out_of_the_stamp():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = next(l for l in mk.splitlines() if l.startswith("OBJS")).split()
    assert "seq_ingest.o" in objs and os.path.exists(os.path.join(CSRC, "seq_ingest.hip"))
    hash_lines = "".join(l for l in mk.splitlines() if "HASH" in l)
    assert "seq_ingest" not in hash_lines and "seq_plan" not in hash_lines
    recipes = [l for l in mk.splitlines() if l.startswith("\t") and "seq_ingest" in l]
    assert recipes == []                               # the generic rule builds it


# ---------------------------------------------------------------------------------------------- the planning header, built for the host
@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("seq_plan_harness")
    exe = str(d / "seq_plan_harness")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "native", "seq_plan_harness.cpp")])

    def run(*args):
        return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout.strip()
    return run, d


def rows_of(data):
    return [line.split() for line in data.split(b"\n") if line.split()]


def test_whitespace_is_the_six_bytes_of_the_c_locale(plan):
    run, _ = plan
    table = run("space")
    assert len(table) == 256
    assert bytes(c for c in range(256) if table[c] == "1") == WS
    for c in range(256):                               # ... which is what bytes.split() with no argument splits on: the tests' second reading
        assert (bytes([c]).split() == []) == (table[c] == "1"), c


def test_layout_offsets_and_sizes(plan):
    run, _ = plan
    assert run("layout", 0) == "| 0 64 0"
    assert run("layout", 0, 0) == "0 | 1 8256 0"
    assert run("layout", 7, 10, 0, 5) == "7 18 19 | 25 8256 15"
    assert run("layout", 0, 8191) == "0 | 8192 8256 8191"
    assert run("layout", 0, 8192) == "0 | 8193 16448 8192"
    assert run("layout", 0, 3 * 2 ** 31, 5) == "0 %d | %d %d %d" % (3 * 2 ** 31 + 1, 3 * 2 ** 31 + 7, (3 * 2 ** 31 // 8192 + 1) * 8192 + 64, 3 * 2 ** 31 + 5)
    assert run("layout", 0, -1) == "refused" and run("layout", -1, 4) == "refused" and run("layout", 0, 2 ** 62, 2 ** 62) == "refused"


def test_files_are_joined_so_that_no_token_and_no_line_crosses_a_file(plan):
    """The buffer the kernels read: prior names one per line, then each file with ONE pad byte behind it — the missing newline when the file does not
    end in one, a blank otherwise — and blanks to the end.  Its rows must be the names' rows followed by every file's own rows, and its newline count
    the names plus every file's lines."""
    run, d = plan
    cases = [
        [b"a b\nc d", b"e f\n", b"g"],                 # no final newline in front of another file: "d" and "e" stay apart
        [b"a b\n", b"c d\n"],
        [b"", b"x", b"", b"y z\n\n", b""],
        [b"a\r\nb\r", b"\rc\r\n"],
        [b"tail  ", b"  head\n", b"\t\x0b\x0c", b"\x85\xa0 \xff"],
        [b"only"],
        [b"\n\n\n", b"\n"],
        [b"x" * 8191], [b"x" * 8192], [b"x" * 8190 + b"\n", b"y"], [b"w " * 5000, b"v\n" * 3000],
    ]
    for k, files in enumerate(cases):
        for prior in ([], ["p0", "p1-x"]):
            paths = []
            for j, data in enumerate(files):
                paths.append(str(d / ("case%d_%d.seq" % (k, j))))
                open(paths[-1], "wb").write(data)
            out = str(d / ("case%d.buf" % k))
            used, padded, text_bytes = map(int, run("join", out, *prior, "--", *paths).split())
            buf = open(out, "rb").read()
            assert len(buf) == padded and text_bytes == sum(map(len, files)) and used == sum(len(p) + 1 for p in prior) + text_bytes + len(files)
            assert padded % 8192 == 64 and padded - 64 >= used and buf[used:] == b" " * (padded - used)
            want = [[p.encode()] for p in prior]
            for data in files:
                want += rows_of(data)
            assert rows_of(buf) == want, (k, prior)
            lines = sum(data.count(b"\n") + (1 if data and not data.endswith(b"\n") else 0) for data in files)
            assert buf.count(b"\n") == len(prior) + lines, (k, prior)


def test_the_name_table_grows_by_eight_up_to_a_size_that_cannot_fill(plan):
    run, _ = plan
    assert run("slots", 10000, 16) == "16 128 1024 8192 32768"
    assert run("slots", 10, 16) == "16 32"
    assert run("slots", 0, 16) == "2"
    assert run("slots", 1000, 0) == "2048"                                  # the default start, capped by what the tokens can need
    assert run("slots", 125000000, 0) == "1048576 8388608 67108864 268435456"
    for tokens, first in ((1, 1), (5, 1), (12345, 100), (3 * 10 ** 9, 0)):
        seq = list(map(int, run("slots", tokens, first).split()))
        assert all(s & (s - 1) == 0 for s in seq) and seq == sorted(set(seq))
        assert seq[-1] >= 2 * tokens > seq[-1] // 2                         # the last table is at most half full whatever the text holds
