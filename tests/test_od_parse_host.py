"""CPU: embedding_amd/csrc/od_parse.h — the two routines every lane of k_od_parse (od_read.hip) runs on the tokens of a .od line — built for the host
(tests/native/od_parse_harness.cpp) and compared bit for bit with libc's strtod and strtoll in the "C" locale.  strtod is correctly rounded: the binary64
nearest the exact decimal value, ties to even.  The harness checks itself (a fixed list and over a million seeded random tokens, harness_od_selfcheck); the
same program, built stand-alone with -fsanitize=address,undefined, runs clean; and the list of the issue is asserted token by token here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "od_parse_harness.cpp")
OK, HOST, BAD = 0, 1, 2
INF = 0x7FF0000000000000

_libc = C.CDLL("libc.so.6")
_libc.strtod.restype = C.c_double
_libc.strtod.argtypes = [C.c_char_p, C.c_void_p]


def strtod_bits(tokens):
    import locale
    assert locale.setlocale(locale.LC_NUMERIC) == "C"
    return np.array([_libc.strtod(t, None) for t in tokens], np.float64).view(np.uint64)


def load_harness(tmp_dir):
    so = os.path.join(str(tmp_dir), "libod_parse_harness.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-Wall", "-o", so, SRC])
    H = C.CDLL(so)
    H.harness_od_parse_f64.argtypes = [C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    H.harness_od_parse_id.argtypes = [C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    H.harness_od_selfcheck.argtypes = [C.c_int64, C.c_uint64, C.c_void_p]
    H.harness_od_selfcheck.restype = C.c_int64

    def blob(tokens):
        off = np.zeros(len(tokens) + 1, np.int64)
        off[1:] = np.cumsum([len(t) for t in tokens])
        return b"".join(tokens), off

    def weights(tokens):
        data, off = blob(tokens)
        bits = np.zeros(len(tokens), np.uint64); status = np.full(len(tokens), 9, np.uint8)
        H.harness_od_parse_f64(data, off.ctypes.data_as(C.c_void_p), len(tokens), bits.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p))
        return bits, status

    def ids(tokens):
        data, off = blob(tokens)
        val = np.zeros(len(tokens), np.int64); ok = np.full(len(tokens), 9, np.uint8)
        H.harness_od_parse_id(data, off.ctypes.data_as(C.c_void_p), len(tokens), val.ctypes.data_as(C.c_void_p), ok.ctypes.data_as(C.c_void_p))
        return val, ok.astype(bool)
    return H, weights, ids


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return load_harness(tmp_path_factory.mktemp("od_parse_harness"))


def test_the_harness_agrees_with_strtod_and_strtoll_on_a_million_random_tokens(harness):
    H = harness[0]
    c = np.zeros(5, np.int64)
    wrong = H.harness_od_selfcheck(1_000_000, 20251018, c.ctypes.data_as(C.c_void_p))
    tokens, host, integers, integers_host, _ = c.tolist()
    print("tokens %d, handed to the host %d (%.1f %%), integers of up to 19 digits %d, of those handed to the host %d" % (tokens, host, 100.0 * host / tokens, integers, integers_host))
    assert wrong == 0 and tokens >= 1_000_000 and integers >= 400_000
    assert integers_host == 0                          # every integer weight of up to 19 digits is decided on the device
    assert 0 < host < tokens // 4                      # ... and the host's share is what lies outside the 128-bit range: wide exponents and long tails


def test_the_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "od_parse_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    run = subprocess.run([exe, "1000000", "7"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert " wrong 0" in run.stdout and " integers_host 0 " in run.stdout


def test_the_fixed_list_of_weights(harness):
    _, weights, _ = harness
    tokens = [b"9007199254740993", b"9007199254740995", b"1.7976931348623157e308", b"1.7976931348623159e308", b"1e309", b"4.9406564584124654e-324", b"2e-324", b"1e-400",
              b"-0", b"5.", b".5", b"3" * 800, b"0." + b"7" * 798, b"1." + b"0" * 797 + b"1", b"9" * 800 + b"e-780", b"3", b"3.0", b"2.5e1", b"1e-3", b"12345678901234567",
              b"1234567890123456789012345", b"9999999999999999999", b"007", b"+7", b"inf", b"-Infinity", b"nan"]
    bits, status = weights(tokens)
    want = strtod_bits(tokens)
    assert (status != BAD).all()
    got = dict(zip(tokens, np.where(status == OK, bits, want).tolist()))          # what the reader holds: a token handed back is finished with strtod
    st = dict(zip(tokens, status.tolist()))
    for t, b, s, w in zip(tokens, bits.tolist(), status.tolist(), want.tolist()):
        if s == OK and t != b"nan":
            assert b == w, (t, hex(b), hex(w))
    assert got[b"9007199254740993"] == np.float64(2.0 ** 53).view(np.uint64) and got[b"9007199254740995"] == np.float64(2.0 ** 53 + 4).view(np.uint64)      # the ties at 2^53 go to even
    assert st[b"9007199254740993"] == OK and st[b"9007199254740995"] == OK and st[b"9999999999999999999"] == OK
    assert got[b"1.7976931348623157e308"] == 0x7FEFFFFFFFFFFFFF and got[b"1.7976931348623159e308"] == INF and got[b"1e309"] == INF and st[b"1e309"] == OK
    assert got[b"4.9406564584124654e-324"] == 1 and got[b"2e-324"] == 0 and got[b"1e-400"] == 0 and st[b"1e-400"] == OK
    assert got[b"-0"] == 1 << 63 and st[b"-0"] == OK and got[b"5."] == np.float64(5).view(np.uint64) and got[b".5"] == np.float64(0.5).view(np.uint64)
    assert got[b"3" * 800] == INF and st[b"3" * 800] == OK                         # 800 threes are far above the format
    assert st[b"1234567890123456789012345"] == HOST and st[b"12345678901234567"] == OK
    for t in (b"3", b"3.0", b"2.5e1", b"1e-3", b"007", b"+7", b"5.", b".5"):
        assert st[t] == OK, t
    assert got[b"inf"] == INF and got[b"-Infinity"] == INF | 1 << 63 and got[b"nan"] & 0x7FFFFFFFFFFFFFFF > INF      # well-formed: the reader refuses them as not finite
    bad = [b"1e", b".", b"0x10", b"nan(1)", b"0x1p3", b"1e+", b"+", b"-", b"", b"1.0f", b"1,5", b"--1", b"e5", b"1..2", b"infinit", b"12a"]
    assert (weights(bad)[1] == BAD).all()


def test_the_fixed_list_of_ids(harness):
    _, _, ids = harness
    good = {b"9223372036854775807": 2 ** 63 - 1, b"-9223372036854775808": -2 ** 63, b"+9223372036854775807": 2 ** 63 - 1, b"+7": 7, b"007": 7, b"7": 7, b"-7": -7, b"0": 0, b"-0": 0,
            b"0" * 40 + b"12": 12, b"1099511627776": 2 ** 40, b"-10100": -10100}
    val, ok = ids(list(good))
    assert ok.all() and val.tolist() == list(good.values())
    bad = [b"9223372036854775808", b"-9223372036854775809", b"+9223372036854775808", b"18446744073709551623", b"9" * 20, b"7.0", b"7.", b"7e0", b"", b"+", b"-", b"+-7", b"7a", b"a7", b"0x7",
           b"1" * 800, b"inf", b"\xef\xbc\x97"]
    assert not ids(bad)[1].any()
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.integers(-2 ** 63, 2 ** 63 - 1, 50_000, dtype=np.int64, endpoint=True), rng.integers(-10 ** 6, 10 ** 6, 50_000)])
    val, ok = ids([b"%d" % x for x in v.tolist()])
    assert ok.all() and np.array_equal(val, v)
