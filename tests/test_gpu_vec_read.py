"""GPU: .vec text read on the device (include/dge.h: dge_vectors_from_vec_text / _files, csrc/vec_read.hip) against a byte-level second reading written
here: data.split(b"\\n"), every line through bytes.split(), libc strtof per value, a dict for ids, the same alignment rule.  Every comparison is exact
equality: of the float32 bits (NaN by NaN-ness and sign), of present, of the names and of every counter of dge_vec_info — host_values among them, against
the classification of the host build of csrc/vec_parse.h."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "taxi_all_head.vec")

_libc = C.CDLL("libc.so.6")
_libc.strtof.restype = C.c_float
_libc.strtof.argtypes = [C.c_char_p, C.c_void_p]


@pytest.fixture(scope="module")
def classify(tmp_path_factory):
    """token -> 1 when the routine of csrc/vec_parse.h hands it to the host (the harness of tests/test_vec_parse_host.py)."""
    so = str(tmp_path_factory.mktemp("vec_parse_harness") / "libvec_parse_harness.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-o", so, os.path.join(ROOT, "tests", "native", "vec_parse_harness.cpp")])
    H = C.CDLL(so)
    H.harness_vec_parse.argtypes = [C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]

    def run(tokens):
        if not tokens:
            return 0
        off = np.zeros(len(tokens) + 1, np.int64); off[1:] = np.cumsum([len(t) for t in tokens])
        bits = np.zeros(len(tokens), np.uint32); status = np.zeros(len(tokens), np.uint8)
        H.harness_vec_parse(b"".join(tokens), off.ctypes.data_as(C.c_void_p), len(tokens), bits.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p))
        assert (status < 2).all()
        return int((status == 1).sum())
    return run


def second_reading(pieces, header=False, prior=(), intern=True, classify=None):
    if isinstance(pieces, (bytes, bytearray)):
        pieces = [bytes(pieces)]
    names = list(prior)
    ids = {n: i for i, n in enumerate(names)}
    table, host_tokens = {}, []
    lines = rows = dropped = 0
    dim = None
    first_d = None
    for data in pieces:
        parts = data.split(b"\n")
        lines += len(parts) - (1 if parts[-1] == b"" else 0)
        at_header = bool(header)
        held = None
        for line in parts:
            toks = line.split()
            if not toks:
                continue
            if at_header:
                at_header = False
                v, d = int(toks[0]), int(toks[1])
                assert len(toks) == 2
                held = [v, d, 0]
                first_d = d if first_d is None else first_d
                continue
            if dim is None:
                dim = len(toks) - 1
            assert len(toks) == dim + 1 >= 2
            rows += 1
            if held:
                held[2] += 1
            i = ids.get(toks[0])
            if i is None:
                if not intern:
                    dropped += 1
                    continue
                i = len(names); ids[toks[0]] = i; names.append(toks[0])
            assert i not in table
            table[i] = [_libc.strtof(t, None) for t in toks[1:]]
            host_tokens += toks[1:]
        if held:
            assert held[0] == held[2]
    if dim is None:
        dim = (first_d or 0) if header else 0
    out = np.zeros((len(names), dim), np.float32)
    present = np.zeros(len(names), bool)
    for i, v in table.items():
        out[i] = v; present[i] = True
    info = dict(bytes=sum(map(len, pieces)), lines=lines, rows=rows, values=rows * dim, dropped=dropped, missing=int((~present).sum()),
                names_added=len(names) - len(prior), dim=dim, host_values=classify(host_tokens) if classify else None)
    return out, present, names, info


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.uint32); b = np.ascontiguousarray(b, np.float32).view(np.uint32)
    nan_a, nan_b = (a & 0x7FFFFFFF) > 0x7F800000, (b & 0x7FFFFFFF) > 0x7F800000
    return a.shape == b.shape and bool(np.where(nan_a | nan_b, nan_a & nan_b & ((a >> 31) == (b >> 31)), a == b).all())


def check(dge, pieces, got, classify, header=False, prior=(), intern=True):
    vec, names, info = got
    out, present, want_names, want = second_reading(pieces, header, prior, intern, classify)
    host = vec.to_host()
    assert host.shape == out.shape and host.dtype == np.float32, (host.shape, out.shape)
    assert same_bits(host, out)
    assert np.array_equal(vec.present(), present)
    assert not host[~present].view(np.uint32).any()                 # absent rows are all-zero bits
    assert names.as_bytes() == want_names
    for k, v in want.items():
        assert info[k] == v, (k, info[k], v)
    assert info["read_ms"] >= 0 and info["kernel_ms"] > 0
    return host


def rows_text(rng, n, dim, fmt=b"%.9g", name=lambda i: b"r%d" % i, sep=b" ", eol=b"\n", scale=0.5):
    v = rng.normal(0, scale, (n, dim)).astype(np.float32)
    return b"".join(name(i) + sep + sep.join(fmt % float(x) for x in v[i]) + eol for i in range(n))


HARD = [b"1.0000000596046447753906251", b"1.00000005960464477539062500", b"16777217", b"16777217.0000000000000000000000001", b"3.40282347e38",
        b"340282356779733661637539395458142568448", b"340282356779733661637539395458142568447", b"1.4e-45", b"7e-46", b"7.1e-46",
        b"7.00649232162408535461864791644958065640130970938257885878590e-46", b"-0", b".5", b"5.", b"+1", b"1E5", b"000.0001", b"0e999999", b"1e-9999", b"1e9999",
        b"12345678901234567890", b"1234567890123456789012345678901234567890", b"3" * 800, b"0." + b"142857" * 133, b"inf", b"-Infinity", b"+INF", b"nan", b"-NaN",
        b"1e30", b"1e-54", b"1e-55", b"9999999999999999999e27", b"1.17549435e-38", b"1.1754942807573643e-38"]


def generated_texts():
    rng = np.random.default_rng(20251017)
    out = {
        "empty": b"", "whitespace only": b" \t \r\n\x0b\x0c\n   ", "one row, dim 1": b"a 1\n", "one row, dim 1, no newline": b"a 1",
        "crlf": b"a 1 2 3\r\nb 4 5 6\r\n\r\nc 7 8 9\r\n", "blank lines between": b"\n\na 1 2\n\n \nb 3 4\n\n", "trailing blanks": b"a 1 2 \nb 3 4\t \n",
        "dim 1": rows_text(rng, 300, 1), "dim 20": rows_text(rng, 321, 20), "dim 128": rows_text(rng, 67, 128), "dim 257": rows_text(rng, 33, 257),
        "six decimals": rows_text(rng, 200, 8, fmt=b"%.6f"), "seventeen digits": rows_text(rng, 100, 8, fmt=b"%.17g", scale=1e-20),
        "a name of 5000 bytes": b"x 1 2\n" + b"n" * 5000 + b" 3 4\ny 5 6\n", "a value of 800 digits": b"x 1 2\ny " + b"3" * 800 + b" 0." + b"7" * 798 + b"\nz 5 6\n",
        "a value across a chunk boundary": b"a " + b"1 " * 4090 + b"\nb " + b"2.5000001 " * 4090 + b"\n",
        "a name across a chunk boundary": b"a " + b" " * 8185 + b"1\nboundary-name-0123456789 2\n",
        "newline on a chunk boundary": b"a " + b" " * 8188 + b"1\nb 2\n",
        "tabs and high bytes": b"\x85\xa0\tinf\x0b-nan\n\xff\xfe\t1e5\x0c-0\n",
        "hard cases": b"".join(b"h%d %s %s\n" % (i, t, HARD[(i * 7 + 3) % len(HARD)]) for i, t in enumerate(HARD)),
    }
    t = out["a name across a chunk boundary"]
    assert out["newline on a chunk boundary"][8191:8192] == b"\n" and t.index(b"boundary") < 8192 < t.index(b"-0123456789")
    t = out["a value across a chunk boundary"]
    assert t[8192:8193] not in b" \n" and t[8191:8192] not in b" \n"          # a value token lies across byte 8192
    fmts = [b"%.9g", b"%.6f", b"%.17g"]
    ws = [b" ", b"\t", b"  ", b" \x0b", b"\x0c"]
    while len(out) < 50:
        k = len(out)
        dim = int(rng.choice([1, 3, 20, 128]))
        lines = []
        for i in range(int(rng.integers(1, 300))):
            toks = [b"n%d-%d" % (k, i)]
            for _ in range(dim):
                c = rng.integers(0, 10)
                x = float(np.float32(rng.normal(0, 1) * 10.0 ** float(rng.integers(-12, 12))))
                toks.append(HARD[int(rng.integers(0, len(HARD)))] if c == 0 else fmts[int(c) % 3] % x)
            sep = ws[int(rng.integers(0, len(ws)))]
            lines.append(sep.join(toks) + (b" " if k % 5 == 0 else b""))
            if rng.integers(0, 10) == 0:
                lines.append(b"  ")
        eol = b"\r\n" if k % 4 == 0 else b"\n"
        out["generated %d" % k] = eol.join(lines) + (eol if k % 3 else b"")
    return out


TEXTS = generated_texts()


@pytest.mark.parametrize("name", list(TEXTS))
def test_generated_texts(dge, classify, name):
    data = TEXTS[name]
    check(dge, data, dge.Vectors.from_vec(data), classify)
    if name in ("hard cases", "dim 20"):
        check(dge, data, dge.Vectors.from_vec(bytearray(data)), classify)


def test_the_host_path_is_counted(dge, classify):
    vec, names, info = dge.Vectors.from_vec(TEXTS["hard cases"])
    assert info["host_values"] == classify([t for line in TEXTS["hard cases"].split(b"\n") for t in line.split()[1:]]) > 0
    assert dge.Vectors.from_vec(TEXTS["dim 128"])[2]["host_values"] == 0 and dge.Vectors.from_vec(TEXTS["six decimals"])[2]["host_values"] == 0
    row = vec.to_host()[0].view(np.uint32)
    assert row[0] == 0x3F800001                                     # the double-rounding trap, read correctly


def test_the_golden_file_with_its_header(dge, classify, tmp_path):
    """tests/golden/taxi_all_head.vec is the HEAD of miscs/taxi_all.txt: its first line still says "77 8", it holds 3 rows, every line ends in a blank.
    As it is, header=1 must refuse it with both numbers; with the first line put right it reads, trailing blanks and all."""
    data = open(GOLDEN, "rb").read()
    lines = data.split(b"\n")
    assert lines[0].split() == [b"77", b"8"] and lines[1].endswith(b" ") and len([l for l in lines if l.split()]) == 4
    msg = fails(dge, lambda: dge.Vectors.from_vec(GOLDEN, header=True))
    assert "says 77 rows of 8 values" in msg and "holds 3 rows of 8" in msg and GOLDEN in msg
    fixed = b"3 8 \n" + data[data.index(b"\n") + 1:]
    path = str(tmp_path / "taxi_all_head3.vec")
    open(path, "wb").write(fixed)
    host = check(dge, [fixed], dge.Vectors.from_vec(path, header=True), classify, header=True)
    assert host.shape == (3, 8) and host[0, 0] == np.float32(0.597378)
    check(dge, fixed, dge.Vectors.from_vec(fixed, header=True), classify, header=True)
    assert "tokens where 2 are expected" in fails(dge, lambda: dge.Vectors.from_vec(GOLDEN))      # header=0: "77 8" is a row of dim 1, the next line is ragged


def fails(dge, call, code=7):
    with pytest.raises(dge.DgeError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    return str(ei.value)


def test_several_files(dge, classify, tmp_path):
    rng = np.random.default_rng(4)
    files = [rows_text(rng, 40, 5, name=lambda i: b"a%d" % i), rows_text(rng, 3, 5, name=lambda i: b"b%d" % i), b"", rows_text(rng, 7, 5, name=lambda i: b"c%d" % i)[:-1]]
    for header in (False, True):
        paths, pieces = [], []
        for k, data in enumerate(files):
            if header:                                               # every file carries its own "V D" line, the empty one too
                data = b"%d 5\n" % sum(1 for line in data.split(b"\n") if line.split()) + data
            pieces.append(data)
            paths.append(str(tmp_path / ("f%d_%d.vec" % (header, k))))
            open(paths[-1], "wb").write(data)
        host = check(dge, pieces, dge.Vectors.from_vec(paths, header=header), classify, header=header)
        assert host.shape == (50, 5)
        assert not pieces[-1].endswith(b"\n")
    # no files at all
    vec, names, info = dge.Vectors.from_vec([])
    assert vec.shape == (0, 0) and len(names) == 0 and info["rows"] == 0 and info["bytes"] == 0


def test_names_and_alignment(dge, classify):
    rng = np.random.default_rng(9)
    data = rows_text(rng, 200, 6)
    held = [b"r%d" % i for i in rng.permutation(200)]
    # prior names in a permuted order: rows land where the names say
    names = dge.Names(held)
    host = check(dge, data, dge.Vectors.from_vec(data, names=names), classify, prior=held)
    plain = dge.Vectors.from_vec(data)[0].to_host()
    assert all(np.array_equal(host[i], plain[int(n[1:])]) for i, n in enumerate(held))
    # prior names (some never in the text) plus new ones
    some = [b"unheld-1", b"r7", b"r3", b"unheld-2", b"r199"]
    names = dge.Names(some)
    vec, _, info = got = dge.Vectors.from_vec(data, names=names)
    check(dge, data, got, classify, prior=some)
    assert info["missing"] == 2 and info["names_added"] == 197 and vec.present()[:5].tolist() == [False, True, True, False, True] and names[5] == "r0"
    # intern off: unknown rows dropped, unheld names missing, names untouched
    names = dge.Names(some)
    vec, _, info = got = dge.Vectors.from_vec(data, names=names, intern=False)
    check(dge, data, got, classify, prior=some, intern=False)
    assert info["dropped"] == 197 and info["missing"] == 2 and info["rows"] == 200 and vec.shape == (5, 6) and names.as_bytes() == some
    # a dropped row's host tokens are not the host's work
    text = b"known 1.0000000596046447753906251\nunknown 1.0000000596046447753906251\n"
    vec, _, info = dge.Vectors.from_vec(text, names=dge.Names([b"known"]), intern=False)
    assert info["host_values"] == 1 and info["dropped"] == 1 and vec.to_host().view(np.uint32).tolist() == [[0x3F800001]]


def test_errors(dge, tmp_path):
    from embedding_amd._native import VecInfo
    names = dge.Names(["a"])
    V = dge.Vectors.from_vec
    msg = fails(dge, lambda: V(b"a 1 2\nb 3\0 4\n", names=names))
    assert "NUL" in msg and "offset 9" in msg
    msg = fails(dge, lambda: V(b"a 1 2\nb 3 4\nc 5\nd 6 7\ne 8 9 10\n", names=names))                  # two ragged rows: the least is named
    assert "line 3" in msg and "has 2 tokens where 3 are expected" in msg
    msg = fails(dge, lambda: V(b"justaname\nb 1\n", names=names))
    assert "line 1" in msg and "has 1 token" in msg
    msg = fails(dge, lambda: V(b"a 1 2\nb 3 0x1p3\nc 1e 5\n", names=names))                              # two bad values: the least offset is named
    assert "offset 10 " in msg and "line 2, column 5" in msg and "piece 0" in msg
    for bad in (b"nan(1)", b"1e", b".", b"1.0f", b"1,5", b"--1", b"e5", b"1e+"):
        assert "offset 4 " in fails(dge, lambda: V(b"a 1 " + bad + b"\n", names=names)), bad
    msg = fails(dge, lambda: V(b"x 1\ny 2\nx 3\ny 4\n", names=names))                                    # duplicates: the least second occurrence
    assert "line 3" in msg and "earlier row" in msg
    msg = fails(dge, lambda: V(b"q 1\na 2\nq 3\n", names=names, intern=False))                           # ... also of a name that would be dropped
    assert "line 3" in msg
    ok, dup = str(tmp_path / "ok.vec"), str(tmp_path / "dup.vec")
    open(ok, "wb").write(b"x 1 2\ny 3 4")
    open(dup, "wb").write(b"z 5 6\ny 7 8\n")
    msg = fails(dge, lambda: V([ok, dup], names=names))                                                  # across files
    assert "piece 1" in msg and dup in msg and "line 2, column 1" in msg
    assert V(b"a 1\nb 2\n", names=dge.Names(["a", "b"]))[2]["names_added"] == 0                          # a prior name on one row is no duplicate
    # a name the caller already holds, on two rows: its first appearance is the prior name, the second ROW is still a duplicate
    held = [b"p", b"a", b"unheld", b"b"]
    one, two = str(tmp_path / "prior1.vec"), str(tmp_path / "prior2.vec")
    open(one, "wb").write(b"b 1 2\na 3 4\nnew 5 6")
    open(two, "wb").write(b"new2 7 8\n\nb 9 10\na 11 12\n")
    for intern in (True, False):
        prior = dge.Names(held)
        msg = fails(dge, lambda: V(b"a 1\na 2\n", names=prior, intern=intern))
        assert "line 2, column 1" in msg and "offset 4 " in msg and "earlier row" in msg
        msg = fails(dge, lambda: V(b"b 1\nx 2\na 3\nb 4\ny 5\na 6\nb 7\n", names=prior, intern=intern))   # the least second occurrence, not the first found
        assert "line 4, column 1" in msg and "earlier row" in msg
        msg = fails(dge, lambda: V(b"x 1\na 2\nx 3\na 4\n", names=prior, intern=intern))                   # a new and a prior name both twice: the least line
        assert "line 3" in msg
        msg = fails(dge, lambda: V(b"a 2\nx 1\na 3\nx 4\n", names=prior, intern=intern))
        assert "line 3" in msg
        msg = fails(dge, lambda: V([one, two], names=prior, intern=intern))                              # across files
        assert "piece 1" in msg and two in msg and "line 3, column 1" in msg and "earlier row" in msg
        assert prior.as_bytes() == held
        vec, _, info = V([one], names=prior, intern=intern)                                              # each of them once is fine
        assert info["missing"] == 2 and info["dropped"] == (0 if intern else 1) and vec.present()[:4].tolist() == [False, True, False, True]
    # precedence: ragged before bad value before duplicate before header counts
    assert "tokens where" in fails(dge, lambda: V(b"x 1\nx zz\ny 1 2\n", names=names))
    assert "not a decimal number" in fails(dge, lambda: V(b"x 1\nx zz\n", names=names))
    assert "earlier row" in fails(dge, lambda: V(b"5 1\nx 1\nx 2\n", names=names, header=True))
    msg = fails(dge, lambda: V(b"3 2\nx 1 2\ny 3 4\n", names=names, header=True))                        # header counts
    assert "says 3 rows of 2 values" in msg and "holds 2 rows of 2" in msg
    msg = fails(dge, lambda: V(b"2 3\nx 1 2\ny 3 4\n", names=names, header=True))
    assert "says 2 rows of 3 values" in msg and "holds 2 rows of 2" in msg
    for hdr in (b"2\n", b"2 2 2\n", b"x 1\n", b"2 2.0\n", b"-2 2\n"):                                    # a header line that is not two integers
        msg = fails(dge, lambda: V(hdr + b"x 1 2\ny 3 4\n", names=names, header=True))
        assert "header line" in msg and "line 1" in msg, msg
    open(ok, "wb").write(b"1 2\nx 1 2\n")
    open(dup, "wb").write(b"z 5 6\n")
    msg = fails(dge, lambda: V([ok, dup], names=names, header=True))                                     # every file carries its own header
    assert "header line" in msg and dup in msg
    missing = str(tmp_path / "missing.vec")
    assert missing in fails(dge, lambda: V([ok, missing], names=names))
    assert names.as_bytes() == [b"a"]                               # refused texts add no names
    lib = dge.lib
    data = b"a 1 2\nb 3\n"
    for call in (lambda out: lib.dge_vectors_from_vec_text(0, data, len(data), 0, names._h, 1, C.byref(out), None),
                 lambda out: lib.dge_vectors_from_vec_files(0, (C.c_char_p * 1)(missing.encode()), 1, 0, names._h, 1, C.byref(out), None)):
        out = C.c_void_p(0xdead)
        assert call(out) == 7 and not out.value
    vec, _, info = V(b"a 1 2\nb 3 4\n", names=names)                # the names object is still good
    assert vec.to_host().tolist() == [[1, 2], [3, 4]] and info["lines"] == 2 and names.as_bytes() == [b"a", b"b"]


def test_two_identical_calls_give_identical_results(dge):
    data = TEXTS["dim 20"] + TEXTS["hard cases"].replace(b"\n", b" 1" * 18 + b"\n")
    runs = []
    for _ in range(3):
        vec, names, info = dge.Vectors.from_vec(data)
        runs.append((vec.to_host().tobytes(), vec.present().tobytes(), names.as_bytes(), {k: v for k, v in info.items() if not k.endswith("_ms")}))
    assert runs[1] == runs[0] and runs[2] == runs[0]


def test_a_text_above_two_to_the_31_bytes(dge, classify):
    """a few rows, 2^31 blanks, a few rows: the rows behind the 2^31 mark read like the ones in front of it."""
    rng = np.random.default_rng(2)
    head = rows_text(rng, 5, 4, name=lambda i: b"head%d" % i)
    tail = rows_text(rng, 5, 4, name=lambda i: b"tail%d" % i) + b"last 1.0000000596046447753906251 -0 1e-9999 inf"
    want, present, want_names, counts = second_reading(head + tail, classify=classify)
    data = head + b" " * 2 ** 31 + tail
    vec, names, info = dge.Vectors.from_vec(data)
    n = len(data)
    del data
    assert info["bytes"] == n > 2 ** 31 and info["rows"] == 11 and info["lines"] == counts["lines"] and info["host_values"] == 1 and info["dim"] == 4
    assert names.as_bytes() == want_names and same_bits(vec.to_host(), want) and vec.present().all()
    print("text of %.2f GB: read %.0f ms, kernels %.0f ms" % (n / 1e9, info["read_ms"], info["kernel_ms"]))


# ------------------------------------------------------------------------------------------ the shared hand-back (csrc/seq_tokens.h: seq_pick, seq_tokens_to_host)
PRIOR3 = [b"r5", b"never-in-the-text", b"r0"]


def host_count_pieces(n_host):
    """200 rows of 3 values over 2 pieces, each with its "V D" line; every second value is one the host finishes (more than 19 significant digits) until n_host
    are placed; every value is distinct"""
    rows = [b"r%d " % r + b" ".join(b"%d.00000000000000000001" % (3 * r + c + 1) if (3 * r + c) % 2 == 0 and (3 * r + c) // 2 < n_host else b"%d" % (3 * r + c + 1) for c in range(3))
            for r in range(200)]
    return [b"120 3\n" + b"\n".join(rows[:120]) + b"\n", b"80 3\n" + b"\n".join(rows[120:]) + b"\n"]


@pytest.mark.parametrize("n_host", [1, 256, 257])
def test_the_hand_back_count_across_a_workgroup(dge, classify, tmp_path, n_host):
    """1, 256 and 257 host values among values the device finishes: one lane, a full workgroup and one lane of a second one in seq_pick's index kernel and in
    the byte copy.  header=True over 2 pieces and 3 prior names, so that P, hdrx and the piece lookup all enter the index arithmetic; a misplaced value shows,
    every value is its own."""
    pieces = host_count_pieces(n_host)
    paths = [str(tmp_path / ("h%d.vec" % k)) for k in range(2)]
    for p, data in zip(paths, pieces):
        open(p, "wb").write(data)
    vec, names, info = got = dge.Vectors.from_vec(paths, header=True, names=dge.Names(PRIOR3))
    check(dge, pieces, got, classify, header=True, prior=PRIOR3)
    assert info["host_values"] == n_host and info["names_added"] == 198


LENGTHS = (1, 7, 8, 9, 16, 17)


def test_lengths_around_the_eight_byte_loop(dge, classify, tmp_path):
    """New names of 1, 7, 8, 9, 16 and 17 bytes and host values of 14 (the shortest vec_parse.h hands back: ten digits and an exponent below -54), 16, 17 and 22
    bytes — seq_tok_len reads 8 bytes at a time.  A new name is the first token of the second piece; a host value is the last token of the last piece with no
    newline behind it."""
    hosts = [b"1234567891e-55", b"123456789123e-57", b"1234567891234e-58", b"7.00000000000000000001"]
    assert [len(h) for h in hosts] == [14, 16, 17, 22] and classify(hosts) == len(hosts)
    names = [bytes([97 + k]) * n for k, n in enumerate(LENGTHS)] + [bytes([65 + k]) * n for k, n in enumerate(LENGTHS)]
    rows = [n + b" %d " % (k + 1) + hosts[k % 4] for k, n in enumerate(names)]
    pieces = [b"\n".join(rows[:6]) + b"\n", b"\n".join(rows[6:])]
    assert pieces[1].startswith(b"A 7 ") and pieces[1].endswith(b" 7.00000000000000000001")
    paths = [str(tmp_path / ("l%d.vec" % k)) for k in range(2)]
    for p, data in zip(paths, pieces):
        open(p, "wb").write(data)
    vec, got_names, info = got = dge.Vectors.from_vec(paths, names=dge.Names(PRIOR3))
    check(dge, pieces, got, classify, prior=PRIOR3)
    assert info["host_values"] == 12 and got_names.as_bytes() == PRIOR3 + names


def test_new_names_across_a_workgroup_with_a_host_value(dge, classify):
    """257 new names behind 3 prior ones: a full workgroup and one lane more in k_seq_name_tok and in the byte copy of seq_tokens_to_host, which the same call
    runs a second time for its one host value.  The Names are the second reading's, in first-appearance order."""
    rows = [b"n%d %d\n" % ((k * 37) % 257, k + 1) for k in range(257)]
    rows[100] = b"n%d 16777217.0000000000000000000000001\n" % ((100 * 37) % 257)
    data = b"r0 1000\n" + b"".join(rows)
    vec, names, info = got = dge.Vectors.from_vec(data, names=dge.Names(PRIOR3))
    check(dge, data, got, classify, prior=PRIOR3)
    assert info["names_added"] == 257 and info["host_values"] == 1 and names.as_bytes()[3:5] == [b"n0", b"n37"]


RAGGED = {           # row -> the message of the parent commit's library for ragged_text(row)
    0: "libdge error 7: dge_vectors_from_vec_text: the row at offset 11 of the text (piece 0), line 3, column 1 has 3 tokens where 2 are expected (a name and 1 values, as on the first row)",
    256: "libdge error 7: dge_vectors_from_vec_text: the row at offset 3061 of the text (piece 0), line 258, column 1 has 2 tokens where 3 are expected (a name and 2 values, as on the first row)",
    299: "libdge error 7: dge_vectors_from_vec_text: the row at offset 3620 of the text (piece 0), line 301, column 1 has 2 tokens where 3 are expected (a name and 2 values, as on the first row)",
}


def ragged_text(row):
    """300 rows of 2 values behind their "V D" line; row `row` lacks its last value"""
    return b"300 2\n" + b"".join(b"r%d %d %d\n" % (r, r + 1, 2 * r) if r != row else b"r%d %d\n" % (r, r + 1) for r in range(300))


@pytest.mark.parametrize("row", [0, 256, 299])
def test_a_ragged_row_is_named_as_before(dge, row):
    """k_seq_ragged with the header line as its skip mask and seq_row_where: a row one token short at row 0 — dim is then its own, and row 1 is the ragged one
    — at row 256 (text row 257 with the header: the second workgroup) and at the last row.  The message — offset, piece, line, column, counts — is the one
    the library gave before the kernel and the read-back were shared."""
    assert fails(dge, lambda: dge.Vectors.from_vec(ragged_text(row), header=True)) == RAGGED[row]


def test_vector_handles_made_and_dropped_on_every_path(dge, tmp_path):
    """Both creators of resident vectors with no row and with one row, and the .vec reader refused after the device has worked (a value that is no number in the
    last line of the last piece): the handle comes back null, the message names the entry, and the next good call on the device gives what the text says."""
    V = dge.Vectors
    # from_host
    for rows in (np.zeros((0, 3), np.float32), np.array([[1.5, -2.0, 0.25]], np.float32)):
        v = V.from_host(rows)
        assert v.shape == rows.shape and np.array_equal(v.to_host(), rows) and v.present().tolist() == [True] * len(rows)
        v.close()
    v = V.from_host(np.array([[7.0, 8.0]], np.float32), present=[0])
    assert v.present().tolist() == [False]
    v.close()
    # from_vec
    v, names, info = V.from_vec(b"")
    assert v.shape == (0, 0) and len(names) == 0 and info["rows"] == 0
    v.close()
    v, names, info = V.from_vec(b"a 1.5 -2\n")
    assert v.to_host().tolist() == [[1.5, -2.0]] and v.present().tolist() == [True] and names.as_bytes() == [b"a"]
    v.close()
    ok, bad, good = (str(tmp_path / name) for name in ("ok.vec", "bad.vec", "good.vec"))
    open(ok, "wb").write(b"a 1 2\nb 3 4\n")
    open(bad, "wb").write(b"c 5 6\nd 7 zz\n")
    open(good, "wb").write(b"c 5 6\nd 7 0.5\n")
    names = dge.Names(["b"])
    text = b"a 1 2\nb 3 zz\n"
    for entry, call in (("dge_vectors_from_vec_text", lambda out: dge.lib.dge_vectors_from_vec_text(0, text, len(text), 0, names._h, 1, C.byref(out), None)),
                        ("dge_vectors_from_vec_files", lambda out: dge.lib.dge_vectors_from_vec_files(0, (C.c_char_p * 2)(ok.encode(), bad.encode()), 2, 0, names._h, 1, C.byref(out), None))):
        out = C.c_void_p(0xdead)
        assert call(out) == 7 and not out.value
        msg = dge.lib.dge_last_error().decode()
        assert entry in msg and "not a decimal number" in msg, msg
    assert names.as_bytes() == [b"b"]                                # a refused text adds no names
    v, names, info = V.from_vec([ok, good], names=names)
    from embedding_amd import io
    by_name = {n: row for path in (ok, good) for n, row in zip(*io.read_vec(path))}                 # the host reader; row i is the vector of names[i]
    assert list(names) == ["b", "a", "c", "d"] and np.array_equal(v.to_host(), np.stack([by_name[n] for n in names])) and v.present().all() and info["rows"] == 4
    v.close()
