"""CPU: embedding_amd/csrc/vec_parse.h — the routine every lane of k_vec_parse (vec_read.hip) runs on one value token of a .vec file — built for the host
(tests/native/vec_parse_harness.cpp) and compared bit for bit with libc's strtof in the "C" locale, which is correctly rounded: the binary32 nearest the
exact decimal value, ties to even.  A reader that goes through a double (np.float32(float(s))) fails the table of hard cases below.  Whenever the routine
says "not mine" (the host finishes the token with strtof) the token must lie outside the set the device is bound to decide: at most 19 significant digits
and |value| in [1e-10, 1e10].  A third, independent reading by fractions.Fraction witnesses a subset."""
import ctypes as C
import os
import random
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, HOST, BAD = 0, 1, 2


@pytest.fixture(scope="module")
def parse(tmp_path_factory):
    d = tmp_path_factory.mktemp("vec_parse_harness")
    so = str(d / "libvec_parse_harness.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-Wall", "-o", so, os.path.join(ROOT, "tests", "native", "vec_parse_harness.cpp")])
    H = C.CDLL(so)
    H.harness_vec_parse.argtypes = [C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]

    def run(tokens):
        off = np.zeros(len(tokens) + 1, np.int64)
        off[1:] = np.cumsum([len(t) for t in tokens])
        bits = np.zeros(len(tokens), np.uint32); status = np.full(len(tokens), 9, np.uint8)
        H.harness_vec_parse(b"".join(tokens), off.ctypes.data_as(C.c_void_p), len(tokens), bits.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p))
        return bits, status
    return run


_libc = C.CDLL("libc.so.6")
_libc.strtof.restype = C.c_float
_libc.strtof.argtypes = [C.c_char_p, C.c_void_p]


def strtof_bits(tokens):
    """glibc strtof; the interpreter keeps LC_NUMERIC at "C" unless a program asks otherwise (asserted)."""
    import locale
    assert locale.setlocale(locale.LC_NUMERIC) == "C"
    return np.array([_libc.strtof(t, None) for t in tokens], np.float32).view(np.uint32)


def decimal_of(token):
    """(sign, exact value as a Fraction, significant digits) of a well-formed finite token."""
    t = token.decode().lower()
    neg = t.startswith("-")
    t = t.lstrip("+-")
    mant, _, exp = t.partition("e")
    ip, _, fp = mant.partition(".")
    digits = (ip + fp).lstrip("0")
    value = Fraction(int(ip + fp or "0")) * Fraction(10) ** (int(exp or 0) - len(fp))
    return neg, value, len(digits.rstrip("0")) if digits else 0


def fraction_bits(token):
    """the independent witness: round the exact Fraction to 24 bits (fewer in the denormals), half to even."""
    neg, v, _ = decimal_of(token)
    sign = 0x80000000 if neg else 0
    if v == 0:
        return sign
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1                                           # 2^e <= v < 2^(e + 1)
    e = max(e, -126)
    q = v / Fraction(2) ** (e - 23)
    m = q.numerator // q.denominator
    r = q - m
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and m & 1):
        m += 1
    return sign | min(((e + 126) << 23) + m, 0x7F800000)


def in_the_devices_set(token):
    neg, v, nd = decimal_of(token)
    return nd <= 19 and (v == 0 or Fraction(1, 10 ** 10) <= v <= 10 ** 10)


def check(parse, tokens, all_on_device=False):
    bits, status = parse(tokens)
    want = strtof_bits(tokens)
    assert not (status == BAD).any(), [t for t, s in zip(tokens, status) if s == BAD][:5]
    assert ((status == OK) | (status == HOST)).all()
    nan = (want & 0x7FFFFFFF) > 0x7F800000
    ok = status == OK
    same = np.where(nan, ((bits & 0x7FFFFFFF) > 0x7F800000) & ((bits >> 31) == (want >> 31)), bits == want)
    wrong = np.nonzero(ok & ~same)[0]
    assert len(wrong) == 0, [(tokens[i], hex(bits[i]), hex(want[i])) for i in wrong[:5]]
    for i in np.nonzero(status == HOST)[0]:             # no token of the guaranteed set is ever refused
        assert not in_the_devices_set(tokens[i]), tokens[i]
    if all_on_device:
        assert ok.all(), [t for t, s in zip(tokens, status) if s != OK][:5]
    return bits, status


def test_nine_digits_of_random_bit_patterns_over_the_whole_range(parse):
    rng = np.random.default_rng(20250901)
    u = rng.integers(0, 2 ** 32, 1_100_000, dtype=np.uint64).astype(np.uint32)
    u = np.concatenate([u, rng.integers(0, 2 ** 23, 50_000, dtype=np.uint64).astype(np.uint32),                      # denormals
                        (rng.integers(0, 2 ** 23, 50_000, dtype=np.uint64).astype(np.uint32) | 0x80000000)])
    f = u.view(np.float32)
    keep = np.isfinite(f)
    assert keep.sum() >= 1_000_000
    tokens = [b"%.9g" % x for x in f[keep].astype(np.float64)]
    bits, status = check(parse, tokens, all_on_device=True)     # nine digits over the whole float range stay inside the 128-bit range
    assert np.array_equal(bits, u[keep])                         # ... and nine digits give every float32 back


def test_line_style_six_decimals(parse):
    rng = np.random.default_rng(7)
    tokens = [b"%.6f" % x for x in rng.normal(0, 0.5, 200_000)] + [b"%.6f" % x for x in rng.uniform(-1e4, 1e4, 50_000)]
    check(parse, tokens, all_on_device=True)


def random_digit_tokens(n, seed):
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        nd = rnd.randint(1, 19)
        out.append(b"%s%de%d" % (rnd.choice([b"", b"-", b"+"]), rnd.randrange(10 ** (nd - 1), 10 ** nd), rnd.randint(-50, 40)))
    return out


def test_random_tokens_of_up_to_19_digits(parse):
    tokens = random_digit_tokens(120_000, 3)
    # the same digits with the point moved inside them
    rnd = random.Random(4)
    for t in random_digit_tokens(30_000, 5):
        sign = t[:1] if t[:1] in b"+-" else b""
        mant, exp = t[len(sign):].split(b"e")
        k = rnd.randint(0, len(mant))
        tokens.append(sign + mant[:k] + b"." + mant[k:] + rnd.choice([b"e", b"E"]) + exp)
    check(parse, tokens)


HALFWAY_OF_1 = b"1.00000005960464477539062500"         # exactly between 1 and the next float


def hard_cases():
    t = [b"1.0000000596046447753906251",                 # the double-rounding trap: a double reads it as the halfway point and rounds to 1.0
         HALFWAY_OF_1, b"1.0000000596046447753906249",
         b"1.00000017881393432617187500", b"1.0000001788139343261718750000000000000000001", b"1.0000001788139343261718749999999999999999999",
         b"16777217", b"16777219", b"16777217.0000000000000000000000001", b"16777216.9999999999999999999999999", b"33554434", b"33554438",
         b"0.50000002980232238769531250", b"0.5000000298023223876953125000000000000000001", b"9007199791611905", b"9007199791611904",
         b"340282346638528859811704183484516925440", b"3.40282347e38", b"340282356779733661637539395458142568447", b"340282356779733661637539395458142568448",
         b"3.4028235677973366e38", b"3.4028235677973367e38", b"3.5e38", b"1e39", b"1e38", b"9.99999999999999999e38", b"1e9999",
         b"1.401298464324817e-45", b"1.4e-45", b"1e-45", b"7.006492321624085354618647916449580656401309709382578858785910e-46",
         b"7.0064923216240853546186479164495806564013097093825788587859e-46", b"7.00649232162408535461864791644958065640130970938257885878590e-46",
         b"7.006492321624085354618647916449580656401309709382578858785909e-46", b"7.006492321624085354618647916449580656401309709382578858785911e-46",
         b"7.1e-46", b"7e-46", b"1e-46", b"1e-9999", b"1.17549435e-38", b"1.17549428e-38", b"1.1754942807573643e-38", b"2.1019476964872256e-45",
         b"-0", b"0", b"+0.0", b"-0e10", b".5", b"5.", b"+1", b"1E5", b"000.0001", b"0e999999", b"-0e-999999", b"1e-9999", b"0.0e0", b"00000", b"-.0",
         b"12345678901234567890", b"1234567890123456789012345678901234567890", b"0.1234567890123456789012345678901234567890",
         b"1" + b"0" * 30, b"1" + b"0" * 45, b"0." + b"0" * 50 + b"1", b"1." + b"0" * 60, b"1." + b"0" * 60 + b"1",
         b"3" * 800, b"0." + b"142857" * 133 + b"14", b"1." + b"7" * 798 + b"e-3", b"9" * 800 + b"e-780",
         b"1e10", b"1e-10", b"9999999999.999999999", b"0.0000000001000000000000000001", b"1e27", b"9999999999999999999e27", b"1e28", b"1e-54", b"1e-55"]
    for sign in (b"", b"+", b"-"):
        for word in (b"inf", b"INF", b"Inf", b"infinity", b"INFINITY", b"InFiNiTy", b"nan", b"NAN", b"NaN", b"nAn"):
            t.append(sign + word)
    # every halfway point between adjacent floats near a few exponents, and that +- 1e-25 relative
    for e in (-149, -140, -127, -126, -30, -1, 0, 1, 23, 24, 60, 126):
        for m in (1, 2, 3, 0x7FFFFF, 0x800000, 0x800001, 0xFFFFFE, 0xFFFFFF):
            mid = Fraction(2 * m + 1, 2) * Fraction(2) ** e
            for v in (mid, mid * (1 + Fraction(1, 10 ** 25)), mid * (1 - Fraction(1, 10 ** 25))):
                n = v.numerator * 10 ** 220 // v.denominator              # 220 decimals: exact for mid (a dyadic rational with at most 173 fraction bits)
                s = b"%d" % n
                s = s.rjust(221, b"0")
                t.append(s[:-220] + b"." + s[-220:])
    return t


def test_hard_cases(parse):
    tokens = hard_cases()
    assert len(tokens) > 350
    bits, status = check(parse, tokens)
    bits = np.where(status == OK, bits, strtof_bits(tokens))         # what the reader returns: a token the routine hands back is finished with strtof
    got = dict(zip(tokens, bits))
    assert got[b"1.0000000596046447753906251"] == 0x3F800001 and got[HALFWAY_OF_1] == 0x3F800000            # above the halfway point / a tie goes to even
    assert np.float32(float("1.0000000596046447753906251")).view(np.uint32) == 0x3F800000                    # ... where the route through a double lands
    assert got[b"-0"] == 0x80000000 and got[b"0e999999"] == 0 and got[b"1e-9999"] == 0 and got[b"-0e-999999"] == 0x80000000
    assert got[b"3.40282347e38"] == 0x7F7FFFFF and got[b"340282356779733661637539395458142568448"] == 0x7F800000
    assert got[b"340282356779733661637539395458142568447"] == 0x7F7FFFFF and got[b"1e9999"] == 0x7F800000
    assert got[b"1.4e-45"] == 1 and got[b"7e-46"] == 0 and got[b"7.1e-46"] == 1
    assert got[b"7.00649232162408535461864791644958065640130970938257885878590e-46"] in (0, 1)
    assert got[b"-inf"] == 0xFF800000 and got[b"+InFiNiTy"] == 0x7F800000 and got[b"-NaN"] & 0xFFC00000 == 0xFFC00000
    st = dict(zip(tokens, status))
    for t in (b"-0", b".5", b"5.", b"+1", b"1E5", b"000.0001", b"0e999999", b"1e-9999", b"1e9999", b"inf", b"-nan", b"1e10", b"1e-10", b"16777217", b"1e27",
              b"12345678901234567890"[:19], b"1." + b"0" * 60):
        assert st.get(t, OK) == OK, t
    assert st[b"3" * 800] == OK and st[b"1.0000000596046447753906251"] == HOST                               # 800 threes are far above the format; the trap is the host's


def test_the_fraction_witness_agrees(parse):
    tokens = random_digit_tokens(9_000, 11) + [t for t in hard_cases() if t.lstrip(b"+-")[:1].lower() not in (b"i", b"n")]
    rng = np.random.default_rng(3)
    tokens += [b"%.9g" % x for x in rng.integers(0, 0x7F800000, 1500, dtype=np.uint64).astype(np.uint32).view(np.float32).astype(np.float64)]
    assert len(tokens) >= 10_000
    bits, status = parse(tokens)
    want = strtof_bits(tokens)
    for t, b, s, w in zip(tokens, bits, status, want):
        f = fraction_bits(t)
        assert f == w, (t, hex(f), hex(w))
        assert s == HOST or b == f, (t, hex(b), hex(f))


def test_rejected_forms(parse):
    bad = [b"0x1p3", b"0x10", b"nan(1)", b"nan()", b"1e", b"1e+", b"1e-", b".", b"+.", b"-", b"+", b"1.0f", b"1,5", b"--1", b"+-1", b"e5", b".e5", b"1e5.0", b"1..2",
           b"1.2.3", b"1e1e1", b"infinit", b"infinityy", b"in", b"na", b"nanx", b"1_000", b"1d5", b"\xef\xbc\x91", b"1 "[:1] + b"\x85", b"12a", b"a12", b"i", b"-e", b""]
    bits, status = parse(bad)
    assert (status == BAD).all(), [t for t, s in zip(bad, status) if s != BAD]
    good = [b"1e5", b"1E+5", b"1e-5", b"1.", b".1", b"+.1e+1", b"-1.e-1", b"007", b"inf", b"NAN"]
    assert (parse(good)[1] == OK).all()
