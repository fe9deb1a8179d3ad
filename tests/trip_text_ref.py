"""The second reading of the trip-text rule (include/dge.h: taxi trip text in), CPU only and without the library: lines, SPLIT, INT, COORD, the two date forms
and the three formats in plain Python, written from the rule.  SPLIT is bytes.split / bytes.translate — no regular-expression engine.  COORD's value is
float(): Python's own correctly rounded decimal-to-binary64 conversion (check_coord compares it with libc's strtod).  Also the corpora the tests and
scripts/trip_text_rate.py share: well-formed lines of every format and the seeded mutations the issue lists."""
import ctypes as C
import math
import random
import struct

OK, BAD_FIELDS, BAD_PARSE, TOO_LONG = 0, 1, 2, 3
MAX_LINE = 65535
BAD_RECORD = (-1, 0, 0, 0, 0)


# ------------------------------------------------------------------------------------------ the rule
def lines_of(piece):
    """BufferedReader.readLine over one piece: "\\n", "\\r\\n" and a lone "\\r" end a line, a last line without a terminator counts."""
    out, start, n = [], 0, len(piece)
    nl, cr = piece.find(b"\n"), piece.find(b"\r")
    while nl >= 0 or cr >= 0:
        if cr < 0 or 0 <= nl < cr:
            out.append(piece[start:nl])
            start = nl + 1
        else:
            out.append(piece[start:cr])
            start = cr + 1
            if start < n and piece[start] == 10:
                start += 1
            cr = piece.find(b"\r", start)
        if nl < start:
            nl = piece.find(b"\n", start)
    if start < n:
        out.append(piece[start:])
    return out


_TABLES = {}


def split(s, seps, plus=False):
    """SPLIT / SPLIT+: cut at every byte of seps (plus: a run cuts once, a leading one still leaves an empty piece); trailing empty pieces go; a text in which
    nothing cuts is one piece.  The cut bytes are first made one byte (they occur in no piece), then bytes.split does the cutting."""
    if len(seps) > 1:
        if seps not in _TABLES:
            _TABLES[seps] = bytes.maketrans(seps, seps[:1] * len(seps))
        s = s.translate(_TABLES[seps])
    if seps[:1] not in s:
        return [s]
    p = s.split(seps[:1])
    if plus:
        p = [x for i, x in enumerate(p) if x or i == 0]
    while p and not p[-1]:
        p.pop()
    return p


def split2(s):
    i = s.find(b" ")
    return [s] if i < 0 else [s[:i], s[i + 1:]]


def parse_int(s, lo, hi):
    d = s[1:] if s[:1] in (b"+", b"-") else s
    if not d or any(c < 48 or c > 57 for c in d):
        return None
    v = int(d) * (-1 if s[:1] == b"-" else 1)
    return v if lo <= v <= hi else None


def parse_byte(s):
    return parse_int(s, -128, 127)


def parse_int32(s):
    return parse_int(s, -2 ** 31, 2 ** 31 - 1)


def _digits(s, i):
    j = i
    while j < len(s) and 48 <= s[j] <= 57:
        j += 1
    return j


def coord(s):
    """-> float or None.  Blanks (<= 0x20) go at both ends; [+-] digits [. digits] [(e|E) [+-] digits] with a mantissa digit; a finite value."""
    a, b = 0, len(s)
    while a < b and s[a] <= 0x20:
        a += 1
    while b > a and s[b - 1] <= 0x20:
        b -= 1
    s = s[a:b]
    i = 1 if s[:1] in (b"+", b"-") else 0
    j = _digits(s, i)
    nd = j - i
    if s[j:j + 1] == b".":
        k = _digits(s, j + 1)
        nd += k - j - 1
        j = k
    if nd == 0:
        return None
    if j < len(s):
        if s[j:j + 1] not in (b"e", b"E"):
            return None
        j += 1
        if s[j:j + 1] in (b"+", b"-"):
            j += 1
        k = _digits(s, j)
        if k == j or k != len(s):
            return None
    v = float(s.decode("ascii"))
    return v if math.isfinite(v) else None


def date1(s):
    f = split(s, b"/ :")
    if len(f) < 5 or None in (parse_byte(f[0]), parse_byte(f[1]), parse_byte(f[4])):
        return None
    return parse_byte(f[3])


def _rem(a, b):                      # Java's %: the sign of the dividend
    return int(math.fmod(a, b))


def date2(date, time):
    d = split(date, b"/")
    if len(d) < 2 or None in (parse_byte(d[0]), parse_byte(d[1])):
        return None
    t = split(time, b" :")
    if len(t) < 4 or parse_byte(t[1]) is None:
        return None
    h = parse_byte(t[0])
    if h is None:
        return None
    return _rem(h, 12) + 12 if t[3] == b"PM" else _rem(h, 12)


def _gps(g):
    if len(g) < 2:
        return None
    q = split(g[1:-1], b",")
    if len(q) < 2:
        return None
    y, x = coord(q[0]), coord(q[1])
    return None if x is None or y is None else (x, y)


def parse_line(line, fmt):
    """-> (status, hour, sx, sy, ex, ey); hour -1 and zeros unless status is OK."""
    if len(line) > MAX_LINE:
        return (TOO_LONG,) + BAD_RECORD
    if fmt == 1:
        p = split(line, b"\t", plus=True)
        if len(p) != 13:
            return (BAD_FIELDS,) + BAD_RECORD
        hour, other, s, e, n = date1(p[7]), date1(p[8]), _gps(p[9]), _gps(p[10]), parse_int32(p[2])
    elif fmt == 2:
        p = split(line, b"\t")
        if len(p) != 17:
            return (BAD_FIELDS,) + BAD_RECORD
        hour, other, n = date2(p[0], p[1]), date1(p[2]), parse_int32(p[15])
        c = [coord(p[k]) for k in (9, 10, 11, 12)]
        s = None if None in c[:2] else tuple(c[:2])
        e = None if None in c[2:] else tuple(c[2:])
    else:
        p = split(line, b",")
        if len(p) != 21:
            return (BAD_FIELDS,) + BAD_RECORD
        a, b = split2(p[0]), split2(p[1])
        hour = date2(a[0], a[1]) if len(a) == 2 else None
        other = date2(b[0], b[1]) if len(b) == 2 else None
        n = parse_int32(p[2])
        c = [coord(p[k]) for k in (16, 15, 19, 18)]
        s = None if None in c[:2] else tuple(c[:2])
        e = None if None in c[2:] else tuple(c[2:])
    if None in (hour, other, s, e, n):
        return (BAD_PARSE,) + BAD_RECORD
    return (OK, hour) + s + e


def parse_texts(pieces, fmt, header):
    """-> records [(status, hour, sx, sy, ex, ey)] of every non-header line in text order, and the counters of dge_trip_text_info a reading of the rule gives."""
    rec, header_lines, lines = [], 0, 0
    for piece in pieces:
        ls = lines_of(bytes(piece))
        lines += len(ls)
        if header and ls:
            header_lines += 1
            ls = ls[1:]
        rec += [parse_line(l, fmt) for l in ls]
    st = [r[0] for r in rec]
    info = dict(bytes=sum(len(p) for p in pieces), lines=lines, header_lines=header_lines, ok=st.count(OK), bad_fields=st.count(BAD_FIELDS), bad_parse=st.count(BAD_PARSE),
                too_long=st.count(TOO_LONG))
    return rec, info


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def arrays(rec):
    """records -> status uint8, hour int32, start float64 [n, 2], end float64 [n, 2]"""
    import numpy as np
    a = np.array(rec, np.float64).reshape(-1, 6)
    return a[:, 0].astype(np.uint8), a[:, 1].astype(np.int32), np.ascontiguousarray(a[:, 2:4]), np.ascontiguousarray(a[:, 4:6])


def check_coord(tokens):
    """float() against libc's strtod in the "C" locale, bit for bit, on tokens coord() accepts"""
    import locale
    assert locale.setlocale(locale.LC_NUMERIC) == "C"
    libc = C.CDLL("libc.so.6")
    libc.strtod.restype = C.c_double
    libc.strtod.argtypes = [C.c_char_p, C.c_void_p]
    n = 0
    for t in tokens:
        v = coord(t)
        if v is not None:
            assert bits(v) == bits(libc.strtod(t.strip(bytes(range(33))), None)), t
            n += 1
    return n


# ------------------------------------------------------------------------------------------ corpora
X0, Y0, SIZE = -87.9, 41.6, 0.5          # the box of trip_ref.quad_mesh


def _num(rng, lo, hi):
    return ("%.*g" % (rng.randint(4, 17), rng.uniform(lo, hi))).encode()


def _point(rng):
    m = 0.04 * SIZE                      # a few points fall outside the mesh
    return _num(rng, X0 - m, X0 + SIZE + m), _num(rng, Y0 - m, Y0 + SIZE + m)


def _clock(rng, hour):
    """an AM/PM time of the given hour of the day"""
    h12 = hour % 12 or 12
    return ("%s:%02d:%02d %s" % (rng.choice(["%d", "%02d"]) % h12, rng.randrange(60), rng.randrange(60), "PM" if hour >= 12 else "AM")).encode()


def _date(rng):
    return ("%d/%d/%d" % (rng.randint(1, 12), rng.randint(1, 28), rng.choice([2013, 13]))).encode()


def _stamp(rng, hour):
    return _date(rng) + (" %d:%02d" % (hour, rng.randrange(60))).encode() + rng.choice([b"", b":%02d" % rng.randrange(60)])


def fields(fmt, rng):
    """one well-formed line as its fields, and which of them hold what (for the mutations)"""
    hour = rng.randrange(24)
    sx, sy = _point(rng)
    ex, ey = _point(rng)
    word = lambda: ("%x" % rng.getrandbits(rng.choice([16, 32, 64]))).encode()
    if fmt == 1:
        f = [word(), word(), b"%d" % rng.randint(0, 7200), word(), word(), b"%.1f" % rng.uniform(0, 30), word(), _stamp(rng, hour), _stamp(rng, rng.randrange(24)),
             b"(" + sy + b"," + sx + b")", b"(" + ey + b"," + ex + b")", word(), word()]
        where = dict(dates=[7, 8], coords=[9, 10], int=2, free=[0, 1, 3, 4, 6, 11, 12])
    elif fmt == 2:
        f = [_date(rng), _clock(rng, hour), _stamp(rng, rng.randrange(24)), word(), word(), b"%.2f" % rng.uniform(0, 30), word(), word(), word(), sx, sy, ex, ey, word(),
             b"%.2f" % rng.uniform(2, 90), b"%d" % rng.randint(0, 7200), word()]
        where = dict(dates=[1], coords=[9, 10, 11, 12], int=15, free=[3, 4, 6, 7, 8, 13, 16])
    else:
        f = [_date(rng) + b" " + _clock(rng, hour), _date(rng) + b" " + _clock(rng, rng.randrange(24)), b"%d" % rng.randint(0, 7200), b"%.1f" % rng.uniform(0, 30), word(), word(),
             word(), word(), b"%.2f" % rng.uniform(2, 90), b"0", b"0", b"%.2f" % rng.uniform(0, 9), b"Cash", word(), word(), sy, sx, b"POINT", ey, ex, b"POINT"]
        where = dict(dates=[0, 1], coords=[15, 16, 18, 19], int=2, free=[4, 5, 6, 7, 13, 14, 17, 20])
    return f, where


MUTATIONS = ("sep_dropped", "sep_doubled", "sep_leading", "sep_trailing", "trailing_empty", "empty_line", "plus5", "zeros007", "byte128", "time_three", "pm_lower", "blanks",
             "one_dot", "dot_five", "one_e2", "nan", "infinity", "hexfloat", "suffix_f", "digits25", "gps_short", "high_byte", "nul")


def mutate(fmt, f, where, what, rng):
    """-> the line's bytes"""
    sep = b"," if fmt == 3 else b"\t"
    f = list(f)
    seps = [sep] * (len(f) - 1)
    k = rng.randrange(len(seps))
    c = rng.choice(where["coords"])

    def in_coord(new, keep=None):
        if fmt == 1:                                                     # "(y,x)": one of the two numbers
            y, x = f[c][1:-1].split(b",")
            f[c] = b"(" + (new if keep is None else keep(y)) + b"," + x + b")" if rng.random() < 0.5 else b"(" + y + b"," + (new if keep is None else keep(x)) + b")"
        else:
            f[c] = new if keep is None else keep(f[c])

    d = rng.choice(where["dates"])
    if what == "sep_dropped":
        seps[k] = b""
    elif what == "sep_doubled":
        seps[k] = sep * 2
    elif what == "sep_leading":
        f[0] = sep + f[0]
    elif what == "sep_trailing":
        f[-1] = f[-1] + sep * rng.randint(1, 3)
    elif what == "trailing_empty":
        for i in range(rng.randint(1, 3)):
            f[-1 - i] = b""
    elif what == "empty_line":
        return b""
    elif what == "plus5":
        f[where["int"]] = b"+5"
    elif what == "zeros007":
        f[where["int"]] = b"007"
    elif what == "byte128":
        f[d] = b"128" + f[d][f[d].index(b"/"):] if b"/" in f[d] else b"128" + f[d][f[d].index(b":"):]
    elif what == "time_three":
        f[d] = f[d].rsplit(b" ", 1)[0] if fmt != 1 else f[d].split(b":")[0]
    elif what == "pm_lower":
        f[d] = f[d].replace(b"PM", b"pm").replace(b"AM", b"am")
    elif what == "blanks":
        in_coord(None, lambda v: b" \x01" + v + b"  ")
    elif what == "one_dot":
        in_coord(b"1.")
    elif what == "dot_five":
        in_coord(b".5")
    elif what == "one_e2":
        in_coord(b"1e2")
    elif what == "nan":
        in_coord(b"NaN")
    elif what == "infinity":
        in_coord(rng.choice([b"Infinity", b"-Infinity", b"1e999"]))
    elif what == "hexfloat":
        in_coord(b"0x1p3")
    elif what == "suffix_f":
        in_coord(rng.choice([b"1.0f", b"1.0d"]))
    elif what == "digits25":
        in_coord(None, lambda v: (v if b"." in v else v + b".") + b"".join(b"%d" % rng.randint(1, 9) for _ in range(25)))
    elif what == "gps_short":
        f[c] = b"(" if fmt == 1 else b""
    elif what in ("high_byte", "nul"):
        b = b"\x00" if what == "nul" else bytes([rng.randint(0x80, 0xFF)])
        if rng.random() < 0.5:
            i = rng.choice(where["free"])
            f[i] = f[i][:1] + b + f[i][1:]
        else:
            in_coord(None, lambda v: v[:2] + b + v[2:])
    out = f[0]
    for s, x in zip(seps, f[1:]):
        out += s + x
    return out


def corpus_lines(fmt, n, seed, mutated=0.35):
    rng = random.Random(seed * 10 + fmt)
    out = []
    for _ in range(n):
        f, where = fields(fmt, rng)
        if rng.random() < mutated:
            out.append(mutate(fmt, f, where, rng.choice(MUTATIONS), rng))
        else:
            sep = b"," if fmt == 3 else b"\t"
            out.append(sep.join(f))
    return out


def join_lines(lines, seed, last_terminated=True):
    """terminators of all three kinds, mixed.  (An empty line behind a lone "\\r" that ends in "\\n" reads as one "\\r\\n": what the text holds is what lines_of says.)"""
    rng = random.Random(seed)
    parts = []
    for i, l in enumerate(lines):
        parts.append(l)
        if i + 1 < len(lines) or last_terminated:
            parts.append(rng.choice([b"\n", b"\n", b"\r\n", b"\r"]))
    return b"".join(parts)


def corpus(fmt, n, seed, **kw):
    return join_lines(corpus_lines(fmt, n, seed, **kw), seed + 1)


def check_not_vacuous(info, n_records):
    assert info["ok"] * 2 >= n_records and info["bad_fields"] >= 100 and info["bad_parse"] >= 100, info
