"""A second reading of the .matrix reader's rule (include/dge.h, ".matrix adjacency text in"), in plain Python and written from the header's text: bytes in;
out either the entries and counters, or the offence at the least (piece, offset).  It walks lines and bytes one at a time and shares nothing with
csrc/matrix_parse.h."""

BAD_BYTE, EMPTY_VALUE, LONG_VALUE, BIG_VALUE, RAGGED, ROWS_MANY, ROWS_FEW = range(1, 8)       # the header's order: it decides between two at one place
NAMES = {BAD_BYTE: "bad byte", EMPTY_VALUE: "empty value", LONG_VALUE: "long value", BIG_VALUE: "value above 2^40", RAGGED: "ragged line",
         ROWS_MANY: "too many rows", ROWS_FEW: "too few rows"}
ERR_RANGE, ERR_IO = 2, 7
MAX_VALUE = 2 ** 40


class Offence(Exception):
    def __init__(self, kind, piece, offset, line, column):
        super().__init__("%s at piece %d, offset %d, line %d, column %d" % (NAMES[kind], piece, offset, line, column))
        self.kind, self.piece, self.offset, self.line, self.column = kind, piece, offset, line, column
        self.status = ERR_RANGE if kind == BIG_VALUE else ERR_IO

    def key(self):
        return (self.status, NAMES[self.kind], self.piece, self.offset, self.line, self.column)


def _lines(text):
    """(start, end of the content, has a terminator) of every line; the terminator's first byte stands at `end`"""
    out, pos, size = [], 0, len(text)
    while pos < size:
        nl = text.find(b"\n", pos)
        if nl < 0:
            out.append((pos, size, False))
            break
        end = nl - 1 if nl > pos and text[nl - 1] == 13 else nl
        out.append((pos, end, True))
        pos = nl + 1
    return out


def read_piece(text, n, sep):
    """-> (entries [(row, column, value)], lines, rows) of one piece, or raises (kind, offset) through a list of every offence found"""
    text = bytes(text)
    s = sep if isinstance(sep, int) else ord(sep)
    found = []                                    # (offset, kind): every offence of the piece
    entries, rows = [], 0
    lines = _lines(text)
    for start, end, _ in lines:
        if end == start:
            continue                              # a line of zero bytes
        if rows == n:
            found.append((start, ROWS_MANY))
        row = rows
        rows += 1
        col, run, run_at = 0, 0, start
        for i in range(start, end + 1):
            c = text[i] if i < end else -1        # -1: the terminator, or the piece's end
            if 48 <= c <= 57:
                if run == 0:
                    run_at = i
                run += 1
                if run == 20:
                    found.append((i, LONG_VALUE))
                continue
            if 1 <= run <= 19:                    # a value: a maximal run of 1 .. 19 digits
                v = int(text[run_at:i])
                if v > MAX_VALUE:
                    found.append((run_at, BIG_VALUE))
                elif v > 0:
                    entries.append((row, col, v))
            run = 0
            if c == s:
                if i == start or text[i - 1] == s:
                    found.append((i, EMPTY_VALUE))
                col += 1
            elif c == -1:
                if text[i - 1] == s:
                    found.append((i, EMPTY_VALUE))
            else:
                found.append((i, BAD_BYTE))
        if col + 1 != n:
            found.append((end, RAGGED))
    if rows < n:
        found.append((len(text), ROWS_FEW))
    return entries, len(lines), rows, found


def where(text, offset, sep):
    s = bytes([sep if isinstance(sep, int) else ord(sep)])
    text = bytes(text)
    line_start = text.rfind(b"\n", 0, offset) + 1
    return 1 + text.count(b"\n", 0, offset), text.count(s, line_start, offset)


def read(pieces, hours, n, sep):
    """pieces: a list of bytes; hours: one per piece -> dict(entries=[(hour, row, column, value)] in text order, and the counters of dge_matrix_read_info that
    do not depend on the machine).  Raises Offence.  Rows and columns number the selected regions in ascending id."""
    out = dict(entries=[], bytes=0, lines=0, rows=0, values=0, zeros=0, total=0, pieces=len(pieces), n=n)
    for k, (text, hour) in enumerate(zip(pieces, hours)):
        entries, lines, rows, found = read_piece(text, n, sep)
        if found:
            offset, kind = min(found)
            line, column = where(text, offset, sep)
            raise Offence(kind, k, offset, line, column)
        out["entries"] += [(hour, r, c, v) for r, c, v in entries]
        out["bytes"] += len(text); out["lines"] += lines; out["rows"] += rows
    out["values"] = out["rows"] * n
    out["total"] = sum(e[3] for e in out["entries"])
    out["zeros"] = out["values"] - len(out["entries"])
    return out
