"""A second reading of the count-table reader's rule (include/dge.h: dge_counts_add_table_texts) in plain Python, byte by byte: re.finditer for the
terminators, bytes.split for the fields, int() for the numbers, dicts for the table.  Nothing is shared with csrc/table_parse.h.  The tests of the host build
(test_counts_host.py) and of the device (test_gpu_counts.py) compare with it; test_counts_ref.py shows it sound against a loop written from the reference."""
import re

import numpy as np

SHORT_LINE, SHORT_KEY, BAD_KEY, KEY_SIGN, EMPTY_VALUE, BAD_VALUE_BYTE, LONG_VALUE, BIG_VALUE, LONG_LINE = range(1, 10)
KIND_NAME = ["", "short line", "short key", "bad key", "key sign", "empty value", "bad value byte", "long value", "value above 2^40", "long line"]
MAX_LINE = 65536
MAX_VALUE = 2 ** 40
DIGITS = b"0123456789"


class Offence(Exception):
    def __init__(self, kind, piece, offset, line, field):
        super().__init__("%s at piece %d, offset %d, line %d, field %d" % (KIND_NAME[kind], piece, offset, line, field))
        self.kind, self.piece, self.offset, self.line, self.field = kind, piece, offset, line, field

    def tuple(self):
        return self.kind, self.piece, self.offset, self.line, self.field


def lines_of(text):
    """-> [(offset of the first byte, the line without its terminator)]: lines end at "\\r\\n", "\\n" or a lone "\\r"; what follows the last terminator is a
    line when it holds a byte"""
    out, at = [], 0
    for m in re.finditer(rb"\r\n|\n|\r", text):
        out.append((at, text[at:m.start()]))
        at = m.end()
    if at < len(text):
        out.append((at, text[at:]))
    return out


def line_offences(line, sep, key_field, key, cols, neg_ok):
    """every offence of one non-empty line as (offset in the line, kind, field), and (key, negative) when the key is good"""
    lo, n = cols
    if len(line) > MAX_LINE:
        return [(0, LONG_LINE, 0)], None
    fields = line.split(sep)
    starts = [0]
    for f in fields[:-1]:
        starts.append(starts[-1] + len(f) + 1)
    found, parsed = [], None
    if len(fields) < max(key_field, lo + n - 1) + 1:
        found.append((len(line), SHORT_LINE, len(fields) - 1))
    if key_field < len(fields):
        f, at = fields[key_field], starts[key_field]
        if len(f) < key[0] + 1:
            found.append((at, SHORT_KEY, key_field))
        else:
            part = f[key[0]:key[1]] if key[1] else f[key[0]:]
            at += key[0]
            neg = part[:1] == b"-"
            if neg and not neg_ok:
                found.append((at, KEY_SIGN, key_field))
            else:
                if neg:
                    part, at = part[1:], at + 1
                bad = next((i for i in range(len(part)) if part[i] not in DIGITS or i == 18), None)
                if len(part) == 0:
                    found.append((at, BAD_KEY, key_field))
                elif bad is not None:
                    found.append((at + bad, BAD_KEY, key_field))
                else:
                    parsed = (int(part), neg)
    for j in range(n):
        if lo + j >= len(fields):
            break
        f, at = fields[lo + j], starts[lo + j]
        if len(f) == 0:
            found.append((at, EMPTY_VALUE, lo + j))
            continue
        bad = next((i for i in range(len(f)) if f[i] not in DIGITS), len(f))
        if bad > 19:                                   # twenty digits in front of anything else
            found.append((at + 19, LONG_VALUE, lo + j))
        elif bad < len(f):
            found.append((at + bad, BAD_VALUE_BYTE, lo + j))
        elif int(f) > MAX_VALUE:
            found.append((at, BIG_VALUE, lo + j))
    return found, parsed


def read(pieces, ids, n_table_cols, sep=",", skip_lines=0, key_field=0, key=(0, 0), cols=(1, 1), col_offset=0, neg_col_offset=None):
    """pieces: a list of bytes; ids: the regions' ids -> dict(table int64 [R, C], entries [(row, col, value)], and the counters of dge_table_read_info that do
    not depend on the transport); raises the Offence at the least (piece, offset), the first of the list among those at one place"""
    sep = sep.encode() if isinstance(sep, str) else sep
    row_of = {int(t): i for i, t in enumerate(sorted(int(t) for t in ids))}
    cells, entries = {}, []
    info = dict(bytes=sum(len(p) for p in pieces), lines=0, skipped=0, empty=0, rows=0, foreign=0, values=0, total=0, pieces=len(pieces))
    for k, text in enumerate(pieces):
        for number, (at, line) in enumerate(lines_of(text), 1):
            info["lines"] += 1
            if number <= skip_lines:
                info["skipped"] += 1
                continue
            if len(line) == 0:
                info["empty"] += 1
                continue
            found, parsed = line_offences(line, sep, key_field, key, cols, neg_col_offset is not None)
            if found:
                off, kind, field = min(found)
                raise Offence(kind, k, at + off, number, field)
            tid, neg = parsed
            if tid not in row_of:
                info["foreign"] += 1
                continue
            info["rows"] += 1
            base = neg_col_offset if neg else col_offset
            for j, f in enumerate(line.split(sep)[cols[0]:cols[0] + cols[1]]):
                v = int(f)
                cells[(row_of[tid], base + j)] = cells.get((row_of[tid], base + j), 0) + v
                entries.append((row_of[tid], base + j, v))
                info["total"] += v
    info["values"] = info["rows"] * cols[1]
    table = np.zeros((len(row_of), n_table_cols), np.int64)
    for (r, c), v in cells.items():
        table[r, c] = v
    return dict(table=table, entries=entries, **info)


def lehd_text(tracts, n_lines, seed, runs=True, header=True, fields=43, terminator=b"\n"):
    """A RAC / WAC shaped text: "h_geocode,C000,..,createdate" and n_lines block lines whose first field is 17031 + a tract of six digits + a block of four,
    42 more numeric fields behind it; the tracts come in sorted runs (runs=True) or shuffled"""
    rng = np.random.default_rng(seed)
    picks = np.sort(rng.integers(0, len(tracts), n_lines)) if runs else rng.integers(0, len(tracts), n_lines)
    out = [b",".join(b"f%d" % i for i in range(fields))] if header else []
    for i, t in enumerate(picks):
        vals = rng.integers(0, 500, fields - 2)
        out.append(b"17031%06d%04d," % (tracts[t], i % 10000) + b",".join(b"%d" % v for v in vals) + b",20160219")
    return terminator.join(out) + terminator
