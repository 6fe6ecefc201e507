"""A read's extended alignment in the coordinates of the sequence it lies on: which sequence, which strand, where in it,
and the CIGAR along that sequence's forward strand -- what a line of PAF says.

This module is the definition (include/spumoni_map.h states it in words; the kernels of spumoni_amd/csrc/spx_map.hip are
held to it bit for bit).  The input is what extend.py gives per read -- the record and the entries -- with the read's
length `len`; per index the piece starts P[0 .. np] with P[np] = n_text, and `strands`.  Without digestion `build` lays
every sequence out as its forward piece followed at once, when strands == 2, by its reverse complement: piece p belongs to
sequence p // strands, is the reverse piece when p % strands == 1, and Lp = P[p + 1] - P[p] is the sequence's length.

For an aligned read:

1. the entries other than 'S' are expanded into columns, in order; a column has an operation and a text position t:
   ref_start plus the text characters consumed before it.  A text-consuming column ('=', 'X', 'D', 'N') lies in the piece
   that holds its t;
2. the home piece is the piece with the most '=' columns, among equals the lowest p;
3. the kept part runs from the first '=' column in the home piece through the last one, with every column between them
   (text positions are monotone: all of them lie in the home piece).  Read-consuming columns in front of it join the left
   clip, those behind it the right clip; text-only columns outside it disappear;
4. the record (MAPPING_DTYPE): target_start = t_first - P[p] and target_end = t_last + 1 - P[p], on a reverse piece
   Lp - end and Lp - start; seq and strand; read_start and read_end of the kept part in the read as given; matches ('=')
   and edits (X + I + D; 'N' is not counted) and block (the columns other than 'N') over the kept columns; cut: bit 0 when a
   column other than 'S' was removed on the left in text order, bit 1 when on the right;
5. the entries: the left clip, the kept operations and the right clip, merged and split by cigar.pack_runs; on a reverse
   piece the whole list is reversed, so that the operations run along the forward sequence;
6. a read that extend left unaligned has seq = UNMAPPED, zeros elsewhere and no entries.

Every input is checked the way the device checks it (check_read below): a read that fails comes back unmapped and
count["error"] is set.

What follows from the rule, over a mapped read's entries: '=', 'X', 'I' and 'S' add up to len; '=', 'X', 'D' and 'N' to
target_end - target_start, which is at most Lp; the first and the last entry that is not 'S' are '='.

The loops below run on Python integers: they cannot overflow.
"""
from __future__ import annotations

import bisect
import sys

import numpy as np

from .align import UNALIGNED
from .cigar import OP_D, OP_EQ, OP_I, OP_N, OP_X, pack_runs
from .extend import OP_S

UNMAPPED = 0xFFFFFFFF
CUT_LEFT, CUT_RIGHT = 1, 2
MAPPING_DTYPE = np.dtype([("target_start", "<u8"), ("target_end", "<u8"), ("seq", "<u4"), ("strand", "<u4"),
                          ("read_start", "<u4"), ("read_end", "<u4"), ("matches", "<u4"), ("edits", "<u4"),
                          ("block", "<u4"), ("cut", "<u4")])
assert MAPPING_DTYPE.itemsize == 48
_READ_OPS = (OP_EQ, OP_X, OP_I)
_TEXT_OPS = (OP_EQ, OP_X, OP_D, OP_N)
_OPS = (OP_I, OP_D, OP_N, OP_S, OP_EQ, OP_X)


def piece_starts(seq_lengths, strands):
    """P[0 .. np]: every sequence's forward piece and, with strands == 2, its reverse piece behind it."""
    if strands not in (1, 2):
        raise ValueError("strands must be 1 or 2")
    P = [0]
    for n in seq_lengths:
        n = int(n)
        if n <= 0:
            raise ValueError("a sequence of the table has length 0")
        for _ in range(strands):
            P.append(P[-1] + n)
    return P


def check_read(rec, entries, length, n_text):
    """(lead, ops) of an aligned read whose record and entries pass the device's checks, else None: the spans lie in
    [0, len] and [0, n_text] in order, below 2^32 in the read; every operation is one of the six; the 'S' in front of the
    first other entry add up to read_start, those behind the last to len - read_end, and none stands between; the
    read-consuming entries add up to read_end - read_start and the text-consuming ones to ref_end - ref_start; there is an
    '=' of length >= 1.  ops: [(op, n)] of the entries other than 'S'."""
    rs, re_, ts, te = int(rec["read_start"]), int(rec["read_end"]), int(rec["ref_start"]), int(rec["ref_end"])
    if length > 0xFFFFFFFF or not (rs <= re_ <= length) or not (ts <= te <= n_text):
        return None
    lead = tail = rsum = tsum = eq = 0
    ops = []
    for e in entries:
        op, n = int(e) & 15, int(e) >> 4
        if op not in _OPS:
            return None
        if op == OP_S:
            if not ops:
                lead += n
            else:
                tail += n
            continue
        if tail:
            return None
        ops.append((op, n))
        rsum += n if op in _READ_OPS else 0
        tsum += n if op in _TEXT_OPS else 0
        eq += n if op == OP_EQ else 0
    if lead != rs or rsum != re_ - rs or tail != length - re_ or tsum != te - ts or eq == 0:
        return None
    return lead, ops


def map_read(rec, entries, length, P, strands):
    """(mapping tuple in MAPPING_DTYPE's order, entries) of one aligned read, or None when it fails check_read."""
    checked = check_read(rec, entries, length, P[-1])
    if checked is None:
        return None
    lead, ops = checked
    # 1. columns
    col_op, col_t, col_piece = [], [], []
    t = int(rec["ref_start"])
    for op, n in ops:
        for _ in range(n):
            col_op.append(op)
            col_t.append(t)
            col_piece.append(bisect.bisect_right(P, t) - 1 if op in _TEXT_OPS else -1)
            t += op in _TEXT_OPS
    # 2. home piece
    eq_count = {}
    for op, p in zip(col_op, col_piece):
        if op == OP_EQ:
            eq_count[p] = eq_count.get(p, 0) + 1
    home = min(eq_count, key=lambda p: (-eq_count[p], p))
    # 3. kept part
    in_home = [k for k in range(len(col_op)) if col_op[k] == OP_EQ and col_piece[k] == home]
    k0, k1 = in_home[0], in_home[-1]
    kept = col_op[k0:k1 + 1]
    left = lead + sum(op in _READ_OPS for op in col_op[:k0])
    right = (length - int(rec["read_end"])) + sum(op in _READ_OPS for op in col_op[k1 + 1:])
    # 4. record
    start, end = col_t[k0] - P[home], col_t[k1] + 1 - P[home]
    Lp = P[home + 1] - P[home]
    strand = home % strands
    if strand:
        start, end = Lp - end, Lp - start
    matches = sum(op == OP_EQ for op in kept)
    edits = sum(op in (OP_X, OP_I, OP_D) for op in kept)
    block = sum(op != OP_N for op in kept)
    cut = (CUT_LEFT if k0 > 0 else 0) | (CUT_RIGHT if k1 + 1 < len(col_op) else 0)
    # 5. entries
    out = pack_runs([(OP_S, left)] + [(op, 1) for op in kept] + [(OP_S, right)])
    if strand:
        out.reverse()
    return (start, end, home // strands, strand, left, length - right, matches, edits, block, cut), out


def map_reference(records, op_offsets, entries, read_offsets, piece_starts_, strands, count=None):
    """(mappings MAPPING_DTYPE[nreads], op_offsets uint64[nreads + 1], entries uint32[op_offsets[-1]]) of
    extend_reference's (records, op_offsets, entries) and the reads' offsets.  piece_starts_: P[0 .. np], P[np] = n_text.
    count: a dict that gets "mapped", "cut", "reverse", "entries_in", "entries_out", "cut_chars" added and "error" set."""
    P = [int(v) for v in piece_starts_]
    ooffs = [int(v) for v in np.asarray(op_offsets, dtype=np.uint64)]
    roffs = [int(v) for v in np.asarray(read_offsets, dtype=np.uint64)]
    nreads = len(records)
    out = np.zeros(nreads, dtype=MAPPING_DTYPE)
    out["seq"] = UNMAPPED
    out_offsets = [0]
    out_entries = []
    stats = {"mapped": 0, "cut": 0, "reverse": 0, "entries_in": 0, "entries_out": 0, "cut_chars": 0, "error": 0}
    for q in range(nreads):
        rec = records[q]
        if int(rec["ref_start"]) != UNALIGNED:
            length = roffs[q + 1] - roffs[q]
            mine = entries[ooffs[q]:ooffs[q + 1]]
            res = map_read(rec, mine, length, P, strands)
            if res is None:
                stats["error"] = 1
            else:
                m, ents = res
                out[q] = m
                out_entries += ents
                stats["mapped"] += 1
                stats["cut"] += m[9] != 0
                stats["reverse"] += m[3]
                stats["entries_in"] += len(mine)
                stats["entries_out"] += len(ents)
                stats["cut_chars"] += (m[4] - int(rec["read_start"])) + (int(rec["read_end"]) - m[5])
        out_offsets.append(len(out_entries))
    if count is not None:
        for k, v in stats.items():
            count[k] = (count.get(k, 0) | int(v)) if k == "error" else count.get(k, 0) + int(v)
    return out, np.array(out_offsets, dtype=np.uint64), np.array(out_entries, dtype=np.uint32)


# ---- the sequence table, <prefix>.fa.seqs ------------------------------------------------------------------------------
_WHITESPACE = b" \t\n\r\x0b\x0c"


def sequence_name(header, ordinal):
    """The name of a sequence: the header's bytes behind '>' up to the first ASCII whitespace; seq<ordinal> (1-based over
    all files) for an empty name or a sequence without a header (header None)."""
    name = b""
    if header is not None:
        header = bytes(header)
        end = len(header)
        for i, c in enumerate(header):
            if c in _WHITESPACE:
                end = i
                break
        name = header[:end]
    return name if name else b"seq%d" % ordinal


def seq_table_bytes(names, lengths, strands):
    """The table's bytes: name<TAB>length<TAB>text_start<TAB>strands per non-empty sequence, in text order.  Duplicate names
    are kept and reported with one warning on stderr."""
    if strands not in (1, 2):
        raise ValueError("strands must be 1 or 2")
    lines = []
    start = 0
    seen, dup = set(), 0
    for name, n in zip(names, lengths):
        n = int(n)
        if n == 0:
            continue
        name = bytes(name)
        dup += name in seen
        seen.add(name)
        lines.append(name + b"\t%d\t%d\t%d\n" % (n, start, strands))
        start += n * strands
    if dup:
        print(f"warning: {dup} sequence name(s) occur more than once in the sequence table", file=sys.stderr)
    return b"".join(lines)


def write_seq_table(path, names, lengths, strands):
    data = seq_table_bytes(names, lengths, strands)
    with open(path, "wb") as f:
        f.write(data)


def read_seq_table(path, n_text=None):
    """(names [bytes], lengths [int], strands) of a table; ValueError on a malformed line, on lines that disagree in strands,
    on a text_start that is not where the sequences before it end and, with n_text, on a total that is not n_text."""
    names, lengths = [], []
    strands = None
    start = 0
    with open(path, "rb") as f:
        for i, line in enumerate(f.read().split(b"\n")):
            if not line:
                continue
            parts = line.split(b"\t")
            try:
                if len(parts) != 4 or not parts[0]:
                    raise ValueError
                n, s, k = int(parts[1]), int(parts[2]), int(parts[3])
            except ValueError:
                raise ValueError(f"{path}: line {i + 1} is not name<TAB>length<TAB>text_start<TAB>strands") from None
            if k not in (1, 2) or (strands is not None and k != strands) or n <= 0 or s != start:
                raise ValueError(f"{path}: line {i + 1}: strands, length or text_start do not fit the lines before it")
            strands = k
            names.append(parts[0])
            lengths.append(n)
            start += n * k
    if strands is None:
        raise ValueError(f"{path}: no sequences")
    if n_text is not None and start != n_text:
        raise ValueError(f"{path}: the sequences add up to {start} characters, the text has {n_text}")
    return names, lengths, strands
