"""Per-base allele counts along every sequence's forward strand -- the pileup of a batch of mappings, accumulated over any
number of batches beside the coverage -- and the single-nucleotide calls they support.

This module is the definition (include/spumoni_call.h states it in words; the kernels of spumoni_amd/csrc/spx_call.hip
are held to it bit for bit).  Per index the input is the sequence table's lengths L[0 .. n_seqs) -- F[s] is the sum of
the lengths before sequence s, G = F[n_seqs] -- and the text, whose forward piece of sequence s starts at
P[s * strands] = F[s] * strands.  Per read the input is map.py's output -- a record of MAPPING_DTYPE and the read's
entries (length << 4 | op), along the forward strand on either strand -- and the read's bytes as given.

A byte has code 0, 1, 2, 3 for A/a, C/c, G/g, T/t and code 4 ("other") for anything else.  The oriented read is the read
itself on strand 0; on any other strand its position j is read byte len - 1 - j, and a code c < 4 becomes 3 - c.

A mapped read (seq = s, target_start = a, target_end = b) is walked from pos = a, j = 0 over all its entries in order:

    'S' n   j += n
    '=' n   pos += n, j += n
    'X' n   per column: alt[4 * (F[s] + pos) + c] += 1 where c < 4 is the oriented read's code at j, other[F[s] + pos] += 1
            where c = 4; then pos and j advance
    'I' n   ins[F[s] + pos] += 1, j += n: pos is the next text position
    'D' n   del[F[s] + pos .. + n) += 1, kept as one +1 and one -1 in ddiff; pos += n
    'N' n   pos += n

An unmapped read (seq = UNMAPPED) adds nothing.

The checks (check_read below): all of cover.py's; the read-consuming lengths ('=', 'X', 'I', 'S') add up to the read's
length by its offsets; the read's offsets do not decrease and do not end beyond in_chars; and -- what makes "pos is the
next text position" hold for every input -- no 'I' stands behind the last text-consuming column ('=', 'X', 'D', 'N' of
a length above 0), where pos would be b and F[s] + b may be G.  map's mappings end with '=' and never fail it.  A read
that fails is skipped whole and count["error"] is set.

The arrays: alt uint32[4 * G], other uint32[G], ins uint32[G], ddiff uint32[G + 1] in 32-bit modular arithmetic; del is
ddiff's running sum.  All of them are sums: the same input gives the same bytes in any order of adds.

The calls come from depth and mism of cover.py and the arrays above (calls_reference).  No floating point anywhere.
"""
from __future__ import annotations

import numpy as np

from .cigar import OP_D, OP_EQ, OP_I, OP_N, OP_X
from .cover import _check as _cover_check
from .cover import seq_starts
from .extend import OP_S
from .map import UNMAPPED

CALL_DTYPE = np.dtype([("pos", "<u8"), ("seq", "<u4"), ("depth", "<u4"), ("alt", "<u4", (4,)), ("other", "<u4"), ("del", "<u4"),
                       ("ins", "<u4"), ("ref", "u1"), ("allele", "u1"), ("reserved", "<u2")])
assert CALL_DTYPE.itemsize == 48
LETTERS = "ACGT"
_MASK = 0xFFFFFFFF
_CODE = np.full(256, 4, dtype=np.uint8)
for _c, _pair in enumerate(("Aa", "Cc", "Gg", "Tt")):
    for _ch in _pair:
        _CODE[ord(_ch)] = _c


def code_of(byte) -> int:
    """0 .. 3 for A/a, C/c, G/g, T/t; 4 for every other byte."""
    return int(_CODE[int(byte)])


def oriented_codes(read, strand):
    """The codes of the oriented read: the read's own on strand 0, reversed and complemented (4 stays 4) otherwise."""
    codes = _CODE[np.asarray(read, dtype=np.uint8)]
    if strand:
        codes = codes[::-1]
        codes = np.where(codes < 4, 3 - codes, 4).astype(np.uint8)
    return codes


def check_read(rec, entries, read_len, F):
    """[(op, n)] of all the entries of a mapped read that passes the device's checks, else None."""
    return _check(int(rec["seq"]), int(rec["target_start"]), int(rec["target_end"]), [int(e) for e in entries], int(read_len), F)


def _check(s, a, b, entries, read_len, F):
    if _cover_check(s, a, b, entries, F) is None:
        return None
    ops = [(e & 15, e >> 4) for e in entries]
    if sum(n for op, n in ops if op in (OP_EQ, OP_X, OP_I, OP_S)) != read_len:
        return None
    pending = False  # an 'I' with no text column behind it so far
    for op, n in ops:
        if op == OP_I:
            pending = True
        elif op in (OP_EQ, OP_X, OP_D, OP_N) and n > 0:
            pending = False
    return None if pending else ops


def zeros(G):
    """(alt uint32[4 * G], other uint32[G], ins uint32[G], ddiff uint32[G + 1]) of nothing."""
    return (np.zeros(4 * G, dtype=np.uint32), np.zeros(G, dtype=np.uint32), np.zeros(G, dtype=np.uint32),
            np.zeros(G + 1, dtype=np.uint32))


def pileup_reference(mappings, op_offsets, entries, reads, read_offsets, seq_lengths, into=None, count=None, in_entries=None,
                     in_chars=None):
    """(alt, other, ins, ddiff) after map_reference's (mappings, op_offsets, entries) and the reads' bytes (reads uint8,
    read_offsets nreads + 1) have been added to `into` (such a quadruple; None: zeros).  `into` is left as it is.
    in_entries, in_chars: how many entries and read bytes there are (default: the arrays' sizes); a read whose offsets
    decrease or end beyond them is skipped.  count: a dict that gets "reads", "mapped", "added", "skipped", "x_columns"
    (all 'X' columns), "other_columns" (those of code 4), "insertions" ('I' entries), "deletions" ('D' entries) and
    "atomics" (one per 'X' column and per 'I', two per 'D') added and "error" set."""
    F = seq_starts(seq_lengths)
    G = F[-1]
    if into is None:
        alt, other, ins, ddiff = zeros(G)
    else:
        alt, other, ins, ddiff = (np.array(a, copy=True) for a in into)
        assert alt.shape == (4 * G,) and other.shape == (G,) and ins.shape == (G,) and ddiff.shape == (G + 1,)
    entries = np.asarray(entries, dtype=np.uint32).tolist()
    reads = np.asarray(reads, dtype=np.uint8)
    if in_entries is None:
        in_entries = len(entries)
    if in_chars is None:
        in_chars = int(reads.size)
    ooffs = np.asarray(op_offsets, dtype=np.uint64).tolist()
    roffs = np.asarray(read_offsets, dtype=np.uint64).tolist()
    seqs, strands, starts, ends = (np.asarray(mappings[f]).tolist() for f in ("seq", "strand", "target_start", "target_end"))
    stats = {"reads": len(mappings), "mapped": 0, "added": 0, "skipped": 0, "x_columns": 0, "other_columns": 0, "insertions": 0,
             "deletions": 0, "atomics": 0, "error": 0}
    adds = [{}, {}, {}, {}]  # word -> what the batch adds to alt, other, ins, ddiff there

    def bump(which, at, v=1):
        adds[which][at] = adds[which].get(at, 0) + v

    for q in range(len(mappings)):
        s = seqs[q]
        if s == UNMAPPED:
            continue
        stats["mapped"] += 1
        i0, i1, r0, r1 = ooffs[q], ooffs[q + 1], roffs[q], roffs[q + 1]
        ops = None
        if i0 <= i1 <= in_entries and r0 <= r1 <= in_chars:
            ops = _check(s, starts[q], ends[q], entries[i0:i1], r1 - r0, F)
        if ops is None:
            stats["skipped"] += 1
            stats["error"] = 1
            continue
        codes = oriented_codes(reads[r0:r1], strands[q]).tolist()
        pos, j = F[s] + starts[q], 0
        for op, n in ops:
            if op == OP_S:
                j += n
            elif op == OP_EQ:
                pos += n
                j += n
            elif op == OP_X:
                for k in range(n):
                    c = codes[j + k]
                    if c < 4:
                        bump(0, 4 * (pos + k) + c)
                    else:
                        bump(1, pos + k)
                        stats["other_columns"] += 1
                stats["x_columns"] += n
                pos += n
                j += n
            elif op == OP_I:
                bump(2, pos)
                stats["insertions"] += 1
                j += n
            elif op == OP_D:
                bump(3, pos)
                bump(3, pos + n, -1)
                stats["deletions"] += 1
                pos += n
            else:
                pos += n
        stats["added"] += 1
    stats["atomics"] = stats["x_columns"] + stats["insertions"] + 2 * stats["deletions"]
    for arr, d in zip((alt, other, ins, ddiff), adds):
        for at, v in d.items():
            arr[at] = (int(arr[at]) + v) & _MASK
    if count is not None:
        for k, v in stats.items():
            count[k] = (count.get(k, 0) | int(v)) if k == "error" else count.get(k, 0) + int(v)
    return alt, other, ins, ddiff


def del_of(ddiff):
    """del uint32[G]: the running sum of ddiff in 32-bit modular arithmetic."""
    return (np.cumsum(np.asarray(ddiff, dtype=np.uint32)[:-1].astype(np.uint64)) & np.uint64(_MASK)).astype(np.uint32)


def calls_reference(depth, mism, alt, other, ins, dele, text, seq_lengths, strands, min_depth=2, min_alt=2, min_permille=500):
    """CALL_DTYPE[] in (sequence, position) order.  At position i of sequence s, ref is the text byte at P[s * strands] + i;
    the candidates are the codes 0 .. 3 other than ref's own; the called allele is the candidate with the largest alt
    count, the lowest code among equals.  The position is a call when depth >= min_depth, that count >= min_alt and
    count * 1000 >= min_permille * depth.  mism does not enter the decision (depth - mism is the record's reader's
    ref_count)."""
    if not (min_depth >= 1 and min_alt >= 1 and 0 <= min_permille <= 1000):
        raise ValueError("min_depth and min_alt must be at least 1, min_permille between 0 and 1000")
    F = seq_starts(seq_lengths)
    G = F[-1]
    depth, other, ins, dele = (np.asarray(a, dtype=np.uint32) for a in (depth, other, ins, dele))
    alt = np.asarray(alt, dtype=np.uint32).reshape(G, 4)
    text = np.asarray(text, dtype=np.uint8)
    assert depth.shape == other.shape == ins.shape == dele.shape == (G,) and np.asarray(mism).shape == (G,)
    out = []
    for s in range(len(F) - 1):
        p0 = F[s] * strands
        for i in range(F[s + 1] - F[s]):
            g = F[s] + i
            ref = int(text[p0 + i])
            rc = code_of(ref)
            best, cnt = -1, -1
            for c in range(4):
                if c != rc and int(alt[g, c]) > cnt:
                    best, cnt = c, int(alt[g, c])
            d = int(depth[g])
            if d >= min_depth and cnt >= min_alt and cnt * 1000 >= min_permille * d:
                out.append((i, s, d, tuple(int(v) for v in alt[g]), int(other[g]), int(dele[g]), int(ins[g]), ref, best, 0))
    return np.array(out, dtype=CALL_DTYPE)
