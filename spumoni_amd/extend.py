"""A read's alignment taken to the read's ends: the CIGAR of spumoni_amd/cigar.py with both ends extended by a banded
dynamic programme whose end point is free, and what is left of the read on either side as soft clips.

This module is the definition (include/spumoni_extend.h states it in words; the kernels of
spumoni_amd/csrc/spx_extend.hip are held to it bit for bit).  Everything of align.py and cigar.py holds unchanged for the
part between the chain's first and last anchor.  R, T, the record and the entries are as there; `len` is the read's
length in the characters the walk saw, n_text the text's length.

- the right end of an aligned read: a = min(len - read_end, max_extend), A = R[read_end : read_end + a];
  b = min(n_text - ref_end, a + band), B = T[ref_end : ref_end + b];
- the table S[i][j] is defined for 0 <= i <= a, 0 <= j <= b, |j - i| <= band.  S[0][0] = 0; every other cell is the
  largest of its candidates whose source cell is in the table: diagonal S[i-1][j-1] + 1 on equal characters and
  S[i-1][j-1] - mismatch otherwise, up S[i-1][j] - indel, left S[i][j-1] - indel;
- the end point is the cell of the largest S; among equal cells the one with the smallest i + j, among those the one with
  the smallest i.  (0, 0) is a cell: an extension is taken only when it gains;
- the path is walked back from the end point to (0, 0) by the FIRST, in the order diagonal, up, left, of the in-table
  candidates that equals the cell: a diagonal step is '=' or 'X', an up step 'I', a left step 'D'.  The steps are read
  from (0, 0) outwards.  These two fixed orders are the only tie rules;
- the left end is the same table on the reversed strings: a = min(read_start, max_extend), b = min(ref_start, a + band),
  A = reverse(R[read_start - a : read_start]), B = reverse(T[ref_start - b : ref_start]); its steps, read from the end
  point back to (0, 0), are the operations in read order;
- the record: read_start and ref_start move down by the left end point's i and j, read_end and ref_end up by the right
  one's; matches and edits grow by the '=' and by the X + I + D of both paths; the other fields are align's;
- the entries of an aligned read: read_start x 'S' (the new value), the left path, cigar's operations, the right path,
  (len - read_end) x 'S', merged and split by cigar.pack_runs over all those borders.  A read without a chain has no
  entries.

The loops below run on Python integers: they cannot overflow.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from .align import UNALIGNED
from .cigar import OP_CHARS as _CIGAR_CHARS
from .cigar import OP_D, OP_EQ, OP_I, OP_X, cigar_reference, pack_runs

OP_S = 4
OP_CHARS = dict(_CIGAR_CHARS)
OP_CHARS[OP_S] = "S"
END_DTYPE = np.dtype([("read_chars", "<u4"), ("text_chars", "<u4"), ("score", "<i4"), ("edits", "<u4")])
MAX_EXTEND_LIMIT = 4096
BAND_LIMIT = 63


class ExtendParams(NamedTuple):
    max_extend: int = 512
    band: int = 16
    mismatch: int = 4
    indel: int = 6


def check_params(params) -> ExtendParams:
    p = ExtendParams(*(int(v) for v in params)) if params is not None else ExtendParams()
    if not 1 <= p.max_extend <= MAX_EXTEND_LIMIT:
        raise ValueError("max_extend must be 1 .. 4096")
    if not 0 <= p.band <= BAND_LIMIT:
        raise ValueError("band must be 0 .. 63")
    if not 0 <= p.mismatch <= 65535:
        raise ValueError("mismatch must be 0 .. 65535")
    if not 0 <= p.indel <= 65535:
        raise ValueError("indel must be 0 .. 65535")
    return p


def band_cells(a, b, band):
    """The cells of the table of an a x b end but (0, 0): what the device counts as evaluated."""
    return sum(min(b, i + band) - max(0, i - band) + 1 for i in range(a + 1) if i - band <= b) - 1


def end_path(A, B, band, mismatch, indel):
    """(i, j, score, steps) of one end: the end point, its S and the path's codes from (0, 0) outwards, by the banded
    table in plain loops."""
    a, b = len(A), len(B)
    S = {(0, 0): 0}
    best = (0, 0, 0)  # (-score, i + j, i): the smallest wins
    for i in range(a + 1):
        for j in range(max(0, i - band), min(b, i + band) + 1):
            if i == 0 and j == 0:
                continue
            cands = []
            if (i - 1, j - 1) in S:
                cands.append(S[i - 1, j - 1] + 1 if A[i - 1] == B[j - 1] else S[i - 1, j - 1] - mismatch)
            if (i - 1, j) in S:
                cands.append(S[i - 1, j] - indel)
            if (i, j - 1) in S:
                cands.append(S[i, j - 1] - indel)
            S[i, j] = max(cands)
            best = min(best, (-S[i, j], i + j, i))
    score, i = -best[0], best[2]
    j = best[1] - i
    end = (i, j)
    steps = []
    while i or j:
        v = S[i, j]
        if (i - 1, j - 1) in S and v == (S[i - 1, j - 1] + 1 if A[i - 1] == B[j - 1] else S[i - 1, j - 1] - mismatch):
            steps.append(OP_EQ if A[i - 1] == B[j - 1] else OP_X)
            i, j = i - 1, j - 1
        elif (i - 1, j) in S and v == S[i - 1, j] - indel:
            steps.append(OP_I)
            i -= 1
        else:
            assert (i, j - 1) in S and v == S[i, j - 1] - indel
            steps.append(OP_D)
            j -= 1
    steps.reverse()
    return end[0], end[1], score, steps


def cigar_text(entries) -> str:
    """Entries as text, each printed as it is stored; '*' for none."""
    entries = [int(e) for e in entries]
    return "".join(f"{e >> 4}{OP_CHARS[e & 15]}" for e in entries) if entries else "*"


def extend_reference(reads, read_offsets, text, match_offsets, records, chains, pred, params=None, extend_params=None,
                     count=None):
    """(alignments ALIGN_DTYPE[nreads], op_offsets uint64[nreads + 1], entries uint32[op_offsets[-1]], ends
    END_DTYPE[2 * nreads]): cigar_reference's results with both ends extended and the rest clipped; the ends are left
    then right per read, zeros for a read without a chain.  The arguments are cigar_reference's, with the extension's
    parameters behind them.  count: a dict that gets "ends", "extended", "cells" and "clipped" added."""
    max_extend, band, mismatch, indel = check_params(extend_params)
    out, coffs, centries = cigar_reference(reads, read_offsets, text, match_offsets, records, chains, pred, params)
    out = out.copy()
    R = bytes(np.asarray(reads, dtype=np.uint8))
    T = bytes(np.asarray(text, dtype=np.uint8))
    n_text = len(T)
    roffs = [int(v) for v in np.asarray(read_offsets, dtype=np.uint64)]
    nreads = len(out)
    ends = np.zeros(2 * nreads, dtype=END_DTYPE)
    op_offsets = [0]
    entries = []
    stats = {"ends": 0, "extended": 0, "cells": 0, "clipped": 0}
    for q in range(nreads):
        if int(out[q]["ref_start"]) == UNALIGNED:
            op_offsets.append(len(entries))
            continue
        ro, length = roffs[q], roffs[q + 1] - roffs[q]
        rs, re_ = int(out[q]["read_start"]), int(out[q]["read_end"])
        ts, te = int(out[q]["ref_start"]), int(out[q]["ref_end"])
        a = min(rs, max_extend)
        b = min(ts, a + band)
        li, lj, ls, lsteps = end_path(R[ro + rs - a:ro + rs][::-1], T[ts - b:ts][::-1], band, mismatch, indel)
        stats["ends"] += a >= 1
        stats["cells"] += band_cells(a, b, band)
        a = min(length - re_, max_extend)
        b = min(n_text - te, a + band)
        ri, rj, rs_, rsteps = end_path(R[ro + re_:ro + re_ + a], T[te:te + b], band, mismatch, indel)
        stats["ends"] += a >= 1
        stats["cells"] += band_cells(a, b, band)
        stats["extended"] += (li + lj > 0) + (ri + rj > 0)
        both = lsteps + rsteps
        ends[2 * q] = (li, lj, ls, sum(s != OP_EQ for s in lsteps))
        ends[2 * q + 1] = (ri, rj, rs_, sum(s != OP_EQ for s in rsteps))
        out[q]["read_start"], out[q]["ref_start"] = rs - li, ts - lj
        out[q]["read_end"], out[q]["ref_end"] = re_ + ri, te + rj
        out[q]["matches"] += sum(s == OP_EQ for s in both)
        out[q]["edits"] += sum(s != OP_EQ for s in both)
        stats["clipped"] += rs - li + length - re_ - ri
        runs = [(OP_S, rs - li)] + [(s, 1) for s in reversed(lsteps)]
        runs += [(int(e) & 15, int(e) >> 4) for e in centries[int(coffs[q]):int(coffs[q + 1])]]
        runs += [(s, 1) for s in rsteps] + [(OP_S, length - re_ - ri)]
        entries += pack_runs(runs)
        op_offsets.append(len(entries))
    if count is not None:
        for k, v in stats.items():
            count[k] = count.get(k, 0) + int(v)
    return out, np.array(op_offsets, dtype=np.uint64), np.array(entries, dtype=np.uint32), ends
