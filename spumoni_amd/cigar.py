"""The path of a read's alignment along its best chain: the alignment of spumoni_amd/align.py with every operation
named, as a CIGAR.

This module is the definition (include/spumoni_cigar.h states it in words; the kernels of
spumoni_amd/csrc/spx_cigar.hip are held to it bit for bit).  Anchors, pred, links, keep, t, the gaps A and B, max_fill
and "filled" are exactly those of align.py.  A read's operations are, in chain order,

1. l_first x '=' for the chain's first anchor;
2. for every link: the operations of its gap, then keep x '='.

A gap's operations: a == 0 gives b x 'D', b == 0 gives a x 'I' (both 0: nothing); a gap that is not filled gives
a x 'I' and then b x 'N'; a filled gap with a, b >= 1 is walked back through its table (gap_path below): W[i][j] is the
word edits << 16 | (0xFFFF - matches) of the align kernels, dir[i][j] the FIRST of diagonal, up, left whose candidate
equals W[i][j], and the path from (a, b) to (0, 0) -- along row 0 left, along column 0 up -- read backwards is the gap's
operations: a diagonal step is '=' on equal characters and 'X' otherwise, an up step 'I', a left step 'D'.  The fixed
order is the only tie rule.

Adjacent equal operations are merged over the whole read, across the borders of anchors and gaps too.  An entry is
length << 4 | op with the BAM codes; a run longer than MAX_LENGTH is written as consecutive entries, all full but the
last.  A read without a chain has no entries.

The loops below run on Python integers: they cannot overflow.
"""
from __future__ import annotations

import numpy as np

from .align import ALIGN_DTYPE, UNALIGNED, align_reference, check_params
from .chain import NO_PRED, UNCHAINED

OP_I, OP_D, OP_N, OP_EQ, OP_X = 1, 2, 3, 7, 8
OP_CHARS = {OP_I: "I", OP_D: "D", OP_N: "N", OP_EQ: "=", OP_X: "X"}
MAX_LENGTH = (1 << 28) - 1
EDIT = 1 << 16


def gap_path(A, B):
    """The operations of a filled gap, one code per step from (0, 0) to (a, b), by the full table in plain loops."""
    a, b = len(A), len(B)
    if a == 0:
        return [OP_D] * b
    if b == 0:
        return [OP_I] * a
    W = [[j * EDIT | 0xFFFF for j in range(b + 1)]]
    for i in range(1, a + 1):
        row = [i * EDIT | 0xFFFF]
        above = W[i - 1]
        for j in range(1, b + 1):
            diag = above[j - 1] - 1 if A[i - 1] == B[j - 1] else above[j - 1] + EDIT
            row.append(min(diag, above[j] + EDIT, row[j - 1] + EDIT))
        W.append(row)
    steps = []
    i, j = a, b
    while i or j:
        if i == 0:
            step = OP_D
        elif j == 0:
            step = OP_I
        else:
            same = A[i - 1] == B[j - 1]
            if W[i][j] == (W[i - 1][j - 1] - 1 if same else W[i - 1][j - 1] + EDIT):
                step = OP_EQ if same else OP_X
            elif W[i][j] == W[i - 1][j] + EDIT:
                step = OP_I
            else:
                assert W[i][j] == W[i][j - 1] + EDIT
                step = OP_D
        steps.append(step)
        i -= step != OP_D
        j -= step != OP_I
    steps.reverse()
    return steps


def runs_of(steps):
    """[(op, length)] of a list of codes, adjacent equal codes merged."""
    runs = []
    for s in steps:
        if runs and runs[-1][0] == s:
            runs[-1][1] += 1
        else:
            runs.append([s, 1])
    return [(op, n) for op, n in runs]


def pack_runs(runs):
    """The entries of [(op, length)]: empty runs dropped, adjacent runs of one operation merged, a merged run longer than
    MAX_LENGTH split into full entries and a last one."""
    merged = []
    for op, n in runs:
        if n == 0:
            continue
        if merged and merged[-1][0] == op:
            merged[-1][1] += n
        else:
            merged.append([op, n])
    entries = []
    for op, n in merged:
        while n > MAX_LENGTH:
            entries.append(MAX_LENGTH << 4 | op)
            n -= MAX_LENGTH
        entries.append(n << 4 | op)
    return entries


def cigar_text(entries) -> str:
    """Entries as text, each printed as it is stored; '*' for none."""
    entries = [int(e) for e in entries]
    return "".join(f"{e >> 4}{OP_CHARS[e & 15]}" for e in entries) if entries else "*"


def cigar_reference(reads, read_offsets, text, match_offsets, records, chains, pred, params=None, count=None):
    """(alignments ALIGN_DTYPE[nreads], op_offsets uint64[nreads + 1], entries uint32[op_offsets[-1]]): the records are
    align_reference's, read q's entries stand from op_offsets[q] on.  The arguments are align_reference's."""
    (max_fill,) = check_params(params)
    out, _, _ = align_reference(reads, read_offsets, text, match_offsets, records, chains, pred, params, count=count)
    assert out.dtype == ALIGN_DTYPE
    R = bytes(np.asarray(reads, dtype=np.uint8))
    T = bytes(np.asarray(text, dtype=np.uint8))
    roffs = [int(v) for v in np.asarray(read_offsets, dtype=np.uint64)]
    moffs = [int(v) for v in np.asarray(match_offsets, dtype=np.uint64)]
    nreads = max(len(moffs) - 1, 0)
    records = np.asarray(records)
    X, Y, L = records["read_pos"].tolist(), records["ref_pos"].tolist(), records["length"].tolist()
    P = np.asarray(pred).tolist()
    op_offsets = [0]
    entries = []
    for q in range(nreads):
        c = chains[q]
        if int(c["ref_start"]) == UNCHAINED or int(c["anchors"]) == 0:
            op_offsets.append(len(entries))
            continue
        assert int(out[q]["ref_start"]) != UNALIGNED
        o, ro = moffs[q], roffs[q]
        i = o + int(c["last"])
        links = []  # from the chain's last link to its first: (runs of the gap, keep)
        while P[i] != NO_PRED:
            j = o + P[i]
            ex, ey = X[i] + L[i] - X[j] - L[j], Y[i] + L[i] - Y[j] - L[j]
            keep = min(L[i], ex, ey)
            t = L[i] - keep
            a, b = ex - keep, ey - keep
            if a <= max_fill and b <= max_fill:
                runs = runs_of(gap_path(R[ro + X[j] + L[j]:ro + X[i] + t], T[Y[j] + L[j]:Y[i] + t]))
            else:
                runs = [(OP_I, a), (OP_N, b)]
            links.append((runs, keep))
            i = j
        runs = [(OP_EQ, L[i])]
        for gap_runs, keep in reversed(links):
            runs += gap_runs
            runs.append((OP_EQ, keep))
        entries += pack_runs(runs)
        op_offsets.append(len(entries))
    return out, np.array(op_offsets, dtype=np.uint64), np.array(entries, dtype=np.uint32)
