"""The alignment of a read along its best chain: every gap between two consecutive anchors filled by an exact
edit-distance dynamic programme.

This module is the definition (include/spumoni_align.h states it in words; the kernels of
spumoni_amd/csrc/spx_align.hip are held to it bit for bit).  A read's anchors, `pred` and its chain record are those of
spumoni_amd/chain.py; R is the read as the walk saw it (the digested read under digestion), T the text the index holds;
characters are compared as plain bytes.

- walk pred from the record's `last` back to `first`.  For every link j -> i, with ex = (x_i + l_i) - (x_j + l_j) and
  ey = (y_i + l_i) - (y_j + l_j): keep = min(l_i, ex, ey) and t = l_i - keep -- the head of anchor i that overlaps j in
  the read or in the text is cut off; an eligible link has keep >= 1;
- the gap of the link is A = R[x_j + l_j : x_i + t], a = len(A) = ex - keep, and B = T[y_j + l_j : y_i + t],
  b = len(B) = ey - keep;
- a gap is filled when a <= max_fill and b <= max_fill.  Its result is (edits, matches): the Levenshtein distance of A
  and B with unit costs, and the largest number of equal-character columns among the alignments of that cost.  Both add up
  along an alignment, so the pair is a lexicographic optimum and unique.  a == 0 or b == 0 gives (max(a, b), 0).  A gap
  that is not filled has edits = UNFILLED and matches = 0;
- the record: spans, anchors and doc from the chain record; matches = l_first + sum of keep + sum of the filled gaps'
  matches; edits = sum of the filled gaps' edits; unfilled = gaps not filled; skipped = sum of max(a, b) over those,
  saturating at 2^32 - 1;
- a read without a chain: ref_start = 2^64 - 1, doc = 0xFFFFFFFF, every other field 0.

The loops below run on Python integers: they cannot overflow.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from .chain import M32, NO_DOC, NO_PRED, UNCHAINED

ALIGN_DTYPE = np.dtype([("ref_start", "<u8"), ("ref_end", "<u8"), ("read_start", "<u4"), ("read_end", "<u4"),
                        ("matches", "<u4"), ("edits", "<u4"), ("anchors", "<u4"), ("unfilled", "<u4"), ("skipped", "<u4"),
                        ("doc", "<u4")])
GAP_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("edits", "<u4"), ("matches", "<u4")])
UNALIGNED = UNCHAINED
UNFILLED = 0xFFFFFFFF
MAX_FILL_LIMIT = 4096


class AlignParams(NamedTuple):
    max_fill: int = 512


def check_params(params) -> AlignParams:
    p = AlignParams(*(int(v) for v in params)) if params is not None else AlignParams()
    if not 1 <= p.max_fill <= MAX_FILL_LIMIT:
        raise ValueError("max_fill must be 1 .. 4096")
    return p


def gap_fill(A, B):
    """(edits, matches) of two byte strings: the lexicographic optimum -- fewest edits, then most matches -- over all
    global alignments, by the full table in plain loops."""
    a, b = len(A), len(B)
    if a == 0 or b == 0:
        return max(a, b), 0
    prev = [(j, 0) for j in range(b + 1)]  # (edits, -matches): tuples compare lexicographically
    for i in range(1, a + 1):
        row = [(i, 0)]
        for j in range(1, b + 1):
            e, m = prev[j - 1]
            best = (e, m - 1) if A[i - 1] == B[j - 1] else (e + 1, m)
            e, m = prev[j]
            if (e + 1, m) < best:
                best = (e + 1, m)
            e, m = row[j - 1]
            if (e + 1, m) < best:
                best = (e + 1, m)
            row.append(best)
        prev = row
    return prev[b][0], -prev[b][1]


def align_reference(reads, read_offsets, text, match_offsets, records, chains, pred, params=None, count=None):
    """(alignments ALIGN_DTYPE[nreads], gap_offsets uint64[nreads + 1], gaps GAP_DTYPE[gap_offsets[-1]]) of the reads
    whose characters are reads[read_offsets[q]:read_offsets[q + 1]], whose anchors are
    records[match_offsets[q]:match_offsets[q + 1]] with pred at the same indices (chain_reference's third result) and
    whose chain is chains[q].  A read's gaps stand in chain order from gap_offsets[q] on.  count: a list whose first
    element gets the table cells added (a * b of every filled gap with a, b >= 1 that is not 1 x 1)."""
    (max_fill,) = check_params(params)
    R = bytes(np.asarray(reads, dtype=np.uint8))
    T = bytes(np.asarray(text, dtype=np.uint8))
    roffs = [int(v) for v in np.asarray(read_offsets, dtype=np.uint64)]
    moffs = [int(v) for v in np.asarray(match_offsets, dtype=np.uint64)]
    nreads = max(len(moffs) - 1, 0)
    records = np.asarray(records)
    X, Y, L = records["read_pos"].tolist(), records["ref_pos"].tolist(), records["length"].tolist()
    P = np.asarray(pred).tolist()
    out = np.zeros(nreads, dtype=ALIGN_DTYPE)
    out["ref_start"] = UNALIGNED
    out["doc"] = NO_DOC
    gap_offsets = [0]
    gaps = []
    cells = 0
    for q in range(nreads):
        c = chains[q]
        n = int(c["anchors"])
        if int(c["ref_start"]) == UNCHAINED or n == 0:
            gap_offsets.append(len(gaps))
            continue
        o, ro = moffs[q], roffs[q]
        i = o + int(c["last"])
        mine = []
        matches = edits = unfilled = skipped = 0
        while P[i] != NO_PRED:
            j = o + P[i]
            ex, ey = X[i] + L[i] - X[j] - L[j], Y[i] + L[i] - Y[j] - L[j]
            keep = min(L[i], ex, ey)
            t = L[i] - keep
            a, b = ex - keep, ey - keep
            assert keep >= 1, (q, i - o, j - o)
            matches += keep
            if a <= max_fill and b <= max_fill:
                A = R[ro + X[j] + L[j]:ro + X[i] + t]
                B = T[Y[j] + L[j]:Y[i] + t]
                assert len(A) == a and len(B) == b, (q, i - o, j - o)
                e, m = gap_fill(A, B)
                edits += e
                matches += m
                if a >= 1 and b >= 1 and (a, b) != (1, 1):
                    cells += a * b
            else:
                e, m = UNFILLED, 0
                unfilled += 1
                skipped += max(a, b)
            mine.append((a, b, e, m))
            i = j
        assert i == o + int(c["first"]) and len(mine) == n - 1, (q, i - o, len(mine), n)
        matches += L[i]
        gaps.extend(reversed(mine))
        gap_offsets.append(len(gaps))
        out[q] = (c["ref_start"], c["ref_end"], c["read_start"], c["read_end"], matches, edits, n, unfilled, min(skipped, M32), c["doc"])
    if count is not None:
        count[0] += cells
    return out, np.array(gap_offsets, dtype=np.uint64), np.array(gaps, dtype=GAP_DTYPE).reshape(-1)
