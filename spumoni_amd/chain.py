"""The best collinear chain of a read's matches: a windowed dynamic programme over the match records.

This module is the definition (include/spumoni_chain.h states it in words; the kernel of
spumoni_amd/csrc/spx_chain.hip is held to it bit for bit).  The anchors of a read are its match records
(spumoni_amd/mems.py: MATCH_DTYPE) in the order the match kernels write them: x = read_pos, y = ref_pos, l = length
and, with ids, a document D.  Input contract: x + l < 2^32 and y + l < 2^63 for every anchor -- what the match kernels
deliver always satisfies it.

- a candidate predecessor of anchor i is j with i - lookback <= j < i inside the same read;
- dx = x_i - x_j, dy = y_i - y_j, ex = dx + l_i - l_j, ey = dy + l_i - l_j (the differences of the ends), d = |dx - dy|;
- j is eligible when dx >= 1, dy >= 1, ex >= 1, ey >= 1, dx <= max_dist, dy <= max_dist, d <= max_gap and, with ids,
  D_j == D_i;
- its candidate score is c_j = f[j] + min(l_i, ex, ey) - gap_penalty * d, and f[i] = max(l_i, max over eligible j of c_j);
- pred[i] is none (0xFFFFFFFF) when l_i >= every candidate: the anchor alone wins a tie.  Otherwise it is the largest j
  that reaches the maximum, counted from the read's first anchor;
- the best chain ends at the smallest i with the largest f[i]; walking pred from there gives the record: ref_start and
  read_start are y and x of the first anchor, ref_end and read_end y + l and x + l of the last, score = f of the last,
  anchors = how many, first / last = their indices within the read, gap = the sum of d along the chain (saturating at
  2^32 - 1), doc = D of the last anchor or 0xFFFFFFFF without ids;
- a read without anchors: ref_start = 2^64 - 1, doc = 0xFFFFFFFF, every other field 0.

1 <= f[i] <= x_i + l_i < 2^32 follows by induction (min(l_i, ex) <= ex = (x_i + l_i) - (x_j + l_j)), so scores fit
uint32.  The loop below runs on Python integers: it cannot overflow.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

CHAIN_DTYPE = np.dtype([("ref_start", "<u8"), ("ref_end", "<u8"), ("read_start", "<u4"), ("read_end", "<u4"),
                        ("score", "<u4"), ("anchors", "<u4"), ("first", "<u4"), ("last", "<u4"), ("gap", "<u4"),
                        ("doc", "<u4")])
NO_DOC = 0xFFFFFFFF
NO_PRED = 0xFFFFFFFF
UNCHAINED = 2**64 - 1
M32 = 2**32 - 1


class ChainParams(NamedTuple):
    lookback: int = 64
    max_dist: int = 5000
    max_gap: int = 500
    gap_penalty: int = 1


def check_params(params) -> ChainParams:
    p = ChainParams(*(int(v) for v in params)) if params is not None else ChainParams()
    if not 1 <= p.lookback <= 64:
        raise ValueError("lookback must be 1 .. 64")
    if not 1 <= p.max_dist <= 2**31 - 1:
        raise ValueError("max_dist must be 1 .. 2^31 - 1")
    if not 0 <= p.max_gap <= 2**31 - 1:
        raise ValueError("max_gap must be 0 .. 2^31 - 1")
    if not 0 <= p.gap_penalty <= 65535:
        raise ValueError("gap_penalty must be 0 .. 65535")
    return p


def chain_reference(match_offsets, records, params=None, docs=None, count=None):
    """(chains CHAIN_DTYPE[nreads], score uint32[len(records)], pred uint32[len(records)]) of the reads whose anchors are
    records[match_offsets[q]:match_offsets[q + 1]] (the same slices of docs).  score and pred stand at the anchor's index
    in `records`; what lies outside match_offsets[0] .. match_offsets[-1] stays 0 and 0xFFFFFFFF.  match_offsets[0] need
    not be 0.  count: a list whose first element gets the number of eligible pairs added."""
    lookback, max_dist, max_gap, gap_penalty = check_params(params)
    offs = [int(v) for v in np.asarray(match_offsets, dtype=np.uint64)]
    nreads = max(len(offs) - 1, 0)
    records = np.asarray(records)
    X, Y, L = records["read_pos"].tolist(), records["ref_pos"].tolist(), records["length"].tolist()
    D = None if docs is None else np.asarray(docs).tolist()
    chains = np.zeros(nreads, dtype=CHAIN_DTYPE)
    chains["ref_start"] = UNCHAINED
    chains["doc"] = NO_DOC
    score = [0] * len(X)
    pred = [NO_PRED] * len(X)
    gap_to_pred = [0] * len(X)
    eligible = 0
    for q in range(nreads):
        o, e = offs[q], offs[q + 1]
        if e <= o:
            continue
        best_f, best_i = -1, o
        for i in range(o, e):
            xi, yi, li = X[i], Y[i], L[i]
            f, p, pd = li, NO_PRED, 0
            for j in range(max(o, i - lookback), i):  # ascending: `>=` keeps the largest j among equals
                dx = xi - X[j]
                if dx < 1 or dx > max_dist:
                    continue
                dy = yi - Y[j]
                if dy < 1 or dy > max_dist:
                    continue
                ex, ey = dx + li - L[j], dy + li - L[j]
                d = abs(dx - dy)
                if ex < 1 or ey < 1 or d > max_gap or (D is not None and D[j] != D[i]):
                    continue
                eligible += 1
                c = score[j] + min(li, ex, ey) - gap_penalty * d
                if c > li and c >= f:
                    f, p, pd = c, j - o, d
            score[i], pred[i], gap_to_pred[i] = f, p, pd
            if f > best_f:
                best_f, best_i = f, i
        n, gap, first = 1, 0, best_i
        while pred[first] != NO_PRED:
            gap += gap_to_pred[first]
            first = o + pred[first]
            n += 1
        chains[q] = (Y[first], Y[best_i] + L[best_i], X[first], X[best_i] + L[best_i], best_f, n, first - o, best_i - o,
                     min(gap, M32), NO_DOC if D is None else D[best_i])
    if count is not None:
        count[0] += eligible
    return chains, np.array(score, dtype=np.uint32), np.array(pred, dtype=np.uint32)
