"""Per-base depth and mismatch counts along every sequence's forward strand, and what they add up to per sequence: the
coverage of a batch of mappings, accumulated over any number of batches.

This module is the definition (include/spumoni_cover.h states it in words; the kernels of spumoni_amd/csrc/spx_cover.hip
are held to it bit for bit).  Per index the input is the sequence table's lengths L[0 .. n_seqs): F[s] is the sum of the
lengths before sequence s and G = F[n_seqs] the length of the forward genome.  Per read the input is map.py's output: a
record of MAPPING_DTYPE and the read's entries (length << 4 | op).

A mapped read (seq = s, target_start = a, target_end = b) is walked from pos = a over its entries other than 'S', in
order -- they run along the forward strand on either strand:

    '=' n        depth[F[s] + pos .. + n) += 1, then pos += n
    'X' n        the same, and mism[...] += 1 over the same range
    'D', 'N' n   pos += n: a deleted or skipped base is not covered
    'I' n        nothing per base

and per sequence reads[s] += 1 and indels[s] += the 'I' and 'D' lengths.  The strand field does not enter the rule; an
unmapped read (seq = UNMAPPED) adds nothing.

Every input is checked the way the device checks it (check_read below): a read that fails is skipped whole -- it leaves
no partial sums -- and count["error"] is set.

The arrays: diff uint32[G + 1] is the difference array of depth (depth[i] = diff[0] + .. + diff[i], in 32-bit modular
arithmetic: diff[G] closes the last interval), mism uint32[G], counts uint64[n_seqs, 2] = (reads, indels).  Fewer than
2^32 mapped reads are added between two resets, so no depth wraps.  All of them are sums: the same input gives the same
bytes in any order of adds.

The loops below run on Python integers: they cannot overflow.
"""
from __future__ import annotations

import numpy as np

from .cigar import OP_D, OP_EQ, OP_I, OP_N, OP_X
from .extend import OP_S
from .map import UNMAPPED

SEQ_COVER_DTYPE = np.dtype([("covered", "<u8"), ("bases", "<u8"), ("mismatches", "<u8"), ("indels", "<u8"), ("reads", "<u8"),
                            ("max_depth", "<u4"), ("reserved", "<u4")])
RUN_DTYPE = np.dtype([("start", "<u8"), ("end", "<u8"), ("seq", "<u4"), ("depth", "<u4"), ("mismatches", "<u4"),
                      ("reserved", "<u4")])
assert SEQ_COVER_DTYPE.itemsize == 48 and RUN_DTYPE.itemsize == 32
_TEXT_OPS = (OP_EQ, OP_X, OP_D, OP_N)
_OPS = (OP_I, OP_D, OP_N, OP_S, OP_EQ, OP_X)
_MASK = 0xFFFFFFFF


def seq_starts(seq_lengths):
    """F[0 .. n_seqs]: where every sequence starts in the forward genome, and G behind the last."""
    F = [0]
    for n in seq_lengths:
        n = int(n)
        if n <= 0:
            raise ValueError("a sequence of the table has length 0")
        F.append(F[-1] + n)
    return F


def check_read(rec, entries, F):
    """(ops, indels) of a mapped read that passes the device's checks, else None: seq is below n_seqs; target_start <=
    target_end <= L[seq]; every operation is one of the six; no 'S' stands between two other entries; the text-consuming
    lengths add up to target_end - target_start.  ops: [(op, n)] of the entries other than 'S'."""
    return _check(int(rec["seq"]), int(rec["target_start"]), int(rec["target_end"]), [int(e) for e in entries], F)


def _check(s, a, b, entries, F):
    if s >= len(F) - 1 or not (a <= b <= F[s + 1] - F[s]):
        return None
    ops = []
    tail = False
    tsum = indels = 0
    for e in entries:
        op, n = e & 15, e >> 4
        if op not in _OPS:
            return None
        if op == OP_S:
            tail = bool(ops)
            continue
        if tail:
            return None
        ops.append((op, n))
        tsum += n if op in _TEXT_OPS else 0
        indels += n if op in (OP_I, OP_D) else 0
    if tsum != b - a:
        return None
    return ops, indels


def cover_reference(mappings, op_offsets, entries, seq_lengths, into=None, count=None, in_entries=None):
    """(diff uint32[G + 1], mism uint32[G], counts uint64[n_seqs, 2]) after map_reference's (mappings, op_offsets,
    entries) have been added to `into` (such a triple; None: zeros).  `into` is left as it is.  in_entries: how many
    entries there are (default: entries.size); a read whose offsets decrease or end beyond it is skipped.
    count: a dict that gets "reads", "mapped", "added", "skipped", "intervals", "atomics" added and "error" set --
    intervals: the maximal stretches of '=' and 'X' columns between two 'D' / 'N' (or the read's ends); atomics: two per
    interval and one per 'X' column."""
    F = seq_starts(seq_lengths)
    G, n_seqs = F[-1], len(F) - 1
    if into is None:
        diff, mism, counts = np.zeros(G + 1, dtype=np.uint32), np.zeros(G, dtype=np.uint32), np.zeros((n_seqs, 2), dtype=np.uint64)
    else:
        diff, mism, counts = (np.array(a, copy=True) for a in into)
        assert diff.shape == (G + 1,) and mism.shape == (G,) and counts.shape == (n_seqs, 2)
    entries = np.asarray(entries, dtype=np.uint32).tolist()
    if in_entries is None:
        in_entries = len(entries)
    ooffs = np.asarray(op_offsets, dtype=np.uint64).tolist()
    seqs, starts, ends = (np.asarray(mappings[f]).tolist() for f in ("seq", "target_start", "target_end"))
    stats = {"reads": len(mappings), "mapped": 0, "added": 0, "skipped": 0, "intervals": 0, "atomics": 0, "error": 0}
    per_seq = {}
    d, x = {}, {}  # position -> what the batch adds to diff and to mism there
    for q in range(len(mappings)):
        s = seqs[q]
        if s == UNMAPPED:
            continue
        stats["mapped"] += 1
        i0, i1 = ooffs[q], ooffs[q + 1]
        checked = _check(s, starts[q], ends[q], entries[i0:i1], F) if i0 <= i1 <= in_entries else None
        if checked is None:
            stats["skipped"] += 1
            stats["error"] = 1
            continue
        ops, indels = checked
        pos = F[s] + starts[q]
        open_at = None
        for op, n in ops:
            if op in (OP_EQ, OP_X):
                if open_at is None:
                    open_at = pos
                if op == OP_X:
                    for at in range(pos, pos + n):
                        x[at] = x.get(at, 0) + 1
                    stats["atomics"] += n
                pos += n
            elif op in (OP_D, OP_N):
                if open_at is not None:
                    d[open_at] = d.get(open_at, 0) + 1
                    d[pos] = d.get(pos, 0) - 1
                    stats["intervals"] += 1
                    open_at = None
                pos += n
        if open_at is not None:
            d[open_at] = d.get(open_at, 0) + 1
            d[pos] = d.get(pos, 0) - 1
            stats["intervals"] += 1
        per_seq[s] = [v + w for v, w in zip(per_seq.get(s, (0, 0)), (1, indels))]
        stats["added"] += 1
    stats["atomics"] += 2 * stats["intervals"]
    for at, v in d.items():
        diff[at] = (int(diff[at]) + v) & _MASK
    for at, v in x.items():
        mism[at] = (int(mism[at]) + v) & _MASK
    for s, (v, w) in per_seq.items():
        counts[s, 0] += np.uint64(v)
        counts[s, 1] += np.uint64(w)
    if count is not None:
        for k, v in stats.items():
            count[k] = (count.get(k, 0) | int(v)) if k == "error" else count.get(k, 0) + int(v)
    return diff, mism, counts


def depth_of(diff):
    """depth uint32[G]: the running sum of diff in 32-bit modular arithmetic."""
    return (np.cumsum(np.asarray(diff, dtype=np.uint32)[:-1].astype(np.uint64)) & np.uint64(_MASK)).astype(np.uint32)


def summary_reference(diff, mism, counts, seq_lengths):
    """SEQ_COVER_DTYPE[n_seqs]: per sequence the positions with depth > 0, the sums of depth and of mism, indels, reads
    and the largest depth."""
    F = seq_starts(seq_lengths)
    depth = depth_of(diff)
    out = np.zeros(len(F) - 1, dtype=SEQ_COVER_DTYPE)
    for s in range(len(F) - 1):
        dd, mm = depth[F[s]:F[s + 1]], np.asarray(mism)[F[s]:F[s + 1]]
        out[s] = (int((dd > 0).sum()), int(dd.sum(dtype=np.uint64)), int(mm.sum(dtype=np.uint64)), int(counts[s][1]), int(counts[s][0]),
                  int(dd.max()), 0)
    return out


def runs_reference(depth, mism, seq_lengths, min_depth=1):
    """RUN_DTYPE[]: inside each sequence the maximal runs of equal depth with depth >= min_depth, in (sequence, start)
    order; start and end are positions in the sequence, mismatches is the sum of mism over the run modulo 2^32.  With
    min_depth 0 the runs of a sequence partition it; a run never crosses a sequence border."""
    F = seq_starts(seq_lengths)
    depth, mism = np.asarray(depth, dtype=np.uint32), np.asarray(mism, dtype=np.uint32)
    G = F[-1]
    assert depth.shape == (G,) and mism.shape == (G,)
    first = np.zeros(G, dtype=bool)
    first[np.array(F[:-1], dtype=np.int64)] = True
    first[1:] |= depth[1:] != depth[:-1]
    starts = np.flatnonzero(first)
    ends = np.r_[starts[1:], G]
    sums = np.r_[0, np.cumsum(mism.astype(np.uint64))]
    seq = np.searchsorted(np.array(F, dtype=np.int64), starts, side="right") - 1
    keep = depth[starts] >= min_depth
    out = np.zeros(int(keep.sum()), dtype=RUN_DTYPE)
    base = np.array(F, dtype=np.int64)[seq[keep]]
    out["start"] = starts[keep] - base
    out["end"] = ends[keep] - base
    out["seq"] = seq[keep]
    out["depth"] = depth[starts[keep]]
    out["mismatches"] = ((sums[ends[keep]] - sums[starts[keep]]) & np.uint64(_MASK)).astype(np.uint32)
    return out
