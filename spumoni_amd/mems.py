"""The matches of a read: where a new exact match with the text starts and is long enough.

This module is the definition (include/spumoni_mems.h states it in words; the kernels of
spumoni_amd/csrc/spx_mems.hip are held to it bit for bit).  For a read with MS lengths L[0..m) and pointers P[0..m),
as an MS query returns them, and optionally document ids D[0..m):

- position i starts a match when i == 0 or L[i] >= L[i - 1] (the extension gives L[i] >= L[i - 1] - 1, with equality
  exactly where the match of i - 1 merely continues);
- a start is reported when L[i] >= min_length (min_length >= 1: a position of length 0 never comes out);
- the record is (ref_pos = P[i], read_pos = i, length = L[i]), with D[i] in a parallel array when ids are given;
- records are ordered by read, then by read_pos; match_offsets[0..nreads] says where each read's records start;
- the value in front of a read's first position belongs to another read and never counts.

The rule is this project's, and it is a rule on the arrays: where the lengths under-report (after a letter the text
does not have), a reported match is still exact but need not be maximal.
"""
from __future__ import annotations

import numpy as np

MATCH_DTYPE = np.dtype([("ref_pos", "<u8"), ("read_pos", "<u4"), ("length", "<u4")])


def mems_reference(lengths, pointers, offs, min_length, docs=None):
    """(match_offsets uint64[nreads + 1], records MATCH_DTYPE[, docs uint32]) of the reads lengths[offs[q]:offs[q + 1]];
    numpy, vectorised.  offs[0] need not be 0."""
    if int(min_length) < 1:
        raise ValueError("min_length must be at least 1")
    offs = np.asarray(offs, dtype=np.uint64).astype(np.int64)
    nreads = max(offs.size - 1, 0)
    lo, hi = (int(offs[0]), int(offs[-1])) if nreads else (0, 0)
    L = np.asarray(lengths)[lo:hi].astype(np.int64)
    start = np.ones(L.size, dtype=bool)
    start[1:] = L[1:] >= L[:-1]
    counts = np.diff(offs)
    start[offs[:-1][counts > 0] - lo] = True
    at = np.flatnonzero(start & (L >= min(int(min_length), 2**62)))
    read = np.searchsorted(offs, at + lo, side="right") - 1  # (the last read that starts at or before: the non-empty one)
    match_offsets = np.searchsorted(at + lo, offs, side="left").astype(np.uint64)
    rec = np.zeros(at.size, dtype=MATCH_DTYPE)
    rec["ref_pos"] = np.asarray(pointers)[lo:hi].astype(np.uint64)[at]
    rec["read_pos"] = at + lo - offs[read]
    rec["length"] = L[at]
    if docs is None:
        return match_offsets, rec
    return match_offsets, rec, np.asarray(docs)[lo:hi].astype(np.uint32)[at]
