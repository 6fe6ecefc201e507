"""The document votes: one record per read from the per-position lengths and document ids of a query.

This module is the definition (include/spumoni_docvote.h states it in words; the kernels of
spumoni_amd/csrc/spx_docvote.hip are held to it bit for bit).  For a read with values L[0..m) and document ids
D[0..m):

- position i votes when L[i] >= min_length; ``voters`` counts the voting positions;
- ``top_doc`` is the document most voting positions name, the smallest id among equals, ``top_votes`` its count;
- ``second_votes`` is the largest count among the other documents, 0 when there is none;
- a read nobody votes in (an empty read too): all counts 0 and ``top_doc`` = NO_DOC.

The rule is this project's: the reference writes the per-position files and stops.
"""
from __future__ import annotations

import numpy as np

NO_DOC = 0xFFFFFFFF
VOTE_DTYPE = np.dtype([("voters", "<u4"), ("top_doc", "<u4"), ("top_votes", "<u4"), ("second_votes", "<u4")])


def votes_reference(lengths, docs, offs, min_length) -> np.ndarray:
    """Records (VOTE_DTYPE, one per read) of the reads lengths[offs[q]:offs[q + 1]] / docs[...]; numpy, vectorised."""
    offs = np.asarray(offs, dtype=np.uint64).astype(np.int64)
    nreads = max(offs.size - 1, 0)
    out = np.zeros(nreads, dtype=VOTE_DTYPE)
    out["top_doc"] = NO_DOC
    if nreads == 0:
        return out
    lo, hi = int(offs[0]), int(offs[-1])
    L = np.asarray(lengths)[lo:hi].astype(np.uint64)
    D = np.asarray(docs)[lo:hi].astype(np.uint64)
    counts = np.diff(offs)
    read = np.repeat(np.arange(nreads, dtype=np.uint64), counts)
    vote = L >= np.uint64(min(int(min_length), 2**64 - 1))
    keys, n = np.unique((read[vote] << np.uint64(32)) | D[vote], return_counts=True)
    if keys.size == 0:
        return out
    rd = (keys >> np.uint64(32)).astype(np.int64)
    doc = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    out["voters"] = np.bincount(rd, weights=n, minlength=nreads).astype(np.uint64)
    # per read: most votes first, the smaller id first among equals
    order = np.lexsort((doc, -n, rd))
    rd, doc, n = rd[order], doc[order], n[order]
    first = np.flatnonzero(np.r_[True, rd[1:] != rd[:-1]])
    out["top_doc"][rd[first]] = doc[first]
    out["top_votes"][rd[first]] = n[first]
    nxt = first + 1
    has = (nxt < rd.size) & (rd[np.minimum(nxt, rd.size - 1)] == rd[first])
    out["second_votes"][rd[first[has]]] = n[nxt[has]]
    return out
