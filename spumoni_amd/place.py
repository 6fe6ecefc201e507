"""Where a read sits on the text: its longest match, extended to both sides without gaps.

This module is the definition (include/spumoni_place.h states it in words; the kernels of
spumoni_amd/csrc/spx_place.hip are held to it bit for bit).  For a read with characters R[0..m) as the walk saw them
(digested under -m / -a), MS lengths L[0..m) and pointers P[0..m) as an MS query returns them, optionally document ids
D[0..m), and the text T[0..n_text) of the index:

- the seed is i* = the smallest i with L[i] = max L; the read is unplaced when m == 0 or L[i*] < min_seed (min_seed >= 1).
  The value in front of a read's first position belongs to another read and never counts;
- read position j faces text position P[i*] - i* + j (the diagonal);
- the right extension starts at read position e = i* + L[i*] and text position te = P[i*] + L[i*] (modulo 2^64) and has
  K = min(m - e, n_text - te) steps, 0 where either is not positive.  s_0 = 0, s_k = s_(k-1) + 1 where
  R[e + k - 1] == T[te + k - 1] and s_(k-1) - mismatch_penalty where not; stop is the smallest k >= 1 with
  max_(u <= k) s_u - s_k > x_drop, or K; right is the smallest k in [0, stop] that maximises s_k;
- the left extension is the mirror image: step k compares R[i* - k] with T[P[i*] - k], K = min(i*, P[i*]) -- and 0 for a
  pointer behind the text (P[i*] > n_text), which has nothing in front of it that could be compared;
- the record: ref_start = P[i*] - left, read_start = i* - left, read_end = i* + L[i*] + right, matches = L[i*] + the equal
  characters inside the two extensions (both modulo 2^32: consistent arrays never get there), seed_pos = i*,
  seed_len = L[i*], doc = D[i*] or 0xFFFFFFFF without ids;
- an unplaced read: ref_start = 2^64 - 1, doc = 0xFFFFFFFF, every other field 0.

The rule is this project's, and it is a rule on the arrays and the text: the seed's characters are trusted, an extension
may cross a sequence boundary of the concatenated text, and where the lengths under-report the seed is still exact but
need not be the longest.  All arithmetic is done in 64 bits.
"""
from __future__ import annotations

import numpy as np

PLACEMENT_DTYPE = np.dtype([("ref_start", "<u8"), ("read_start", "<u4"), ("read_end", "<u4"), ("matches", "<u4"),
                            ("seed_pos", "<u4"), ("seed_len", "<u4"), ("doc", "<u4")])
NO_DOC = 0xFFFFFFFF
UNPLACED = 2**64 - 1
M64, M32 = 2**64 - 1, 2**32 - 1


def _extend(eq, penalty, x_drop):
    """(length, equal characters inside) of one x-drop extension over the comparisons eq[0..K), nearest first."""
    if eq.size == 0:
        return 0, 0
    s = np.zeros(eq.size + 1, dtype=np.int64)
    np.cumsum(np.where(eq, 1, -int(penalty)), dtype=np.int64, out=s[1:])
    over = np.flatnonzero(np.maximum.accumulate(s) - s > int(x_drop))
    stop = int(over[0]) if over.size else eq.size
    best = int(np.argmax(s[: stop + 1]))  # (the first of equals)
    return best, int(np.count_nonzero(eq[:best]))


def place_reference(seqs, lengths, pointers, offs, text, min_seed, mismatch_penalty=4, x_drop=16, docs=None):
    """PLACEMENT_DTYPE[nreads] of the reads seqs[offs[q]:offs[q + 1]] (the same slices of lengths, pointers and docs);
    numpy: the argmax vectorised, the extensions read by read.  offs[0] need not be 0."""
    if int(min_seed) < 1:
        raise ValueError("min_seed must be at least 1")
    if not 0 <= int(mismatch_penalty) <= 65535:
        raise ValueError("mismatch_penalty must be 0 .. 65535")
    if not 0 <= int(x_drop) <= 2**31 - 1:
        raise ValueError("x_drop must be 0 .. 2^31 - 1")
    offs = np.asarray(offs, dtype=np.uint64).astype(np.int64)
    nreads = max(offs.size - 1, 0)
    out = np.zeros(nreads, dtype=PLACEMENT_DTYPE)
    out["ref_start"] = UNPLACED
    out["doc"] = NO_DOC
    if nreads == 0:
        return out
    R, T = np.asarray(seqs, dtype=np.uint8), np.asarray(text, dtype=np.uint8)
    n_text = int(T.size)
    lo, hi = int(offs[0]), int(offs[-1])
    L = np.asarray(lengths)[lo:hi].astype(np.uint64)
    counts = np.diff(offs)
    P, D = np.asarray(pointers), None if docs is None else np.asarray(docs)
    full = np.flatnonzero(counts > 0)
    if full.size == 0:
        return out
    # the seed: the largest length, the smallest position among equals = the maximum of length << 32 | ~position
    read_of = np.repeat(np.arange(nreads), counts)
    pos = (np.arange(lo, hi) - offs[read_of]).astype(np.uint64)
    key = (L << np.uint64(32)) | (np.uint64(M32) - pos)
    top = np.maximum.reduceat(key, offs[full] - lo)
    seed_len = (top >> np.uint64(32)).astype(np.int64)
    seed_pos = (np.uint64(M32) - (top & np.uint64(M32))).astype(np.int64)
    long_enough = seed_len >= min(int(min_seed), 2**62)
    for q, sl, i in zip(full[long_enough].tolist(), seed_len[long_enough].tolist(), seed_pos[long_enough].tolist()):
        o, m = int(offs[q]), int(counts[q])
        p = int(P[o + i])
        e, te = i + sl, (p + sl) & M64
        k = max(min(m - e, n_text - te), 0)
        right, eq_r = _extend(R[o + e: o + e + k] == T[te: te + k], mismatch_penalty, x_drop)
        k = min(i, p) if p <= n_text else 0
        left, eq_l = _extend(R[o + i - k: o + i][::-1] == T[p - k: p][::-1], mismatch_penalty, x_drop)
        out[q] = (p - left, i - left, (e + right) & M32, (sl + eq_l + eq_r) & M32, i, sl,
                  NO_DOC if docs is None else int(D[o + i]))
    return out
