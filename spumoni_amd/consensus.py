"""The consensus: per base of every sequence's forward strand the byte that the coverage's depth and the pileup's counts
imply, and the sequences they spell as FASTA body text.

This module is the definition (include/spumoni_consensus.h states it in words; the kernels of
spumoni_amd/csrc/spx_consensus.hip are held to it byte for byte).  The input is the sequence table's lengths -- F[s] is the
sum of the lengths before sequence s, G = F[n_seqs] --, the text, whose forward piece of sequence s starts at
P[s * strands] = F[s] * strands, depth[G] of cover.py and alt[4 * G], ins[G] and del[G] of call.py; other and mism do not
enter.  The parameters are the calls' min_depth >= 1, min_alt >= 1 and min_permille in 0 .. 1000, a mask byte (0: "write
the reference's byte") and line_width in 0 .. 2^31 - 1 (0: one line per sequence).  Integers only.

At position i of sequence s: g = F[s] + i, ref = text[P[s * strands] + i], d = depth[g], dl = del[g], span = d + dl.  The
first rule that holds decides:

    1  span < min_depth                                        masked: emits mask, or ref when mask is 0
    2  dl >= min_alt and dl * 1000 >= min_permille * span      deleted: emits nothing
    3  d < min_depth                                           masked, as in rule 1
    4  the calls' best candidate (the codes other than ref's own, the largest alt count, the lowest code among equals)
       has count >= min_alt and count * 1000 >= min_permille * d
                                                               substituted: emits "ACGT"[allele]
    5  otherwise                                               kept: emits ref as it is, case included

Among the positions rules 1 - 3 leave, a position is substituted exactly where call.calls_reference with the same three
thresholds calls it.  A position that rule 1 does not mask is an insertion site when ins[g] >= min_alt and
ins[g] * 1000 >= min_permille * span; sites are counted, not applied (the pileup keeps how many insertions start at a base,
not their letters).

The body is one byte buffer for all sequences in table order: sequence s contributes its emitted bytes in position order, a
newline behind every line_width-th letter and a newline behind the last letter unless one was just written (line_width 0:
only that last one); a sequence without a letter contributes nothing.  So body_bytes(s) = letters +
(ceil(letters / line_width) if line_width else (letters > 0)) and body_start is the running sum of body_bytes.
"""
from __future__ import annotations

import numpy as np

from .call import LETTERS, code_of
from .cover import seq_starts

SEQ_DTYPE = np.dtype([("body_start", "<u8"), ("letters", "<u8"), ("substituted", "<u8"), ("deleted", "<u8"), ("masked", "<u8"),
                      ("ins_sites", "<u8")])
assert SEQ_DTYPE.itemsize == 48
MAX_LINE_WIDTH = 2**31 - 1


def body_bytes(letters: int, line_width: int) -> int:
    """The bytes a sequence of `letters` emitted letters takes in the body."""
    return letters + (-(-letters // line_width) if line_width else int(letters > 0))


def consensus_reference(depth, alt, ins, dele, text, seq_lengths, strands, min_depth=2, min_alt=2, min_permille=500, mask=ord("N"),
                        line_width=60):
    """(records SEQ_DTYPE[n_seqs], body uint8[]) of the arrays.  mask: a byte as an int, or bytes of length 1."""
    if isinstance(mask, (bytes, bytearray)):
        if len(mask) != 1:
            raise ValueError("mask must be one byte")
        mask = mask[0]
    if not (min_depth >= 1 and min_alt >= 1 and 0 <= min_permille <= 1000):
        raise ValueError("min_depth and min_alt must be at least 1, min_permille between 0 and 1000")
    if not (0 <= line_width <= MAX_LINE_WIDTH and 0 <= mask <= 255):
        raise ValueError("line_width must be between 0 and 2^31 - 1, mask one byte")
    F = seq_starts(seq_lengths)
    G = F[-1]
    depth, ins, dele = (np.asarray(a, dtype=np.uint32) for a in (depth, ins, dele))
    alt = np.asarray(alt, dtype=np.uint32).reshape(G, 4)
    text = np.asarray(text, dtype=np.uint8)
    assert depth.shape == ins.shape == dele.shape == (G,)
    depth, ins, dele, alt = depth.tolist(), ins.tolist(), dele.tolist(), alt.tolist()  # (Python integers: no overflow anywhere)
    records = np.zeros(len(F) - 1, dtype=SEQ_DTYPE)
    body = bytearray()
    for s in range(len(F) - 1):
        p0 = F[s] * strands
        refs = text[p0:p0 + F[s + 1] - F[s]].tolist()
        out = bytearray()
        substituted = deleted = masked = sites = 0
        for i, ref in enumerate(refs):
            g = F[s] + i
            d, dl = depth[g], dele[g]
            span = d + dl
            low = mask if mask else ref
            if span < min_depth:  # rule 1
                masked += 1
                out.append(low)
                continue
            sites += ins[g] >= min_alt and ins[g] * 1000 >= min_permille * span
            if dl >= min_alt and dl * 1000 >= min_permille * span:  # rule 2
                deleted += 1
                continue
            if d < min_depth:  # rule 3
                masked += 1
                out.append(low)
                continue
            rc = code_of(ref)
            best, cnt = -1, -1
            for c in range(4):
                if c != rc and alt[g][c] > cnt:
                    best, cnt = c, alt[g][c]
            if cnt >= min_alt and cnt * 1000 >= min_permille * d:  # rule 4
                substituted += 1
                out.append(ord(LETTERS[best]))
            else:  # rule 5
                out.append(ref)
        records[s] = (len(body), len(out), substituted, deleted, masked, sites)
        if line_width:
            for k in range(0, len(out), line_width):
                body += out[k:k + line_width] + b"\n"
        elif out:
            body += out + b"\n"
        assert len(body) - int(records[s]["body_start"]) == body_bytes(len(out), line_width)
    return records, np.frombuffer(bytes(body), dtype=np.uint8).copy()


def fasta_of(names, records, body) -> bytes:
    """The FASTA file of (records, body): per sequence `>name` and its slice of the body; a sequence without letters gets
    its header only.  names: bytes or str, one per record."""
    body = np.asarray(body, dtype=np.uint8).tobytes()
    assert len(names) == len(records)
    out = []
    for s, (name, rec) in enumerate(zip(names, records)):
        start, letters = int(rec["body_start"]), int(rec["letters"])
        end = int(records[s + 1]["body_start"]) if s + 1 < len(records) else len(body)
        assert start <= end <= len(body) and (end - start > letters if letters else end == start)
        out.append(b">" + (name.encode() if isinstance(name, str) else bytes(name)) + b"\n" + body[start:end])
    return b"".join(out)


def tsv_of(names, seq_lengths, records) -> bytes:
    """`spumoni consensus`'s table: name, length, letters, substituted, deleted, masked, insertion sites per sequence."""
    return b"".join(b"%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (name.encode() if isinstance(name, str) else bytes(name), int(n), int(r["letters"]),
                                                        int(r["substituted"]), int(r["deleted"]), int(r["masked"]), int(r["ins_sites"]))
                    for name, n, r in zip(names, seq_lengths, records))
