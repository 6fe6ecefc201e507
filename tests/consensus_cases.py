"""What tests/test_consensus_cpu.py and tests/test_gpu_consensus.py share: the planted genome -- a reference of two sequences on
two strands, a copy of it with ten substitutions and one deletion, and reads cut from the copy -- with the consensus the
reads must give back, computed from where the reads were cut and not from the rule; and the Python reference chain from the
oracle's matching statistics to the coverage and the pileup.

What was chosen (tests/README_consensus.md): sequences of 1 500 and 1 300 bases; reads of 100 bases every 5 bases of the copy, every
second one from the reverse strand; no reads from [600, 800) of the second sequence's copy; substitutions at least 150 bases
from every end of a covered stretch and 60 from each other; the deletion of 3 bases at the first place behind base 700 of
the first sequence where it cannot shift (t[p - 1] != t[p + 2] and t[p] != t[p + 3]); anchors of at least 12 characters;
min_depth 3."""
import numpy as np

from spumoni_amd.call import pileup_reference
from spumoni_amd.chain import chain_reference
from spumoni_amd.cover import cover_reference
from spumoni_amd.extend import extend_reference
from spumoni_amd.map import map_reference, piece_starts
from spumoni_amd.mems import mems_reference

LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
LENGTHS = [1500, 1300]
STRANDS = 2
NAMES = [b"first", b"second"]
READ, STEP, MIN_LENGTH, MIN_DEPTH = 100, 5, 12, 3
SUBS = [(0, 200), (0, 330), (0, 455), (0, 580), (0, 900), (0, 1100), (0, 1290), (1, 170), (1, 400), (1, 1050)]
BARE = (1, 600, 800)  # no read is cut from this stretch of the second sequence's copy
DELETED = 3


def revcomp(s):
    return bytes(s).translate(COMP)[::-1]


def planted():
    """A dict: "seqs" (the reference's sequences, bytes), "text" (uint8: every sequence's forward piece and its reverse
    complement behind it), "copies" (the sample's sequences), "deletion" (sequence, position), "reads" ([bytes]),
    "seqs_offs" (the reads as one array and their offsets) and "expected" (per sequence the consensus letters the reads
    imply at min_depth 3: the copy's letter where at least three reads were cut over it, N elsewhere)."""
    rng = np.random.default_rng(4190)
    seqs = [LETTERS[rng.integers(0, 4, n)].tobytes() for n in LENGTHS]
    copies = [bytearray(s) for s in seqs]
    for s, at in SUBS:
        copies[s][at] = b"ACGT"[(b"ACGT".index(seqs[s][at]) + 1 + (at % 3)) % 4]
    t = seqs[0]
    p = next(p for p in range(700, 800) if t[p - 1] != t[p + DELETED - 1] and t[p] != t[p + DELETED])
    assert all(abs(at - p) > 60 for s, at in SUBS if s == 0)
    del copies[0][p:p + DELETED]
    copies = [bytes(c) for c in copies]
    reads, expected = [], []
    for s, c in enumerate(copies):
        depth = np.zeros(len(c), dtype=np.int64)
        for q, at in enumerate(range(0, len(c) - READ + 1, STEP)):
            if s == BARE[0] and at < BARE[2] and at + READ > BARE[1]:
                continue
            depth[at:at + READ] += 1
            reads.append(revcomp(c[at:at + READ]) if q % 2 else c[at:at + READ])
        expected.append(bytes(np.where(depth >= MIN_DEPTH, np.frombuffer(c, dtype=np.uint8), ord("N")).astype(np.uint8)))
        assert (depth >= MIN_DEPTH).sum() > len(c) // 2 and (depth < MIN_DEPTH).any()
    text = np.frombuffer(b"".join(s + revcomp(s) for s in seqs), dtype=np.uint8).copy()
    offs = np.r_[0, np.cumsum([len(r) for r in reads])].astype(np.uint64)
    return dict(seqs=seqs, text=text, copies=copies, deletion=(0, p), reads=reads,
                seqs_offs=(np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), offs), expected=expected)


def wrap(s, width):
    return b"".join(s[i:i + width] + b"\n" for i in range(0, len(s), width)) if width else (s + b"\n" if s else b"")


def expected_body(plant, line_width=60, mask=b"N"):
    return b"".join(wrap(e.replace(b"N", mask), line_width) for e in plant["expected"])


def reference_arrays(oracle_mod, raw, text, seqs, offs, lengths=LENGTHS, strands=STRANDS, into=(None, None), min_length=MIN_LENGTH):
    """(cover_reference's triple, pileup_reference's quadruple) of the reads: the oracle's matching statistics -> mems ->
    chain -> extend -> map -> cover + pileup, added to `into`."""
    ms = oracle_mod.OracleIndex.from_raw(raw).ms(seqs, offs, text=text)
    mo, rec = mems_reference(ms["lengths"], ms["pointers"], offs, min_length)
    chains, _, pred = chain_reference(mo, rec)
    ext = extend_reference(seqs, offs, text, mo, rec, chains, pred)
    maps, m_offs, m_ents = map_reference(ext[0], ext[1], ext[2], offs, piece_starts(lengths, strands), strands)
    return (cover_reference(maps, m_offs, m_ents, lengths, into=into[0]),
            pileup_reference(maps, m_offs, m_ents, seqs, offs, lengths, into=into[1]))
