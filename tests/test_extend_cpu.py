"""The rule of the extended CIGARs (spumoni_amd/extend.py: end_path, extend_reference) against an enumeration of every
in-band path, hand-computed cases and its own invariants; the header as C99; the command's usage and refusals.  No GPU."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from spumoni_amd import capi
from spumoni_amd.align import ALIGN_DTYPE, UNALIGNED, AlignParams, align_reference
from spumoni_amd.chain import CHAIN_DTYPE, NO_DOC, chain_reference
from spumoni_amd.cigar import MAX_LENGTH, OP_D, OP_EQ, OP_I, OP_N, OP_X, cigar_reference, pack_runs
from spumoni_amd.extend import (END_DTYPE, OP_S, ExtendParams, band_cells, check_params, cigar_text, end_path, extend_reference)
from tests.test_align_cpu import _index, _planted, _recs
from tests.test_chain_cpu import planted_reads
from tests.test_cigar_cpu import crafted, two_letter_reads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
HEADER = os.path.join(ROOT, "include", "spumoni_extend.h")
RANK = {OP_EQ: 0, OP_X: 0, OP_I: 1, OP_D: 2}  # the rule's order: diagonal, up, left


@pytest.fixture(scope="module")
def built(built_all):
    return capi.lib()


# ---- end_path against every in-band path --------------------------------------------------------------------------------
def _enumerate(A, B, band, mismatch, indel):
    """{(i, j): (best score, the steps the walk back picks)} over every monotone path from (0, 0) that stays in the band: the
    score of a cell is the largest over its paths; among the best paths into a cell the walk back prefers, from the END
    backwards, diagonal over up over left."""
    a, b = len(A), len(B)
    best = {}

    def go(i, j, score, steps):
        key = tuple(RANK[s] for s in reversed(steps))
        if (i, j) not in best or (-score, key) < best[i, j][0]:
            best[i, j] = ((-score, key), list(steps))
        if i < a and j < b:
            same = A[i] == B[j]
            go(i + 1, j + 1, score + 1 if same else score - mismatch, steps + [OP_EQ if same else OP_X])
        if i < a and abs(j - (i + 1)) <= band:
            go(i + 1, j, score - indel, steps + [OP_I])
        if j < b and abs(j + 1 - i) <= band:
            go(i, j + 1, score - indel, steps + [OP_D])

    go(0, 0, 0, [])
    return {cell: (-v[0][0], v[1]) for cell, v in best.items()}


def replay_end(A, B, steps, band, mismatch, indel):
    """The score of a path of one end, walked from (0, 0) inside the band."""
    i = j = score = 0
    for s in steps:
        if s in (OP_EQ, OP_X):
            assert (A[i] == B[j]) == (s == OP_EQ)
            score += 1 if s == OP_EQ else -mismatch
            i, j = i + 1, j + 1
        else:
            score -= indel
            i, j = i + (s == OP_I), j + (s == OP_D)
        assert abs(j - i) <= band and i <= len(A) and j <= len(B)
    return i, j, score


@pytest.mark.parametrize("band,costs", [(0, (4, 6)), (1, (1, 1)), (2, (0, 0)), (5, (4, 6)), (1, (2, 1)), (0, (0, 0)), (2, (4, 6))])
def test_end_path_against_every_in_band_path_up_to_5_by_5(band, costs):
    mismatch, indel = costs
    cases = 0
    for a, b in itertools.product(range(0, 6), range(0, 6)):
        pairs = list(itertools.product(itertools.product(b"AC", repeat=a), itertools.product(b"AC", repeat=b)))
        # every pair of strings up to 128 pairs a shape (a + b <= 7); of the larger shapes a spread, the first and the last among them
        for A, B in pairs if len(pairs) <= 128 else pairs[::len(pairs) // 24] + pairs[-1:]:
            A, B = bytes(A), bytes(B)
            cells = _enumerate(A, B, band, mismatch, indel)
            assert len(cells) == band_cells(a, b, band) + 1
            top = max(v[0] for v in cells.values())
            end = min((i + j, i) for (i, j), v in cells.items() if v[0] == top)
            i, j, score, steps = end_path(A, B, band, mismatch, indel)
            assert (i + j, i) == end and score == top, (A, B, band, costs)
            assert steps == cells[i, j][1], (A, B, band, costs, steps, cells[i, j][1])
            assert replay_end(A, B, steps, band, mismatch, indel) == (i, j, score)
            cases += 1
    assert cases > 1300


def test_both_tie_rules_by_hand():
    # free edits: every cell scores what its best diagonal run gives; the shortest best one, then the smallest i
    assert end_path(b"AAAA", b"AA", 5, 0, 0) == (2, 2, 2, [OP_EQ, OP_EQ])
    assert end_path(b"AA", b"AAAA", 5, 0, 0) == (2, 2, 2, [OP_EQ, OP_EQ])
    # (1, 2) and (2, 1) score alike with free indels (A matched once): i + j ties, the smaller i wins -- but (1, 1) is shorter
    assert end_path(b"AC", b"AG", 5, 0, 0)[:3] == (1, 1, 1)
    # nothing gains: (0, 0) is a cell
    assert end_path(b"CCCC", b"AAAA", 16, 4, 6) == (0, 0, 0, [])
    assert end_path(b"", b"AAAA", 16, 4, 6) == (0, 0, 0, []) and end_path(b"AAAA", b"", 16, 0, 0) == (0, 0, 0, [])
    # a mismatch is crossed when what follows pays for it, and not when it only breaks even (the shorter end wins the tie)
    assert end_path(b"AACAAAAA", b"AAGAAAAA", 3, 4, 6) == (8, 8, 3, [OP_EQ, OP_EQ, OP_X] + [OP_EQ] * 5)
    assert end_path(b"AACAAAA", b"AAGAAAA", 3, 4, 6)[:3] == (2, 2, 2)
    # the walk back prefers the diagonal: with free edits X X reaches (2, 2) as I D would
    i, j, score, steps = end_path(b"CCA", b"GGA", 2, 0, 0)
    assert (i, j, score, steps) == (3, 3, 1, [OP_X, OP_X, OP_EQ])
    # up before left: A against nothing-in-common-but-later; score 1 at (2, 2) by I then D?  no -- (1, 2) by D then '=' is shorter
    assert end_path(b"A", b"CA", 1, 5, 0) == (1, 2, 1, [OP_D, OP_EQ])
    assert end_path(b"CA", b"A", 1, 5, 0) == (2, 1, 1, [OP_I, OP_EQ])
    # band 0 is the diagonal alone
    assert end_path(b"ACGT", b"AGGT", 0, 1, 0) == (4, 4, 2, [OP_EQ, OP_X, OP_EQ, OP_EQ])
    with pytest.raises(ValueError, match="max_extend must be 1 .. 4096"):
        check_params((0, 16, 4, 6))
    with pytest.raises(ValueError, match="max_extend must be 1 .. 4096"):
        check_params((4097, 16, 4, 6))
    with pytest.raises(ValueError, match="band must be 0 .. 63"):
        check_params((512, 64, 4, 6))
    with pytest.raises(ValueError, match="mismatch must be 0 .. 65535"):
        check_params((512, 16, 65536, 6))
    with pytest.raises(ValueError, match="indel must be 0 .. 65535"):
        check_params((512, 16, 4, -1))
    assert check_params(None) == ExtendParams(512, 16, 4, 6)


# ---- extend_reference ----------------------------------------------------------------------------------------------------
def _one(R, T, anchors, ep=None, max_fill=512, front=0):
    """One read chained over all of `anchors`, with `front` characters and records of another in front of it."""
    args = crafted([np.frombuffer(b"N" * front, dtype=np.uint8), np.frombuffer(R, dtype=np.uint8)], list(anchors), [0, len(anchors)], front=front)
    out, op_offsets, entries, ends = extend_reference(args[0], args[1], np.frombuffer(T, dtype=np.uint8), args[3], args[2], args[4], args[5],
                                                      AlignParams(max_fill), ep)
    assert int(op_offsets[1]) == 0 and ends[:2].tolist() == [(0, 0, 0, 0)] * 2  # (the read in front has no chain)
    return cigar_text(entries[int(op_offsets[1]):]), out[1].tolist(), ends[2:].tolist()


def test_the_left_end_is_the_mirror_of_the_right_end():
    rng = np.random.default_rng(1)
    L = np.frombuffer(b"AC", dtype=np.uint8)
    for _ in range(40):
        T = L[rng.integers(0, 2, 90)].tobytes()
        core = T[40:50]
        flank = L[rng.integers(0, 2, int(rng.integers(0, 25)))].tobytes()
        ep = ExtendParams(int(rng.integers(1, 30)), int(rng.integers(0, 6)), int(rng.integers(0, 3)), int(rng.integers(0, 3)))
        right = _one(core + flank, T, [(0, 40, 10)], ep)
        left = _one(flank[::-1] + core[::-1], T[::-1], [(len(flank), 40, 10)], ep)
        assert left[2][0] == right[2][1]  # the same end point, score and edits
        assert left[2][1] == right[2][0] == (0, 0, 0, 0)  # (the other side of either read has a = 0)
        # the same operations in the opposite order; S, '=' ... are their own mirror images
        ops = re.findall(r"(\d+)(.)", right[0])
        assert left[0] == "".join(n + c for n, c in reversed(ops)), (T, flank, ep)
        assert left[1][4:6] == right[1][4:6]


def test_text_edges():
    T = b"ACGTTGCAACGTAGGCTTAC"
    # ref_start = 0: nothing of the text is left, the read's head is clipped
    text, rec, ends = _one(b"GGG" + T[0:8] + b"TT", T, [(3, 0, 8)], ExtendParams(512, 4, 1, 1))
    assert text == "3S8=2S" and rec[:4] == (0, 8, 3, 11) and ends == [(0, 0, 0, 0), (0, 0, 0, 0)]
    # ref_start < a + band: b is what the text has (2 characters); the third read character would need a third
    text, rec, ends = _one(b"TAC" + T[2:10], T, [(3, 2, 8)], ExtendParams(512, 4, 1, 1))
    assert text == "1S10=" and rec[:4] == (0, 10, 1, 11) and ends[0] == (2, 2, 2, 0)
    # ref_end = n_text: clipped, whatever the read goes on with; one character before the end: that one character
    assert _one(T[10:20] + b"AC", T, [(0, 10, 10)])[0] == "10=2S"
    text, rec, ends = _one(T[9:19] + b"CC", T, [(0, 9, 10)])
    assert text == "11=1S" and rec[1] == 20 and ends[1] == (1, 1, 1, 0)
    # the text's first and last character in one read
    text, rec, ends = _one(T, T, [(5, 5, 10)])
    assert text == "20=" and rec[:6] == (0, 20, 0, 20, 20, 0) and ends == [(5, 5, 5, 0), (5, 5, 5, 0)]
    # max_extend cuts the end: only 3 characters are looked at
    assert _one(T, T, [(5, 5, 10)], ExtendParams(3, 16, 4, 6))[0] == "2S16=2S"


def test_hand_computed_cigars():
    T = b"." * 100 + b"ACGTACGTAC" + b"GG" + b"TTTTTTTTTT" + b"ACT" + b"CCCCCCCCCC" + b"." * 20
    #                   100            110     112             122      125
    # an extension that merges with the first anchor, and one that merges with the last
    assert _one(b"GTAC" + b"GG" + b"TTTTTTTTTT", T, [(6, 112, 10)]) == ("16=", (106, 122, 0, 16, 16, 0, 1, 0, 0, 1), [(6, 6, 6, 0), (0, 0, 0, 0)])
    assert _one(b"TTTTTTTTTT" + b"ACTCC", T, [(0, 112, 10)])[0] == "15="
    # a fully clipped end on either side: the read's characters are none of the text's
    text, rec, ends = _one(b"xxxx" + b"TTTTTTTTTT" + b"yyy", T, [(4, 112, 10)], front=3)
    assert text == "4S10=3S" and rec[:6] == (112, 122, 4, 14, 10, 0) and ends == [(0, 0, 0, 0)] * 2
    # a substitution five characters in is crossed (4 + 1 - 4 + 5 > 4 ... the run behind it pays), an indel likewise
    text, rec, ends = _one(b"TTTTTTTTTT" + b"ACTCGCCCCCCC", T, [(0, 112, 10)])
    assert text == "14=1X7=" and rec[4:6] == (21, 1) and ends[1] == (12, 12, 7, 1)
    # T of ACT is missing from the read: with the defaults a substitution and nine matches (2 - 4 + 9) beat the deletion and
    # ten (2 - 6 + 10); with a mismatch of 8 the deletion wins
    assert _one(b"TTTTTTTTTT" + b"ACCCCCCCCCCC", T, [(0, 112, 10)])[0] == "12=1X9="
    text, rec, ends = _one(b"TTTTTTTTTT" + b"ACCCCCCCCCCC", T, [(0, 112, 10)], ExtendParams(512, 16, 8, 6))
    assert text == "12=1D10=" and rec[:6] == (112, 135, 0, 22, 22, 1) and ends[1] == (12, 13, 6, 1)
    # between the anchors nothing changes: cigar's operations with the ends around them
    text, rec, _ = _one(b"GG" + b"TTTTTTTTTTACGCCCCCCCCCC" + b"y", T, [(2, 112, 10), (15, 125, 10)])
    assert text == "14=1X10=1S" and rec[:6] == (110, 135, 0, 25, 24, 1)
    # a clip beyond 2^28 - 1 is split like every run (pack_runs: the rule of the entries is cigar's)
    assert pack_runs([(OP_S, MAX_LENGTH + 6), (OP_EQ, 10), (OP_S, 0)]) == [MAX_LENGTH << 4 | OP_S, 6 << 4 | OP_S, 10 << 4 | OP_EQ]
    assert cigar_text([MAX_LENGTH << 4 | OP_S, 6 << 4 | OP_S, 10 << 4 | OP_EQ]) == f"{MAX_LENGTH}S6S10="
    # no reads; a read without a chain
    none = extend_reference(np.zeros(0, dtype=np.uint8), [0], np.zeros(0, dtype=np.uint8), [0], _recs([]), np.zeros(0, dtype=CHAIN_DTYPE), [])
    assert none[0].size == 0 and none[1].tolist() == [0] and none[2].size == 0 and none[3].size == 0 and none[3].dtype == END_DTYPE
    chains, _, pred = chain_reference([0, 0], _recs([]))
    out, op_offsets, entries, ends = extend_reference(np.zeros(3, dtype=np.uint8), [0, 3], np.zeros(0, dtype=np.uint8), [0, 0], _recs([]), chains, pred)
    assert out[0].tolist() == (UNALIGNED, 0, 0, 0, 0, 0, 0, 0, 0, NO_DOC) and op_offsets.tolist() == [0, 0] and cigar_text(entries) == "*"


def replay(entries, R, T, rec):
    """Walks a read's entries along the WHOLE read and the text: clips only at the ends, '=' columns equal, 'X' columns
    unequal, and the spans add up.  Returns the sums per operation."""
    entries = [int(e) for e in entries]
    sums = dict.fromkeys((OP_I, OP_D, OP_N, OP_EQ, OP_X, OP_S), 0)
    x, y = 0, int(rec["ref_start"])
    kinds = [e & 15 for e in entries]
    inner = [k for k in kinds if k != OP_S]
    assert kinds == [OP_S] * kinds[:kinds.index(inner[0])].count(OP_S) + inner + [OP_S] * (len(kinds) - kinds.index(inner[0]) - len(inner))
    for t, e in enumerate(entries):
        op, n = e & 15, e >> 4
        assert 1 <= n <= MAX_LENGTH and (t == 0 or kinds[t - 1] != op or entries[t - 1] >> 4 == MAX_LENGTH)
        sums[op] += n
        if op == OP_S:
            assert x in (0, int(rec["read_end"]))
            x += n
            continue
        if x == sums[OP_S]:
            assert x == int(rec["read_start"]) or sums[OP_EQ] + sums[OP_X] + sums[OP_I] + sums[OP_D] + sums[OP_N] > n
        if op in (OP_EQ, OP_X):
            a, b = np.frombuffer(R[x:x + n], dtype=np.uint8), np.frombuffer(T[y:y + n], dtype=np.uint8)
            assert a.size == n and b.size == n and ((a == b) if op == OP_EQ else (a != b)).all(), (op, x, y, n)
            x, y = x + n, y + n
        elif op == OP_I:
            x += n
        else:
            y += n
    assert x == len(R) and y == int(rec["ref_end"])
    return sums


def check_invariants(out, op_offsets, entries, R, roffs, T):
    R, T = bytes(R), bytes(T)
    for q in range(out.size):
        mine = entries[int(op_offsets[q]):int(op_offsets[q + 1])]
        if out[q]["ref_start"] == np.uint64(UNALIGNED):
            assert mine.size == 0
            continue
        read = R[int(roffs[q]):int(roffs[q + 1])]
        s = replay(mine, read, T, out[q])
        assert s[OP_EQ] + s[OP_X] + s[OP_I] + s[OP_S] == len(read), q
        assert s[OP_EQ] + s[OP_X] + s[OP_D] + s[OP_N] == int(out[q]["ref_end"]) - int(out[q]["ref_start"]), q
        assert s[OP_EQ] == int(out[q]["matches"]), q
        assert s[OP_EQ] + s[OP_X] + s[OP_I] == int(out[q]["read_end"]) - int(out[q]["read_start"]), q


def with_flanks(rng, text, reads, anchors, counts, letters, rate=0.08):
    """The reads of two_letter_reads with both ends grown: the text on either side of the chain with a share of its
    characters replaced, dropped or doubled, or (every fourth end) random characters."""
    L = np.frombuffer(letters, dtype=np.uint8)
    out_reads, out_anchors, k = [], [], 0
    for read, h in zip(reads, counts):
        mine = anchors[k:k + h]
        k += h
        if not h:
            out_reads.append(read)
            continue
        sides = []
        for side in (0, 1):
            n = int(rng.integers(0, 40))
            at = mine[0][1] - n if side == 0 else mine[-1][1] + mine[-1][2]
            seg = text[max(at, 0):max(at, 0) + n] if rng.random() < 0.75 else L[rng.integers(0, L.size, n)]
            keep = rng.random(seg.size)
            seg = np.concatenate([np.r_[c, c] if u < rate / 3 else (L[rng.integers(0, L.size, 1)] if u < 2 * rate / 3 else np.array([c], dtype=np.uint8))
                                  for c, u in zip(seg, keep) if u > rate / 4] + [seg[:0]]).astype(np.uint8)
            sides.append(seg)
        out_reads.append(np.r_[sides[0], read, sides[1]])
        out_anchors += [(x + sides[0].size, y, l) for x, y, l in mine]
    return out_reads, out_anchors, counts


@pytest.mark.parametrize("letters", [b"AC", b"ACGT"])
def test_invariants_and_replay_over_planted_reads(letters):
    rng = np.random.default_rng(len(letters))
    text = np.frombuffer(letters, dtype=np.uint8)[rng.integers(0, len(letters), 3000)]
    reads, anchors, counts = two_letter_reads(rng, text, 60, letters)
    bare = crafted(reads, anchors, counts, front=2)
    R, roffs, rec, moffs, chains, pred = crafted(*with_flanks(rng, text, reads, anchors, counts, letters), front=2)
    extended = clipped = 0
    for ep in (None, ExtendParams(512, 3, 1, 1), ExtendParams(8, 0, 0, 0), ExtendParams(1, 63, 65535, 65535)):
        count = {}
        out, op_offsets, entries, ends = extend_reference(R, roffs, text, moffs, rec, chains, pred, None, ep, count=count)
        assert out.dtype == ALIGN_DTYPE and op_offsets.dtype == np.uint64 and entries.dtype == np.uint32 and ends.dtype == END_DTYPE
        assert op_offsets.size == out.size + 1 and int(op_offsets[-1]) == entries.size and ends.size == 2 * out.size
        check_invariants(out, op_offsets, entries, R, roffs, text)
        # with both ends' operations and the clips stripped, the entries are cigar_reference's up to merging
        want, c_offs, c_entries = cigar_reference(R, roffs, text, moffs, rec, chains, pred)
        for q in range(out.size):
            if want[q]["ref_start"] == np.uint64(UNALIGNED):
                assert out[q] == want[q] and ends[2 * q:2 * q + 2].tolist() == [(0, 0, 0, 0)] * 2
                continue
            steps = [e & 15 for e in map(int, entries[int(op_offsets[q]):int(op_offsets[q + 1])]) for _ in range(e >> 4)]
            inner = [s for s in steps if s != OP_S]
            l, r = ends[2 * q], ends[2 * q + 1]

            def nsteps(e):  # the steps of an end's path: i + j less the diagonal ones, which count on both sides
                lo = max(int(e["read_chars"]), int(e["text_chars"]))
                return lo, int(e["read_chars"]) + int(e["text_chars"])

            core = [e & 15 for e in map(int, c_entries[int(c_offs[q]):int(c_offs[q + 1])]) for _ in range(e >> 4)]
            assert any(inner[k:k + len(core)] == core for k in range(nsteps(l)[0], nsteps(l)[1] + 1)), q
            assert int(out[q]["read_start"]) == int(want[q]["read_start"]) - int(l["read_chars"])
            assert int(out[q]["ref_end"]) == int(want[q]["ref_end"]) + int(r["text_chars"])
            assert int(out[q]["edits"]) == int(want[q]["edits"]) + int(l["edits"]) + int(r["edits"])
            assert [out[q][f] for f in ("anchors", "unfilled", "skipped", "doc")] == [want[q][f] for f in ("anchors", "unfilled", "skipped", "doc")]
            assert int(l["score"]) >= 0 and int(r["score"]) >= 0
        assert count["extended"] == int(((ends["read_chars"] > 0) | (ends["text_chars"] > 0)).sum()) and count["ends"] >= count["extended"]
        extended += count["extended"]
        clipped += count["clipped"]
    assert extended > 60 and clipped > 500
    # where both ends have a = 0 the records are align_reference's and the entries cigar_reference's
    out, op_offsets, entries, ends = extend_reference(*bare[:2], text, bare[3], bare[2], bare[4], bare[5])
    want, c_offs, c_entries = cigar_reference(*bare[:2], text, bare[3], bare[2], bare[4], bare[5])
    assert np.array_equal(out, align_reference(*bare[:2], text, bare[3], bare[2], bare[4], bare[5])[0])
    assert np.array_equal(op_offsets, c_offs) and np.array_equal(entries, c_entries) and not ends["read_chars"].any()


def test_planted_reads_are_extended_to_their_ends(oracle_mod):
    """The planted reads of the chain tests (7 edits in 4 places): whatever the first and the last anchor left out is
    taken in, the whole read is aligned, and the middle stays cigar's."""
    text, seqs, offs, cuts = planted_reads()
    mo, rec, chains, _ = _planted(oracle_mod, text, seqs, offs)
    _, _, pred = chain_reference(mo, rec)
    out, op_offsets, entries, ends = extend_reference(seqs, offs, text, mo, rec, chains, pred)
    check_invariants(out, op_offsets, entries, seqs, offs, text)
    lens = np.diff(np.asarray(offs).astype(np.int64))
    assert (out["read_start"] == 0).all() and (out["read_end"] == lens).all() and OP_S not in {int(e) & 15 for e in entries}


# ---- header and command ------------------------------------------------------------------------------------------------
def _declared():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return code, sorted(set(re.findall(r"\b(spe_[a-z_0-9]+)\s*\(", code)))


def test_extend_header_is_plain_c(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include "spumoni_extend.h"\nint main(void) { spe_params p; spe_end e; spe_extend_stats s; (void)p; (void)e; (void)s; '
                   'return sizeof(spa_alignment) == 48 && sizeof(spe_params) == 16 && sizeof(spe_end) == 16 && '
                   'sizeof(spe_extend_stats) == 128 && SPE_OP_S == 4 && SPG_OP_EQ == 7 ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "c"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "c")]).returncode == 0
    code, _ = _declared()
    assert "hipStream_t" not in code and "std::" not in code and "#include <hip" not in code
    assert re.findall(r'#include\s+[<"]([^>"]+)', code) == ["stdint.h", "spumoni_cigar.h"]
    assert "typedef struct spa_alignment" not in code  # (the record is spumoni_align.h's, reused)


def test_extend_header_symbols_exported(built):
    _, names = _declared()
    assert names == sorted(capi.EXTEND_EXPORTS) and len(names) == 4
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(spe_[a-z_0-9]+)\b", out))) == names
    for other in (capi.EXPORTS, capi.DOCVOTE_EXPORTS, capi.MEMS_EXPORTS, capi.PLACE_EXPORTS, capi.CHAIN_EXPORTS, capi.ALIGN_EXPORTS,
                  capi.CIGAR_EXPORTS, capi.REFTEXT_EXPORTS):
        assert not set(capi.EXTEND_EXPORTS) & set(other)
    assert capi.C.sizeof(capi.SpeExtendStats) == 128 and capi.C.sizeof(capi.SpeParams) == 16 and capi.C.sizeof(capi.SpeEnd) == 16
    assert END_DTYPE.itemsize == 16 and [f[0] for f in capi.SpeEnd._fields_] == list(END_DTYPE.names)
    assert [f[0] for f in capi.SpeExtendStats._fields_] == ["reads", "aligned_reads", "gaps", "filled_gaps", "cells", "entries", "path_words",
                                                            "ends", "extended_ends", "band_cells", "clipped", "error", "overflow",
                                                            "kernel_ms", "step_ms", "reserved"]
    for method in ("extend_device", "extend_host", "extend_stats"):
        assert callable(getattr(capi.Index, method))


def test_extend_begin_without_device_fails_loudly(built):
    L = capi._spe()
    seqs, offs = np.frombuffer(b"ACGT", dtype=np.uint8), np.array([0, 4], dtype=np.uint64)
    out = np.zeros(1, dtype=ALIGN_DTYPE)
    n = capi.C.c_uint64(0)
    rc = L.spe_extend_begin(None, 0, 0, 0, seqs.ctypes.data, offs.ctypes.data, 1, 1, 0, capi.SpcParams(64, 5000, 500, 1), capi.SpaParams(512),
                            capi.SpeParams(512, 16, 4, 6), out.ctypes.data, None, None, None, capi.C.byref(n))
    if built.spx_device_count() > 0:  # (with a device the call gets as far as its first argument)
        assert rc == -1 and b"index must be non-null" in L.spx_last_error()
    else:
        assert rc == -3 and b"no CPU fallback" in L.spx_last_error()


def _extend(args, cwd, env=None):
    return subprocess.run([BIN, "extend"] + args, cwd=cwd, capture_output=True, text=True, env=env, timeout=120)


def test_usage_without_arguments(built, tmp_path):
    r = _extend([], str(tmp_path))
    assert r.returncode == 1
    assert "spumoni extend - " in r.stderr
    for opt in ("-h, --help", "-r, --ref", "-p, --pattern", "-n, --no-digest", "-m, --minimizer-alphabet", "-a, --dna-minimizer",
                "-K, --small-window", "-W, --large-window", "-d, --doc-array", "-L, --min-length", "-S, --max-dist", "-G, --max-gap",
                "-B, --gap-penalty", "-H, --lookback", "-F, --max-fill", "-E, --max-extend", "-O, --band", "-N, --mismatch", "-I, --indel"):
        assert opt in r.stderr, opt
    for limits in ("1 or more", "1 .. 2147483647", "0 .. 2147483647", "0 .. 65535", "1 .. 64", "1 .. 4096", "0 .. 63", "268435455"):
        assert limits in r.stderr, limits
    assert "-P, --PML" not in r.stderr and "<pattern>.extended" in r.stderr and "= X I D" in r.stderr
    assert re.search(r"skipped\[, doc\], length and the CIGAR", r.stderr)  # the column order is stated
    top = subprocess.run([BIN], capture_output=True, text=True)
    assert top.returncode == 1
    for cmd in ("extend", "cigar", "align", "chain", "place", "mems", "assign", "run", "build"):
        assert f"\t{cmd}\t" in top.stderr, cmd


@pytest.mark.parametrize("args,message", [
    (["-p", "reads.fa", "-n"], "Both a reference file (-r) and pattern file (-p) must be provided."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-P"], "-P cannot be used with `spumoni extend`"),
    (["-r", "ref", "-p", "reads.fa", "-n", "-M", "-P"], "-P cannot be used with `spumoni extend`"),
    (["-r", "nosuch", "-p", "reads.fa", "-n"], "The following path is not valid: nosuch.fa"),
    (["-r", "ref", "-p", "missing.fa", "-n"], "The following path is not valid: missing.fa"),
    (["-r", "ref", "-p", "reads.txt", "-n"], "The pattern file provided does not appear to be a FASTA"),
    (["-r", "ref", "-p", "reads.fa", "-m", "-a"], "Only one type of minimizer can be specified from either -m or -a."),
    (["-r", "ref", "-p", "reads.fa"], "A minimizer type must be specified using -m or -a."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-L", "0"], "the minimum match length (-L) must be at least 1."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-S", "0"], "the largest distance (-S) must be between 1 and 2147483647."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-G", "2147483648"], "the largest gap (-G) must be between 0 and 2147483647."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-B", "65536"], "the gap penalty (-B) must be between 0 and 65535."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-H", "65"], "the lookback (-H) must be between 1 and 64."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-F", "4097"], "the largest filled gap (-F) must be between 1 and 4096."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-E", "0"], "the largest extended end (-E) must be between 1 and 4096."),
    (["-r", "ref", "-p", "reads.fa", "-n", "--max-extend", "4097"], "the largest extended end (-E) must be between 1 and 4096."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-E", "-1"], "the largest extended end (-E) must be between 1 and 4096."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-O", "64"], "the band (-O) must be between 0 and 63."),
    (["-r", "ref", "-p", "reads.fa", "-n", "--band", "-1"], "the band (-O) must be between 0 and 63."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-N", "65536"], "the mismatch cost (-N) must be between 0 and 65535."),
    (["-r", "ref", "-p", "reads.fa", "-n", "--mismatch", "-2"], "the mismatch cost (-N) must be between 0 and 65535."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-I", "65536"], "the indel cost (-I) must be between 0 and 65535."),
    (["-r", "ref", "-p", "reads.fa", "-n", "--indel", "-1"], "the indel cost (-I) must be between 0 and 65535."),
])
def test_validation_messages(built, tmp_path, args, message):
    _index(tmp_path)
    shutil.copy(tmp_path / "reads.fa", tmp_path / "reads.txt")
    before = sorted(os.listdir(tmp_path))
    r = _extend(args, str(tmp_path))
    assert r.returncode == 1
    assert message in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_doc_ids_without_doc_file_are_refused(built, tmp_path):
    _index(tmp_path, doc=False)
    before = sorted(os.listdir(tmp_path))
    r = _extend(["-r", "ref", "-p", "reads.fa", "-n", "-d"], str(tmp_path))
    assert r.returncode == 1
    assert "document array file (ref.fa.doc) is not present, so it cannot be used." in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_missing_entry_point_on_the_fake_device(built, fake_device, tmp_path):
    _index(tmp_path)
    before = sorted(os.listdir(tmp_path))
    env = dict(os.environ, LD_LIBRARY_PATH=fake_device + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = _extend(["-r", "ref", "-p", "reads.fa", "-n", "-L", "4"], str(tmp_path), env=env)
    assert r.returncode == 1
    assert "has no spe_extend_begin" in r.stderr and "`spumoni extend`" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_a_failing_run_writes_nothing(built, tmp_path):
    """Without a device the command stops at its entry points; with one, at a read that is empty: either way no file."""
    _index(tmp_path)
    if built.spx_device_count() > 0:
        with open(tmp_path / "reads.fa", "ab") as f:
            f.write(b">bad_one\n>after\nACGT\n")
    before = sorted(os.listdir(tmp_path))
    r = _extend(["-r", "ref", "-p", "reads.fa", "-n", "-d"], str(tmp_path))
    assert r.returncode == 1
    if built.spx_device_count() > 0:
        assert "bad_one was empty" in r.stderr, r.stderr
    else:
        assert "no usable gfx950 device" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before
