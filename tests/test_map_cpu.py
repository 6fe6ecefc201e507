"""The rule of the mappings (spumoni_amd/map.py: map_reference) against a restatement by per-column arrays, hand-computed
cases and its own invariants; the sequence table's reader, writer and name rule; the header as C99 and the exports; the
command's usage and refusals.  No GPU."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from spumoni_amd import capi
from spumoni_amd.align import ALIGN_DTYPE, UNALIGNED
from spumoni_amd.cigar import MAX_LENGTH, OP_D, OP_EQ, OP_I, OP_N, OP_X
from spumoni_amd.extend import OP_S, cigar_text
from spumoni_amd.map import (CUT_LEFT, CUT_RIGHT, MAPPING_DTYPE, UNMAPPED, map_reference, piece_starts, read_seq_table,
                             seq_table_bytes, sequence_name, write_seq_table)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
HEADER = os.path.join(ROOT, "include", "spumoni_map.h")
CODE = {"=": OP_EQ, "X": OP_X, "I": OP_I, "D": OP_D, "N": OP_N, "S": OP_S}
READ_OPS, TEXT_OPS = (OP_EQ, OP_X, OP_I), (OP_EQ, OP_X, OP_D, OP_N)


@pytest.fixture(scope="module")
def built(built_all):
    return capi.lib()


def entries_of(text):
    """'3S4=1X' as entries, each as written."""
    return [int(n) << 4 | CODE[c] for n, c in re.findall(r"(\d+)(.)", text)]


def alignment(cigar, ref_start):
    """(ALIGN_DTYPE record, entries, len) of a CIGAR given as text or as entries, standing at ref_start: what extend would
    report for it (matches and edits as extend counts them)."""
    entries = entries_of(cigar) if isinstance(cigar, str) else list(cigar)
    kinds = [e & 15 for e in entries]
    inner = [k for k, op in enumerate(kinds) if op != OP_S]
    lead = sum(e >> 4 for e in entries[:inner[0]]) if inner else 0
    reads = sum(e >> 4 for e in entries if e & 15 in READ_OPS)
    texts = sum(e >> 4 for e in entries if e & 15 in TEXT_OPS)
    total = reads + sum(e >> 4 for e in entries if e & 15 == OP_S)
    rec = np.zeros(1, dtype=ALIGN_DTYPE)[0]
    rec["ref_start"], rec["ref_end"], rec["read_start"], rec["read_end"] = ref_start, ref_start + texts, lead, lead + reads
    rec["matches"] = sum(e >> 4 for e in entries if e & 15 == OP_EQ)
    rec["edits"] = sum(e >> 4 for e in entries if e & 15 in (OP_X, OP_I, OP_D))
    rec["anchors"] = 1
    return rec, entries, total


def batch(alignments):
    """(records, op_offsets, entries, read_offsets) of [(rec, entries, len) or None for a read extend left unaligned]."""
    recs = np.zeros(len(alignments), dtype=ALIGN_DTYPE)
    ooffs, roffs, ents = [0], [0], []
    for q, a in enumerate(alignments):
        if a is None:
            recs[q]["ref_start"] = UNALIGNED
            roffs.append(roffs[-1] + 5)
        else:
            recs[q] = a[0]
            ents += a[1]
            roffs.append(roffs[-1] + a[2])
        ooffs.append(len(ents))
    return recs, np.array(ooffs, dtype=np.uint64), np.array(ents, dtype=np.uint32), np.array(roffs, dtype=np.uint64)


def map_one(cigar, ref_start, lengths, strands, count=None):
    """(record as a tuple, CIGAR text) of one alignment against a table."""
    out, offs, ents = map_reference(*batch([alignment(cigar, ref_start)]), piece_starts(lengths, strands), strands, count=count)
    assert offs.tolist() == [0, ents.size]
    return out[0].tolist(), cigar_text(ents)


# ---- the rule against a restatement by per-column arrays ---------------------------------------------------------------
def restated(ops, ref_start, lead, tail, P, strands):
    """The rule once more, on lists with one element per column: expand, label every column with its piece, take the
    argmax of the '=' counts, slice, reverse, re-pack.  None without an '='."""
    ops = list(ops)
    consumes_text = [op in TEXT_OPS for op in ops]
    consumes_read = [op in READ_OPS for op in ops]
    t = [ref_start + sum(consumes_text[:k]) for k in range(len(ops))]
    piece = [max(p for p in range(len(P) - 1) if P[p] <= tk) for tk in t]
    votes = [sum(1 for k, op in enumerate(ops) if op == OP_EQ and piece[k] == p) for p in range(len(P) - 1)]
    if sum(votes) == 0:
        return None
    home = votes.index(max(votes))  # (the first of the largest)
    mine = [k for k, op in enumerate(ops) if op == OP_EQ and piece[k] == home]
    k0, k1 = mine[0], mine[-1] + 1
    assert all(piece[k] == home for k in range(k0, k1) if consumes_text[k])
    left, right = lead + sum(consumes_read[:k0]), tail + sum(consumes_read[k1:])
    start, end = t[k0] - P[home], t[k1 - 1] + 1 - P[home]
    Lp = P[home + 1] - P[home]
    strand = home % strands
    if strand:
        start, end = Lp - end, Lp - start
    kept = ops[k0:k1]
    line = [OP_S] * left + kept + [OP_S] * right
    if strand:
        line = line[::-1]
    ents = [len(list(g)) << 4 | op for op, g in itertools.groupby(line)]
    rec = (start, end, home // strands, strand, left, lead + sum(consumes_read) + tail - right, kept.count(OP_EQ),
           sum(op in (OP_X, OP_I, OP_D) for op in kept), sum(op != OP_N for op in kept), (k0 > 0) * CUT_LEFT | (k1 < len(ops)) * CUT_RIGHT)
    return rec, ents


def _tables():
    return [(lens, strands) for n in (1, 2, 3) for lens in itertools.product(range(1, 5), repeat=n) for strands in (1, 2)]


def test_rule_against_the_restatement_over_every_cigar_up_to_6_columns():
    """Every CIGAR of up to 3 columns against every table and every place it fits; every CIGAR of 4 to 6 columns against four
    tables each, dealt round robin so that every table meets thousands of them, at two places."""
    tables = _tables()
    assert len(tables) == 2 * (4 + 16 + 64)
    cases = mapped = errors = 0
    cigars = [c for n in range(1, 7) for c in itertools.product((OP_EQ, OP_X, OP_I, OP_D, OP_N), repeat=n)]
    assert len(cigars) == sum(5 ** n for n in range(1, 7))
    alignments, want = [], []

    def flush(P, strands):
        nonlocal mapped, errors
        count = {}
        out, offs, ents = map_reference(*batch(alignments), P, strands, count=count)
        for q, w in enumerate(want):
            got = ents[int(offs[q]):int(offs[q + 1])].tolist()
            if w is None:
                assert out[q]["seq"] == UNMAPPED and not got and out[q].tolist()[:2] == (0, 0)
                errors += 1
            else:
                assert out[q].tolist() == w[0] and got == w[1], (alignments[q], P, strands, w)
                mapped += 1
        assert count["error"] == (None in want) and count["mapped"] == sum(w is not None for w in want)
        alignments.clear()
        want.clear()

    for c, ops in enumerate(cigars):
        text_cols = sum(op in TEXT_OPS for op in ops)
        mine = tables if len(ops) <= 3 else [tables[(c * 5 + j * 43) % len(tables)] for j in range(4)]
        for lens, strands in mine:
            P = piece_starts(lens, strands)
            if text_cols > P[-1]:
                continue
            starts = range(P[-1] - text_cols + 1)
            if len(ops) > 3:
                starts = sorted({starts[c % len(starts)], starts[(c // 7) % len(starts)]})
            for s in starts:
                lead, tail = c % 3, (c // 3) % 2
                ents = [lead << 4 | OP_S] * (lead > 0) + [1 << 4 | op for op in ops] + [tail << 4 | OP_S] * (tail > 0)
                alignments.append(alignment(ents, s))
                want.append(restated(ops, s, lead, tail, P, strands))
                cases += 1
            flush(P, strands)
    assert cases > 150_000 and mapped > 100_000 and errors > 5_000


# ---- hand cases ---------------------------------------------------------------------------------------------------------
def test_borders_by_hand():
    two = ([10, 8], 1)  # P = 0, 10, 18
    # an alignment that ends exactly at a piece's end is not cut; one that crosses by a single column is
    assert map_one("6=", 4, *two) == ((4, 10, 0, 0, 0, 6, 6, 0, 6, 0), "6=")
    assert map_one("7=", 4, *two) == ((4, 10, 0, 0, 0, 6, 6, 0, 6, CUT_RIGHT), "6=1S")
    assert map_one("7=", 9, *two) == ((0, 6, 1, 0, 1, 7, 6, 0, 6, CUT_LEFT), "1S6=")
    assert map_one("2S8=1S", 10, *two) == ((0, 8, 1, 0, 2, 10, 8, 0, 8, 0), "2S8=1S")
    # a 'D' run and an 'N' run that straddle a border disappear with the side that is cut
    assert map_one("3=4D4=", 5, *two) == ((2, 6, 1, 0, 3, 7, 4, 0, 4, CUT_LEFT), "3S4=")
    assert map_one("4=4D3=", 4, *two) == ((4, 8, 0, 0, 0, 4, 4, 0, 4, CUT_RIGHT), "4=3S")
    assert map_one("3=2I4N4=", 5, *two) == ((2, 6, 1, 0, 5, 9, 4, 0, 4, CUT_LEFT), "5S4=")
    assert map_one("4=4N1X3=", 4, *two) == ((4, 8, 0, 0, 0, 4, 4, 0, 4, CUT_RIGHT), "4=4S")
    # ... and stay, with edits and block as the rule counts them, where they lie inside the home piece
    assert map_one("2=2D1=1N2=1X1=", 0, *two) == ((0, 10, 0, 0, 0, 7, 6, 3, 9, 0), "2=2D1=1N2=1X1=")
    # an 'I' standing at a border goes to the clip of the side that is cut
    assert map_one("4=2I3=", 6, *two) == ((6, 10, 0, 0, 0, 4, 4, 0, 4, CUT_RIGHT), "4=5S")
    assert map_one("2=2I3=", 8, *two) == ((0, 3, 1, 0, 4, 7, 3, 0, 3, CUT_LEFT), "4S3=")
    # a tie between two pieces goes to the lower one
    assert map_one("3=4D3=", 5, *two) == ((5, 8, 0, 0, 0, 3, 3, 0, 3, CUT_RIGHT), "3=3S")
    assert map_one("6=", 7, *two) == ((7, 10, 0, 0, 0, 3, 3, 0, 3, CUT_RIGHT), "3=3S")
    # the kept part begins and ends with '=': an 'X' at the home piece's edge is clipped, one inside it stays
    assert map_one("1X3=1X2=1X", 10, *two) == ((1, 7, 1, 0, 1, 7, 5, 1, 6, CUT_LEFT | CUT_RIGHT), "1S3=1X2=1S")
    # three pieces under one alignment: the last has most, or the middle one
    assert map_one("9=", 3, [5, 3, 6], 1) == ((0, 4, 2, 0, 5, 9, 4, 0, 4, CUT_LEFT), "5S4=")
    assert map_one("1S8=", 3, [5, 4, 6], 1) == ((0, 4, 1, 0, 3, 7, 4, 0, 4, CUT_LEFT | CUT_RIGHT), "3S4=2S")
    # pieces of length 1: one column is kept
    assert map_one("3=", 2, [1, 1, 1, 1, 1], 1) == ((0, 1, 2, 0, 0, 1, 1, 0, 1, CUT_RIGHT), "1=2S")


def test_reverse_pieces_by_hand():
    table = ([10, 8], 2)  # P = 0, 10, 20, 28, 36
    # text 12 .. 16 of the reverse piece of sequence 0 is 4 .. 8 of its forward strand, and the list is turned round
    assert map_one("1S2=1X1=2S", 12, *table) == ((4, 8, 0, 1, 1, 5, 3, 1, 4, 0), "2S1=1X2=1S")
    # forward into reverse of the same sequence: a border like any other; the tie goes to the forward piece
    assert map_one("8=", 6, *table) == ((6, 10, 0, 0, 0, 4, 4, 0, 4, CUT_RIGHT), "4=4S")
    assert map_one("9=", 6, *table) == ((5, 10, 0, 1, 4, 9, 5, 0, 5, CUT_LEFT), "5=4S")
    # cut bits are in text order: removed on the left of the text stays CUT_LEFT on '-'
    assert map_one("3=1I5=", 17, *table) == ((0, 5, 1, 0, 4, 9, 5, 0, 5, CUT_LEFT), "4S5=")
    assert map_one("5=1I3=", 23, *table) == ((3, 8, 1, 0, 0, 5, 5, 0, 5, CUT_RIGHT), "5=4S")
    assert map_one("3=1D5=", 25, *table) == ((2, 7, 1, 1, 3, 8, 5, 0, 5, CUT_LEFT), "5=3S")


def test_clips_that_merge_beyond_the_longest_entry_are_split():
    lead = [(MAX_LENGTH - 2) << 4 | OP_S]
    rec, text = map_one(lead + entries_of("5=8="), 5, [10, 8], 1)
    assert text == f"{MAX_LENGTH}S3S8=" and rec == (0, 8, 1, 0, MAX_LENGTH + 3, MAX_LENGTH + 11, 8, 0, 8, CUT_LEFT)
    rec, text = map_one(entries_of("8=5=") + [MAX_LENGTH << 4 | OP_S, 7 << 4 | OP_S], 2, [10, 8], 1)
    assert text == f"8={MAX_LENGTH}S12S" and rec == (2, 10, 0, 0, 0, 8, 8, 0, 8, CUT_RIGHT)
    # on a reverse piece the split entries are turned round with the rest: the short one first
    rec, text = map_one(lead + entries_of("5=8="), 5, [10, 4], 2)
    assert text == f"8=3S{MAX_LENGTH}S" and rec[:4] == (2, 10, 0, 1)
    # adjacent equal entries of the input are merged like every run
    assert map_one("2=3=1X1X4=", 0, [11], 1) == ((0, 11, 0, 0, 0, 11, 9, 2, 11, 0), "5=2X4=")


@pytest.mark.parametrize("cigar,start,why", [
    ("3X2I", 0, "no '='"), ("4D", 0, "no '='"), ("0=3X", 0, "an '=' of length 0 is none"),
    ("3=1S3=", 0, "a clip between two operations"), ("3=", 17, "beyond the text"),
])
def test_bad_input_comes_back_unmapped(cigar, start, why):
    count = {}
    a = alignment(cigar, start)
    out, offs, ents = map_reference(*batch([a, alignment("3=", 1)]), piece_starts([10, 8], 1), 1, count=count)
    assert out[0].tolist() == (0, 0, UNMAPPED, 0, 0, 0, 0, 0, 0, 0), why
    assert out[1]["seq"] == 0 and offs.tolist() == [0, 0, 1] and count == dict(count, error=1, mapped=1)


def test_bad_records_and_operations_come_back_unmapped():
    P = piece_starts([10, 8], 1)
    good = alignment("2S5=1S", 3)

    def run(change):
        rec, ents, length = good[0].copy(), list(good[1]), good[2]
        rec, ents, length = change(rec, ents, length)
        count = {}
        out, offs, got = map_reference(*batch([(rec, ents, length)]), P, 1, count=count)
        return out[0]["seq"], got.size, count["error"]

    assert run(lambda r, e, n: (r, e, n)) == (0, 3, 0)

    def setf(field, value):
        def change(r, e, n):
            r[field] = value
            return r, e, n
        return change

    for field, value in (("read_start", 1), ("read_start", 8), ("read_end", 6), ("read_end", 9), ("ref_start", 4), ("ref_end", 9),
                         ("ref_end", 19), ("ref_start", 9)):
        assert run(setf(field, value)) == (UNMAPPED, 0, 1), (field, value)
    assert run(lambda r, e, n: (r, e, n + 1)) == (UNMAPPED, 0, 1) and run(lambda r, e, n: (r, e, n - 1)) == (UNMAPPED, 0, 1)
    for bad in (0, 5, 6, 9, 15):
        assert run(lambda r, e, n: (r, e[:1] + [5 << 4 | bad] + e[2:], n)) == (UNMAPPED, 0, 1), bad
    # matches, edits and the other fields of the record are not looked at
    assert run(setf("matches", 99)) == (0, 3, 0) and run(setf("doc", 7)) == (0, 3, 0)


def test_unaligned_reads_and_empty_batches():
    P = piece_starts([10], 2)
    out, offs, ents = map_reference(*batch([None, alignment("4=", 3), None]), P, 2)
    assert out.dtype == MAPPING_DTYPE and offs.dtype == np.uint64 and ents.dtype == np.uint32
    assert out["seq"].tolist() == [UNMAPPED, 0, UNMAPPED] and offs.tolist() == [0, 0, 1, 1]
    assert out[0].tolist() == (0, 0, UNMAPPED, 0, 0, 0, 0, 0, 0, 0)
    out, offs, ents = map_reference(*batch([]), P, 2)
    assert out.size == 0 and offs.tolist() == [0] and ents.size == 0
    with pytest.raises(ValueError, match="strands must be 1 or 2"):
        piece_starts([3], 3)
    with pytest.raises(ValueError, match="length 0"):
        piece_starts([3, 0], 1)


# ---- invariants and the mirror -----------------------------------------------------------------------------------------
def random_alignment(rng, n_text, max_runs=8, max_len=9):
    """A random alignment that fits the text: runs of the five operations with clips around them."""
    while True:
        runs = [(int(rng.choice((OP_EQ, OP_EQ, OP_X, OP_I, OP_D, OP_N))), int(rng.integers(1, max_len + 1)))
                for _ in range(int(rng.integers(1, max_runs + 1)))]
        text = sum(n for op, n in runs if op in TEXT_OPS)
        if text <= n_text and any(op == OP_EQ for op, _ in runs):
            break
    lead, tail = int(rng.integers(0, 4)), int(rng.integers(0, 4))
    ents = [lead << 4 | OP_S] * (lead > 0) + [n << 4 | op for op, n in runs] + [tail << 4 | OP_S] * (tail > 0)
    return alignment(ents, int(rng.integers(0, n_text - text + 1)))


def check_invariants(out, offs, ents, recs, roffs, P, strands):
    for q in range(out.size):
        mine = [int(e) for e in ents[int(offs[q]):int(offs[q + 1])]]
        if out[q]["seq"] == UNMAPPED:
            assert not mine
            continue
        sums = dict.fromkeys(CODE.values(), 0)
        for k, e in enumerate(mine):
            assert 1 <= e >> 4 <= MAX_LENGTH and (k == 0 or mine[k - 1] & 15 != e & 15 or MAX_LENGTH in (e >> 4, mine[k - 1] >> 4))
            sums[e & 15] += e >> 4
        m = out[q]
        p = int(m["seq"]) * strands + int(m["strand"])
        Lp = P[p + 1] - P[p]
        assert sums[OP_EQ] + sums[OP_X] + sums[OP_I] + sums[OP_S] == int(roffs[q + 1]) - int(roffs[q])
        assert sums[OP_EQ] + sums[OP_X] + sums[OP_D] + sums[OP_N] == int(m["target_end"]) - int(m["target_start"]) <= Lp
        assert int(m["target_end"]) <= Lp and int(m["strand"]) < strands
        inner = [e & 15 for e in mine if e & 15 != OP_S]
        assert inner[0] == OP_EQ and inner[-1] == OP_EQ
        kinds = [e & 15 for e in mine]
        assert OP_S not in kinds[kinds.index(OP_EQ):len(kinds) - kinds[::-1].index(OP_EQ)]
        assert sums[OP_EQ] == int(m["matches"]) and sums[OP_X] + sums[OP_I] + sums[OP_D] == int(m["edits"])
        assert sums[OP_EQ] + sums[OP_X] + sums[OP_I] + sums[OP_D] == int(m["block"])
        assert sums[OP_EQ] + sums[OP_X] + sums[OP_I] == int(m["read_end"]) - int(m["read_start"])
        r = recs[q]
        assert int(r["read_start"]) <= int(m["read_start"]) and int(m["read_end"]) <= int(r["read_end"])
        # every column consumes read or text: nothing was cut exactly when both spans are extend's
        whole = (int(m["read_start"]), int(m["read_end"])) == (int(r["read_start"]), int(r["read_end"])) and \
            int(m["target_end"]) - int(m["target_start"]) == int(r["ref_end"]) - int(r["ref_start"])
        assert (int(m["cut"]) == 0) == whole


@pytest.mark.parametrize("strands", [1, 2])
def test_invariants_over_random_alignments(strands):
    rng = np.random.default_rng(10 + strands)
    cut = reverse = 0
    for _ in range(30):
        lens = [int(v) for v in rng.integers(1, 40, int(rng.integers(1, 7)))]
        P = piece_starts(lens, strands)
        alignments = [random_alignment(rng, P[-1]) if rng.random() < 0.9 else None for _ in range(40)]
        args = batch(alignments)
        count = {}
        out, offs, ents = map_reference(*args, P, strands, count=count)
        check_invariants(out, offs, ents, args[0], args[3], P, strands)
        assert count["error"] == 0 and count["mapped"] == sum(a is not None for a in alignments)
        assert count["cut"] == int((out["cut"] != 0).sum()) and count["reverse"] == int(out["strand"].sum())
        assert count["entries_out"] == ents.size and count["entries_in"] == args[2].size
        mapped = out["seq"] != UNMAPPED
        assert count["cut_chars"] == int((args[0]["read_end"][mapped].astype(np.int64) - args[0]["read_start"][mapped]).sum() -
                                         (out["read_end"][mapped].astype(np.int64) - out["read_start"][mapped]).sum())
        cut += count["cut"]
        reverse += count["reverse"]
    assert cut > 200 and (reverse > 200) == (strands == 2)


def test_the_reverse_strand_is_the_mirror_of_the_forward_strand():
    """An alignment in a forward piece and its mirror image in the reverse piece -- the same columns in the opposite
    order, as far from the reverse piece's end as the original is from the forward piece's start -- map to the same
    target span and the same entries; read_start and read_end swap ends."""
    rng = np.random.default_rng(5)
    seen = 0
    for _ in range(300):
        lens = [int(v) for v in rng.integers(4, 30, 3)]
        P = piece_starts(lens, 2)
        s = int(rng.integers(0, 3))
        rec, ents, length = random_alignment(rng, lens[s], max_runs=5, max_len=5)
        off, text = int(rec["ref_start"]), int(rec["ref_end"]) - int(rec["ref_start"])
        fwd = alignment(ents, P[2 * s] + off)
        rev = alignment(ents[::-1], P[2 * s + 1] + lens[s] - off - text)
        out, offs, got = map_reference(*batch([fwd, rev]), P, 2)
        a, b = out[0], out[1]
        assert (a["seq"], a["strand"], b["seq"], b["strand"]) == (s, 0, s, 1)
        assert a["target_start"] == b["target_start"] and a["target_end"] == b["target_end"]
        assert (a["read_start"], a["read_end"]) == (length - b["read_end"], length - b["read_start"])
        assert a.tolist()[6:9] == b.tolist()[6:9]
        assert got[:int(offs[1])].tolist() == got[int(offs[1]):].tolist()
        assert int(b["cut"]) == (int(a["cut"]) >> 1 | (int(a["cut"]) & 1) << 1)  # (the cut bits are in text order)
        seen += int(a["cut"]) != 0
    assert seen > 20


# ---- the sequence table -------------------------------------------------------------------------------------------------
def test_the_name_rule():
    assert sequence_name(b"chr1", 1) == b"chr1"
    assert sequence_name(b"chr1 Homo sapiens", 3) == b"chr1" and sequence_name(b"chr2\tx", 3) == b"chr2"
    assert sequence_name(b"a\x0bb", 1) == b"a" and sequence_name(b"a\x0cb", 1) == b"a" and sequence_name(b"a\rb", 1) == b"a"
    assert sequence_name(b"", 4) == b"seq4" and sequence_name(b" described only", 5) == b"seq5" and sequence_name(None, 12) == b"seq12"
    assert sequence_name(b"a|b:c\xc3\xa9", 1) == b"a|b:c\xc3\xa9"  # (bytes, whatever they are)


def test_table_writer_and_reader(tmp_path, capsys):
    data = seq_table_bytes([b"one", b"empty", b"two"], [5, 0, 7], 2)
    assert data == b"one\t5\t0\t2\ntwo\t7\t10\t2\n"  # (an empty sequence has no line and no place in the text)
    assert capsys.readouterr().err == ""
    assert seq_table_bytes([b"a", b"b"], [3, 4], 1) == b"a\t3\t0\t1\nb\t4\t3\t1\n"
    path = str(tmp_path / "ref.fa.seqs")
    write_seq_table(path, [b"dup", b"x", b"dup", b"dup"], [1, 2, 3, 4], 2)
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "warning" in err and "more than once" in err  # one warning, however many
    assert open(path, "rb").read() == b"dup\t1\t0\t2\nx\t2\t2\t2\ndup\t3\t6\t2\ndup\t4\t12\t2\n"
    assert read_seq_table(path) == ([b"dup", b"x", b"dup", b"dup"], [1, 2, 3, 4], 2)
    assert read_seq_table(path, n_text=20)[2] == 2
    with pytest.raises(ValueError, match="add up to 20 characters, the text has 21"):
        read_seq_table(path, n_text=21)
    with pytest.raises(ValueError, match="strands must be 1 or 2"):
        seq_table_bytes([b"a"], [1], 0)
    for bad, what in ((b"a\t3\t0\n", "line 1 is not"), (b"a\t3\t0\t1\nb\tx\t3\t1\n", "line 2 is not"), (b"\t3\t0\t1\n", "line 1 is not"),
                      (b"a\t3\t0\t1\nb\t3\t3\t2\n", "line 2"), (b"a\t3\t1\t1\n", "line 1"), (b"a\t0\t0\t1\n", "line 1"),
                      (b"a\t3\t0\t3\n", "line 1"), (b"", "no sequences")):
        with open(path, "wb") as f:
            f.write(bad)
        with pytest.raises(ValueError, match=what):
            read_seq_table(path)


# ---- header and exports ------------------------------------------------------------------------------------------------
def _declared():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return code, sorted(set(re.findall(r"\b(spn_[a-z_0-9]+)\s*\(", code)))


def test_map_header_is_plain_c(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include "spumoni_map.h"\nint main(void) { spn_mapping m; spn_map_stats s; (void)m; (void)s; '
                   'return sizeof(spn_mapping) == 48 && sizeof(spn_map_stats) == 80 && sizeof(spa_alignment) == 48 && '
                   'SPN_UNMAPPED == 0xFFFFFFFFu && SPN_CUT_LEFT == 1 && SPN_CUT_RIGHT == 2 && SPE_OP_S == 4 ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "c"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "c")]).returncode == 0
    code, _ = _declared()
    assert "hipStream_t" not in code and "std::" not in code and "#include <hip" not in code
    assert re.findall(r'#include\s+[<"]([^>"]+)', code) == ["stdint.h", "spumoni_extend.h"]
    assert "typedef struct spa_alignment" not in code


def test_map_header_symbols_exported(built):
    _, names = _declared()
    assert names == sorted(capi.MAP_EXPORTS) and len(names) == 5
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(spn_[a-z_0-9]+)\b", out))) == names
    for other in (capi.EXPORTS, capi.DOCVOTE_EXPORTS, capi.MEMS_EXPORTS, capi.PLACE_EXPORTS, capi.CHAIN_EXPORTS, capi.ALIGN_EXPORTS,
                  capi.CIGAR_EXPORTS, capi.EXTEND_EXPORTS, capi.REFTEXT_EXPORTS):
        assert not set(capi.MAP_EXPORTS) & set(other)
    assert capi.C.sizeof(capi.SpnMapStats) == 80 and MAPPING_DTYPE.itemsize == 48
    assert list(MAPPING_DTYPE.names) == ["target_start", "target_end", "seq", "strand", "read_start", "read_end", "matches", "edits",
                                         "block", "cut"]
    assert [f[0] for f in capi.SpnMapStats._fields_] == ["reads", "mapped", "cut_reads", "reverse_reads", "entries_in", "entries_out",
                                                         "cut_chars", "error", "overflow", "kernel_ms", "step_ms", "reserved"]
    for method in ("set_sequences", "map_device", "map_host", "map_stats"):
        assert callable(getattr(capi.Index, method))


def test_map_calls_without_an_index_fail_loudly(built):
    L = capi._spn()
    n = capi.C.c_uint64(0)
    lens = np.array([4], dtype=np.uint64)
    assert L.spn_set_sequences(None, lens.ctypes.data, 1, 2) == -1 and b"non-null" in L.spx_last_error()
    assert L.spn_map_begin(None, 0, 0, 0, None, None, 0, 1, 0, None, None, None, None, None, capi.C.byref(n)) == -1
    assert b"index must be non-null" in L.spx_last_error()
    assert L.spn_map_device(None, None, None, None, 0, None, 0, 0, None, None, None, None) == -1
    assert L.spn_map_fetch(None, None, None) == -1 and L.spn_last_map_stats(None, None) == -1


# ---- build_index --seq-table ---------------------------------------------------------------------------------------------
def _write_fastas(d):
    """Two files, three sequences: one without a header, one with a description behind its name; and an empty record."""
    (d / "a.fa").write_bytes(b"ACGTAC\nGTT\n>chrB some description\tmore\nGGGCC\n  \n>empty\n\n")
    (d / "b.fa").write_bytes(b">\nTTTTACGT\nAC\n")
    (d / "list.txt").write_text(f"{d / 'a.fa'}\n{d / 'b.fa'}\n")


@pytest.mark.parametrize("rev_comp", [True, False])
def test_build_index_writes_the_table_by_hand(built, tmp_path, rev_comp, capfd):
    from spumoni_amd import build_index

    _write_fastas(tmp_path)
    out = tmp_path / "out"
    out.mkdir()
    build_index.main(["-l", str(tmp_path / "list.txt"), "-o", str(out / "ref"), "--seq-table"] + ([] if rev_comp else ["--no-rev-comp"]))
    want = b"seq1\t9\t0\t2\nchrB\t5\t18\t2\nseq3\t10\t28\t2\n" if rev_comp else b"seq1\t9\t0\t1\nchrB\t5\t9\t1\nseq3\t10\t14\t1\n"
    assert (out / "ref.fa.seqs").read_bytes() == want
    names, lengths, strands = read_seq_table(str(out / "ref.fa.seqs"), n_text=os.path.getsize(out / "ref.fa.rawtext"))
    assert (names, lengths, strands) == ([b"seq1", b"chrB", b"seq3"], [9, 5, 10], 2 if rev_comp else 1)
    text = (out / "ref.fa.rawtext").read_bytes()
    P = piece_starts(lengths, strands)
    assert text[P[strands]:P[strands] + 5] == b"GGGCC" and (not rev_comp or text[P[3]:P[4]] == b"GGCCC")
    # without the option the same files but the table
    plain = tmp_path / "plain"
    plain.mkdir()
    build_index.main(["-l", str(tmp_path / "list.txt"), "-o", str(plain / "ref")] + ([] if rev_comp else ["--no-rev-comp"]))
    assert sorted(os.listdir(out)) == sorted(os.listdir(plain) + ["ref.fa.seqs"])
    for f in os.listdir(plain):
        assert (plain / f).read_bytes() == (out / f).read_bytes(), f


def test_build_index_refuses_the_table_under_digestion(built, tmp_path, capsys):
    from spumoni_amd import build_index

    _write_fastas(tmp_path)
    out = tmp_path / "out"
    out.mkdir()
    for digestion in ("-m", "-a"):
        with pytest.raises(SystemExit):
            build_index.main(["-l", str(tmp_path / "list.txt"), "-o", str(out / "ref"), "--seq-table", digestion])
        assert "--seq-table cannot be used with a digestion" in capsys.readouterr().err
    assert os.listdir(out) == []


def test_duplicate_names_are_kept_and_reported_once(built, tmp_path, capfd):
    from spumoni_amd import build_index

    (tmp_path / "d.fa").write_bytes(b">x 1\nACGTT\n>x 2\nGGA\n>y\nCCCA\n>x\nTTG\n")
    build_index.main(["-r", str(tmp_path / "d.fa"), "-o", str(tmp_path / "ref"), "--seq-table"])
    assert (tmp_path / "ref.fa.seqs").read_bytes() == b"x\t5\t0\t2\nx\t3\t10\t2\ny\t4\t16\t2\nx\t3\t24\t2\n"
    assert capfd.readouterr().err.count("more than once in the sequence table") == 1


# ---- the commands --------------------------------------------------------------------------------------------------------
def _map(args, cwd, env=None):
    return subprocess.run([BIN, "map"] + args, cwd=cwd, capture_output=True, text=True, env=env, timeout=120)


def _golden_index(tmp_path, table=b"whole\t%d\t0\t1\n"):
    from tests.test_align_cpu import _index

    _index(tmp_path)
    if table is not None:
        n = os.path.getsize(tmp_path / "ref.fa.rawtext")
        (tmp_path / "ref.fa.seqs").write_bytes(table % n if b"%d" in table else table)


def test_map_usage_without_arguments(built, tmp_path):
    r = _map([], str(tmp_path))
    assert r.returncode == 1
    assert "spumoni map - " in r.stderr
    for opt in ("-h, --help", "-r, --ref", "-p, --pattern", "-n, --no-digest", "-m, --minimizer-alphabet", "-a, --dna-minimizer",
                "-d, --doc-array", "-L, --min-length", "-S, --max-dist", "-G, --max-gap", "-B, --gap-penalty", "-H, --lookback",
                "-F, --max-fill", "-E, --max-extend", "-O, --band", "-N, --mismatch", "-I, --indel"):
        assert opt in r.stderr, opt
    for word in ("<pattern>.paf", "NM:i:", "an:i:", "ct:i:", "dc:i:", "cg:Z:", "255", ".fa.seqs", "spumoni build -n -s"):
        assert word in r.stderr, word
    top = subprocess.run([BIN], capture_output=True, text=True)
    assert top.returncode == 1
    for cmd in ("map", "extend", "cigar", "align", "chain", "place", "mems", "assign", "run", "build"):
        assert f"\t{cmd}\t" in top.stderr, cmd
    usage = subprocess.run([BIN, "build"], capture_output=True, text=True).stderr
    assert "-s, --seq-table" in usage and ".fa.seqs" in usage


@pytest.mark.parametrize("args,table,message", [
    (["-p", "reads.fa", "-n"], None, "Both a reference file (-r) and pattern file (-p) must be provided."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-P"], None, "-P cannot be used with `spumoni map`"),
    (["-r", "ref", "-p", "reads.fa", "-m"], None, "-m / -a cannot be used with `spumoni map`"),
    (["-r", "ref", "-p", "reads.fa", "-a"], None, "-m / -a cannot be used with `spumoni map`"),
    (["-r", "ref", "-p", "reads.fa", "-n", "-m"], None, "-m / -a cannot be used with `spumoni map`"),
    (["-r", "ref", "-p", "reads.fa"], None, "`spumoni map` needs -n"),
    (["-r", "nosuch", "-p", "reads.fa", "-n"], None, "The following path is not valid: nosuch.fa"),
    (["-r", "ref", "-p", "missing.fa", "-n"], None, "The following path is not valid: missing.fa"),
    (["-r", "ref", "-p", "reads.fa", "-n", "-L", "0"], None, "the minimum match length (-L) must be at least 1."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-E", "4097"], None, "the largest extended end (-E) must be between 1 and 4096."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-O", "64"], None, "the band (-O) must be between 0 and 63."),
    (["-r", "ref", "-p", "reads.fa", "-n"], None, "the index has no sequence table (ref.fa.seqs): build it with -s"),
    (["-r", "ref", "-p", "reads.fa", "-n"], b"a\t5\t0\n", "ref.fa.seqs: line 1 is not name<TAB>length<TAB>text_start<TAB>strands"),
    (["-r", "ref", "-p", "reads.fa", "-n"], b"a\t5\t0\t2\nb\tx\t10\t2\n", "ref.fa.seqs: line 2 is not name"),
    (["-r", "ref", "-p", "reads.fa", "-n"], b"a\t5\t0\t2\nb\t4\t10\t1\n", "ref.fa.seqs: line 2: strands, length or text_start"),
    (["-r", "ref", "-p", "reads.fa", "-n"], b"a\t5\t3\t1\n", "ref.fa.seqs: line 1: strands, length or text_start"),
    (["-r", "ref", "-p", "reads.fa", "-n"], b"a\t0\t0\t1\n", "ref.fa.seqs: line 1: strands, length or text_start"),
    (["-r", "ref", "-p", "reads.fa", "-n"], b"a\t5\t0\t3\n", "ref.fa.seqs: line 1: strands, length or text_start"),
    (["-r", "ref", "-p", "reads.fa", "-n"], b"\n", "ref.fa.seqs: no sequences"),
])
def test_map_refusals_leave_no_file(built, tmp_path, args, table, message):
    _golden_index(tmp_path, table)
    before = sorted(os.listdir(tmp_path))
    r = _map(args, str(tmp_path))
    assert r.returncode == 1
    assert message in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_map_missing_entry_point_on_the_fake_device(built, fake_device, tmp_path):
    _golden_index(tmp_path)
    before = sorted(os.listdir(tmp_path))
    env = dict(os.environ, LD_LIBRARY_PATH=fake_device + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = _map(["-r", "ref", "-p", "reads.fa", "-n", "-L", "4"], str(tmp_path), env=env)
    assert r.returncode == 1
    assert "has no spn_set_sequences" in r.stderr and "`spumoni map`" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_a_failing_map_run_writes_nothing(built, tmp_path):
    """Without a device the command stops at its entry points; with one, at a table that does not add up to the text, and
    then at a read that is empty: either way no file."""
    _golden_index(tmp_path)
    before = sorted(os.listdir(tmp_path))
    if built.spx_device_count() > 0:
        n = os.path.getsize(tmp_path / "ref.fa.rawtext")
        (tmp_path / "ref.fa.seqs").write_bytes(b"whole\t%d\t0\t1\n" % (n - 1))
        r = _map(["-r", "ref", "-p", "reads.fa", "-n"], str(tmp_path))
        assert r.returncode == 1 and f"ref.fa.seqs: the sequences add up to {n - 1} characters, the text has {n}" in r.stderr, r.stderr
        assert sorted(os.listdir(tmp_path)) == before
        (tmp_path / "ref.fa.seqs").write_bytes(b"whole\t%d\t0\t1\n" % n)
        with open(tmp_path / "reads.fa", "ab") as f:
            f.write(b">bad_one\n>after\nACGT\n")
    r = _map(["-r", "ref", "-p", "reads.fa", "-n", "-d"], str(tmp_path))
    assert r.returncode == 1
    if built.spx_device_count() > 0:
        assert "bad_one was empty" in r.stderr, r.stderr
    else:
        assert "no usable gfx950 device" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_build_refuses_the_table_under_digestion(built, tmp_path):
    _write_fastas(tmp_path)
    (tmp_path / "out").mkdir()
    for digestion in (["-m"], ["-t"], []):
        r = subprocess.run([BIN, "build", "-r", str(tmp_path / "a.fa"), "-o", str(tmp_path / "out" / "x"), "-M", "-s"] + digestion,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "the sequence table (-s) cannot be written for a digested text" in r.stderr, r.stderr
        assert os.listdir(tmp_path / "out") == []
