"""CPU tier of the CIGARs: the path rule (spumoni_amd/cigar.py: gap_path) against an enumeration of all alignments, hand
written cases of the tie rule and closed forms; the definition (cigar_reference) by its invariants, by a replay of every
CIGAR against the read and the text, against align_reference's records and on hand-computed cases; the plain-C header
include/spumoni_cigar.h and the library's exports, the loud failure without a device, and `spumoni cigar`'s usage,
validation messages and its failure against a library without the cigar kernels.  What the kernels and the command
compute is tests/test_gpu_cigar.py's business."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from spumoni_amd import capi
from spumoni_amd.align import ALIGN_DTYPE, UNALIGNED, UNFILLED, AlignParams, align_reference, gap_fill
from spumoni_amd.chain import CHAIN_DTYPE, NO_DOC, NO_PRED, UNCHAINED, ChainParams, chain_reference
from spumoni_amd.cigar import (MAX_LENGTH, OP_D, OP_EQ, OP_I, OP_N, OP_X, cigar_reference, cigar_text, gap_path, pack_runs,
                               runs_of)
from tests.test_align_cpu import _index, _planted, _recs, clustered_reads
from tests.test_chain_cpu import planted_reads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
HEADER = os.path.join(ROOT, "include", "spumoni_cigar.h")


@pytest.fixture(scope="module")
def built(built_all):
    return capi.lib()


# ---- the path rule -----------------------------------------------------------------------------------------------------
def _all_paths(A, B):
    """EVERY global alignment of A and B as its list of steps from (0, 0) to (a, b), by recursion over its first column."""
    if not A and not B:
        yield []
        return
    if A:
        for rest in _all_paths(A[1:], B):
            yield [OP_I] + rest
    if B:
        for rest in _all_paths(A, B[1:]):
            yield [OP_D] + rest
    if A and B:
        for rest in _all_paths(A[1:], B[1:]):
            yield [OP_EQ if A[0] == B[0] else OP_X] + rest


def _cost(steps):
    return sum(s != OP_EQ for s in steps), sum(s == OP_EQ for s in steps)


RANK = {OP_EQ: 0, OP_X: 0, OP_I: 1, OP_D: 2}  # the rule's order: diagonal, up, left


def _picked(A, B):
    """The rule without a table: among the optimal alignments the one whose steps, read from (a, b) BACK to (0, 0), come
    first in the order diagonal, up, left.  (Every prefix of an optimal alignment is optimal for its cell, so "the first
    candidate that equals W[i][j]" is "the first last step an optimal alignment of that cell can have".)"""
    paths = [(_cost(p), p) for p in _all_paths(A, B)]
    best = min((e, -m) for (e, m), _ in paths)
    optimal = [p for (e, m), p in paths if (e, -m) == best]
    return min(optimal, key=lambda p: [RANK[s] for s in reversed(p)]), (best[0], -best[1]), len(optimal)


def test_path_against_every_alignment_up_to_5_by_5():
    strings = [bytes(s) for n in range(6) for s in itertools.product(b"AC", repeat=n)]
    assert len(strings) == 63
    ties = 0
    for A in strings:
        for B in strings:
            want, cost, n_optimal = _picked(A, B)
            got = gap_path(A, B)
            assert _cost(got) == cost == gap_fill(A, B), (A, B)
            assert got == want, (A, B, got, want)
            ties += n_optimal > 1
    assert ties > 1000  # (the order decides something)
    rng = np.random.default_rng(3)
    for _ in range(40):
        A, B = (bytes(rng.choice(list(b"ACGT"), int(rng.integers(1, 6))).astype(np.uint8)) for _ in range(2))
        assert gap_path(A, B) == _picked(A, B)[0], (A, B)


def _text_of(A, B):
    return cigar_text(pack_runs(runs_of(gap_path(A, B))))


def test_the_tie_rule_by_hand():
    # AAAA against AA: the diagonal comes first, so the two matches stand at the END and the insertions in front of them
    assert _text_of(b"AAAA", b"AA") == "2I2="
    assert _text_of(b"AA", b"AAAA") == "2D2="
    # ACA against AA: (3, 2) is a match; at (2, 1) the diagonal (C on A) costs 2, up costs 1: the C is inserted
    assert _text_of(b"ACA", b"AA") == "1=1I1="
    assert _text_of(b"AA", b"ACA") == "1=1D1="
    for n in (1, 2, 7, 40):
        S = bytes(np.random.default_rng(n).choice(list(b"ACGT"), n).astype(np.uint8))
        assert _text_of(S, S) == f"{n}="
        assert _text_of(b"A" * n, b"C" * n) == f"{n}X"
    # disjoint letters and unequal lengths: substitutions at the end, the surplus in front
    assert _text_of(b"AAA", b"CC") == "1I2X" and _text_of(b"CC", b"AAA") == "1D2X"
    # an empty side
    assert _text_of(b"", b"ACG") == "3D" and _text_of(b"ACG", b"") == "3I" and gap_path(b"", b"") == []
    # up before left: AC against CA has two optimal paths of 2 edits and 1 match; the walk back from (2, 2) finds C on A
    # unequal (diagonal: 2 edits, 0 matches: not the optimum), then up (A on A behind it: 1 + 0 edits... the optimum)
    assert _text_of(b"AC", b"CA") == "1D1=1I"
    assert _picked(b"AC", b"CA")[0] == [OP_D, OP_EQ, OP_I]


def test_pack_runs_merges_and_splits():
    assert pack_runs([(OP_EQ, 3), (OP_EQ, 0), (OP_EQ, 4), (OP_I, 0), (OP_EQ, 1), (OP_X, 2)]) == [8 << 4 | OP_EQ, 2 << 4 | OP_X]
    assert pack_runs([]) == [] and cigar_text([]) == "*"
    assert pack_runs([(OP_N, MAX_LENGTH)]) == [MAX_LENGTH << 4 | OP_N]
    assert pack_runs([(OP_N, MAX_LENGTH + 1)]) == [MAX_LENGTH << 4 | OP_N, 1 << 4 | OP_N]
    assert pack_runs([(OP_D, 5), (OP_D, 2 * MAX_LENGTH)]) == [MAX_LENGTH << 4 | OP_D] * 2 + [5 << 4 | OP_D]
    assert cigar_text([12 << 4 | OP_EQ, 1 << 4 | OP_X, 30 << 4 | OP_EQ, 2 << 4 | OP_I, 3 << 4 | OP_D, 9 << 4 | OP_N]) == "12=1X30=2I3D9N"
    assert MAX_LENGTH == 2**28 - 1 and (OP_I, OP_D, OP_N, OP_EQ, OP_X) == (1, 2, 3, 7, 8)


# ---- cigar_reference: invariants and replay ----------------------------------------------------------------------------
def replay(entries, R, T, rec):
    """Walks a read's entries along the read and the text: '=' columns are equal characters, 'X' columns unequal ones, and
    the spans add up.  Returns the sums per operation."""
    x, y = int(rec["read_start"]), int(rec["ref_start"])
    sums = dict.fromkeys((OP_I, OP_D, OP_N, OP_EQ, OP_X), 0)
    last = None
    for e in (int(e) for e in entries):
        op, n = e & 15, e >> 4
        assert op in sums and 1 <= n <= MAX_LENGTH
        assert op != last or prev_n == MAX_LENGTH, "adjacent entries of one operation: only behind a full one"
        last, prev_n = op, n
        sums[op] += n
        if op in (OP_EQ, OP_X):
            a, b = np.frombuffer(R[x:x + n], dtype=np.uint8), np.frombuffer(T[y:y + n], dtype=np.uint8)
            assert a.size == n and b.size == n
            assert ((a == b) if op == OP_EQ else (a != b)).all(), (op, x, y, n)
            x, y = x + n, y + n
        elif op == OP_I:
            x += n
        else:
            y += n
    assert (x, y) == (int(rec["read_end"]), int(rec["ref_end"]))
    return sums


def check_invariants(out, op_offsets, entries, goffs, gaps, R, roffs, T):
    """The five invariants of include/spumoni_cigar.h and the replay, read by read."""
    R, T = bytes(R), bytes(T)
    for q in range(out.size):
        mine = entries[int(op_offsets[q]):int(op_offsets[q + 1])]
        if out[q]["ref_start"] == np.uint64(UNALIGNED):
            assert mine.size == 0
            continue
        g = gaps[int(goffs[q]):int(goffs[q + 1])]
        un = g[g["edits"] == UNFILLED]
        un_i, un_ab = int(un["a"].astype(np.int64).sum()), int((un["a"].astype(np.int64) + un["b"].astype(np.int64)).sum())
        s = replay(mine, R[int(roffs[q]):int(roffs[q + 1])], T, out[q])
        assert s[OP_EQ] == int(out[q]["matches"]), q
        assert s[OP_X] + s[OP_I] + s[OP_D] == int(out[q]["edits"]) + un_i, q
        assert s[OP_N] + un_i == un_ab, q
        assert s[OP_EQ] + s[OP_X] + s[OP_I] == int(out[q]["read_end"]) - int(out[q]["read_start"]), q
        assert s[OP_EQ] + s[OP_X] + s[OP_D] + s[OP_N] == int(out[q]["ref_end"]) - int(out[q]["ref_start"]), q


def two_letter_reads(rng, text, nreads, letters=b"AC"):
    """Reads made of stretches of the text -- every anchor a true match -- with random characters between them, anchors that
    overlap their predecessor in the text (a stretch that starts d characters before the last one ended: a = d, b = 0) or in
    the read (a stretch whose first d characters are the last one's final d: a = 0), and some reads without anchors."""
    L = np.frombuffer(letters, dtype=np.uint8)
    reads, anchors, counts = [], [], []
    for q in range(nreads):
        h = int(rng.integers(1, 7)) if q % 6 else 0
        y_end = int(rng.integers(10, text.size - 400))
        parts, x = [], 0
        for t in range(h):
            l, d, kind = int(rng.integers(3, 12)), int(rng.integers(1, 3)), rng.random() if t else 1.0
            if kind < 0.25:
                y = y_end - d
                parts.append(text[y:y + l])
                anchors.append((x, y, l))
                x += l
            elif kind < 0.5 and any((text[y2:y2 + d] == text[y_end - d:y_end]).all() for y2 in range(y_end, y_end + 9)):
                y = next(y2 for y2 in range(y_end, y_end + 9) if (text[y2:y2 + d] == text[y_end - d:y_end]).all())
                parts.append(text[y + d:y + l])
                anchors.append((x - d, y, l))
                x += l - d
            else:
                a, b = (int(rng.integers(0, 9)), int(rng.integers(0, 9))) if t else (0, 0)
                parts.append(L[rng.integers(0, L.size, a)])
                y = y_end + b
                parts.append(text[y:y + l])
                anchors.append((x + a, y, l))
                x += a + l
            y_end = y + l
        reads.append(np.concatenate(parts) if parts else np.full(3, ord("N"), dtype=np.uint8))
        counts.append(h)
    return reads, anchors, counts


def crafted(reads, anchors, counts, front=0):
    """(R, roffs, records, moffs, chains, pred): every read chained over ALL of its anchors in order."""
    counts = np.asarray(counts, dtype=np.int64)
    moffs = (front + np.r_[0, np.cumsum(counts)]).astype(np.uint64)
    roffs = np.r_[0, np.cumsum([r.size for r in reads])].astype(np.uint64)
    rec = _recs([(1, 1, 1)] * front + list(anchors))
    chains = np.zeros(counts.size, dtype=CHAIN_DTYPE)
    chains["ref_start"], chains["doc"] = UNCHAINED, NO_DOC
    pred = np.full(rec.size, NO_PRED, dtype=np.uint32)
    for q, h in enumerate(counts):
        if h:
            o = int(moffs[q])
            first, last = rec[o], rec[o + h - 1]
            chains[q] = (first["ref_pos"], int(last["ref_pos"]) + int(last["length"]), first["read_pos"],
                         int(last["read_pos"]) + int(last["length"]), 0, h, 0, h - 1, 0, q % 5)
            pred[o + 1:o + h] = np.arange(h - 1)
    return np.concatenate(reads) if reads else np.zeros(0, dtype=np.uint8), roffs, rec, moffs, chains, pred


@pytest.mark.parametrize("seed", range(3))
def test_invariants_and_replay_over_two_letters(seed):
    rng = np.random.default_rng(seed)
    text = np.frombuffer(b"AC", dtype=np.uint8)[rng.integers(0, 2, 3000)]
    R, roffs, rec, moffs, chains, pred = crafted(*two_letter_reads(rng, text, 60), front=seed)
    tables = unfilled = 0
    for max_fill in (512, 4, 1):
        p = AlignParams(max_fill)
        out, op_offsets, entries = cigar_reference(R, roffs, text, moffs, rec, chains, pred, p)
        want, goffs, gaps = align_reference(R, roffs, text, moffs, rec, chains, pred, p)
        assert out.dtype == ALIGN_DTYPE and np.array_equal(out, want)
        assert op_offsets.dtype == np.uint64 and op_offsets.size == out.size + 1 and entries.dtype == np.uint32
        assert int(op_offsets[-1]) == entries.size and (np.diff(op_offsets.astype(np.int64)) >= 0).all()
        check_invariants(out, op_offsets, entries, goffs, gaps, R, roffs, text)
        tables += int(((gaps["a"] > 1) & (gaps["b"] > 1) & (gaps["edits"] != UNFILLED)).sum())
        unfilled += int((gaps["edits"] == UNFILLED).sum())
    assert tables > 20 and unfilled > 20  # (of the input: tables with ties, and gaps left unfilled)


def test_records_equal_align_reference_on_both_planted_sets(oracle_mod):
    text, seqs, offs, cuts = planted_reads()
    mo, rec, chains, (want, goffs, gaps) = _planted(oracle_mod, text, seqs, offs)
    _, _, pred = chain_reference(mo, rec)
    out, op_offsets, entries = cigar_reference(seqs, offs, text, mo, rec, chains, pred)
    assert np.array_equal(out, want)
    check_invariants(out, op_offsets, entries, goffs, gaps, seqs, offs, text)
    for q in range(len(cuts)):  # two substitutions, three characters deleted, two inserted: 7 edits in 4 places
        ops = [int(e) & 15 for e in entries[int(op_offsets[q]):int(op_offsets[q + 1])]]
        assert ops == [OP_EQ, OP_X, OP_EQ, OP_D, OP_EQ, OP_X, OP_EQ, OP_I, OP_EQ], (q, ops)
    text, seqs, offs = clustered_reads()
    mo, rec, chains, (want, goffs, gaps) = _planted(oracle_mod, text, seqs, offs)
    _, _, pred = chain_reference(mo, rec)
    out, op_offsets, entries = cigar_reference(seqs, offs, text, mo, rec, chains, pred)
    assert np.array_equal(out, want) and int(op_offsets[-1]) > 12 * 20
    check_invariants(out, op_offsets, entries, goffs, gaps, seqs, offs, text)


def _one(R, T, anchors, max_fill=512, front=0):
    """One read chained over all of `anchors`, with `front` characters and records of another in front of it."""
    args = crafted([np.frombuffer(b"N" * front, dtype=np.uint8), np.frombuffer(R, dtype=np.uint8)], list(anchors), [0, len(anchors)], front=front)
    out, op_offsets, entries = cigar_reference(args[0], args[1], np.frombuffer(T, dtype=np.uint8), *args[3:4], args[2], *args[4:],
                                               AlignParams(max_fill))
    assert int(op_offsets[1]) == 0  # (the read in front has no chain)
    return cigar_text(entries[int(op_offsets[1]):]), out[1].tolist()


def test_hand_computed_cigars():
    T = b"." * 100 + b"ACGTACGTAC" + b"GG" + b"TTTTTTTTTT" + b"ACT" + b"CCCCCCCCCC" + b"." * 20
    #                   100            110     112             122      125
    assert _one(b"ACGTACGTAC", T, [(0, 100, 10)])[0] == "10="
    assert _one(b"ACGTACGTAC", T, [(0, 100, 10)], front=3)[0] == "10="
    # merging across a gap and its anchors: the gap ACT against ACT is three matches between two anchors
    assert _one(b"TTTTTTTTTTACTCCCCCCCCCC", T, [(0, 112, 10), (13, 125, 10)]) == ("23=", (112, 135, 0, 23, 23, 0, 2, 0, 0, 1))
    # ... with a substitution at its end the last match run is the anchor's alone
    assert _one(b"TTTTTTTTTTACGCCCCCCCCCC", T, [(0, 112, 10), (13, 125, 10)])[0] == "12=1X10="
    # AA against ACT: (2, 3): A on T unequal, the diagonal (AA / AC: 1 edit 1 match, + 1) ties with left (AA / AC + 1)?  no:
    # left is W[2][2] + 1 = (1, 1) + 1 = (2, 1) and so is the diagonal: the diagonal comes first
    assert _one(b"TTTTTTTTTTAACCCCCCCCCC", T, [(0, 112, 10), (12, 125, 10)], front=2)[0] == "11=1D1X10="
    # overlaps: a = 0 (two text characters more), b = 0 (two read characters more)
    assert _one(b"x" * 16, T, [(0, 100, 10), (6, 108, 10)])[0] == "10=2D6="
    assert _one(b"x" * 19, T, [(0, 100, 10), (9, 107, 10)])[0] == "10=2I7="
    # an unfilled gap: the read's side is inserted, the text's side skipped
    text, rec = _one(b"TTTTTTTTTTACGCCCCCCCCCC", T, [(0, 112, 10), (13, 125, 10)], max_fill=2)
    assert text == "10=3I3N10=" and rec[4:9] == (20, 0, 2, 1, 3)
    # three anchors, the first gap a deletion, the second one not filled (b = 3 > 2)
    assert _one(b"ACGTACGTACTTTTTTTTTTAACCCCCCCCCC", T, [(0, 100, 10), (10, 112, 10), (22, 125, 10)], max_fill=2)[0] == "10=2D10=2I3N10="
    # the split of a run of 2^28 + 5: an unfilled gap of as many text characters
    far = 2**28 + 5
    text, rec = _one(b"x" * 20, T, [(0, 100, 10), (10, 110 + far, 10)])
    assert text == f"10={2**28 - 1}N6N10=" and rec[1] == 120 + far and rec[7:9] == (1, far)
    # no reads; a read without a chain
    out, op_offsets, entries = cigar_reference(np.zeros(0, dtype=np.uint8), [0], np.zeros(0, dtype=np.uint8), [0], _recs([]),
                                               np.zeros(0, dtype=CHAIN_DTYPE), [])
    assert out.size == 0 and op_offsets.tolist() == [0] and entries.size == 0 and entries.dtype == np.uint32
    chains, _, pred = chain_reference([0, 0], _recs([]))
    out, op_offsets, entries = cigar_reference(np.zeros(0, dtype=np.uint8), [0, 0], np.zeros(0, dtype=np.uint8), [0, 0], _recs([]), chains, pred)
    assert out[0].tolist() == (UNALIGNED, 0, 0, 0, 0, 0, 0, 0, 0, NO_DOC) and op_offsets.tolist() == [0, 0]
    with pytest.raises(ValueError, match="max_fill must be 1 .. 4096"):
        cigar_reference(np.zeros(0, dtype=np.uint8), [0], np.zeros(0, dtype=np.uint8), [0], _recs([]), np.zeros(0, dtype=CHAIN_DTYPE), [], (0,))


# ---- header and command ------------------------------------------------------------------------------------------------
def _declared():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return code, sorted(set(re.findall(r"\b(spg_[a-z_0-9]+)\s*\(", code)))


def test_cigar_header_is_plain_c(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include "spumoni_cigar.h"\nint main(void) { spa_alignment c; spg_cigar_stats s; (void)c; (void)s; '
                   'return sizeof(spa_alignment) == 48 && sizeof(spg_cigar_stats) == 104 && sizeof(spa_params) == 4 && '
                   'SPG_MAX_LENGTH == 268435455u && SPG_OP_I == 1 && SPG_OP_D == 2 && SPG_OP_N == 3 && SPG_OP_EQ == 7 && SPG_OP_X == 8 '
                   '? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "c"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "c")]).returncode == 0
    code, _ = _declared()
    assert "hipStream_t" not in code and "std::" not in code and "#include <hip" not in code
    assert re.findall(r'#include\s+[<"]([^>"]+)', code) == ["stdint.h", "spumoni_align.h"]
    assert "typedef struct spa_alignment" not in code  # (the record is spumoni_align.h's, reused)


def test_cigar_header_symbols_exported(built):
    _, names = _declared()
    assert names == sorted(capi.CIGAR_EXPORTS) and len(names) == 4
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(spg_[a-z_0-9]+)\b", out))) == names
    for other in (capi.EXPORTS, capi.DOCVOTE_EXPORTS, capi.MEMS_EXPORTS, capi.PLACE_EXPORTS, capi.CHAIN_EXPORTS, capi.ALIGN_EXPORTS,
                  capi.REFTEXT_EXPORTS):
        assert not set(capi.CIGAR_EXPORTS) & set(other)
    assert capi.C.sizeof(capi.SpgCigarStats) == 104
    assert [f[0] for f in capi.SpgCigarStats._fields_] == ["reads", "aligned_reads", "gaps", "filled_gaps", "cells", "entries", "path_words",
                                                           "wave_fill_ticks", "wave_back_ticks", "error", "overflow", "kernel_ms", "step_ms"]
    for method in ("cigar_device", "cigar_host", "cigar_stats"):
        assert callable(getattr(capi.Index, method))


def test_cigar_begin_without_device_fails_loudly(built):
    if built.spx_device_count() > 0:
        pytest.skip("a device is visible: the no-device path is this machine's CPU tier")
    L = capi._spg()
    seqs, offs = np.frombuffer(b"ACGT", dtype=np.uint8), np.array([0, 4], dtype=np.uint64)
    out = np.zeros(1, dtype=ALIGN_DTYPE)
    n = capi.C.c_uint64(0)
    rc = L.spg_cigar_begin(None, 0, 0, 0, seqs.ctypes.data, offs.ctypes.data, 1, 1, 0, capi.SpcParams(64, 5000, 500, 1), capi.SpaParams(512),
                           out.ctypes.data, None, None, capi.C.byref(n))
    assert rc == -3 and b"no CPU fallback" in L.spx_last_error()


def _cigar(args, cwd, env=None):
    return subprocess.run([BIN, "cigar"] + args, cwd=cwd, capture_output=True, text=True, env=env, timeout=120)


def test_usage_without_arguments(built, tmp_path):
    r = _cigar([], str(tmp_path))
    assert r.returncode == 1
    assert "spumoni cigar - " in r.stderr
    for opt in ("-h, --help", "-r, --ref", "-p, --pattern", "-n, --no-digest", "-m, --minimizer-alphabet", "-a, --dna-minimizer",
                "-K, --small-window", "-W, --large-window", "-d, --doc-array", "-L, --min-length", "-S, --max-dist", "-G, --max-gap",
                "-B, --gap-penalty", "-H, --lookback", "-F, --max-fill"):
        assert opt in r.stderr, opt
    for limits in ("1 or more", "1 .. 2147483647", "0 .. 2147483647", "0 .. 65535", "1 .. 64", "1 .. 4096", "268435455"):  # the ranges are stated
        assert limits in r.stderr, limits
    assert "-P, --PML" not in r.stderr and "<pattern>.cigars" in r.stderr and "= X I D" in r.stderr
    top = subprocess.run([BIN], capture_output=True, text=True)
    assert top.returncode == 1
    for cmd in ("cigar", "align", "chain", "place", "mems", "assign", "run", "build"):
        assert f"\t{cmd}\t" in top.stderr, cmd


@pytest.mark.parametrize("args,message", [
    (["-p", "reads.fa", "-n"], "Both a reference file (-r) and pattern file (-p) must be provided."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-P"], "-P cannot be used with `spumoni cigar`"),
    (["-r", "ref", "-p", "reads.fa", "-n", "-M", "-P"], "-P cannot be used with `spumoni cigar`"),
    (["-r", "nosuch", "-p", "reads.fa", "-n"], "The following path is not valid: nosuch.fa"),
    (["-r", "ref", "-p", "missing.fa", "-n"], "The following path is not valid: missing.fa"),
    (["-r", "ref", "-p", "reads.txt", "-n"], "The pattern file provided does not appear to be a FASTA"),
    (["-r", "ref", "-p", "reads.fa", "-m", "-a"], "Only one type of minimizer can be specified from either -m or -a."),
    (["-r", "ref", "-p", "reads.fa"], "A minimizer type must be specified using -m or -a."),
    (["-r", "ref", "-p", "reads.fa", "-a", "-K", "5", "-W", "11"], "small window size (k) cannot be larger than 4 characters."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-L", "0"], "the minimum match length (-L) must be at least 1."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-S", "0"], "the largest distance (-S) must be between 1 and 2147483647."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-G", "2147483648"], "the largest gap (-G) must be between 0 and 2147483647."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-B", "65536"], "the gap penalty (-B) must be between 0 and 65535."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-H", "65"], "the lookback (-H) must be between 1 and 64."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-F", "0"], "the largest filled gap (-F) must be between 1 and 4096."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-F", "4097"], "the largest filled gap (-F) must be between 1 and 4096."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-F", "-1"], "the largest filled gap (-F) must be between 1 and 4096."),
])
def test_validation_messages(built, tmp_path, args, message):
    _index(tmp_path)
    shutil.copy(tmp_path / "reads.fa", tmp_path / "reads.txt")
    before = sorted(os.listdir(tmp_path))
    r = _cigar(args, str(tmp_path))
    assert r.returncode == 1
    assert message in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_doc_ids_without_doc_file_are_refused(built, tmp_path):
    _index(tmp_path, doc=False)
    before = sorted(os.listdir(tmp_path))
    r = _cigar(["-r", "ref", "-p", "reads.fa", "-n", "-d"], str(tmp_path))
    assert r.returncode == 1
    assert "document array file (ref.fa.doc) is not present, so it cannot be used." in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_missing_entry_point_on_the_fake_device(built, fake_device, tmp_path):
    _index(tmp_path)
    before = sorted(os.listdir(tmp_path))
    env = dict(os.environ, LD_LIBRARY_PATH=fake_device + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = _cigar(["-r", "ref", "-p", "reads.fa", "-n", "-L", "4"], str(tmp_path), env=env)
    assert r.returncode == 1
    assert "has no spg_cigar_begin" in r.stderr and "`spumoni cigar`" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_no_device_fails_loudly_and_writes_nothing(built, tmp_path):
    if built.spx_device_count() > 0:
        pytest.skip("a device is visible: the no-device path is this machine's CPU tier")
    _index(tmp_path)
    before = sorted(os.listdir(tmp_path))
    r = _cigar(["-r", "ref", "-p", "reads.fa", "-n", "-d"], str(tmp_path))
    assert r.returncode == 1
    assert "no usable gfx950 device" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_the_entries_and_their_text_under_the_sanitizers(tmp_path):
    """The host code that gathers a super-batch's entries piece by piece and writes the CIGARs (spumoni_amd/csrc/host/
    cigar_text.hpp) in a stand-alone program (tests/cigar_text_check.cpp) with the address and undefined-behaviour
    sanitizers: five reads in two pieces, pieces and reads without entries, every op code, the longest run, and `map`'s
    form without the clips.  The text is written out by hand here."""
    exe = str(tmp_path / "cigar_text_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(ROOT, "tests", "cigar_text_check.cpp")], check=True)
    p = subprocess.run([exe, str(tmp_path / "out.txt")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "cigar text ok" in p.stdout, p.stdout + p.stderr
    lines = (tmp_path / "out.txt").read_text().split("\n")
    # two pieces (reads 0-2, reads 3-4): read 3's CIGAR is its own, not a slice of the first piece's entries
    assert lines[:5] == ["3S10=1X2I", "*", "5=4D6N7=", "2S9=1S", "268435455=1="]
    assert lines[5:10] == ["10=1X2I", "", "5=4D6N7=", "9=", "268435455=1="]  # `map`: no S, no *
    assert lines[10:14] == ["1=", "*", "*", "2X"]  # a piece without entries between two with
    assert lines[14:16] == ["*", "*"]
    assert lines[16:18] == ["1?2I3D4N5S6?7?8=9X10?11?12?13?14?15?16?", "1?2I3D4N6?7?8=9X10?11?12?13?14?15?16?"]  # op codes 0 .. 15
    assert lines[18:] == ["", ""]  # a read of clips only in `map`'s form, and the end of the file
