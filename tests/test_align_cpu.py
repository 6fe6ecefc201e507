"""CPU tier of the alignments: the gap rule (spumoni_amd/align.py: gap_fill) against an exhaustive recursion over all
alignments, a textbook Levenshtein and closed forms; the definition (align_reference) against a second, separately
written loop, on hand-computed records and on two planted cases; the plain-C header include/spumoni_align.h and the
library's exports, the loud failure without a device, and `spumoni align`'s usage, validation messages and its failure
against a library without the align kernels.  What the kernels and the command compute is tests/test_gpu_align.py's
business."""
import functools
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from spumoni_amd import capi, synth
from spumoni_amd.align import (ALIGN_DTYPE, GAP_DTYPE, UNALIGNED, UNFILLED, AlignParams, align_reference, check_params,
                               gap_fill)
from spumoni_amd.chain import CHAIN_DTYPE, NO_DOC, NO_PRED, UNCHAINED, ChainParams, chain_reference
from spumoni_amd.mems import MATCH_DTYPE, mems_reference
from tests.test_chain_cpu import planted_reads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
HEADER = os.path.join(ROOT, "include", "spumoni_align.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "files", "dna_fastq")


@pytest.fixture(scope="module")
def built(built_all):
    return capi.lib()


# ---- the gap rule ------------------------------------------------------------------------------------------------------
def _all_alignments(A, B):
    """(edits, matches) of EVERY global alignment of A and B, by recursion over its first column."""
    if not A and not B:
        yield 0, 0
        return
    if A:
        for e, m in _all_alignments(A[1:], B):
            yield e + 1, m
    if B:
        for e, m in _all_alignments(A, B[1:]):
            yield e + 1, m
    if A and B:
        same = A[0] == B[0]
        for e, m in _all_alignments(A[1:], B[1:]):
            yield e + (not same), m + same


def _exhaustive(A, B):
    best = min(e for e, _ in _all_alignments(A, B))
    return best, max(m for e, m in _all_alignments(A, B) if e == best)


def levenshtein(A, B):
    """The textbook two-row table."""
    prev = list(range(len(B) + 1))
    for i, ca in enumerate(A, start=1):
        row = [i]
        for j, cb in enumerate(B, start=1):
            row.append(min(prev[j] + 1, row[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = row
    return prev[len(B)]


def test_gap_rule_against_every_alignment():
    strings = [bytes(s) for n in range(5) for s in itertools.product(b"AC", repeat=n)]
    assert len(strings) == 31
    for A in strings:
        for B in strings:
            assert gap_fill(A, B) == _exhaustive(A, B), (A, B)
    rng = np.random.default_rng(3)
    for _ in range(60):
        A, B = (bytes(rng.choice(list(b"ACGT"), int(rng.integers(0, 8))).astype(np.uint8)) for _ in range(2))
        assert gap_fill(A, B) == _exhaustive(A, B), (A, B)


def test_gap_rule_edits_are_levenshtein_and_closed_forms():
    rng = np.random.default_rng(4)
    for _ in range(200):
        A, B = (bytes(rng.choice(list(b"ACGT"), int(rng.integers(0, 40))).astype(np.uint8)) for _ in range(2))
        e, m = gap_fill(A, B)
        assert e == levenshtein(A, B) and m <= min(len(A), len(B)) and e + m >= max(len(A), len(B)), (A, B)
    for a in (0, 1, 2, 5, 16, 17, 40):
        S = bytes(rng.choice(list(b"ACGT"), a).astype(np.uint8))
        assert gap_fill(S, S) == (0, a)
        for b in (0, 1, 3, 16, 17, 33):
            assert gap_fill(b"A" * a, b"A" * b) == (abs(a - b), min(a, b))
            assert gap_fill(b"A" * a, b"C" * b) == (max(a, b), 0)


# ---- align_reference ---------------------------------------------------------------------------------------------------
def _recs(anchors):
    """MATCH_DTYPE records from (x, y, l) triples."""
    return np.array([(y, x, l) for x, y, l in anchors], dtype=MATCH_DTYPE)


@functools.lru_cache(maxsize=None)
def _memo(A, B):
    """The lexicographic optimum (edits, -matches) top down, with a memo: written apart from gap_fill's table."""
    if not A or not B:
        return len(A) + len(B), 0
    e, m = _memo(A[:-1], B[:-1])
    best = (e, m - 1) if A[-1] == B[-1] else (e + 1, m)
    for e, m in (_memo(A[:-1], B), _memo(A, B[:-1])):
        best = min(best, (e + 1, m))
    return best


def _second(R, T, anchors, pred, chain, max_fill):
    """One read's record and gaps by a FORWARD pass with two cursors: where the alignment stands in the read and in the
    text.  The next anchor loses the head that lies behind either cursor."""
    if chain["ref_start"] == np.uint64(UNCHAINED):
        return (UNALIGNED, 0, 0, 0, 0, 0, 0, 0, 0, NO_DOC), []
    path = [int(chain["last"])]
    while pred[path[-1]] != NO_PRED:
        path.append(int(pred[path[-1]]))
    path.reverse()
    x, y, l = anchors[path[0]]
    cr, ct, matches, edits, unfilled, skipped, gaps = x + l, y + l, l, 0, 0, 0, []
    for i in path[1:]:
        x, y, l = anchors[i]
        cut = max(0, cr - x, ct - y)
        a, b = x + cut - cr, y + cut - ct
        matches += l - cut
        if max(a, b) > max_fill:
            gaps.append((a, b, UNFILLED, 0))
            unfilled += 1
            skipped += max(a, b)
        else:
            e, m = _memo(R[cr:x + cut], T[ct:y + cut])
            gaps.append((a, b, e, -m))
            edits += e
            matches -= m
        cr, ct = x + l, y + l
    return (int(chain["ref_start"]), int(chain["ref_end"]), int(chain["read_start"]), int(chain["read_end"]), matches, edits, len(path),
            unfilled, min(skipped, 2**32 - 1), int(chain["doc"])), gaps


def _noisy_read(rng, text, h):
    """A read made of h stretches of the text with small edits between them, and its anchors (the stretches, some grown
    into their neighbours so that they overlap in the read or in the text)."""
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    y = int(rng.integers(0, 200))
    parts, anchors, x = [], [], 0
    for t in range(h):
        l = int(rng.integers(3, 30))
        parts.append(text[y:y + l])
        anchors.append([x, y, l])
        x += l
        y += l
        ins, dele = int(rng.integers(0, 6)), int(rng.integers(0, 6))
        parts.append(letters[rng.integers(0, 4, ins)])
        x += ins
        y += dele
    for t in range(1, h):  # overlaps: an anchor that starts early (its head is not a match: the rule cuts it off, whatever it says)
        if rng.random() < 0.3:
            back = int(rng.integers(1, 5))
            if anchors[t][0] >= back and anchors[t][1] >= back:
                anchors[t][0] -= back
                anchors[t][1] -= back + int(rng.integers(0, 2))
                anchors[t][2] += back
    return np.concatenate(parts), [tuple(a) for a in anchors]


@pytest.mark.parametrize("seed", range(3))
def test_reference_against_a_forward_pass(seed):
    rng = np.random.default_rng(seed)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 3000)]
    reads, all_anchors, counts = [], [], []
    for q in range(30):
        h = int(rng.integers(0, 12)) if q % 7 else 0
        rd, an = _noisy_read(rng, text, h) if h else (np.zeros(3, dtype=np.uint8), [])
        reads.append(rd)
        all_anchors.append(an)
        counts.append(len(an))
    front = seed  # match_offsets[0] != 0
    moffs = (front + np.r_[0, np.cumsum(counts)]).astype(np.uint64)
    roffs = np.r_[0, np.cumsum([r.size for r in reads])].astype(np.uint64)
    rec = _recs([(1, 1, 1)] * front + [a for an in all_anchors for a in an])
    R = np.concatenate(reads)
    chains, _, pred = chain_reference(moffs, rec, ChainParams(64, 5000, 500, 0))
    several = overlaps = 0
    for max_fill in (512, 4, 1):
        out, goffs, gaps = align_reference(R, roffs, text, moffs, rec, chains, pred, AlignParams(max_fill))
        assert out.dtype == ALIGN_DTYPE and gaps.dtype == GAP_DTYPE and goffs.dtype == np.uint64 and goffs.size == len(reads) + 1
        assert goffs.tolist() == np.r_[0, np.cumsum(np.maximum(chains["anchors"].astype(np.int64) - 1, 0))].tolist()
        for q in range(len(reads)):
            o, ro = int(moffs[q]), int(roffs[q])
            want, want_gaps = _second(bytes(R[ro:int(roffs[q + 1])]), bytes(text), all_anchors[q], pred[o:int(moffs[q + 1])], chains[q], max_fill)
            assert out[q].tolist() == want, (q, max_fill)
            assert gaps[int(goffs[q]):int(goffs[q + 1])].tolist() == want_gaps, (q, max_fill)
            several += want[6] > 2
            overlaps += any(0 in g[:2] for g in want_gaps)
    assert several > 10 and overlaps > 5


def _one(R, T, anchors, pred, first, last, max_fill=512, front=0):
    """One read, with `front` characters and records of another in front of it."""
    rec = _recs([(0, 0, 1)] * front + list(anchors))
    chain = np.zeros(1, dtype=CHAIN_DTYPE)
    n, i = 1, last
    while pred[i] != NO_PRED:
        i, n = pred[i], n + 1
    x0, y0, _ = anchors[first]
    x1, y1, l1 = anchors[last]
    chain[0] = (y0, y1 + l1, x0, x1 + l1, 0, n, first, last, 0, 7)
    out, goffs, gaps = align_reference(np.frombuffer(b"N" * front + R, dtype=np.uint8), [front, front + len(R)], np.frombuffer(T, dtype=np.uint8),
                                       [front, front + len(anchors)], rec, chain, np.array([NO_PRED] * front + list(pred), dtype=np.uint32),
                                       AlignParams(max_fill))
    assert goffs.tolist() == [0, n - 1]
    return out[0].tolist(), gaps.tolist()


def test_hand_computed_records():
    N = NO_PRED
    T = b"." * 100 + b"ACGTACGTAC" + b"GG" + b"TTTTTTTTTT" + b"ACT" + b"CCCCCCCCCC" + b"." * 20
    #                   100            110     112             122      125
    # one anchor
    assert _one(b"ACGTACGTAC", T, [(0, 100, 10)], [N], 0, 0) == ((100, 110, 0, 10, 10, 0, 1, 0, 0, 7), [])
    assert _one(b"ACGTACGTAC", T, [(0, 100, 10)], [N], 0, 0, front=3) == ((100, 110, 0, 10, 10, 0, 1, 0, 0, 7), [])
    # an overlap in the read: ex = 6 < l, ey = 8: keep 6, the text has two characters more (b = 2, a = 0)
    assert _one(b"x" * 16, T, [(0, 100, 10), (6, 108, 10)], [N, 0], 0, 1) == ((100, 118, 0, 16, 16, 2, 2, 0, 0, 7), [(0, 2, 2, 0)])
    # an overlap in the text: ex = 9, ey = 7: keep 7, the read has two characters more (a = 2, b = 0)
    assert _one(b"x" * 19, T, [(0, 100, 10), (9, 107, 10)], [N, 0], 0, 1) == ((100, 117, 0, 19, 17, 2, 2, 0, 0, 7), [(2, 0, 2, 0)])
    # a = 0 without an overlap (a deletion of GG), b = 0 without one (an insertion of AA)
    assert _one(b"ACGTACGTACTTTTTTTTTT", T, [(0, 100, 10), (10, 112, 10)], [N, 0], 0, 1) == \
        ((100, 122, 0, 20, 20, 2, 2, 0, 0, 7), [(0, 2, 2, 0)])
    assert _one(b"TTTTTTTTTTAACCCCCCCCCC", T, [(0, 112, 10), (12, 125, 10)], [N, 0], 0, 1, front=2) == \
        ((112, 135, 0, 22, 21, 2, 2, 0, 0, 7), [(2, 3, 2, 1)])  # AA against ACT: A = A, then a substitution and an insertion
    # a gap of 3 x 3 with one substitution: ACG against ACT
    assert _one(b"TTTTTTTTTTACGCCCCCCCCCC", T, [(0, 112, 10), (13, 125, 10)], [N, 0], 0, 1) == \
        ((112, 135, 0, 23, 22, 1, 2, 0, 0, 7), [(3, 3, 1, 2)])
    # ... exactly at max_fill it is filled, one above it is not
    assert _one(b"TTTTTTTTTTACGCCCCCCCCCC", T, [(0, 112, 10), (13, 125, 10)], [N, 0], 0, 1, max_fill=3)[1] == [(3, 3, 1, 2)]
    assert _one(b"TTTTTTTTTTACGCCCCCCCCCC", T, [(0, 112, 10), (13, 125, 10)], [N, 0], 0, 1, max_fill=2) == \
        ((112, 135, 0, 23, 20, 0, 2, 1, 3, 7), [(3, 3, UNFILLED, 0)])
    # three anchors, the middle one of another chain: pred skips it; the first gap is filled, the second is not (b = 3 > 2)
    three = [(0, 100, 10), (3, 50, 4), (10, 112, 10), (22, 125, 10)]
    assert _one(b"ACGTACGTACTTTTTTTTTTAACCCCCCCCCC", T, three, [N, N, 0, 2], 0, 3, max_fill=2) == \
        ((100, 135, 0, 32, 30, 2, 3, 1, 3, 7), [(0, 2, 2, 0), (2, 3, UNFILLED, 0)])
    # the saturating sum: two gaps of 2^31 + 5 text characters each
    far = 2**31 + 5
    wide = [(0, 100, 10), (10, 110 + far, 10), (20, 120 + 2 * far, 10)]
    got, gaps = _one(b"x" * 30, T, wide, [N, 0, 1], 0, 2)
    assert got == (100, 130 + 2 * far, 0, 30, 30, 0, 3, 2, 2**32 - 1, 7) and gaps == [(0, far, UNFILLED, 0)] * 2
    # no reads; a read without a chain
    empty = np.zeros(0, dtype=CHAIN_DTYPE)
    out, goffs, gaps = align_reference(np.zeros(0, dtype=np.uint8), [0], np.zeros(0, dtype=np.uint8), [0], _recs([]), empty, [])
    assert out.size == 0 and goffs.tolist() == [0] and gaps.size == 0 and gaps.dtype == GAP_DTYPE
    chains, _, pred = chain_reference([0, 0], _recs([]))
    out, goffs, gaps = align_reference(np.zeros(0, dtype=np.uint8), [0, 0], np.zeros(0, dtype=np.uint8), [0, 0], _recs([]), chains, pred)
    assert out[0].tolist() == (UNALIGNED, 0, 0, 0, 0, 0, 0, 0, 0, NO_DOC) and goffs.tolist() == [0, 0]
    for bad in ((0,), (4097,), (-1,)):
        with pytest.raises(ValueError, match="max_fill must be 1 .. 4096"):
            check_params(bad)
    assert check_params(None) == (512,) and check_params((1,)) == (1,) and check_params((4096,)) == (4096,)


# ---- the planted cases -------------------------------------------------------------------------------------------------
def _lev_rows(A, B):
    """Levenshtein of two uint8 arrays a row at a time (the running minimum along a row as a prefix minimum)."""
    idx = np.arange(B.size + 1)
    prev = idx.copy()
    for i in range(A.size):
        best = np.minimum(prev[1:] + 1, prev[:-1] + (B != A[i]))
        row = np.r_[i + 1, best]
        prev = np.minimum.accumulate(row - idx) + idx
    return int(prev[-1])


def clustered_reads():
    """The second planted case: (text, seqs, offs).  12 reads cut from about 400 text characters with two CLUSTERS of edits
    whose stretches between the edits are shorter than min_length 12, so that no anchor lies inside a cluster: from 100 on
    a substitution every 5 characters over 40 characters with 3 characters deleted in their middle, and from 250 on
    substitutions at 0, 6, 11 and 17."""
    rng = np.random.default_rng(2026)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    text = letters[rng.integers(0, 4, 20_000)]
    cuts = rng.integers(0, text.size - 400, 12)
    reads = []
    for c in cuts:
        rd = text[c:c + 400].copy()
        for at in list(range(100, 141, 5)) + [250, 256, 261, 267]:
            rd[at] = letters[(int(np.flatnonzero(letters == rd[at])[0]) + 1 + int(rng.integers(0, 3))) % 4]
        reads.append(np.r_[rd[:118], rd[121:]])
    return text, np.concatenate(reads), np.r_[0, np.cumsum([r.size for r in reads])].astype(np.uint64)


def _planted(oracle_mod, text, seqs, offs):
    raw = synth.index_from_text(torch.from_numpy(text))
    w = oracle_mod.OracleIndex.from_raw(raw).ms(seqs, offs, text=text)
    mo, rec = mems_reference(w["lengths"], w["pointers"], offs, 12)
    chains, _, pred = chain_reference(mo, rec)
    return mo, rec, chains, align_reference(seqs, offs, text, mo, rec, chains, pred)


def test_planted_reads_align_over_their_indels(oracle_mod):
    """tests/test_chain_cpu.py's planted reads: two substitutions (1 x 1), three characters deleted (0 x 3) and two inserted
    (2 x 0): 7 edits, and every other character of the 302 a match but the two substituted and the two inserted ones."""
    text, seqs, offs, cuts = planted_reads()
    mo, rec, chains, (out, goffs, gaps) = _planted(oracle_mod, text, seqs, offs)
    for q, c in enumerate(cuts):
        got = out[q]
        assert (int(got["edits"]), int(got["matches"]), int(got["unfilled"])) == (7, 298, 0), (q, got)
        assert (int(got["read_start"]), int(got["read_end"]), int(got["ref_start"]), int(got["ref_end"])) == (0, 302, int(c), int(c) + 303)
        assert [g[:2] for g in gaps[int(goffs[q]):int(goffs[q + 1])].tolist()] == [(1, 1), (0, 3), (1, 1), (2, 0)], q


def test_clustered_reads_fill_gaps_that_need_a_table(oracle_mod):
    text, seqs, offs = clustered_reads()
    mo, rec, chains, (out, goffs, gaps) = _planted(oracle_mod, text, seqs, offs)
    # the preconditions, on the reference's own output
    assert ((gaps["a"] >= 8) & (gaps["b"] >= 8) & (gaps["a"] != gaps["b"])).any(), gaps
    assert (gaps["matches"] > 0).any() and (out["unfilled"] == 0).all() and (out["anchors"] >= 3).all(), out
    for q in range(offs.size - 1):
        r = out[q]
        A = seqs[int(offs[q]) + int(r["read_start"]):int(offs[q]) + int(r["read_end"])]
        B = text[int(r["ref_start"]):int(r["ref_end"])]
        assert A.size >= 380, (q, r)  # (the chain crosses both clusters)
        lev = _lev_rows(A, B)
        assert int(r["edits"]) >= lev, (q, r, lev)  # a chain-constrained alignment is an alignment
        assert int(r["matches"]) + int(r["edits"]) >= max(A.size, B.size), (q, r)
    rng = np.random.default_rng(5)
    for _ in range(20):  # the row-wise helper is the textbook table
        A, B = (rng.integers(0, 3, int(rng.integers(0, 50))).astype(np.uint8) for _ in range(2))
        assert _lev_rows(A, B) == levenshtein(bytes(A), bytes(B))


# ---- header and command ------------------------------------------------------------------------------------------------
def _declared():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return code, sorted(set(re.findall(r"\b(spa_[a-z_0-9]+)\s*\(", code)))


def test_align_header_is_plain_c(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include "spumoni_align.h"\nint main(void) { spa_alignment c; spa_gap g; spa_params p; spa_align_stats s; (void)c; (void)g; '
                   '(void)p; (void)s; return sizeof(spa_alignment) == 48 && sizeof(spa_gap) == 16 && sizeof(spa_params) == 4 && '
                   'SPA_UNALIGNED + 1 == 0 && SPA_UNFILLED == 4294967295u ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "c"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "c")]).returncode == 0
    code, _ = _declared()
    assert "hipStream_t" not in code and "std::" not in code and "#include <hip" not in code
    assert re.findall(r'#include\s+[<"]([^>"]+)', code) == ["stdint.h", "spumoni_chain.h"]


def test_align_header_symbols_exported(built):
    _, names = _declared()
    assert names == sorted(capi.ALIGN_EXPORTS) and len(names) == 3
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(spa_[a-z_0-9]+)\b", out))) == names
    for other in (capi.EXPORTS, capi.DOCVOTE_EXPORTS, capi.MEMS_EXPORTS, capi.PLACE_EXPORTS, capi.CHAIN_EXPORTS, capi.REFTEXT_EXPORTS):
        assert not set(capi.ALIGN_EXPORTS) & set(other)
    assert np.dtype(ALIGN_DTYPE).itemsize == 48 and np.dtype(GAP_DTYPE).itemsize == 16
    assert ALIGN_DTYPE.names == ("ref_start", "ref_end", "read_start", "read_end", "matches", "edits", "anchors", "unfilled", "skipped", "doc")
    assert GAP_DTYPE.names == ("a", "b", "edits", "matches")
    assert [f[0] for f in capi.SpaParams._fields_] == list(AlignParams._fields) and AlignParams() == (512,)
    assert capi.C.sizeof(capi.SpaAlignStats) == 72


def test_align_batch_without_device_fails_loudly(built):
    if built.spx_device_count() > 0:
        pytest.skip("a device is visible: the no-device path is this machine's CPU tier")
    L = capi._spa()
    seqs, offs = np.frombuffer(b"ACGT", dtype=np.uint8), np.array([0, 4], dtype=np.uint64)
    out = np.zeros(1, dtype=ALIGN_DTYPE)
    rc = L.spa_align_batch(None, 0, 0, 0, seqs.ctypes.data, offs.ctypes.data, 1, 1, 0, capi.SpcParams(64, 5000, 500, 1), capi.SpaParams(512),
                           out.ctypes.data, None, None)
    assert rc == -3 and b"no CPU fallback" in L.spx_last_error()


def _align(args, cwd, env=None):
    return subprocess.run([BIN, "align"] + args, cwd=cwd, capture_output=True, text=True, env=env, timeout=120)


def test_usage_without_arguments(built, tmp_path):
    r = _align([], str(tmp_path))
    assert r.returncode == 1
    assert "spumoni align - " in r.stderr
    for opt in ("-h, --help", "-r, --ref", "-p, --pattern", "-n, --no-digest", "-m, --minimizer-alphabet", "-a, --dna-minimizer",
                "-K, --small-window", "-W, --large-window", "-d, --doc-array", "-L, --min-length", "-S, --max-dist", "-G, --max-gap",
                "-B, --gap-penalty", "-H, --lookback", "-F, --max-fill"):
        assert opt in r.stderr, opt
    for limits in ("1 or more", "1 .. 2147483647", "0 .. 2147483647", "0 .. 65535", "1 .. 64", "1 .. 4096"):  # the ranges are stated
        assert limits in r.stderr, limits
    assert "-P, --PML" not in r.stderr and "<pattern>.alignments" in r.stderr
    top = subprocess.run([BIN], capture_output=True, text=True)
    assert top.returncode == 1
    for cmd in ("align", "chain", "place", "mems", "assign", "run", "build"):
        assert f"\t{cmd}\t" in top.stderr, cmd


def _index(tmp_path, doc=True):
    for f in os.listdir(GOLDEN):
        if os.path.isfile(os.path.join(GOLDEN, f)) and (doc or not f.endswith(".doc")):
            shutil.copy(os.path.join(GOLDEN, f), tmp_path / f)
            if f.startswith("ref.fa"):  # the same files under the name -m looks for
                shutil.copy(os.path.join(GOLDEN, f), tmp_path / ("ref.bin" + f[len("ref.fa"):]))


@pytest.mark.parametrize("args,message", [
    (["-p", "reads.fa", "-n"], "Both a reference file (-r) and pattern file (-p) must be provided."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-P"], "-P cannot be used with `spumoni align`"),
    (["-r", "ref", "-p", "reads.fa", "-n", "-M", "-P"], "-P cannot be used with `spumoni align`"),
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
    r = _align(args, str(tmp_path))
    assert r.returncode == 1
    assert message in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_doc_ids_without_doc_file_are_refused(built, tmp_path):
    _index(tmp_path, doc=False)
    before = sorted(os.listdir(tmp_path))
    r = _align(["-r", "ref", "-p", "reads.fa", "-n", "-d"], str(tmp_path))
    assert r.returncode == 1
    assert "document array file (ref.fa.doc) is not present, so it cannot be used." in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_missing_entry_point_on_the_fake_device(built, fake_device, tmp_path):
    _index(tmp_path)
    before = sorted(os.listdir(tmp_path))
    env = dict(os.environ, LD_LIBRARY_PATH=fake_device + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = _align(["-r", "ref", "-p", "reads.fa", "-n", "-L", "4"], str(tmp_path), env=env)
    assert r.returncode == 1
    assert "has no spa_align_batch" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_no_device_fails_loudly_and_writes_nothing(built, tmp_path):
    if built.spx_device_count() > 0:
        pytest.skip("a device is visible: the no-device path is this machine's CPU tier")
    _index(tmp_path)
    before = sorted(os.listdir(tmp_path))
    r = _align(["-r", "ref", "-p", "reads.fa", "-n", "-d"], str(tmp_path))
    assert r.returncode == 1
    assert "no usable gfx950 device" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before
