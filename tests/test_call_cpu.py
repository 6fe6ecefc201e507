"""The pileup's rule and the calls (spumoni_amd/call.py) against an independent per-column restatement, the hand cases, the
checks and the thresholds' edges; the header as C99 and the exports; `spumoni call`'s usage and refusals.  No GPU."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from spumoni_amd import capi
from spumoni_amd.call import CALL_DTYPE, calls_reference, check_read, code_of, del_of, oriented_codes, pileup_reference, zeros
from spumoni_amd.cigar import OP_D, OP_EQ, OP_I, OP_N, OP_X
from spumoni_amd.cover import seq_starts
from spumoni_amd.extend import OP_S
from spumoni_amd.map import MAPPING_DTYPE
from tests.test_cover_cpu import BAD, BAD_LENGTHS, mapping, mbatch, pack, spoiled
from tests.test_map_cpu import _golden_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
HEADER = os.path.join(ROOT, "include", "spumoni_call.h")
TEXT_OPS = (OP_EQ, OP_X, OP_D, OP_N)
READ_OPS = (OP_EQ, OP_X, OP_I, OP_S)
ALPHABET = np.frombuffer(b"ACGTNacgt", dtype=np.uint8)
COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


@pytest.fixture(scope="module")
def built(built_all):
    return capi.lib()


def read_length(entries):
    return sum(e >> 4 for e in entries if e & 15 in READ_OPS)


def rbatch(mappings, reads):
    """(records, op_offsets, entries, read bytes, read offsets) of [(rec, entries) or None] and their reads (bytes)."""
    roffs = np.r_[0, np.cumsum([len(r) for r in reads])].astype(np.uint64)
    return mbatch(mappings) + (np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), roffs)


def restated(entries, read, strand):
    """What one read adds over its span, counted column by column from (text position, op, oriented letter): (alt[span][4],
    other[span], ins[span], del[span], x columns, 'I' entries, 'D' entries), or None when an 'I' column is the last one
    that is not a clip.  The oriented read is made with bytes.translate and a slice, not with codes."""
    oriented = read.translate(COMPLEMENT)[::-1] if strand else read
    cols, t, j = [], 0, 0
    for e in entries:
        for _ in range(e >> 4):
            op = e & 15
            if op != OP_S:
                cols.append((t, op, chr(oriented[j]) if op in READ_OPS else None))
                t += op in TEXT_OPS
            j += op in READ_OPS
    assert j == len(read)
    if cols and cols[-1][1] == OP_I:
        return None
    alt, other, ins, dele = [[0] * 4 for _ in range(t)], [0] * t, [0] * t, [0] * t
    n_ins = n_del = 0
    for i, (at, op, letter) in enumerate(cols):
        before = cols[i - 1][1] if i else None
        if op == OP_X:
            k = "ACGT".find(letter.upper())
            if k >= 0:
                alt[at][k] += 1
            else:
                other[at] += 1
        elif op == OP_I and before != OP_I:  # (a packed CIGAR has no two 'I' entries side by side)
            ins[at] += 1
            n_ins += 1
        elif op == OP_D:
            dele[at] += 1
            n_del += before != OP_D
    return alt, other, ins, dele, sum(op == OP_X for _, op, _ in cols), n_ins, n_del


def _cigars():
    """Every CIGAR of up to 5 columns over = X I D N, run-length packed, each with one of the four clip shapes in turn, a
    read drawn from ACGTNacgt and a strand; with its restatement."""
    rng = np.random.default_rng(2024)
    out = []
    for k in range(1, 6):
        for i, cols in enumerate(itertools.product((OP_EQ, OP_X, OP_I, OP_D, OP_N), repeat=k)):
            lead, tail = ([], [2 << 4 | OP_S], [], [1 << 4 | OP_S])[i % 4], ([], [], [3 << 4 | OP_S], [1 << 4 | OP_S])[i % 4]
            ents = lead + pack(cols) + tail
            read = ALPHABET[rng.integers(0, ALPHABET.size, read_length(ents))].tobytes()
            strand = (i // 4 + k) % 2
            out.append((ents, read, strand, restated(ents, read, strand), sum(c in TEXT_OPS for c in cols)))
    return out


def _arrays(state, G):
    alt, other, ins, ddiff = state
    return alt.reshape(G, 4).astype(np.int64), other.astype(np.int64), ins.astype(np.int64), del_of(ddiff).astype(np.int64)


def test_rule_against_the_restatement_over_every_cigar_up_to_5_columns():
    """Every CIGAR on both strands at every place of a sequence of 1-4 bases, read by read; then every table of 1-3 such
    sequences with all its reads in one batch against the summed restatements."""
    cigars = _cigars()
    assert len(cigars) == sum(5 ** k for k in range(1, 6))
    by_len = {t: [c for c in cigars if c[4] == t] for t in range(6)}
    reads = skipped = 0
    for L in range(1, 5):
        for t in range(0, L + 1):
            for a in range(0, L - t + 1):
                for ents, read, strand, _, _ in by_len[t]:
                    for st in (strand, 1 - strand):
                        want = restated(ents, read, st)
                        count = {}
                        state = pileup_reference(*rbatch([mapping(ents, 0, a, strand=st)], [read]), [L], count=count)
                        alt, other, ins, dele = _arrays(state, L)
                        if want is None:
                            assert not any(x.any() for x in state) and (count["skipped"], count["error"], count["added"]) == (1, 1, 0)
                            skipped += 1
                            continue
                        w = [np.zeros((L, 4), dtype=np.int64), np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64)]
                        for arr, part in zip(w, want[:4]):
                            arr[a:a + t] = part
                        assert all(np.array_equal(g, x) for g, x in zip((alt, other, ins, dele), w)), (L, a, ents, read, st)
                        assert (count["added"], count["error"], count["x_columns"], count["insertions"], count["deletions"]) == \
                            (1, 0, want[4], want[5], want[6])
                        assert count["other_columns"] == sum(want[1]) and count["atomics"] == want[4] + want[5] + 2 * want[6]
                        assert int(state[3].astype(np.uint64).sum()) % 2**32 == 0
                        reads += 1
        # a read that does not fit the sequence is skipped
        for ents, read, strand, _, _ in by_len[L + 1][:40]:
            count = {}
            state = pileup_reference(*rbatch([mapping(ents, 0, 0, strand=strand)], [read]), [L], count=count)
            assert not any(x.any() for x in state) and (count["skipped"], count["error"]) == (1, 1)
    assert reads > 8_000 and skipped > 1_000, (reads, skipped)
    tables = [T for n in (1, 2, 3) for T in itertools.product(range(1, 5), repeat=n)]
    assert len(tables) == 84
    total = 0
    for T in tables:
        F = seq_starts(T)
        G = F[-1]
        w = [np.zeros((G, 4), dtype=np.int64), np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.int64)]
        maps, rds, n_bad = [], [], 0
        for s, L in enumerate(T):
            for t in range(0, L + 1):
                for a in range(0, L - t + 1):
                    for ents, read, strand, want, _ in by_len[t][(s + a) % 3::3]:
                        maps.append(mapping(ents, s, a, strand=strand))
                        rds.append(read)
                        if want is None:
                            n_bad += 1
                            continue
                        for arr, part in zip(w, want[:4]):
                            arr[F[s] + a:F[s] + a + t] += np.array(part, dtype=np.int64).reshape((t,) + arr.shape[1:])
        count = {}
        state = pileup_reference(*rbatch(maps, rds), T, count=count)
        assert all(np.array_equal(g, x) for g, x in zip(_arrays(state, G), w)), T
        assert (count["added"], count["skipped"], count["error"]) == (len(maps) - n_bad, n_bad, int(n_bad > 0))
        total += len(maps)
    assert total > 30_000, total


def _one(cigar, read, seq, start, lengths, strand=0):
    count = {}
    state = pileup_reference(*rbatch([mapping(cigar, seq, start, strand=strand)], [read]), lengths, count=count)
    alt, other, ins, dele = _arrays(state, sum(lengths))
    return alt.tolist(), other.tolist(), ins.tolist(), dele.tolist(), count, state[3].tolist()


def test_the_hand_cases_on_both_strands():
    # forward: the read's own letter at the column's base
    alt, other, ins, dele, count, _ = _one("2=1X", b"AAC", 1, 0, [2, 3])
    assert alt == [[0] * 4, [0] * 4, [0] * 4, [0] * 4, [0, 1, 0, 0]] and not any(other) and count["atomics"] == 1
    # reverse: the read as given is the reverse complement of what lies on the forward strand.  Read AAC maps on strand 1;
    # along the forward strand it reads GTT, so the 'X' column at the third base carries T (the complement of the read's
    # first byte A), and lands at the forward position start + 2
    alt, other, ins, dele, count, _ = _one("2=1X", b"AAC", 1, 0, [2, 3], strand=1)
    assert alt == [[0] * 4, [0] * 4, [0] * 4, [0] * 4, [0, 0, 0, 1]]
    alt, _, _, _, _, _ = _one("1X2=", b"AAC", 1, 0, [2, 3], strand=1)
    assert alt == [[0] * 4, [0] * 4, [0, 0, 1, 0], [0] * 4, [0] * 4]  # (the read's last byte C, complemented: G)
    # clips are walked on the oriented read: read ttACGn, strand 1, oriented nCGTaa; 1S skips n, the 'X' column carries G
    alt, other, _, _, _, _ = _one("1S1=1X1=2S", b"ttACGn", 0, 1, [4], strand=1)
    assert alt == [[0] * 4, [0] * 4, [0, 0, 1, 0], [0] * 4] and not any(other)
    # a byte outside ACGT goes to `other` on either strand, lower case counts as upper
    alt, other, _, _, count, _ = _one("3X", b"aNg", 0, 0, [3])
    assert alt == [[1, 0, 0, 0], [0] * 4, [0, 0, 1, 0]] and other == [0, 1, 0] and (count["x_columns"], count["other_columns"]) == (3, 1)
    alt, other, _, _, _, _ = _one("3X", b"aNg", 0, 0, [3], strand=1)
    assert alt == [[0, 1, 0, 0], [0] * 4, [0, 0, 0, 1]] and other == [0, 1, 0]
    # an 'I' before the last column counts at the next text position, on both strands at the same forward base
    for strand in (0, 1):
        _, _, ins, _, count, _ = _one("2=2I1=", b"ACGTA", 0, 1, [5], strand=strand)
        assert ins == [0, 0, 0, 1, 0] and (count["insertions"], count["atomics"]) == (1, 1)
    # ... and at the sequence's last base, which is the genome's last
    _, _, ins, _, _, _ = _one("1I1=", b"AC", 1, 2, [2, 3])
    assert ins == [0, 0, 0, 0, 1]
    # a 'D' is one +1 and one -1, the -1 at G when the deletion ends the genome's last-but-one column
    _, _, _, dele, count, ddiff = _one("1=2D1=", b"AC", 0, 0, [4])
    assert dele == [0, 1, 1, 0] and ddiff == [0, 1, 0, 0xFFFFFFFF, 0] and (count["deletions"], count["atomics"]) == (1, 2)
    _, _, _, dele, _, ddiff = _one("1=1D", b"A", 0, 2, [4])
    assert dele == [0, 0, 0, 1] and ddiff == [0, 0, 0, 1, 0xFFFFFFFF]
    # 'N' moves the text position and counts nothing
    alt, _, _, dele, _, _ = _one("1=2N1X", b"AT", 0, 0, [4])
    assert alt[3] == [0, 0, 0, 1] and not any(dele)
    # an unmapped read and an empty batch add nothing
    count = {}
    state = pileup_reference(*rbatch([None, None], [b"ACG", b""]), [3], count=count)
    assert not any(x.any() for x in state) and (count["reads"], count["mapped"], count["error"]) == (2, 0, 0)
    state = pileup_reference(*rbatch([], []), [3])
    assert [x.shape for x in state] == [(12,), (3,), (3,), (4,)] and all(x.dtype == np.uint32 for x in state)
    assert [x.shape for x in zeros(3)] == [(12,), (3,), (3,), (4,)]
    assert [code_of(b) for b in b"AaCcGgTtNn-\x00\xff"] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 4, 4, 4]
    assert oriented_codes(np.frombuffer(b"ACNt", dtype=np.uint8), 1).tolist() == [0, 4, 2, 3]


def test_adds_accumulate_in_any_order():
    rng = np.random.default_rng(1)
    lengths = [7, 1, 12]
    maps, reads = [], []
    for _ in range(80):
        s = int(rng.integers(0, 3))
        t = int(rng.integers(1, lengths[s] + 1))
        ents = pack([int(v) for v in rng.choice([OP_EQ, OP_X, OP_D], t)])
        maps.append(mapping(ents, s, int(rng.integers(0, lengths[s] - t + 1)), strand=int(rng.integers(0, 2))))
        reads.append(ALPHABET[rng.integers(0, ALPHABET.size, read_length(ents))].tobytes())
    whole = pileup_reference(*rbatch(maps, reads), lengths)
    first = pileup_reference(*rbatch(maps[:30], reads[:30]), lengths)
    kept = [a.copy() for a in first]
    both = pileup_reference(*rbatch(maps[30:], reads[30:]), lengths, into=first)
    assert all(np.array_equal(a, b) for a, b in zip(first, kept))  # `into` is left as it is
    other = pileup_reference(*rbatch(maps[:30], reads[:30]), lengths, into=pileup_reference(*rbatch(maps[30:][::-1], reads[30:][::-1]), lengths))
    for a, b, c in zip(whole, both, other):
        assert a.dtype == np.uint32 and a.tobytes() == b.tobytes() == c.tobytes()
    assert whole[0].any() and whole[3].any()


GOOD_READS = [b"ACGT", b"ACG", b"T"]  # of test_cover_cpu.spoiled's three good reads
CALL_BAD = BAD + ["read_too_short", "read_too_long", "read_offsets_decrease", "read_offsets_beyond_in_chars", "insertion_behind_the_last_column"]


def spoiled_call(kind):
    """(a batch of three good reads and a bad one behind them, the same batch with the bad one unmapped, in_entries,
    in_chars): the coverage's bad reads, and the pileup's own."""
    if kind in BAD:
        args, clean, in_entries = spoiled(kind)
        n = read_length(args[2][int(args[1][3]):int(args[1][4])].tolist()) if args[1][4] >= args[1][3] else 5
        reads = GOOD_READS + [b"ACGTA"[:n] + b"A" * max(0, n - 5)]
        roffs = np.r_[0, np.cumsum([len(r) for r in reads])].astype(np.uint64)
        rd = np.frombuffer(b"".join(reads), dtype=np.uint8).copy()
        return tuple(args) + (rd, roffs), tuple(clean) + (rd, roffs), in_entries, rd.size
    rec, ents = mapping("2=1I2=", 1, 0)
    read = b"ACGTA"
    if kind == "read_too_short":
        read = b"ACGT"
    elif kind == "read_too_long":
        read = b"ACGTAC"
    elif kind == "insertion_behind_the_last_column":
        rec, ents = mapping("4=1I", 1, 0)
    elif kind not in ("read_offsets_decrease", "read_offsets_beyond_in_chars"):
        raise ValueError(kind)
    good = [mapping("3=1X", 0, 1), mapping("2=2D1=", 1, 0), mapping("1X", 1, 4)]
    args = list(rbatch(good + [(rec, ents)], GOOD_READS + [read]))
    clean = rbatch(good + [None], GOOD_READS + [read])
    in_chars = args[3].size
    if kind == "read_offsets_decrease":
        args[4][4] = args[4][3] - 1
    if kind == "read_offsets_beyond_in_chars":
        in_chars -= 1
    return tuple(args), clean, args[2].size, in_chars


@pytest.mark.parametrize("kind", CALL_BAD)
def test_each_check_failing_alone_skips_the_read_and_changes_nothing(kind):
    args, clean, in_entries, in_chars = spoiled_call(kind)
    count, count_clean = {}, {}
    got = pileup_reference(*args, BAD_LENGTHS, count=count, in_entries=in_entries, in_chars=in_chars)
    want = pileup_reference(*clean, BAD_LENGTHS, count=count_clean)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), kind
    assert (count["error"], count["skipped"], count["added"], count["mapped"]) == (1, 1, 3, 4)
    assert (count_clean["error"], count_clean["skipped"], count_clean["added"], count_clean["mapped"]) == (0, 0, 3, 3)
    # the good version of the same read does add: the check is what skipped it
    fine = pileup_reference(*rbatch([mapping("3=1X", 0, 1), mapping("2=2D1=", 1, 0), mapping("1X", 1, 4), mapping("2=1I2=", 1, 0)],
                                    GOOD_READS + [b"ACGTA"]), BAD_LENGTHS)
    assert fine[2].tobytes() != want[2].tobytes() and want[0].any() and want[3].any()
    rec, ents = mapping("2=1I2=", 1, 0)
    assert check_read(rec, ents, 5, seq_starts(BAD_LENGTHS)) is not None and check_read(rec, ents, 4, seq_starts(BAD_LENGTHS)) is None


def _calls(depth, alt, text, lengths, strands=1, other=None, ins=None, dele=None, **kw):
    G = len(depth)
    z = np.zeros(G, dtype=np.uint32)
    return calls_reference(depth, z, np.array(alt, dtype=np.uint32).reshape(-1), z if other is None else other, z if ins is None else ins,
                           z if dele is None else dele, np.frombuffer(text, dtype=np.uint8), lengths, strands, **kw)


def test_calls_at_the_edges_of_the_thresholds():
    # count equal to min_alt and one below
    alt = [[0, 3, 0, 0], [0, 2, 0, 0]]
    out = _calls([4, 4], alt, b"AA", [2], min_depth=1, min_alt=3, min_permille=0)
    assert out.dtype == CALL_DTYPE and [(int(c["pos"]), int(c["allele"])) for c in out] == [(0, 1)]
    assert [out[0][f].tolist() for f in CALL_DTYPE.names] == [0, 0, 4, [0, 3, 0, 0], 0, 0, 0, ord("A"), 1, 0]
    # count * 1000 equal to min_permille * depth and one below: 3 of 8 is 375 thousandths
    for permille, n in ((375, 1), (376, 0), (374, 1)):
        assert _calls([8], [[0, 0, 3, 0]], b"T", [1], min_depth=1, min_alt=1, min_permille=permille).size == n
    # 64-bit products: a count and a depth near 2^32
    assert _calls([0xFFFFFFFF], [[0, 0xFFFFFFFF, 0, 0]], b"A", [1], min_permille=1000).size == 1
    assert _calls([0xFFFFFFFF], [[0, 0xFFFFFFFE, 0, 0]], b"A", [1], min_permille=1000).size == 0
    # depth equal to min_depth and one below
    assert _calls([5], [[0, 5, 0, 0]], b"A", [1], min_depth=5).size == 1 and _calls([4], [[0, 5, 0, 0]], b"A", [1], min_depth=5).size == 0
    # a tie between two alleles: the lowest code; a larger count wins over a lower code
    assert int(_calls([9], [[0, 0, 4, 4]], b"A", [1], min_permille=0)[0]["allele"]) == 2
    assert int(_calls([9], [[0, 3, 4, 5]], b"A", [1], min_permille=0)[0]["allele"]) == 3
    # an alt count on the reference's own code is ignored, in either case of the text's letter
    assert _calls([9], [[0, 0, 9, 0]], b"G", [1]).size == 0 and _calls([9], [[0, 0, 9, 0]], b"g", [1]).size == 0
    assert int(_calls([9], [[2, 0, 9, 0]], b"G", [1], min_permille=0)[0]["allele"]) == 0
    # ref not in ACGT: all four are candidates
    out = _calls([9], [[5, 0, 0, 0]], b"N", [1])
    assert (int(out[0]["allele"]), int(out[0]["ref"])) == (0, ord("N"))
    # min_permille 0 and 1000
    assert _calls([1000], [[0, 2, 0, 0]], b"A", [1], min_permille=0).size == 1 and _calls([1000], [[0, 999, 0, 0]], b"A", [1], min_permille=1000).size == 0
    assert _calls([1000], [[0, 1000, 0, 0]], b"A", [1], min_permille=1000).size == 1
    # parameters outside their ranges
    for kw in (dict(min_depth=0), dict(min_alt=0), dict(min_permille=1001)):
        with pytest.raises(ValueError):
            _calls([1], [[0, 0, 0, 0]], b"A", [1], **kw)
    # the last base of one sequence and the first of the next are judged apart, each by its own reference letter; the
    # record carries the position in its sequence, the text is read at the forward piece (strands = 2: pieces alternate)
    alt = [[0] * 4, [0, 0, 0, 6], [0, 0, 0, 6], [0] * 4, [7, 0, 0, 0]]
    text = b"ACGT" + b"CTA" + b"TAG"  # sequence 0 = AC (GT its reverse piece), sequence 1 = CTA (TAG its reverse piece)
    out = _calls([6, 6, 6, 6, 7], alt, text, [2, 3], strands=2, other=np.arange(5, dtype=np.uint32), ins=np.arange(5, dtype=np.uint32) * 2,
                 dele=np.arange(5, dtype=np.uint32) * 3)
    assert [(int(c["seq"]), int(c["pos"]), chr(c["ref"]), int(c["allele"])) for c in out] == [(0, 1, "C", 3), (1, 0, "C", 3)]  # (A at (1, 2) is the reference's own)
    assert [(int(c["other"]), int(c["ins"]), int(c["del"])) for c in out] == [(1, 2, 3), (2, 4, 6)]
    one = _calls([6, 6, 6, 6, 7], alt, b"AC" + b"CTA", [2, 3], strands=1)
    assert [(int(c["seq"]), int(c["pos"])) for c in one] == [(0, 1), (1, 0)]


# ---- header and exports ------------------------------------------------------------------------------------------------
def _declared():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return code, sorted(set(re.findall(r"\b(spl_[a-z_0-9]+)\s*\(", code)))


def test_call_header_is_plain_c(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include <stddef.h>\n#include "spumoni_call.h"\nint main(void) { spl_call c; spl_call_stats s; (void)c; (void)s; '
                   'return sizeof(spl_call) == 48 && sizeof(spl_call_stats) == 104 && offsetof(spl_call, alt) == 16 && '
                   'offsetof(spl_call, ref) == 44 && sizeof(spd_run) == 32 && sizeof(spn_mapping) == 48 ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "c"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "c")]).returncode == 0
    code, _ = _declared()
    assert "hipStream_t" not in code and "std::" not in code and "#include <hip" not in code and "spx_" not in code.replace("spx_index", "")
    assert re.findall(r'#include\s+[<"]([^>"]+)', code) == ["stdint.h", "spumoni_cover.h"]


def test_call_header_symbols_exported(built):
    _, names = _declared()
    assert names == sorted(capi.CALL_EXPORTS) and len(names) == 9
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(spl_[a-z_0-9]+)\b", out))) == names
    for other in (capi.EXPORTS, capi.DOCVOTE_EXPORTS, capi.MEMS_EXPORTS, capi.PLACE_EXPORTS, capi.CHAIN_EXPORTS, capi.ALIGN_EXPORTS,
                  capi.CIGAR_EXPORTS, capi.EXTEND_EXPORTS, capi.REFTEXT_EXPORTS, capi.MAP_EXPORTS, capi.COVER_EXPORTS):
        assert not set(capi.CALL_EXPORTS) & set(other)
    assert capi.C.sizeof(capi.SplCallStats) == 104 and CALL_DTYPE.itemsize == 48
    assert list(CALL_DTYPE.names) == ["pos", "seq", "depth", "alt", "other", "del", "ins", "ref", "allele", "reserved"]
    assert [CALL_DTYPE.fields[n][1] for n in CALL_DTYPE.names] == [0, 8, 12, 16, 32, 36, 40, 44, 45, 46]
    assert [f[0] for f in capi.SplCallStats._fields_] == ["reads", "mapped", "added", "skipped", "x_columns", "other_columns", "insertions",
                                                          "deletions", "atomics", "calls", "error", "overflow", "step_ms", "reserved"]
    for method in ("pileup_add_device", "pileup_finish_device", "calls_device", "call_reset", "call_add_host", "calls", "pileup_counts",
                   "call_stats"):
        assert callable(getattr(capi.Index, method))


def test_call_entry_points_without_an_index_fail_loudly(built):
    L = capi._spl()
    n = capi.C.c_uint64(0)
    assert L.spl_call_reset(None) == -1 and b"index must be non-null" in L.spx_last_error()
    assert L.spl_call_add_batch(None, 0, 0, 0, None, None, 0, 1, 0, None, None, None, None) == -1
    assert b"index must be non-null" in L.spx_last_error()
    assert L.spl_pileup_add_device(None, None, None, None, 0, None, None, 0, 0, None, None, None, None, None) == -1
    assert L.spl_pileup_finish_device(None, None, None, None) == -1
    assert L.spl_calls_device(None, None, None, None, None, None, None, 1, 1, 0, 0, None, None, None) == -1
    assert L.spl_calls_begin(None, 1, 1, 0, capi.C.byref(n)) == -1 and L.spl_calls_fetch(None, None) == -1
    assert L.spl_pileup_counts(None, 0, 0, None, None, None, None) == -1 and L.spl_last_call_stats(None, None) == -1


# ---- the command -----------------------------------------------------------------------------------------------------------
def _call(args, cwd, env=None):
    return subprocess.run([BIN, "call"] + args, cwd=cwd, capture_output=True, text=True, env=env, timeout=120)


def test_call_usage_without_arguments(built, tmp_path):
    r = _call([], str(tmp_path))
    assert r.returncode == 1
    assert "spumoni call - " in r.stderr
    for opt in ("-h, --help", "-r, --ref", "-p, --pattern", "-n, --no-digest", "-m, --minimizer-alphabet", "-a, --dna-minimizer",
                "-d, --doc-array", "-D, --min-depth", "-A, --min-alt", "-Q, --min-permille", "-L -S -G -B -H", "-F -E -O -N -I"):
        assert opt in r.stderr, opt
    for word in ("<pattern>.vcf", "VCFv4.2", "(default: 2)", "(default: 500)", ".fa.seqs", "spumoni build -n -s", "counted, not called"):
        assert word in r.stderr, word
    top = subprocess.run([BIN], capture_output=True, text=True)
    assert top.returncode == 1 and "\tcall\t" in top.stderr and "\tcover\t" in top.stderr
    assert _call(["-h"], str(tmp_path)).returncode == 1


@pytest.mark.parametrize("args,table,message", [
    (["-p", "reads.fa", "-n"], None, "Both a reference file (-r) and pattern file (-p) must be provided."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-P"], None, "-P cannot be used with `spumoni call`"),
    (["-r", "ref", "-p", "reads.fa", "-m"], None, "-m / -a cannot be used with `spumoni call`"),
    (["-r", "ref", "-p", "reads.fa", "-a"], None, "-m / -a cannot be used with `spumoni call`"),
    (["-r", "ref", "-p", "reads.fa", "-n", "-m"], None, "-m / -a cannot be used with `spumoni call`"),
    (["-r", "ref", "-p", "reads.fa"], None, "`spumoni call` needs -n"),
    (["-r", "nosuch", "-p", "reads.fa", "-n"], None, "The following path is not valid: nosuch.fa"),
    (["-r", "ref", "-p", "missing.fa", "-n"], None, "The following path is not valid: missing.fa"),
    (["-r", "ref", "-p", "reads.fa", "-n", "-L", "0"], None, "the minimum match length (-L) must be at least 1."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-E", "4097"], None, "the largest extended end (-E) must be between 1 and 4096."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-D", "0"], None, "the smallest depth (-D) must be between 1 and 4294967295."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-D", "4294967296"], None, "the smallest depth (-D) must be between 1 and 4294967295."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-A", "0"], None, "the fewest reads with the called letter (-A) must be between 1 and 4294967295."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-A", "-3"], None, "the fewest reads with the called letter (-A) must be between 1 and 4294967295."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-Q", "1001"], None, "the smallest share (-Q) must be between 0 and 1000 thousandths."),
    (["-r", "ref", "-p", "reads.fa", "-n"], None, "the index has no sequence table (ref.fa.seqs): build it with -s"),
    (["-r", "ref", "-p", "reads.fa", "-n"], b"a\t5\t0\n", "ref.fa.seqs: line 1 is not name<TAB>length<TAB>text_start<TAB>strands"),
    (["-r", "ref", "-p", "reads.fa", "-n"], b"\n", "ref.fa.seqs: no sequences"),
])
def test_call_refusals_leave_no_file(built, tmp_path, args, table, message):
    _golden_index(tmp_path, table)
    before = sorted(os.listdir(tmp_path))
    r = _call(args, str(tmp_path))
    assert r.returncode == 1
    assert message in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_call_missing_entry_point_on_the_fake_device(built, fake_device, tmp_path):
    _golden_index(tmp_path)
    before = sorted(os.listdir(tmp_path))
    env = dict(os.environ, LD_LIBRARY_PATH=fake_device + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = _call(["-r", "ref", "-p", "reads.fa", "-n", "-L", "4"], str(tmp_path), env=env)
    assert r.returncode == 1
    assert "has no spl_call_add_batch" in r.stderr and "`spumoni call`" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_a_failing_call_run_writes_no_vcf(built, tmp_path):
    """Without a device the command stops at its entry points; with one, at a table that does not add up to the text, and
    then at a read that is empty: either way no file."""
    _golden_index(tmp_path)
    before = sorted(os.listdir(tmp_path))
    if built.spx_device_count() > 0:
        n = os.path.getsize(tmp_path / "ref.fa.rawtext")
        (tmp_path / "ref.fa.seqs").write_bytes(b"whole\t%d\t0\t1\n" % (n - 1))
        r = _call(["-r", "ref", "-p", "reads.fa", "-n"], str(tmp_path))
        assert r.returncode == 1 and f"ref.fa.seqs: the sequences add up to {n - 1} characters, the text has {n}" in r.stderr, r.stderr
        assert sorted(os.listdir(tmp_path)) == before
        (tmp_path / "ref.fa.seqs").write_bytes(b"whole\t%d\t0\t1\n" % n)
        # (a FASTA file of the test's own: the golden reads are FASTQ records under this name)
        text = (tmp_path / "ref.fa.rawtext").read_bytes()
        (tmp_path / "reads.fa").write_bytes(b">good\n" + text[:40] + b"\n>bad_one\n>after\n" + text[5:45] + b"\n")
    r = _call(["-r", "ref", "-p", "reads.fa", "-n", "-d"], str(tmp_path))
    assert r.returncode == 1
    if built.spx_device_count() > 0:
        assert "bad_one was empty" in r.stderr, r.stderr
    else:
        assert "no usable gfx950 device" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before
    assert not any(name.endswith(".vcf") for name in os.listdir(tmp_path))


def test_the_file_writer_under_the_sanitizers(tmp_path):
    """The host code that formats the .vcf (spumoni_amd/csrc/host/call_vcf.hpp) in a stand-alone program
    (tests/call_vcf_check.cpp) with the address and undefined-behaviour sanitizers: a handful of records, the counts at
    their largest, and records the writer must refuse."""
    exe = str(tmp_path / "call_vcf_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(ROOT, "tests", "call_vcf_check.cpp")], check=True)
    p = subprocess.run([exe, str(tmp_path / "out.vcf")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "call vcf ok" in p.stdout, p.stdout + p.stderr
    lines = (tmp_path / "out.vcf").read_text().split("\n")
    assert lines[:4] == ["##fileformat=VCFv4.2", "##contig=<ID=one,length=5>", "##contig=<ID=a name with spaces,length=1>",
                         "##contig=<ID=three,length=18446744073709551615>"]
    assert [line[:13] for line in lines[4:10]] == ["##INFO=<ID=DP", "##INFO=<ID=AD", "##INFO=<ID=BC", "##INFO=<ID=OT", "##INFO=<ID=DL", "##INFO=<ID=IN"]
    assert lines[10] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
    assert lines[11:] == ["one\t1\t.\tA\tC\t.\t.\tDP=7;AD=1,4;BC=0,4,1,0;OT=1;DL=2;IN=3",
                          "one\t5\t.\tc\tT\t.\t.\tDP=2;AD=0,2;BC=0,0,0,2;OT=0;DL=0;IN=0",
                          "a name with spaces\t1\t.\tN\tA\t.\t.\tDP=4294967295;AD=0,4294967295;BC=4294967295,0,0,0;OT=0;DL=0;IN=0",
                          "three\t18446744073709551615\t.\tT\tG\t.\t.\tDP=9;AD=3,3;BC=1,2,3,0;OT=4294967295;DL=4294967295;IN=4294967295",
                          "three\t11\t.\tG\tA\t.\t.\tDP=3;AD=4294967294,3;BC=3,0,0,0;OT=0;DL=0;IN=0", ""]
