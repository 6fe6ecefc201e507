"""The consensus rule (spumoni_amd/consensus.py) against hand-computed answers for each of its five rules, the newline
arithmetic, the calls' reference on random arrays and the planted genome through the Python reference chain; the header as
C99 and the exports; `spumoni consensus`'s usage and refusals; the file writer under the sanitizers.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from spumoni_amd import capi, synth
from spumoni_amd.call import calls_reference, del_of
from spumoni_amd.consensus import MAX_LINE_WIDTH, SEQ_DTYPE, body_bytes, consensus_reference, fasta_of, tsv_of
from spumoni_amd.cover import depth_of, seq_starts
from tests import consensus_cases as cc
from tests.test_map_cpu import _golden_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
HEADER = os.path.join(ROOT, "include", "spumoni_consensus.h")


@pytest.fixture(scope="module")
def built(built_all):
    return capi.lib()


def _one(depth, alt, dele, text, ins=None, lengths=None, strands=1, **kw):
    """(records as tuples, body bytes) of one table; alt: one row of four per position."""
    G = len(depth)
    ins = [0] * G if ins is None else ins
    rec, body = consensus_reference(depth, np.array(alt, dtype=np.uint32).reshape(-1), ins, dele, np.frombuffer(text, dtype=np.uint8),
                                    [G] if lengths is None else lengths, strands, **kw)
    assert rec.dtype == SEQ_DTYPE and body.dtype == np.uint8
    return [tuple(int(v) for v in r) for r in rec], body.tobytes()


Z = [0, 0, 0, 0]


def test_each_rule_by_hand():
    # rule 1: span = depth + del below min_depth -> the mask; nothing else is looked at (alt, ins would pass)
    assert _one([1], [[0, 9, 0, 0]], [0], b"A", ins=[9], min_depth=2) == ([(0, 1, 0, 0, 1, 0)], b"N\n")
    # rule 2: deleted -- 2 of span 4 is 500 thousandths
    assert _one([2], [Z], [2], b"A") == ([(0, 0, 0, 1, 0, 0)], b"")
    assert _one([3], [Z], [2], b"A") == ([(0, 1, 0, 0, 0, 0)], b"A\n")  # 2 of 5: 400, kept
    assert _one([9], [Z], [1], b"A", min_permille=0) == ([(0, 1, 0, 0, 0, 0)], b"A\n")  # below min_alt
    # rule 3 on its own: span >= min_depth > d, not deleted (1 of span 3 is 333 thousandths)
    assert _one([2], [[0, 2, 0, 0]], [1], b"A", min_depth=3, min_alt=1) == ([(0, 1, 0, 0, 1, 0)], b"N\n")
    # ... where an insertion site still counts: rule 1 did not mask it (2 of span 3)
    assert _one([2], [Z], [1], b"A", ins=[2], min_depth=3) == ([(0, 1, 0, 0, 1, 1)], b"N\n")
    # rule 4: substituted, the calls' choice: the largest count, the lowest code among equals, never ref's own
    assert _one([4], [[0, 2, 0, 0]], [0], b"A") == ([(0, 1, 1, 0, 0, 0)], b"C\n")
    assert _one([4], [[0, 0, 2, 2]], [0], b"A") == ([(0, 1, 1, 0, 0, 0)], b"G\n")
    assert _one([4], [[0, 2, 2, 3]], [0], b"a", min_permille=0) == ([(0, 1, 1, 0, 0, 0)], b"T\n")
    assert _one([4], [[0, 4, 0, 0]], [0], b"C") == ([(0, 1, 0, 0, 0, 0)], b"C\n")  # the reference's own code
    assert _one([5], [[0, 2, 0, 0]], [0], b"A") == ([(0, 1, 0, 0, 0, 0)], b"A\n")  # 400 thousandths of d
    # rule 4 measures against d, rule 2 against span: 2 of d = 4 substitutes although it is 333 thousandths of span 6
    assert _one([4], [[0, 2, 0, 0]], [2], b"A") == ([(0, 1, 1, 0, 0, 0)], b"C\n")
    # rule 5: kept as it is, lower case and bytes outside ACGT included
    assert _one([4, 4, 4], [Z, Z, Z], [0, 0, 0], b"gNt") == ([(0, 3, 0, 0, 0, 0)], b"gNt\n")
    # the order of rules 2 and 4 when both hold, at min_permille 0 and 250: deleted
    for permille in (0, 250):
        assert _one([6], [[0, 3, 0, 0]], [2], b"A", min_permille=permille) == ([(0, 0, 0, 1, 0, 0)], b"")
        assert _one([6], [[0, 3, 0, 0]], [1], b"A", min_permille=permille) == ([(0, 1, 1, 0, 0, 0)], b"C\n")  # del below min_alt
    # ref of code 4: all four are candidates, A among them
    for k, letter in enumerate(b"ACGT"):
        alt = [0] * 4
        alt[k] = 3
        assert _one([3], [alt], [0], b"N") == ([(0, 1, 1, 0, 0, 0)], bytes([letter]) + b"\n")
    assert _one([3], [[2, 2, 2, 2]], [0], b"-") == ([(0, 1, 1, 0, 0, 0)], b"A\n")
    # mask: another byte, and 0 for the reference's byte (rules 1 and 3 alike)
    assert _one([0, 2], [Z, Z], [0, 1], b"cg", min_depth=3, mask=ord("n")) == ([(0, 2, 0, 0, 2, 0)], b"nn\n")
    assert _one([0, 2], [Z, Z], [0, 1], b"cg", min_depth=3, mask=b"x") == ([(0, 2, 0, 0, 2, 0)], b"xx\n")
    assert _one([0, 2], [Z, Z], [0, 1], b"cg", min_depth=3, mask=0) == ([(0, 2, 0, 0, 2, 0)], b"cg\n")
    # insertion sites: counted on kept, substituted and deleted positions, against span; never applied
    rec, body = _one([4, 4, 2, 0], [Z, [0, 0, 4, 0], Z, Z], [0, 0, 2, 0], b"AAAA", ins=[2, 2, 2, 9])
    assert (rec, body) == ([(0, 3, 1, 1, 1, 3)], b"AGN\n")
    assert _one([4], [Z], [0], b"A", ins=[1])[0] == [(0, 1, 0, 0, 0, 0)] and _one([5], [Z], [0], b"A", ins=[2])[0] == [(0, 1, 0, 0, 0, 0)]
    # 64 bits: del * 1000 beyond 2^32, and a span beyond 2^32
    assert _one([5_000_000], [Z], [5_000_000], b"A") == ([(0, 0, 0, 1, 0, 0)], b"")
    assert _one([5_000_001], [Z], [5_000_000], b"A") == ([(0, 1, 0, 0, 0, 0)], b"A\n")
    assert _one([2**31 + 1], [Z], [2**31 + 1], b"A") == ([(0, 0, 0, 1, 0, 0)], b"")
    assert _one([2**31 + 1], [Z], [2**31 + 1], b"A", min_depth=2**32 - 1) == ([(0, 0, 0, 1, 0, 0)], b"")  # span 2^32 + 2 passes min_depth
    assert _one([2**31 + 2], [Z], [2**31 + 1], b"A") == ([(0, 1, 0, 0, 0, 0)], b"A\n")
    # parameters outside their ranges
    for kw in (dict(min_depth=0), dict(min_alt=0), dict(min_permille=1001), dict(line_width=-1), dict(line_width=2**31), dict(mask=256),
               dict(mask=b"NN")):
        with pytest.raises(ValueError):
            _one([1], [Z], [0], b"A", **kw)


def test_sequences_are_judged_apart_and_an_all_deleted_one_leaves_nothing():
    """Two strands: the forward piece of sequence s starts at P[2 s].  The middle sequence is deleted whole: no bytes, and
    the next one starts where the first ended."""
    text = b"ACG" + b"CGT" + b"TT" + b"AA" + b"GGCA" + b"TGCC"
    depth, dele = [4, 4, 4, 1, 1, 4, 4, 4, 0], [0, 0, 0, 3, 3, 0, 0, 0, 0]
    alt = [Z, [0, 0, 0, 4], Z, Z, Z, Z, [4, 0, 0, 0], Z, Z]
    rec, body = _one(depth, alt, dele, text, lengths=[3, 2, 4], strands=2, line_width=2)
    assert rec == [(0, 3, 1, 0, 0, 0), (5, 0, 0, 2, 0, 0), (5, 4, 1, 0, 1, 0)]
    assert body == b"AT\nG\n" + b"" + b"GA\nCN\n"
    assert fasta_of([b"a", "b", b"c d"], *consensus_reference(depth, np.array(alt).reshape(-1), [0] * 9, dele, np.frombuffer(text, dtype=np.uint8),
                                                            [3, 2, 4], 2, line_width=2)) == b">a\nAT\nG\n>b\n>c d\nGA\nCN\n"
    recs = consensus_reference(depth, np.array(alt).reshape(-1), [0] * 9, dele, np.frombuffer(text, dtype=np.uint8), [3, 2, 4], 2)[0]
    assert tsv_of([b"a", "b", b"c d"], [3, 2, 4], recs) == b"a\t3\t3\t1\t0\t0\t0\nb\t2\t0\t0\t2\t0\t0\nc d\t4\t4\t1\t0\t1\t0\n"
    # every sequence deleted: an empty body
    rec, body = _one([0, 0], [Z, Z], [2, 2], b"AC", lengths=[1, 1])
    assert rec == [(0, 0, 0, 1, 0, 0), (0, 0, 0, 1, 0, 0)] and body == b""
    assert fasta_of(["x", "y"], np.array(rec, dtype=SEQ_DTYPE), np.zeros(0, dtype=np.uint8)) == b">x\n>y\n"


@pytest.mark.parametrize("w", [0, 1, 7, 60])
def test_newlines_at_every_letter_count_around_the_width(w):
    base = w if w else 5
    for letters in sorted({0, 1, max(base - 1, 0), base, base + 1, 2 * base}):
        # a sequence of letters + 2 bases, two of them deleted; a second sequence behind it shows where the first ended
        G = letters + 2
        text = (b"ACGT" * (G // 4 + 1))[:G]
        depth, dele = [4] * G + [4], [0] * G + [0]
        for at in (0, G // 2 + (1 if G // 2 == 0 else 0)):
            depth[at], dele[at] = 0, 4
        rec, body = _one(depth, [Z] * (G + 1), dele, text + b"T", lengths=[G, 1], line_width=w)
        kept = bytes(b for i, b in enumerate(text) if dele[i] == 0)
        assert len(kept) == letters
        want = cc.wrap(kept, w)
        assert len(want) == body_bytes(letters, w) == letters + ((letters + w - 1) // w if w else int(letters > 0))
        assert rec == [(0, letters, 0, 2, 0, 0), (len(want), 1, 0, 0, 0, 0)] and body == want + b"T\n", (w, letters)
        if letters:
            assert body[len(want) - 1:len(want)] == b"\n" and b"\n\n" not in body
    assert body_bytes(MAX_LINE_WIDTH, MAX_LINE_WIDTH) == MAX_LINE_WIDTH + 1 and body_bytes(MAX_LINE_WIDTH + 1, MAX_LINE_WIDTH) == MAX_LINE_WIDTH + 3


@pytest.mark.parametrize("params", [(1, 1, 0), (2, 2, 500), (1, 2, 1000), (3, 1, 250)])
def test_substituted_positions_are_the_calls_that_rules_1_to_3_leave(params):
    rng = np.random.default_rng(sum(params))
    lengths = [700, 1, 299]
    F = seq_starts(lengths)
    G = F[-1]
    for strands in (1, 2):
        text = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)[rng.integers(0, 9, G * strands)]
        depth = rng.integers(0, 7, G).astype(np.uint32)
        dele = (rng.integers(0, 5, G) * (rng.random(G) < 0.4)).astype(np.uint32)
        alt = rng.integers(0, 4, 4 * G).astype(np.uint32)
        ins = rng.integers(0, 4, G).astype(np.uint32)
        min_depth, min_alt, permille = params
        rec, body = consensus_reference(depth, alt, ins, dele, text, lengths, strands, *params, line_width=0)
        calls = calls_reference(depth, depth, alt, ins, ins, dele, text, lengths, strands, *params)
        called = {F[int(c["seq"])] + int(c["pos"]): b"ACGT"[int(c["allele"])] for c in calls}
        span = depth.astype(np.int64) + dele
        gone = (dele >= min_alt) & (dele.astype(np.int64) * 1000 >= permille * span) & (span >= min_depth)
        low = (span < min_depth) | (~gone & (depth < min_depth))
        lines = body.tobytes().split(b"\n")
        n_sub = 0
        for s in range(3):
            want = bytearray()
            for g in range(F[s], F[s + 1]):
                if low[g]:
                    want.append(ord("N"))
                elif not gone[g]:
                    want.append(called.get(g, int(text[F[s] * strands + g - F[s]])))
            subs = sum(1 for g in range(F[s], F[s + 1]) if g in called and not low[g] and not gone[g])
            n_sub += subs
            assert (int(rec[s]["letters"]), int(rec[s]["substituted"]), int(rec[s]["deleted"]), int(rec[s]["masked"])) == \
                (len(want), subs, int(gone[F[s]:F[s + 1]].sum()), int(low[F[s]:F[s + 1]].sum())), (s, strands)
            if want:
                assert lines.pop(0) == bytes(want), (s, strands)
        assert lines == [b""] and n_sub > 20 and gone.sum() > 20 and low.sum() > 5


def test_the_planted_genome_comes_back_from_the_reference_chain(oracle_mod):
    """Reads cut from a copy with ten substitutions and a deletion of three bases: the oracle's matching statistics ->
    mems -> chain -> extend -> map -> cover + pileup -> consensus gives the copy's letters wherever three reads or more were
    cut, and N elsewhere."""
    plant = cc.planted()
    text = plant["text"]
    seqs, offs = plant["seqs_offs"]
    raw = synth.index_from_text(torch.from_numpy(text.copy()))
    cov, pile = cc.reference_arrays(oracle_mod, raw, text, seqs, offs)
    depth, dele = depth_of(cov[0]), del_of(pile[3])
    rec, body = consensus_reference(depth, pile[0], pile[2], dele, text, cc.LENGTHS, cc.STRANDS, min_depth=cc.MIN_DEPTH)
    assert body.tobytes() == cc.expected_body(plant)
    assert fasta_of(cc.NAMES, rec, body) == b"".join(b">" + n + b"\n" + cc.wrap(e, 60) for n, e in zip(cc.NAMES, plant["expected"]))
    masked = [e.count(b"N") for e in plant["expected"]]
    assert [tuple(int(v) for v in r)[1:5] for r in rec] == [(cc.LENGTHS[0] - 3, 7, 3, masked[0]), (cc.LENGTHS[1], 3, 0, masked[1])]
    assert 10 <= masked[0] < 30 and masked[1] > 200 and int(rec["ins_sites"].sum()) == 0
    # the reference's letters for the masked bases: the copy has no change where no read was cut
    rec0, body0 = consensus_reference(depth, pile[0], pile[2], dele, text, cc.LENGTHS, cc.STRANDS, min_depth=cc.MIN_DEPTH, mask=0, line_width=0)
    assert body0.tobytes() == b"".join(c + b"\n" for c in plant["copies"]) and np.array_equal(rec0["masked"], rec["masked"])


# ---- header and exports ------------------------------------------------------------------------------------------------
def _declared():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return code, sorted(set(re.findall(r"\b(sps_[a-z_0-9]+)\s*\(", code)))


def test_consensus_header_is_plain_c(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include <stddef.h>\n#include "spumoni_consensus.h"\nint main(void) { sps_params p; sps_seq r; sps_consensus_stats s; '
                   '(void)p; (void)r; (void)s; return sizeof(sps_params) == 20 && sizeof(sps_seq) == 48 && sizeof(sps_consensus_stats) == 80 '
                   '&& offsetof(sps_params, mask) == 16 && offsetof(sps_seq, ins_sites) == 40 && offsetof(sps_consensus_stats, overflow) == 64 '
                   '&& sizeof(spl_call) == 48 ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "c"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "c")]).returncode == 0
    code, _ = _declared()
    assert "hipStream_t" not in code and "std::" not in code and "#include <hip" not in code and "spx_" not in code.replace("spx_index", "")
    assert re.findall(r'#include\s+[<"]([^>"]+)', code) == ["stdint.h", "spumoni_call.h"]


def test_consensus_header_symbols_exported(built):
    _, names = _declared()
    assert names == sorted(capi.CONSENSUS_EXPORTS) and len(names) == 4
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(sps_[a-z_0-9]+)\b", out))) == names
    for other in (capi.EXPORTS, capi.DOCVOTE_EXPORTS, capi.MEMS_EXPORTS, capi.PLACE_EXPORTS, capi.CHAIN_EXPORTS, capi.ALIGN_EXPORTS,
                  capi.CIGAR_EXPORTS, capi.EXTEND_EXPORTS, capi.REFTEXT_EXPORTS, capi.MAP_EXPORTS, capi.COVER_EXPORTS, capi.CALL_EXPORTS):
        assert not set(capi.CONSENSUS_EXPORTS) & set(other)
    assert capi.C.sizeof(capi.SpsParams) == 20 and capi.C.sizeof(capi.SpsConsensusStats) == 80 and SEQ_DTYPE.itemsize == 48
    assert list(SEQ_DTYPE.names) == ["body_start", "letters", "substituted", "deleted", "masked", "ins_sites"]
    assert [f[0] for f in capi.SpsConsensusStats._fields_] == ["positions", "kept", "substituted", "deleted", "masked", "ins_sites", "letters",
                                                               "bytes", "overflow", "step_ms"]
    for method in ("consensus_device", "consensus", "consensus_stats"):
        assert callable(getattr(capi.Index, method))


def test_consensus_entry_points_without_an_index_fail_loudly(built):
    L = capi._sps()
    n = capi.C.c_uint64(0)
    p = capi.SpsParams(2, 2, 500, 60, ord("N"))
    assert L.sps_consensus_device(None, None, None, None, None, capi.C.byref(p), 0, None, None, None, None) == -1
    assert b"index must be non-null" in L.spx_last_error()
    assert L.sps_consensus_begin(None, capi.C.byref(p), capi.C.byref(n)) == -1 and b"index and n_bytes must be non-null" in L.spx_last_error()
    assert L.sps_consensus_fetch(None, None, None) == -1 and L.sps_last_consensus_stats(None, None) == -1


# ---- the command -----------------------------------------------------------------------------------------------------------
def _consensus(args, cwd, env=None):
    return subprocess.run([BIN, "consensus"] + args, cwd=cwd, capture_output=True, text=True, env=env, timeout=120)


def test_consensus_usage_without_arguments(built, tmp_path):
    r = _consensus([], str(tmp_path))
    assert r.returncode == 1
    assert "spumoni consensus - " in r.stderr
    for opt in ("-h, --help", "-r, --ref", "-p, --pattern", "-n, --no-digest", "-m, --minimizer-alphabet", "-a, --dna-minimizer",
                "-d, --doc-array", "-D, --min-depth", "-A, --min-alt", "-Q, --min-permille", "-U, --mask", "-u, --keep-low", "-J, --line-width",
                "-L -S -G -B -H", "-F -E -O -N -I"):
        assert opt in r.stderr, opt
    for word in ("<pattern>.consensus.fa", "<pattern>.consensus.tsv", "(default: 2)", "(default: 500)", "(default: N)", "(default: 60)",
                 ".fa.seqs", "spumoni build -n -s", "counted, not applied"):
        assert word in r.stderr, word
    top = subprocess.run([BIN], capture_output=True, text=True)
    assert top.returncode == 1 and "\tconsensus\t" in top.stderr and "\tcall\t" in top.stderr
    assert _consensus(["-h"], str(tmp_path)).returncode == 1


@pytest.mark.parametrize("args,table,message", [
    (["-p", "reads.fa", "-n"], None, "Both a reference file (-r) and pattern file (-p) must be provided."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-P"], None, "-P cannot be used with `spumoni consensus`"),
    (["-r", "ref", "-p", "reads.fa", "-m"], None, "-m / -a cannot be used with `spumoni consensus`"),
    (["-r", "ref", "-p", "reads.fa", "-a"], None, "-m / -a cannot be used with `spumoni consensus`"),
    (["-r", "ref", "-p", "reads.fa"], None, "`spumoni consensus` needs -n"),
    (["-r", "nosuch", "-p", "reads.fa", "-n"], None, "The following path is not valid: nosuch.fa"),
    (["-r", "ref", "-p", "reads.fa", "-n", "-D", "0"], None, "the smallest depth (-D) must be between 1 and 4294967295."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-A", "0"], None, "(-A) must be between 1 and 4294967295."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-Q", "1001"], None, "the smallest share (-Q) must be between 0 and 1000 thousandths."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-U", "NN"], None, "the mask (-U) must be one byte"),
    (["-r", "ref", "-p", "reads.fa", "-n", "-U", ""], None, "the mask (-U) must be one byte"),
    (["-r", "ref", "-p", "reads.fa", "-n", "-J", "2147483648"], None, "the line width (-J) must be between 0 and 2147483647."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-J", "-1"], None, "the line width (-J) must be between 0 and 2147483647."),
    (["-r", "ref", "-p", "reads.fa", "-n"], None, "the index has no sequence table (ref.fa.seqs): build it with -s"),
    (["-r", "ref", "-p", "reads.fa", "-n"], b"\n", "ref.fa.seqs: no sequences"),
    # the rest of `call`'s table (tests/test_call_cpu.py), with this command's wording of -A in full
    (["-r", "ref", "-p", "reads.fa", "-n", "-m"], None, "-m / -a cannot be used with `spumoni consensus`"),
    (["-r", "ref", "-p", "missing.fa", "-n"], None, "The following path is not valid: missing.fa"),
    (["-r", "ref", "-p", "reads.fa", "-n", "-L", "0"], None, "the minimum match length (-L) must be at least 1."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-E", "4097"], None, "the largest extended end (-E) must be between 1 and 4096."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-D", "4294967296"], None, "the smallest depth (-D) must be between 1 and 4294967295."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-A", "0"], None,
     "the fewest reads with a substituted letter or a deletion (-A) must be between 1 and 4294967295."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-A", "-3"], None,
     "the fewest reads with a substituted letter or a deletion (-A) must be between 1 and 4294967295."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-U", ">"], None, "the mask (-U) must be one byte other than a newline and '>'."),
    (["-r", "ref", "-p", "reads.fa", "-n"], b"a\t5\t0\n", "ref.fa.seqs: line 1 is not name<TAB>length<TAB>text_start<TAB>strands"),
])
def test_consensus_refusals_leave_no_file(built, tmp_path, args, table, message):
    _golden_index(tmp_path, table)
    before = sorted(os.listdir(tmp_path))
    r = _consensus(args, str(tmp_path))
    assert r.returncode == 1
    assert message in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_consensus_missing_entry_point_on_the_fake_device(built, fake_device, tmp_path):
    _golden_index(tmp_path)
    before = sorted(os.listdir(tmp_path))
    env = dict(os.environ, LD_LIBRARY_PATH=fake_device + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = _consensus(["-r", "ref", "-p", "reads.fa", "-n", "-L", "4"], str(tmp_path), env=env)
    assert r.returncode == 1
    assert "has no spl_call_add_batch" in r.stderr and "`spumoni consensus`" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_the_file_writer_under_the_sanitizers(tmp_path):
    """The host code that writes the two files (spumoni_amd/csrc/host/consensus_fasta.hpp) in a stand-alone program
    (tests/consensus_fasta_check.cpp) with the address and undefined-behaviour sanitizers: a few sequences, one without
    letters, counts at their largest, and records the writer must refuse."""
    exe = str(tmp_path / "consensus_fasta_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(ROOT, "tests", "consensus_fasta_check.cpp")], check=True)
    p = subprocess.run([exe, str(tmp_path / "out.fa"), str(tmp_path / "out.tsv")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "consensus fasta ok" in p.stdout, p.stdout + p.stderr
    assert (tmp_path / "out.fa").read_bytes() == b">one\nACG\nT\n>a name with spaces\n>three\nnn\n"
    assert (tmp_path / "out.tsv").read_bytes() == (b"one\t5\t4\t1\t1\t0\t2\na name with spaces\t1\t0\t0\t1\t0\t0\n"
                                                    b"three\t18446744073709551615\t2\t18446744073709551615\t18446744073709551615\t2\t"
                                                    b"18446744073709551615\n")
