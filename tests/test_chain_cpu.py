"""CPU tier of the chains: the definition (spumoni_amd/chain.py: chain_reference) against an independent loop without a
window, on hand-computed tables and on a planted case with a known answer, the plain-C header include/spumoni_chain.h
and the library's exports, the loud failure without a device, and `spumoni chain`'s usage, validation messages and its
failure against a library without the chain kernel.  What the kernel and the command compute is
tests/test_gpu_chain.py's business."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from spumoni_amd import capi, synth
from spumoni_amd.chain import CHAIN_DTYPE, NO_DOC, NO_PRED, UNCHAINED, ChainParams, chain_reference
from spumoni_amd.mems import MATCH_DTYPE, mems_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
HEADER = os.path.join(ROOT, "include", "spumoni_chain.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "files", "dna_fastq")


@pytest.fixture(scope="module")
def built(built_all):
    return capi.lib()


def _recs(anchors):
    """MATCH_DTYPE records from (x, y, l) triples."""
    return np.array([(y, x, l) for x, y, l in anchors], dtype=MATCH_DTYPE)


def _full(anchors, params, D=None):
    """f, pred and the record of ONE read by a loop over every pair (no window), the walk back over pred done apart."""
    _, max_dist, max_gap, penalty = params
    f, pred = [], []
    for i, (xi, yi, li) in enumerate(anchors):
        best, arg = li, None
        for j in range(i - 1, -1, -1):  # descending: `>` keeps the largest j among equals
            xj, yj, lj = anchors[j]
            dx, dy = xi - xj, yi - yj
            ends = (xi + li - xj - lj, yi + li - yj - lj)
            if min(dx, dy, *ends) < 1 or max(dx, dy) > max_dist or abs(dx - dy) > max_gap or (D is not None and D[i] != D[j]):
                continue
            c = f[j] + min(li, *ends) - penalty * abs(dx - dy)
            if c > best:
                best, arg = c, j
        f.append(best)
        pred.append(arg)
    if not anchors:
        return f, pred, (UNCHAINED, 0, 0, 0, 0, 0, 0, 0, 0, NO_DOC)
    last = f.index(max(f))
    path = [last]
    while pred[path[-1]] is not None:
        path.append(pred[path[-1]])
    path.reverse()
    gap = sum(abs((anchors[b][0] - anchors[a][0]) - (anchors[b][1] - anchors[a][1])) for a, b in zip(path, path[1:]))
    x0, y0, _ = anchors[path[0]]
    x1, y1, l1 = anchors[last]
    return f, pred, (y0, y1 + l1, x0, x1 + l1, f[last], len(path), path[0], last, min(gap, 2**32 - 1), NO_DOC if D is None else D[last])


def _random_read(rng, h, spread):
    """h anchors that mostly follow a diagonal with indels, some out of order, some overlapping."""
    x = np.sort(rng.integers(0, 40 * max(h, 1), h))
    y = 1000 + x + np.cumsum(rng.integers(-spread, spread + 1, h))
    swap = rng.random(h) < 0.1
    y[swap] = rng.integers(0, 3000, int(swap.sum()))
    l = rng.integers(1, 60, h)
    return [(int(a), int(b), int(c)) for a, b, c in zip(x, y, l)]


@pytest.mark.parametrize("seed", range(4))
def test_reference_against_a_loop_over_every_pair(seed):
    rng = np.random.default_rng(seed)
    chained = alone = 0
    for params in (ChainParams(), ChainParams(64, 200, 10, 3), ChainParams(64, 5000, 0, 0), ChainParams(64, 2**31 - 1, 2**31 - 1, 65535)):
        reads = [_random_read(rng, int(h), 1 + 3 * (seed % 2)) for h in rng.integers(0, 65, 25)]  # h <= lookback: no window
        reads[3], reads[10], reads[-1] = [], [], []
        front = [(5, 5, 5)] * (seed % 3)  # match_offsets[0] != 0
        offs = np.r_[0, np.cumsum([len(r) for r in reads])].astype(np.uint64) + np.uint64(len(front))
        flat = front + [a for r in reads for a in r]
        for with_docs in (False, True):
            D = rng.integers(0, 2, len(flat)).tolist() if with_docs else None
            chains, score, pred = chain_reference(offs, _recs(flat), params, D)
            assert chains.dtype == CHAIN_DTYPE and score.dtype == np.uint32 and pred.dtype == np.uint32
            assert score.size == pred.size == len(flat)
            assert not score[:len(front)].any() and (pred[:len(front)] == NO_PRED).all()
            for q, r in enumerate(reads):
                o = int(offs[q])
                f, p, rec = _full(r, params, None if D is None else D[o:o + len(r)])
                assert score[o:o + len(r)].tolist() == f, (q, params)
                assert pred[o:o + len(r)].tolist() == [NO_PRED if v is None else v for v in p], (q, params)
                assert chains[q].tolist() == rec, (q, params)
                chained += rec[5] > 1
                alone += rec[5] == 1
    assert chained > 50 and alone > 5


def _one(anchors, params=None, D=None):
    chains, score, pred = chain_reference([0, len(anchors)], _recs(anchors), params, D)
    return score.tolist(), [None if p == NO_PRED else p for p in pred.tolist()], chains[0].tolist()


def test_hand_computed_tables():
    # two anchors on one diagonal: dx = dy = ex = ey = 15, d = 0, c = 10 + 10
    assert _one([(0, 100, 10), (15, 115, 10)]) == ([10, 20], [None, 0], (100, 125, 0, 25, 20, 2, 0, 1, 0, NO_DOC))
    # an overlap in the read: ex = 6 < l, dy = 8, d = 2: c = 10 + 6 - 2
    assert _one([(0, 100, 10), (6, 108, 10)]) == ([10, 14], [None, 0], (100, 118, 0, 16, 14, 2, 0, 1, 2, NO_DOC))
    # an overlap in the text: dx = 9, dy = 7, ey = 7 < l, d = 2: c = 10 + 7 - 2
    assert _one([(0, 100, 10), (9, 107, 10)]) == ([10, 15], [None, 0], (100, 117, 0, 19, 15, 2, 0, 1, 2, NO_DOC))
    # dy = 0 and dy < 0: not eligible; two ends with f = 10: the smaller i is the chain
    assert _one([(0, 100, 10), (20, 100, 10)]) == ([10, 10], [None, None], (100, 110, 0, 10, 10, 1, 0, 0, 0, NO_DOC))
    assert _one([(0, 100, 10), (20, 90, 10)]) == ([10, 10], [None, None], (100, 110, 0, 10, 10, 1, 0, 0, 0, NO_DOC))
    # ex = 0: the second anchor ends where the first does (10 + 10 - 20); one step further it is eligible: c = 20 + 1
    assert _one([(0, 100, 20), (10, 110, 10)]) == ([20, 10], [None, None], (100, 120, 0, 20, 20, 1, 0, 0, 0, NO_DOC))
    assert _one([(0, 100, 20), (11, 111, 10)]) == ([20, 21], [None, 0], (100, 121, 0, 21, 21, 2, 0, 1, 0, NO_DOC))
    # a tie between two predecessors (no gap cost: 10 + 10 from either): the larger j wins
    free = ChainParams(gap_penalty=0)
    assert _one([(0, 100, 10), (1, 90, 10), (30, 240, 10)], free) == \
        ([10, 10, 20], [None, None, 1], (90, 250, 1, 40, 20, 2, 1, 2, 121, NO_DOC))
    # ... and with ids that differ from the last anchor's, the only eligible one
    assert _one([(0, 100, 10), (1, 90, 10), (30, 240, 10)], free, [7, 8, 7]) == \
        ([10, 10, 20], [None, None, 0], (100, 250, 0, 40, 20, 2, 0, 2, 110, 7))
    # a candidate equal to l_i (10 + 10 - 10): the anchor alone wins
    assert _one([(0, 100, 10), (20, 130, 10)]) == ([10, 10], [None, None], (100, 110, 0, 10, 10, 1, 0, 0, 0, NO_DOC))
    assert _one([(0, 100, 10), (20, 129, 10)]) == ([10, 11], [None, 0], (100, 139, 0, 30, 11, 2, 0, 1, 9, NO_DOC))
    # two ends with equal f, the second one out of reach of the chain (dy > max_dist): the smaller i wins
    assert _one([(0, 100, 10), (15, 115, 10), (100, 9000, 20)]) == \
        ([10, 20, 20], [None, 0, None], (100, 125, 0, 25, 20, 2, 0, 1, 0, NO_DOC))
    # the limits themselves: dx = dy = max_dist, d = max_gap
    assert _one([(0, 100, 10), (5000, 5100, 10)])[0] == [10, 20] and _one([(0, 100, 10), (5001, 5101, 10)])[0] == [10, 10]
    assert _one([(0, 100, 10), (20, 620, 10)], free)[0] == [10, 20] and _one([(0, 100, 10), (20, 621, 10)], free)[0] == [10, 10]
    # the window: with lookback 1 the anchor two back is not seen
    three = [(0, 100, 10), (12, 3000, 10), (20, 120, 10)]
    assert _one(three)[0] == [10, 10, 20] and _one(three, ChainParams(lookback=2))[0] == [10, 10, 20]
    assert chain_reference([0, 3], _recs(three), ChainParams(lookback=1))[1].tolist() == [10, 10, 10]
    # no reads, no anchors
    chains, score, pred = chain_reference([0], _recs([]))
    assert chains.size == 0 and score.size == 0 and pred.size == 0
    chains, _, _ = chain_reference([0, 0], _recs([]))
    assert chains[0].tolist() == (UNCHAINED, 0, 0, 0, 0, 0, 0, 0, 0, NO_DOC)
    for bad in ((0, 5000, 500, 1), (65, 5000, 500, 1), (64, 0, 500, 1), (64, 2**31, 500, 1), (64, 5000, -1, 1), (64, 5000, 2**31, 1),
                (64, 5000, 500, -1), (64, 5000, 500, 65536)):
        with pytest.raises(ValueError):
            chain_reference([0, 2], _recs([(0, 100, 10), (15, 115, 10)]), bad)


def planted_reads():
    """The planted case of DESIGN.md 4.12: (text, seqs, offs, cuts).  30 reads of 302 characters, each cut from 303 text
    characters with substitutions at 40 and 210, text characters 120 .. 122 deleted and two random letters inserted at
    text position 260."""
    rng = np.random.default_rng(2025)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    text = letters[rng.integers(0, 4, 20_000)]
    cuts = rng.integers(0, text.size - 303, 30)
    reads = []
    for c in cuts:
        rd = text[c:c + 303].copy()
        for at in (40, 210):
            rd[at] = letters[(int(np.flatnonzero(letters == rd[at])[0]) + 1 + int(rng.integers(0, 3))) % 4]  # a different letter
        rd = np.r_[rd[:120], rd[123:260], letters[rng.integers(0, 4, 2)], rd[260:]]
        assert rd.size == 302
        reads.append(rd)
    return text, np.concatenate(reads), np.arange(0, 302 * len(reads) + 1, 302).astype(np.uint64), cuts


def test_planted_reads_chain_over_their_indels(oracle_mod):
    """Five exact stretches of 40, 79, 87, 49 and 43 characters, a gap of 3 at the deletion and of 2 at the insertion:
    score 298 - 5.  A stretch that runs on by chance into its neighbour is cut back by min(l, ex, ey)."""
    text, seqs, offs, cuts = planted_reads()
    raw = synth.index_from_text(torch.from_numpy(text))
    w = oracle_mod.OracleIndex.from_raw(raw).ms(seqs, offs, text=text)
    mo, rec = mems_reference(w["lengths"], w["pointers"], offs, 12)
    whole = bytes(text)
    for q in range(len(cuts)):  # the test's own preconditions
        mine = rec[int(mo[q]):int(mo[q + 1])]
        assert mine.size in (5, 6), (q, mine)
        for r in mine:
            p, n = int(r["ref_pos"]), int(r["length"])
            assert whole.count(whole[p:p + n]) == 1, (q, r)
    chains, score, pred = chain_reference(mo, rec)
    for q, c in enumerate(cuts):
        got = chains[q]
        assert (int(got["read_start"]), int(got["read_end"]), int(got["ref_start"]), int(got["ref_end"]), int(got["anchors"]),
                int(got["gap"]), int(got["score"])) == (0, 302, int(c), int(c) + 303, 5, 5, 293), (q, got)


def _declared():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return code, sorted(set(re.findall(r"\b(spc_[a-z_0-9]+)\s*\(", code)))


def test_chain_header_is_plain_c(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include "spumoni_chain.h"\nint main(void) { spc_chain c; spc_params p; spc_chain_stats s; (void)c; (void)p; (void)s; '
                   'return sizeof(spc_chain) == 48 && sizeof(spc_params) == 16 && SPC_UNCHAINED + 1 == 0 && SPC_NO_DOC == 4294967295u '
                   '? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "c"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "c")]).returncode == 0
    code, _ = _declared()
    assert "hipStream_t" not in code and "std::" not in code and "#include <hip" not in code
    assert re.findall(r'#include\s+[<"]([^>"]+)', code) == ["stdint.h", "spumoni_mems.h"]


def test_chain_header_symbols_exported(built):
    _, names = _declared()
    assert names == sorted(capi.CHAIN_EXPORTS) and len(names) == 3
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(spc_[a-z_0-9]+)\b", out))) == names
    for other in (capi.EXPORTS, capi.DOCVOTE_EXPORTS, capi.MEMS_EXPORTS, capi.PLACE_EXPORTS, capi.REFTEXT_EXPORTS):
        assert not set(capi.CHAIN_EXPORTS) & set(other)
    assert np.dtype(CHAIN_DTYPE).itemsize == 48
    assert CHAIN_DTYPE.names == ("ref_start", "ref_end", "read_start", "read_end", "score", "anchors", "first", "last", "gap", "doc")
    assert [f[0] for f in capi.SpcParams._fields_] == list(ChainParams._fields) and ChainParams() == (64, 5000, 500, 1)


def test_chain_batch_without_device_fails_loudly(built):
    if built.spx_device_count() > 0:
        pytest.skip("a device is visible: the no-device path is this machine's CPU tier")
    L = capi._spc()
    seqs, offs = np.frombuffer(b"ACGT", dtype=np.uint8), np.array([0, 4], dtype=np.uint64)
    out = np.zeros(1, dtype=CHAIN_DTYPE)
    p = capi.SpcParams(64, 5000, 500, 1)
    rc = L.spc_chain_batch(None, 0, 0, 0, seqs.ctypes.data, offs.ctypes.data, 1, 1, 0, p, out.ctypes.data, None)
    assert rc == -3 and b"no CPU fallback" in L.spx_last_error()


def _chain(args, cwd, env=None):
    return subprocess.run([BIN, "chain"] + args, cwd=cwd, capture_output=True, text=True, env=env, timeout=120)


def test_usage_without_arguments(built, tmp_path):
    r = _chain([], str(tmp_path))
    assert r.returncode == 1
    assert "spumoni chain - " in r.stderr
    for opt in ("-h, --help", "-r, --ref", "-p, --pattern", "-n, --no-digest", "-m, --minimizer-alphabet", "-a, --dna-minimizer",
                "-K, --small-window", "-W, --large-window", "-d, --doc-array", "-L, --min-length", "-S, --max-dist", "-G, --max-gap",
                "-B, --gap-penalty", "-H, --lookback"):
        assert opt in r.stderr, opt
    for limits in ("1 or more", "1 .. 2147483647", "0 .. 2147483647", "0 .. 65535", "1 .. 64"):  # the ranges are stated
        assert limits in r.stderr, limits
    assert "-P, --PML" not in r.stderr
    top = subprocess.run([BIN], capture_output=True, text=True)
    assert top.returncode == 1
    for cmd in ("chain", "place", "mems", "assign", "run", "build"):
        assert f"\t{cmd}\t" in top.stderr, cmd


def _index(tmp_path, doc=True):
    for f in os.listdir(GOLDEN):
        if os.path.isfile(os.path.join(GOLDEN, f)) and (doc or not f.endswith(".doc")):
            shutil.copy(os.path.join(GOLDEN, f), tmp_path / f)
            if f.startswith("ref.fa"):  # the same files under the name -m looks for
                shutil.copy(os.path.join(GOLDEN, f), tmp_path / ("ref.bin" + f[len("ref.fa"):]))


@pytest.mark.parametrize("args,message", [
    (["-p", "reads.fa", "-n"], "Both a reference file (-r) and pattern file (-p) must be provided."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-P"], "-P cannot be used with `spumoni chain`"),
    (["-r", "ref", "-p", "reads.fa", "-n", "-M", "-P"], "-P cannot be used with `spumoni chain`"),
    (["-r", "nosuch", "-p", "reads.fa", "-n"], "The following path is not valid: nosuch.fa"),
    (["-r", "ref", "-p", "missing.fa", "-n"], "The following path is not valid: missing.fa"),
    (["-r", "ref", "-p", "reads.txt", "-n"], "The pattern file provided does not appear to be a FASTA"),
    (["-r", "ref", "-p", "reads.fa", "-m", "-a"], "Only one type of minimizer can be specified from either -m or -a."),
    (["-r", "ref", "-p", "reads.fa"], "A minimizer type must be specified using -m or -a."),
    (["-r", "ref", "-p", "reads.fa", "-a", "-K", "5", "-W", "11"], "small window size (k) cannot be larger than 4 characters."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-L", "0"], "the minimum match length (-L) must be at least 1."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-S", "0"], "the largest distance (-S) must be between 1 and 2147483647."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-S", "2147483648"], "the largest distance (-S) must be between 1 and 2147483647."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-G", "2147483648"], "the largest gap (-G) must be between 0 and 2147483647."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-G", "-1"], "the largest gap (-G) must be between 0 and 2147483647."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-B", "65536"], "the gap penalty (-B) must be between 0 and 65535."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-H", "0"], "the lookback (-H) must be between 1 and 64."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-H", "65"], "the lookback (-H) must be between 1 and 64."),
])
def test_validation_messages(built, tmp_path, args, message):
    _index(tmp_path)
    shutil.copy(tmp_path / "reads.fa", tmp_path / "reads.txt")
    before = sorted(os.listdir(tmp_path))
    r = _chain(args, str(tmp_path))
    assert r.returncode == 1
    assert message in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_doc_ids_without_doc_file_are_refused(built, tmp_path):
    _index(tmp_path, doc=False)
    before = sorted(os.listdir(tmp_path))
    r = _chain(["-r", "ref", "-p", "reads.fa", "-n", "-d"], str(tmp_path))
    assert r.returncode == 1
    assert "document array file (ref.fa.doc) is not present, so it cannot be used." in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_missing_entry_point_on_the_fake_device(built, fake_device, tmp_path):
    _index(tmp_path)
    before = sorted(os.listdir(tmp_path))
    env = dict(os.environ, LD_LIBRARY_PATH=fake_device + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = _chain(["-r", "ref", "-p", "reads.fa", "-n", "-L", "4"], str(tmp_path), env=env)
    assert r.returncode == 1
    assert "has no spc_chain_batch" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_no_device_fails_loudly_and_writes_nothing(built, tmp_path):
    if built.spx_device_count() > 0:
        pytest.skip("a device is visible: the no-device path is this machine's CPU tier")
    _index(tmp_path)
    before = sorted(os.listdir(tmp_path))
    r = _chain(["-r", "ref", "-p", "reads.fa", "-n", "-d"], str(tmp_path))
    assert r.returncode == 1
    assert "no usable gfx950 device" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before
