"""-m gpu: the query path in MS mode -- the walks and k_ms_extend -- held to matching statistics from first principles.

Every other GPU test compares HIP with oracle/, our own restatement of the reference: a misreading shared by both passes
them all.  Here the expectation is mathematics: tests/brute_ms.c (binary search over the suffix array of
tests/brute_index.c, character by character) gives the true MS of every read position of the catalogue tests/ms_cases.py;
the index is the BruteIndex fields handed to capi.Index.from_raw (neither synth.index_from_text nor the HIP builder is in
the loop) and the text is set in the checked form.  For every read made of the text's letters, at EVERY position:
lengths == true MS, text[p: p + l] == read[i: i + l] with p + l <= n_text, PML <= MS; for the reads with an absent letter
(the reference's fake pointer 0 may under-report after them): lengths <= MS and PML <= MS.  Document ids are not asserted
(a pointer walks across a document boundary while the id stays the sample's).  The oracle is not consulted.

Each test asserts the path it is about: compact rows (`describe()`), general rows (SPX_ROWS_WIDE), every slot escaped
(SPX_FAT_ALL_ESC), the chunked walk (`last_chunk_stats()["chunk_len"]`; `fallback_reads` is printed, not asserted), pieces
(`flat_runs > r`, and `== r` with SPX_NO_PIECES), the 16-bit entry point wherever the reads are shorter than 65 536 and
the 32-bit one everywhere.  No case is compared before its `reaches` holds.  The module is in the old-walk leg too
(tests/test_gpu_old_walk.py)."""
import os
import subprocess

import numpy as np
import pytest
import torch

from spumoni_amd import capi
from spumoni_amd.mems import mems_reference
from tests import brute, cases, ms_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
# the tail cases differ in the text's and the last read's length mod 8, which is k_ms_extend's business alone: one per text
# where the test is about the rows
SMALL = [c for c in ms_cases.CASES if not c.name.startswith("tail_") or c.name.endswith("_suffix_500")]
SMALL_NAMES = {c.name for c in SMALL}


@pytest.fixture(scope="module")
def answers(built_all):
    """The first-principles index and matching statistics of every case, computed once; every case reaches what it is for."""
    assert torch.cuda.is_available()
    out = {}
    for case in ms_cases.CASES:
        text, docs, ref, seqs, offs, ms = ms_cases.reference(case)
        assert case.unmet(text, ref.sa, ref.lcp, ms) == [], case.name
        out[case.name] = (text, docs, ref, seqs, offs, ms)
    return out


def _index(case, answers, with_text=True):
    text, _, ref, _, _, _ = answers[case.name]
    ix = capi.Index.from_raw(ms_cases.raw_index(ref), 0)
    assert ix.n == text.size + 1 and ix.r == ref.r
    if with_text:
        ix.set_text(torch.from_numpy(text.copy()))  # the checked form: the text against the index
    return ix


def _held_to_the_mathematics(case, answers, ix):
    """MS with lengths and PML through the 32-bit entry point, and through the 16-bit one where the reads allow it."""
    text, _, _, seqs, offs, ms = answers[case.name]
    narrow = int(np.diff(offs).max()) < 65536
    for bits in (32, 16) if narrow else (32,):
        got = ix.query_host(capi.SPX_MODE_MS, seqs, offs, bits=bits)
        pml = ix.query_host(capi.SPX_MODE_PML, seqs, offs, bits=bits)["lengths"]
        assert got["lengths"].dtype == (np.uint16 if bits == 16 else np.uint32)
        compared = ms_cases.check_answers(case, got["lengths"], got["pointers"], pml=pml)
        assert compared >= 0.8 * ms.size
        if case.name in ms_cases.UNIQUE_SUFFIX:
            assert ms_cases.last_suffix_ends_the_text(case, got["lengths"], got["pointers"])
    if not narrow:
        with pytest.raises(capi.SpxError):
            ix.query_host(capi.SPX_MODE_MS, seqs, offs, bits=16)
    return narrow


@pytest.mark.parametrize("case", ms_cases.CASES, ids=lambda c: c.name)
def test_plain_walk_over_compact_rows(answers, case):
    """k_walk_fast (k_walk_lanes in the old-walk leg) and k_ms_extend."""
    ix = _index(case, answers)
    ix.set_option("chunk_mode", 1)  # never: the plain walk
    d = ix.describe()
    assert d["compact_rows"] == 1 and d["flat_runs"] >= d["r"] == answers[case.name][2].r, d
    _held_to_the_mathematics(case, answers, ix)
    assert ix.last_chunk_stats()["chunk_len"] == 0
    ix.close()


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_general_rows(answers, case, monkeypatch):
    """The 16-byte rows, walked by k_walk_lanes."""
    monkeypatch.setenv("SPX_ROWS_WIDE", "1")
    ix = _index(case, answers)
    d = ix.describe()
    assert d["compact_rows"] == 0 and d["flat_runs"] == d["r"], d
    _held_to_the_mathematics(case, answers, ix)
    ix.close()


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_every_slot_escaped(answers, case, monkeypatch):
    """No fat slot holds its landing row: every jump goes on to the row itself."""
    monkeypatch.setenv("SPX_FAT_ALL_ESC", "1")
    ix = _index(case, answers)
    assert os.environ["SPX_FAT_ALL_ESC"] == "1" and ix.describe()["compact_rows"] == 1
    ix.set_option("chunk_mode", 1)
    _held_to_the_mathematics(case, answers, ix)
    ix.close()


@pytest.mark.parametrize("chunk_len", [32, 128])
@pytest.mark.parametrize("name", ms_cases.LONG_READS)
def test_chunked_walk(answers, name, chunk_len):
    """Chunks walked speculatively and joined: every case with a read of 1 000 characters or more -- the whole text of
    65 535 as one read (some 2 000 chunks of 32 through the 16-bit entry point at its limit) and the reads of 65 536 and
    66 120 that it refuses among them."""
    case = ms_cases.BY_NAME[name]
    ix = _index(case, answers)
    assert ix.describe()["compact_rows"] == 1  # (an index with general rows is never chunked)
    ix.set_option("chunk_mode", 2)
    ix.set_option("chunk_len", chunk_len)
    text, _, _, seqs, offs, ms = answers[name]
    narrow = int(np.diff(offs).max()) < 65536
    if not narrow:  # the chunked pass has a refusal of its own for the 16-bit entry point
        with pytest.raises(capi.SpxError):
            ix.query_host(capi.SPX_MODE_MS, seqs, offs, bits=16)
    for bits in (32, 16) if narrow else (32,):
        got = ix.query_host(capi.SPX_MODE_MS, seqs, offs, bits=bits)
        cs = ix.last_chunk_stats()
        assert cs["chunk_len"] == chunk_len, cs
        print(name, chunk_len, bits, "fallback_reads", cs["fallback_reads"], "rewalked_chars", cs["rewalked_chars"])
        pml = ix.query_host(capi.SPX_MODE_PML, seqs, offs, bits=bits)["lengths"]
        assert ix.last_chunk_stats()["chunk_len"] == chunk_len
        ms_cases.check_answers(case, got["lengths"], got["pointers"], pml=pml)
    ix.close()


def test_reads_dealt_on_demand(answers):
    """More reads than the launch has lanes (one block of 256 threads per CU at waves_per_cu = 4): k_walk_fast deals only
    the first round by lane index, the wavefronts claim the rest."""
    case = ms_cases.BY_NAME["dealt_on_demand"]
    ix = _index(case, answers)
    ix.set_option("waves_per_cu", 4)
    ix.set_option("chunk_mode", 1)
    lanes = torch.cuda.get_device_properties(0).multi_processor_count * 256
    assert answers[case.name][4].size - 1 >= 2 * lanes + 65 and ix.describe()["compact_rows"] == 1
    _held_to_the_mathematics(case, answers, ix)
    ix.close()


@pytest.mark.parametrize("pieces", [True, False])
def test_run_of_2_to_the_16_as_pieces_and_whole(answers, pieces, monkeypatch):
    """A BWT run of 2^16 positions and more does not fit a compact row's 16-bit length: it is cut into pieces, or -- with
    SPX_NO_PIECES -- the index takes the general rows."""
    case = ms_cases.BY_NAME["pieces_run_of_66000"]
    if not pieces:
        monkeypatch.setenv("SPX_NO_PIECES", "1")
    ix = _index(case, answers)
    d = ix.describe()
    if pieces:
        assert d["flat_runs"] > d["r"] and d["compact_rows"] == 1, d
    else:
        assert d["flat_runs"] == d["r"] and d["compact_rows"] == 0, d
    _held_to_the_mathematics(case, answers, ix)
    ix.close()


def test_match_past_16_bits_takes_the_32_bit_entry_point(answers):
    """A read of 66 120 characters with a match of 66 000: the 16-bit entry point refuses the batch (asserted in
    _held_to_the_mathematics), k_ms_extend stores that read's lengths one by one, and some exceed 65 535."""
    case = ms_cases.BY_NAME["match_of_66000"]
    ix = _index(case, answers)
    assert _held_to_the_mathematics(case, answers, ix) is False
    _, _, _, seqs, offs, _ = answers[case.name]
    assert int(ix.query_host(capi.SPX_MODE_MS, seqs, offs)["lengths"].max()) >= 65536
    ix.close()


@pytest.mark.parametrize("case", ms_cases.CASES, ids=lambda c: c.name)
def test_text_rebuilt_from_the_index(answers, case):
    """rebuild_text() on an index made without a text: the text, byte for byte, and the queries over it."""
    text = answers[case.name][0]
    ix = _index(case, answers, with_text=False)
    ix.rebuild_text()
    assert np.array_equal(ix.text(), text)
    if case.name in SMALL_NAMES:
        _held_to_the_mathematics(case, answers, ix)
    ix.close()


@pytest.mark.parametrize("name", ["repetitive_65536", "binary_tied_minima", "pieces_run_of_66000"])
def test_hip_builder_end_to_end(answers, name):
    """The index from capi.build_raw(text, doc_lengths) instead of the first-principles one: the same assertions."""
    case = ms_cases.BY_NAME[name]
    text, docs, ref, _, _, _ = answers[name]
    raw = capi.build_raw(text, doc_lengths=docs)
    assert ref.mismatches(raw) == []
    ix = capi.Index.from_raw(raw, 0)  # (with raw.text: set in the checked form)
    assert np.array_equal(ix.text(), text)
    _held_to_the_mathematics(case, answers, ix)
    ix.close()


@pytest.mark.parametrize("name", ["repetitive_4096", "acgtn_30000"])
def test_maximal_matches_are_those_of_the_true_ms(answers, name):
    """mems_host: the (read_pos, length) pairs of every read made of the text's letters are those of mems_reference over the
    TRUE matching statistics, and each ref_pos names an occurrence."""
    case = ms_cases.BY_NAME[name]
    text, _, _, seqs, offs, ms = answers[name]
    ix = _index(case, answers)
    ok = case.in_alphabet()
    for min_length in (1, 20):
        want_offs, want = mems_reference(ms, np.zeros(ms.size, dtype=np.uint64), offs, min_length)
        got_offs, got = ix.mems_host(seqs, offs.astype(np.uint64), min_length)[:2]
        assert int(want_offs[-1]) > 50
        for q in np.flatnonzero(ok).tolist():
            w = want[int(want_offs[q]): int(want_offs[q + 1])]
            g = got[int(got_offs[q]): int(got_offs[q + 1])]
            assert np.array_equal(g["read_pos"], w["read_pos"]) and np.array_equal(g["length"], w["length"]), (name, q, min_length)
            for rec in g:
                p, i, l = int(rec["ref_pos"]), int(offs[q]) + int(rec["read_pos"]), int(rec["length"])
                assert p + l <= text.size and np.array_equal(text[p: p + l], seqs[i: i + l]), (name, q, rec)
    ix.close()


def _values(path):
    """The value lines of an output file: one list per read."""
    return [[int(v) for v in ln.split()] for ln in open(path).read().splitlines() if not ln.startswith(">")]


def test_cli_build_then_run_holds_the_true_ms(answers, tmp_path):
    """`spumoni build -M -n` on a two-record FASTA, then `spumoni run -M -n`: the .lengths and .pointers files against the
    true MS over idx.fa.rawtext (the records and their reverse complements)."""
    assert os.path.exists(BIN)
    rng = np.random.default_rng(91)
    recs = [cases.repetitive_text(rng, n, ms_cases.DNA) for n in (3000, 2001)]
    with open(tmp_path / "x.fa", "w") as f:
        for i, g in enumerate(recs):
            f.write(f">rec{i}\n")
            s = g.tobytes().decode()
            f.writelines(s[j: j + 70] + "\n" for j in range(0, len(s), 70))
    ref_prefix = str(tmp_path / "idx")
    r = subprocess.run([BIN, "build", "-r", str(tmp_path / "x.fa"), "-o", ref_prefix, "-M", "-n"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    text = np.fromfile(ref_prefix + ".fa.rawtext", dtype=np.uint8)
    assert text.size == 2 * (3000 + 2001) and np.array_equal(text[:3000], recs[0])
    sa = brute.BruteIndex(text).sa
    letters = np.unique(text)
    reads = [ms_cases._substring(rng, text, m, rate, letters) for rate in ms_cases.RATES for m in ms_cases.LENGTHS[1:]]
    reads += [text[text.size - k:].copy() for k in ms_cases.SUFFIXES] + [recs[1][::-1].copy()]
    seqs, offs = ms_cases.batch(reads)
    ms = brute.brute_ms(text, sa, seqs, offs)
    assert int(ms.max()) >= 500
    with open(tmp_path / "reads.fa", "w") as f:
        for q, rd in enumerate(reads):
            f.write(f">read_{q}\n{rd.tobytes().decode()}\n")
    env = dict(os.environ)
    env.pop("SPUMONI_TEXT", None)  # the text is rebuilt from the index
    r = subprocess.run([BIN, "run", "-r", ref_prefix, "-p", str(tmp_path / "reads.fa"), "-M", "-n"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    lengths, pointers = _values(str(tmp_path / "reads.fa") + ".lengths"), _values(str(tmp_path / "reads.fa") + ".pointers")
    assert len(lengths) == len(pointers) == len(reads)
    L, P = np.concatenate([np.asarray(v, dtype=np.int64) for v in lengths]), np.concatenate([np.asarray(v, dtype=np.uint64) for v in pointers])
    assert L.size == ms.size and np.array_equal(L, ms)
    assert ms_cases.occurrences_wrong(text, seqs, offs, L, P, np.ones(len(reads), dtype=bool)) == []
