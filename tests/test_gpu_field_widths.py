"""-m gpu: every packed field of the flat layout at its full width -- n at the 40-bit limit, 16-bit document ids.

The other GPU tests vary the index's SHAPE; their offsets stay below 2^18 and their document ids below 200.  Here the
index (tests/cases.py: wide_case) has 3000 runs, some 150 of them 2^16 .. 2^35 positions long and one of 2^39 .. 2^39.1 (half
of all positions: a 40-bit length, offsets with bits 38 and 39 set), and exactly
n = 2^40 - 3 positions: the largest BWT the flatten step accepts.  The walk never expands positions, so this costs the
oracle milliseconds and the device a gigabyte (the long runs become 1.7 * 10^7 pieces of the compact encoding).  Samples
are drawn from [0, n) and document ids from [0, 65536); n - 1, 0, the single bits 24 / 31 / 32 / 39 (the split of
samples_last across the two words of an Aux) and the ids 0, 255, 256, 32768, 65535 are written in by hand.

Every test first asserts on its inputs and on the ORACLE's answers that it reaches what it is for (cases.wide_reach):
longest run >= 2^39, the reference's walk visits an offset >= 2^38 inside a run (cases.walk_offsets), >= 90 % of the expected MS pointers >= 2^32 and one of 40 bits, >= 90 % of the expected document
ids >= 256 and one >= 2^15.  Measured on seeds 0 .. 11: pointers 93.1 - 97.0 % (the rest follow a letter the index
does not have, where the reference restarts from sample 0 and counts down below zero), document ids 95.5 - 99.6 %, longest
run 2^39.00 .. 2^39.06, the next 2^33.7 .. 2^34.9; 0.6 - 43 % of the visited positions lie at an offset >= 2^38.  The reference of every comparison is the oracle (tier T2, and tier T1 says the same)."""
import filecmp
import os

import numpy as np
import pytest
import torch

from spumoni_amd import capi
from tests import cases
from tests.test_gpu_parity import _compare_all
from tests.test_gpu_text import _expect, _fill

pytestmark = pytest.mark.gpu

# SPX_WIDE_SEEDS seeds from SPX_WIDE_FIRST on (default 0 .. 7; a longer sweep is a matter of two environment variables)
_FIRST = int(os.environ.get("SPX_WIDE_FIRST", "0"))
_SEEDS = range(_FIRST, _FIRST + int(os.environ.get("SPX_WIDE_SEEDS", "8")))
# The general rows -- the only encoding whose fields hold 40-bit offsets -- take every seed (0.05 s each).  A compact index
# costs 5.6 s: the flatten step cuts the run of 2^39 positions into 8.4 * 10^6 pieces in one thread, once per balancing
# pass.  Its rows hold 16-bit offsets whatever the seed, so it takes the first SPX_WIDE_COMPACT_SEEDS of them (3): with all
# eight the module and its old-walk leg would add a quarter to the suite's 12 min 39 s; as it is they add 108 s.
_COMPACT_SEEDS = _SEEDS[: int(os.environ.get("SPX_WIDE_COMPACT_SEEDS", "3"))]
_PARITY_CASES = [(s, "general") for s in _SEEDS] + [(s, "compact") for s in _COMPACT_SEEDS]


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    capi.lib()
    return 0


def _zero_threshold_that_is_not_a_first(raw):
    """Move the stored threshold of a letter's second run onto its first run and leave a zero behind: thr_bv skips zeros,
    so every run of the letter reads the value it read before (thresholds_ds.hpp:421-423, 484-488) -- but the run list
    now has a zero threshold that is not a letter's first, and the flatten step keeps the general row encoding itself."""
    h = raw.heads.numpy()
    for c in np.unique(h[h > 1]):
        ks = np.flatnonzero(h == c)
        if ks.size >= 3 and int(raw.thr[ks[1]]) > 0:
            raw.thr[ks[0]], raw.thr[ks[1]] = int(raw.thr[ks[1]]), 0
            return
    raise AssertionError("no letter with three runs")


def _wide(oracle_mod, seed, nreads=600, length=60):
    """(raw, letters, seqs, offs, orc, want): a wide index, its reads, the oracle and the oracle's answers; the vacuity
    asserts on both, and tier T1 against tier T2."""
    raw, letters = cases.wide_case(seed)
    seqs, offs = cases.wide_reads(raw, letters, seed, nreads, length)
    assert raw.n == cases.N_LIMIT == (1 << 40) - 3
    orc = oracle_mod.OracleIndex.from_raw(raw)
    want = orc.ms(seqs, offs, want_docs=True)
    want["pml"], want["pml_docs"] = orc.pml(seqs, offs, want_docs=True)
    reach = cases.wide_reach(raw, want, want["docs"])
    cases.wide_reach(raw, want, want["pml_docs"])
    visited = cases.walk_offsets(orc, raw, seqs, offs, nreads=100)
    assert (visited >= (1 << 38)).any(), "the walk never stands at an offset of 2^38 or more inside a run"
    t1 = oracle_mod.OracleT1Index.from_raw(raw)
    l1, d1 = t1.pml(seqs, offs, want_docs=True)
    m1 = t1.ms(seqs, offs, want_docs=True)
    assert np.array_equal(l1, want["pml"]) and np.array_equal(d1, want["pml_docs"])
    assert np.array_equal(m1["pointers"], want["pointers"]) and np.array_equal(m1["docs"], want["docs"])
    return raw, letters, seqs, offs, orc, want, reach


def _assert_encoding(ix, raw, encoding):
    d = ix.describe()
    assert d["r"] == raw.r
    if encoding == "compact":  # the long runs are laid out as pieces of < 2^16 positions
        pieces = int(((raw.lens + 65534) // 65535).sum())  # (more where an LF image is cut for the runs it covers)
        assert d["compact_rows"] == 1 and d["flat_runs"] >= pieces > raw.r + raw.n // 65536, d
    else:
        assert d["compact_rows"] == 0 and d["flat_runs"] == raw.r, d
    return d


def _set_encoding(monkeypatch, raw, encoding):
    if encoding == "general":
        monkeypatch.setenv("SPX_ROWS_WIDE", "1")
    elif encoding == "general_by_threshold":
        _zero_threshold_that_is_not_a_first(raw)


@pytest.mark.parametrize("seed,encoding", _PARITY_CASES)
def test_walk_parity_at_full_width(gpu, oracle_mod, seed, encoding, monkeypatch):
    """PML, PML + doc, MS pointers + doc, the 16- and 32-bit entry points and the classifier (test_gpu_parity:
    _compare_all) on an index of 2^40 - 3 positions with 65 536 documents: compact rows + pieces (k_walk_fast), and the
    general 16-byte rows with their 40-bit fields (k_walk_lanes)."""
    raw, letters, seqs, offs, orc, want, _ = _wide(oracle_mod, seed)
    _set_encoding(monkeypatch, raw, encoding)
    ix = capi.Index.from_raw(raw, 0)
    _assert_encoding(ix, raw, encoding)
    assert ix.n == raw.n
    _compare_all(oracle_mod, raw, None, seqs, offs, ix=ix)
    ix.close()


@pytest.mark.parametrize("seed", [1, 2])
def test_general_rows_chosen_by_the_flatten_step(gpu, oracle_mod, seed):
    """A zero threshold that is not a letter's first forbids pieces: the flatten step keeps the general encoding without
    being told to (no environment switch here), the run of 2^39 positions and all."""
    raw, letters = cases.wide_case(seed)
    _zero_threshold_that_is_not_a_first(raw)
    seqs, offs = cases.wide_reads(raw, letters, seed)
    orc = oracle_mod.OracleIndex.from_raw(raw)
    want = orc.ms(seqs, offs, want_docs=True)
    cases.wide_reach(raw, want, want["docs"])
    assert "SPX_ROWS_WIDE" not in os.environ
    ix = capi.Index.from_raw(raw, 0)
    _assert_encoding(ix, raw, "general")
    _compare_all(oracle_mod, raw, None, seqs, offs, ix=ix)
    ix.close()


@pytest.mark.parametrize("knob", ["all_esc", "thin_table"])
@pytest.mark.parametrize("encoding", ["compact", "general"])
def test_full_jump_rows_answer_at_full_width(gpu, oracle_mod, encoding, knob, monkeypatch):
    """Every fat digest marked as not holding its row (SPX_FAT_ALL_ESC=1), and a table of 0.3 slots per run whose
    slots mostly name a run before the walk's: the jumps are answered from the full JumpRow, with its 40-bit THRoff and
    sLFoff, through fat_j and through the directory scan."""
    if knob == "all_esc":
        monkeypatch.setenv("SPX_FAT_ALL_ESC", "1")
    else:
        monkeypatch.setenv("SPX_FAT_SLOTS_PER_RUN", "0.3")
    raw, letters, seqs, offs, orc, want, _ = _wide(oracle_mod, 3)
    _set_encoding(monkeypatch, raw, encoding)
    ix = capi.Index.from_raw(raw, 0)
    _assert_encoding(ix, raw, encoding)
    _, st = _compare_all(oracle_mod, raw, None, seqs, offs, ix=ix)
    assert st["jumps"] > 1000
    ix.close()


@pytest.mark.parametrize("encoding", ["compact", "general"])
def test_chunked_walk_at_full_width(gpu, oracle_mod, encoding, monkeypatch):
    """Reads of 2500 characters.  On the compact index they are cut into chunks that are walked concurrently and joined
    (the checkpoints between the passes carry run and offset; the offsets are those of pieces, below 2^16, while the run
    index has 25 bits).  An index with general rows is never chunked: there the same reads are walked whole, 2500 steps
    of one lane each, through the run of 2^39 positions."""
    raw, letters, seqs, offs, orc, want, _ = _wide(oracle_mod, 4, nreads=12, length=2500)
    _set_encoding(monkeypatch, raw, encoding)
    ix = capi.Index.from_raw(raw, 0)
    _assert_encoding(ix, raw, encoding)
    ix.set_option("chunk_mode", 2)
    got = ix.query_host(capi.SPX_MODE_PML, seqs, offs, classify=(150, 5))
    if encoding == "compact":  # (launch_walk_chunked declines an index with general rows: there the same long reads are
        # walked whole by k_walk_lanes, 2500 steps with 40-bit offsets on one lane each)
        assert ix.last_chunk_stats()["chunk_len"] > 0, "the long-read batch did not take the chunked walk"
    assert np.array_equal(got["lengths"], want["pml"])
    _, a, b, s = oracle_mod.classify(want["pml"], offs, 150, 5)
    assert np.array_equal(got["class"]["above"], a) and np.array_equal(got["class"]["sum_max"], s)
    got = ix.query_host(capi.SPX_MODE_PML, seqs, offs, want_docs=True)
    assert encoding != "compact" or ix.last_chunk_stats()["chunk_len"] > 0
    assert np.array_equal(got["lengths"], want["pml"]) and np.array_equal(got["docs"], want["pml_docs"])
    got = ix.query_host(capi.SPX_MODE_MS, seqs, offs, want_lengths=False, want_docs=True)
    assert np.array_equal(got["pointers"], want["pointers"]) and np.array_equal(got["docs"], want["docs"])
    ix.close()


def _digits(v):
    return len(str(int(v)))


@pytest.mark.parametrize("encoding", ["compact", "general"])
def test_text_on_the_device_at_full_width(gpu, oracle_mod, encoding, monkeypatch):
    """spx_text.hip on 64-bit values that need them: pointers of 13 digits (and the 20 digits of a pointer that was
    counted down below zero), document ids of 5 digits, and a values line on which 1-, 5- and 13-digit values alternate
    across the 64-value boundary of a wavefront's pass."""
    raw, letters, seqs, offs, orc, want, _ = _wide(oracle_mod, 5, nreads=200, length=150)
    _set_encoding(monkeypatch, raw, encoding)
    ids = [b"read_%d%s" % (q, b" descr" * (q % 3)) for q in range(offs.size - 1)]
    gap = np.array([len(i) + 2 for i in ids], dtype=np.uint32)
    ix = capi.Index.from_raw(raw, 0)
    _assert_encoding(ix, raw, encoding)
    exp_p, exp_d = _expect(want["pointers"], offs, ids), _expect(want["docs"], offs, ids)
    ptr = want["pointers"].astype(np.uint64)
    assert max(_digits(v) for v in ptr[ptr < (1 << 63)]) == 13 and _digits(want["docs"].max()) == 5
    assert 1 in {_digits(v) for v in want["docs"]}
    got = ix.query_text(capi.SPX_MODE_MS, seqs, offs, gap, capi.SPX_TEXT_POINTERS | capi.SPX_TEXT_DOCS)
    assert got["text"][0] is None
    assert _fill(got["text"][1], got["line_start"][1], ids) == exp_p
    assert _fill(got["text"][2], got["line_start"][2], ids) == exp_d
    lens, docs = want["pml"], want["pml_docs"]
    got = ix.query_text(capi.SPX_MODE_PML, seqs, offs, gap, capi.SPX_TEXT_LENGTHS | capi.SPX_TEXT_DOCS)
    assert _fill(got["text"][0], got["line_start"][0], ids) == _expect(lens, offs, ids)
    assert _fill(got["text"][2], got["line_start"][2], ids) == _expect(docs, offs, ids)
    # values lines on which the digit counts alternate around the 64th value, where the wavefront's second pass
    # continues the line: 1 and 13 (or 20) digits among the pointers, 1 and 5 among the document ids
    def around_64(vals, small, large):
        w = [_digits(v) for v in vals[56:72]]
        return min(w) <= small and max(w) >= large
    rd = [slice(offs[q], offs[q + 1]) for q in range(offs.size - 1)]
    assert any(around_64(ptr[q], 1, 13) for q in rd), "no pointers line mixes 1 and 13 digits around its 64th value"
    assert any(around_64(want["docs"][q], 1, 5) for q in rd), "no document line mixes 1 and 5 digits around its 64th value"
    ix.close()


@pytest.mark.parametrize("encoding", ["compact", "general"])
def test_cache_and_clone_at_full_width(gpu, oracle_mod, tmp_path, encoding, monkeypatch):
    """.spx cache: save -> load_flat -> save gives the same bytes and the same answers; a same-device clone answers the
    same after its source is closed."""
    raw, letters, seqs, offs, orc, want, _ = _wide(oracle_mod, 6)
    _set_encoding(monkeypatch, raw, encoding)
    fresh = capi.Index.from_raw(raw, 0)
    _assert_encoding(fresh, raw, encoding)
    a, b = str(tmp_path / "a.spx"), str(tmp_path / "b.spx")
    fresh.save(a)
    desc = fresh.describe()
    dup = fresh.clone(0)
    assert dup.describe() == desc
    fresh.close()  # the clone owns its arrays
    _compare_all(oracle_mod, raw, None, seqs, offs, ix=dup)
    dup.close()
    loaded = capi.Index.load_flat(a, 0)
    assert (loaded.n, loaded.r) == (raw.n, raw.r) and loaded.describe() == desc
    loaded.save(b)
    assert filecmp.cmp(a, b, shallow=False), "cache of a loaded index differs from the cache of the fresh one"
    os.remove(b)
    _compare_all(oracle_mod, raw, None, seqs, offs, ix=loaded)
    loaded.close()
    os.remove(a)


@pytest.mark.parametrize("encoding", ["compact", "general"])
def test_raw_files_at_full_width(gpu, oracle_mod, tmp_path, encoding, monkeypatch):
    """spx_index_load_raw on .bwt.len / .thr_pos / .ssa / .esa files whose 5-byte entries use all 40 bits, flattened
    into either encoding.  (The raw files hold no document array: lengths and pointers are what there is to compare.)"""
    raw, letters, seqs, offs, orc, want, _ = _wide(oracle_mod, 7)
    _set_encoding(monkeypatch, raw, encoding)
    prefix = str(tmp_path / "idx")
    raw.write_raw_files(prefix)
    ix = capi.Index.load_raw(prefix, capi.SPX_MODE_PML, 0)
    assert (ix.n, ix.r) == (raw.n, raw.r)
    _assert_encoding(ix, raw, encoding)
    assert np.array_equal(ix.query_host(capi.SPX_MODE_PML, seqs, offs)["lengths"], want["pml"])
    ix.close()
    ix = capi.Index.load_raw(prefix, capi.SPX_MODE_MS, 0)
    assert (ix.n, ix.r) == (raw.n, raw.r)
    _assert_encoding(ix, raw, encoding)
    got = ix.query_host(capi.SPX_MODE_MS, seqs, offs, want_lengths=False)
    assert np.array_equal(got["pointers"], orc.ms(seqs, offs)["pointers"])
    ix.close()
