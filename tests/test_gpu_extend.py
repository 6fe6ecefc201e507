"""-m gpu: the extended CIGARs (spumoni_amd/csrc/spx_extend.hip, include/spumoni_extend.h) against the definition
(spumoni_amd/extend.py: extend_reference), bit for bit: the records, the ends, the op offsets and every entry.

extend_device gets crafted reads, anchors, chains and pred (tests/test_gpu_align.py's Batch, with both ends of a read grown)
on an index whose text is handed in; extend_host is held to the oracle's MS arrays -> mems_reference -> chain_reference ->
extend_reference, and `spumoni extend` to the same over the committed golden files.  An end is one wavefront's table, two
diagonals of the band a lane; its trace stands in LDS up to 2048 words (ceil(a / 16) * (2 * band + 1)) and in device memory
above: the crafted ends lie around 1, 16, 64 and 128 rows, at max_extend and one above, and on both sides of 2048 words."""
import os
import shutil

import numpy as np
import pytest
import torch

from spumoni_amd import capi, synth
from spumoni_amd.align import ALIGN_DTYPE, UNALIGNED, AlignParams
from spumoni_amd.chain import CHAIN_DTYPE, ChainParams, chain_reference
from spumoni_amd.cigar import OP_D, OP_EQ, OP_I, OP_X, cigar_reference
from spumoni_amd.extend import END_DTYPE, OP_S, ExtendParams, cigar_text, extend_reference
from spumoni_amd.mems import MATCH_DTYPE, mems_reference
from tests import cases
from tests.test_chain_cpu import planted_reads
from tests.test_extend_cpu import check_invariants
from tests.test_gpu_align import (DNA, FENCE, FILES, K, LETTERS, N_TEXT, RUN_A, UNALIGNED_REC, W, Batch, _bad_batch, _cli, _parse_values,
                                  _sequences)
from tests.test_gpu_cigar import _spoil

pytestmark = pytest.mark.gpu
NO_END = (0, 0, 0, 0)


@pytest.fixture(scope="module")
def gpu(built_all):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    capi.lib()
    return 0


@pytest.fixture(scope="module")
def text():
    t = LETTERS[np.random.default_rng(100).integers(0, 4, N_TEXT)].copy()
    t[RUN_A:RUN_A + 5000] = ord("A")
    return t


def _index_with(text):
    ix = capi.Index.from_raw(synth.statistical_rlbwt(5000, 60, 4.0, seed=3, with_samples=True, n_docs=8), 0)
    ix.set_text(torch.from_numpy(text.copy()), unchecked=True)
    return ix


@pytest.fixture(scope="module")
def text_index(gpu, text):
    """Any index, with the crafted text handed in: the kernels read the text and nothing else of the index."""
    ix = _index_with(text)
    yield ix
    ix.close()


def noisy(rng, seg, rate):
    """seg with a share of its characters replaced, dropped or doubled."""
    u = rng.random(seg.size)
    parts = [np.r_[c, c] if x < rate / 3 else (LETTERS[rng.integers(0, 4, 1)] if x < 2 * rate / 3 else np.array([c], dtype=np.uint8))
             for c, x in zip(seg, u) if x > rate / 4]
    return np.concatenate(parts + [seg[:0]]).astype(np.uint8)


class Ends(Batch):
    """Batch whose reads go on beyond their chain: `left` and `right` characters of the text's neighbourhood, noisy."""

    def add_ends(self, text, rng, y0, gaps, left, right, rate=0.06, lengths=None):
        h = len(gaps) + 1
        self.add(text, rng, y0, gaps, lengths)
        core = self.reads.pop()
        y1 = self.anchors[-1][1] + self.anchors[-1][2]
        L = noisy(rng, text[max(y0 - left - 8, 0):y0], rate)[::-1]
        L = np.resize(L, left)[::-1] if L.size else LETTERS[rng.integers(0, 4, left)]
        R = noisy(rng, text[y1:y1 + right + 8], rate)
        R = np.resize(R, right) if R.size else LETTERS[rng.integers(0, 4, right)]
        self.reads.append(np.r_[L, core, R].astype(np.uint8))
        self.anchors[-h:] = [(x + left, y, l) for x, y, l in self.anchors[-h:]]


def _generous(arrays):
    R, roffs, rec, moffs, chains, pred = arrays
    return 2 * R.size + 2 * rec.size + 3 * moffs.size + 64


def _run(ix, arrays, params=None, ep=None, cap=None, op_cap=None, ends=True):
    """extend_device with every output fenced; returns (records, op_offsets, entries, ends) -- entries up to min(total, op_cap)."""
    R, roffs, rec, moffs, chains, pred = arrays
    nreads = moffs.size - 1
    n = rec.size
    d_R = torch.from_numpy(np.r_[R, np.zeros(8, dtype=np.uint8)]).cuda()
    d_roffs = torch.from_numpy(np.asarray(roffs, dtype=np.uint64).view(np.int64).copy()).cuda()
    d_rec = torch.from_numpy(np.concatenate([rec, np.zeros(1, dtype=MATCH_DTYPE)]).view(np.int32).reshape(-1, 4).copy()).cuda()[:n]
    d_moffs = torch.from_numpy(np.asarray(moffs, dtype=np.uint64).view(np.int64).copy()).cuda()
    d_chains = torch.from_numpy(np.concatenate([chains, np.zeros(1, dtype=CHAIN_DTYPE)]).view(np.int32).reshape(-1, 12).copy()).cuda()[:nreads]
    d_pred = torch.from_numpy(np.r_[pred, np.zeros(1, dtype=np.uint32)].view(np.int32).copy()).cuda()[:n]
    cap = n if cap is None else cap
    op_cap = _generous(arrays) if op_cap is None else op_cap
    fenced = torch.full((nreads + 3, 12), FENCE, dtype=torch.int32, device="cuda")
    d_ooffs = torch.full((nreads + 1 + 4,), FENCE, dtype=torch.int64, device="cuda")
    d_ops = torch.full((op_cap + 4,), FENCE, dtype=torch.int32, device="cuda")
    d_ends = torch.full((2 * nreads + 4, 4), FENCE, dtype=torch.int32, device="cuda") if ends else None
    out, _, _, _ = ix.extend_device(d_R, d_roffs, d_rec, d_moffs, d_chains, d_pred, params, ep, gap_capacity=cap, op_capacity=op_cap,
                                    d_out=fenced[:nreads], d_out_op_offsets=d_ooffs, d_out_ops=d_ops, d_out_ends=d_ends, want_ends=ends)
    torch.cuda.synchronize()
    assert (fenced[nreads:] == FENCE).all().item()
    records = out.cpu().numpy().view(ALIGN_DTYPE).reshape(-1)
    ooffs = d_ooffs.cpu().numpy()
    assert (ooffs[nreads + 1:] == FENCE).all()
    ooffs = ooffs[:nreads + 1].view(np.uint64)
    fit = ooffs[1:][ooffs[1:] <= op_cap]
    written = int(fit.max(initial=0))
    ops = d_ops.cpu().numpy()
    assert (ops[written:] == FENCE).all()  # nothing is written past the reads that fit (or past the capacity)
    got_ends = None
    if ends:
        e = d_ends.cpu().numpy()
        assert (e[2 * nreads:] == FENCE).all()
        got_ends = e[:2 * nreads].copy().view(END_DTYPE).reshape(-1)
    return records, ooffs, ops[:written].copy().view(np.uint32), got_ends


def _check(ix, text, arrays, params=None, ep=None, ref=None):
    R, roffs, rec, moffs, chains, pred = arrays
    if ref is None:
        count = {}
        ref = extend_reference(R, roffs, text, moffs, rec, chains, pred, params, ep, count=count) + (count,)
    want, w_ooffs, w_ops, w_ends, count = ref
    got, ooffs, ops, ends = _run(ix, arrays, params, ep)
    bad = np.flatnonzero(ends != w_ends)
    assert bad.size == 0, (ep, bad[:5], ends[bad[:5]], w_ends[bad[:5]])
    assert np.array_equal(ooffs, w_ooffs), (ep, np.flatnonzero(ooffs != w_ooffs)[:5])
    bad = np.flatnonzero(ops != w_ops)
    assert bad.size == 0, (ep, bad[:5], ops[bad[:5]], w_ops[bad[:5]])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (ep, bad[:5], got[bad[:5]], want[bad[:5]])
    st = ix.extend_stats()
    ok = want["ref_start"] != np.uint64(UNALIGNED)
    assert st["reads"] == moffs.size - 1 and st["aligned_reads"] == int(ok.sum()) and st["entries"] == w_ops.size, st
    assert (st["ends"], st["extended_ends"], st["band_cells"], st["clipped"]) == (count["ends"], count["extended"], count["cells"],
                                                                                   count["clipped"]), (st, count)
    assert st["error"] == 0 and st["overflow"] == 0 and len(st["step_ms"]) == 6, st
    return ref


SIDES = [0, 1, 2, 15, 16, 17, 63, 64, 65, 129, 512, 513]  # none, around a trace word of 16 rows and a wavefront, max_extend, one above


@pytest.mark.parametrize("alphabet", [b"ACGT", b"AC"], ids=["four_letters", "two_letters"])
def test_every_end_side_left_right_both_and_mixed(gpu, text, text_index, alphabet):
    """Over two letters the text is a copy with G -> A and T -> C: ties are everywhere."""
    rng = np.random.default_rng(len(alphabet))
    fold = np.arange(256, dtype=np.uint8)
    if len(alphabet) == 2:
        fold[ord("G")], fold[ord("T")] = ord("A"), ord("C")
        text = fold[text]
        ix = _index_with(text)
    else:
        ix = text_index
    B = Ends(front=3)
    for s in SIDES:
        B.add_ends(text, rng, int(rng.integers(1000, 900_000)), [(3, 4)], s, 0)
        B.add_ends(text, rng, int(rng.integers(1000, 900_000)), [], 0, s)
        B.add_ends(text, rng, int(rng.integers(1000, 900_000)), [(20, 18), (1, 1)], s, s)
    for l, r in zip(SIDES, rng.permutation(SIDES)):
        B.add_ends(text, rng, int(rng.integers(1000, 900_000)), [(2, 2)], int(l), int(r), rate=0.15)
        B.add_empty()
    arrays = B.arrays()
    arrays = (fold[arrays[0]],) + arrays[1:]
    want, ooffs, ops, ends, count = _check(ix, text, arrays)
    assert {int(e) & 15 for e in ops} == {OP_EQ, OP_X, OP_I, OP_D, OP_S} and count["extended"] > 50
    check_invariants(want, ooffs, ops, arrays[0], arrays[1], text)  # (the reference's own test; here it guards the crafted input)
    assert int(ends["read_chars"].max()) == 512  # an end of 513 is cut at max_extend, and the noise is crossed
    _check(ix, text, arrays, AlignParams(4), ExtendParams(512, 3, 1, 1))
    if len(alphabet) == 2:
        ix.close()


@pytest.mark.parametrize("band", [0, 1, 15, 16, 31, 32, 63])
def test_bands(gpu, text, text_index, band):
    rng = np.random.default_rng(band)
    B = Ends()
    for s in (1, 5, 40, 100, 200, 263):  # (263 rows at band 63 are 17 * 127 = 2159 words: the trace leaves LDS)
        B.add_ends(text, rng, int(rng.integers(1000, 900_000)), [(2, 3)], s, s, rate=0.12)
    for ep in (ExtendParams(512, band, 4, 6), ExtendParams(512, band, 1, 1)):
        _, _, _, ends, _ = _check(text_index, text, B.arrays(), None, ep)
        assert (np.abs(ends["read_chars"].astype(np.int64) - ends["text_chars"].astype(np.int64)) <= band).all()


@pytest.mark.parametrize("max_extend", [1, 16, 512, 4096])
def test_max_extend_with_ends_at_the_limit_and_one_above(gpu, text, text_index, max_extend):
    """At 4096 and band 63 one end's trace is 256 * 127 words in device memory."""
    rng = np.random.default_rng(max_extend)
    m = max_extend
    band = 63 if m == 4096 else 16
    B = Ends(front=1)
    if m == 4096:  # (two large ends: the rule's plain loops take a second each)
        B.add_ends(text, rng, 100_000, [(2, 2)], 17, m, rate=0.02)
        B.add_ends(text, rng, 300_000, [], m + 1, 17, rate=0.02)
    else:
        B.add_ends(text, rng, 100_000, [(2, 2)], m, m + 1, rate=0.02)
        B.add_ends(text, rng, 300_000, [], m + 1, min(m, 40), rate=0.02)
    if m == 512:
        B.add_ends(text, rng, 500_000, [], 0, 512, rate=0.0)
    want, ooffs, ops, ends, count = _check(text_index, text, B.arrays(), None, ExtendParams(m, band, 4, 6))
    assert int(ends["read_chars"].max()) <= m and count["ends"] >= 4
    assert count["clipped"] >= 1  # (the character beyond max_extend)
    if m == 4096:
        assert int(ends["read_chars"].max()) > 4000 and text_index.extend_stats()["band_cells"] > 2 * 4000 * 127


@pytest.mark.parametrize("costs", [(0, 0), (1, 1), (4, 6), (65535, 65535), (0, 65535)])
def test_costs(gpu, text, text_index, costs):
    rng = np.random.default_rng(sum(costs))
    fold = np.arange(256, dtype=np.uint8)
    fold[ord("G")], fold[ord("T")] = ord("A"), ord("C")
    B = Ends()
    for s in (3, 17, 70, 300):
        B.add_ends(text, rng, int(rng.integers(1000, 900_000)), [(1, 2)], s, s, rate=0.2)
    B.add_ends(text, rng, 40_000, [], 4096, 4096, rate=0.3)  # the lowest cells: 8192 steps of 65535 stay above -2^30
    _check(text_index, text, B.arrays(), None, ExtendParams(4096, 7, *costs))
    two = _index_with(fold[text])
    arrays = B.arrays()
    _check(two, fold[text], (fold[arrays[0]],) + arrays[1:], None, ExtendParams(512, 16, *costs))
    two.close()


def test_closed_forms_and_the_texts_edges(gpu, text, text_index):
    """An end of 4096 equal characters merges with its anchor into one '=' run; an end of all-unequal characters is clipped
    whole; at the text's first and last character nothing before T[0] or behind T[n - 1] is read."""
    B = Batch()
    n = N_TEXT
    other = np.zeros(256, dtype=np.uint8)
    other[LETTERS] = np.roll(LETTERS, 1)
    B.reads = [text[200_000:204_116].copy(),                                    # 4096 equal characters behind a 20-character anchor
               text[300_000:304_116].copy(),                                    # ... and in front of one
               np.r_[other[text[400_000:400_100]], text[400_100:400_120], other[text[400_120:400_220]]],  # all unequal on both sides
               text[0:60].copy(),                                               # the text's first character, by extension
               np.r_[LETTERS[[0, 1, 2]], text[0:30]],                           # ref_start = 0: three characters clipped
               text[n - 50:n].copy(),                                           # the text's last character, by extension
               np.r_[text[n - 30:n], LETTERS[[3, 2]]],                          # ref_end = n_text
               np.r_[text[3:20], text[20:40]]]                                  # ref_start = 3 < a + band
    B.anchors = [(0, 200_000, 20), (4096, 304_096, 20), (100, 400_100, 20), (20, 20, 20), (3, 0, 30), (10, n - 40, 20), (0, n - 30, 30),
                 (17, 20, 20)]
    B.counts = [1] * 8
    arrays = B.arrays()
    ep = ExtendParams(4096, 16, 4, 6)
    got, ooffs, ops, ends = _run(text_index, arrays, None, ep)
    cigars = [cigar_text(ops[int(ooffs[q]):int(ooffs[q + 1])]) for q in range(8)]
    assert cigars == ["4116=", "4116=", "100S20=100S", "60=", "3S30=", "50=", "30=2S", "37="], cigars
    assert ends.tolist() == [NO_END, (4096, 4096, 4096, 0), (4096, 4096, 4096, 0), NO_END, NO_END, NO_END, (20, 20, 20, 0), (20, 20, 20, 0),
                             NO_END, NO_END, (10, 10, 10, 0), (20, 20, 20, 0), NO_END, NO_END, (17, 17, 17, 0), NO_END]
    assert [(int(r["ref_start"]), int(r["ref_end"]), int(r["read_start"]), int(r["read_end"])) for r in got[3:7]] == \
        [(0, 60, 0, 60), (0, 30, 3, 33), (n - 50, n, 0, 50), (n - 30, n, 0, 30)]
    _check(text_index, text, arrays, None, ep)
    st = text_index.extend_stats()
    assert st["clipped"] == 205 and st["extended_ends"] == 7 and st["ends"] == 11, st


@pytest.mark.parametrize("nreads", [0, 1, 63, 64, 65, 3000])
def test_read_counts_around_the_wavefront(gpu, text, text_index, nreads):
    rng = np.random.default_rng(nreads)
    B = Ends(front=nreads % 3)
    for q in range(nreads):
        h = int(rng.integers(0, 4))
        if h:
            B.add_ends(text, rng, int(rng.integers(1000, 900_000)), [(int(a), int(b)) for a, b in rng.integers(0, 20, (h - 1, 2))],
                       int(rng.integers(0, 30)), int(rng.integers(0, 30)), rate=0.1)
        else:
            B.add_empty()
    _check(text_index, text, B.arrays())
    if nreads == 65:
        assert _run(text_index, B.arrays(), ends=False)[3] is None  # the ends are on request


def _capacity_batch(text):
    rng = np.random.default_rng(6)
    B = Ends()
    for gaps in ([(3, 4), (20, 20)], [], [(5, 5)], [(2, 2), (1, 1), (0, 3)]):
        B.add_ends(text, rng, int(rng.integers(1000, 900_000)), gaps, 25, 30, rate=0.1)
    return B.arrays()


def test_op_capacity_zero_short_exact_and_above(gpu, text, text_index):
    arrays = _capacity_batch(text)
    want, w_ooffs, w_ops, w_ends = extend_reference(arrays[0], arrays[1], text, arrays[3], arrays[2], arrays[4], arrays[5])
    total = int(w_ooffs[-1])
    assert (np.diff(w_ooffs.astype(np.int64)) >= 1).all() and total > 12
    for op_cap in (0, total - 1, int(w_ooffs[2]) + 1, int(w_ooffs[1]), total, total + 9):
        got, ooffs, ops, ends = _run(text_index, arrays, op_cap=op_cap)
        assert np.array_equal(ooffs, w_ooffs), op_cap
        fits = w_ooffs[1:] <= op_cap
        assert np.array_equal(got[fits], want[fits]) and all(r.tolist() == UNALIGNED_REC for r in got[~fits]), op_cap
        assert np.array_equal(ends, np.where(np.repeat(fits, 2), w_ends, np.zeros(1, dtype=END_DTYPE))), op_cap
        whole = int(w_ooffs[1:][fits].max(initial=0))
        assert ops.size == whole and np.array_equal(ops, w_ops[:whole]), op_cap
        st = text_index.extend_stats()
        assert st["overflow"] == int(not fits.all()) and st["error"] == 0 and st["aligned_reads"] == int(fits.sum()), (op_cap, st)
        assert st["entries"] == whole, (op_cap, st)


@pytest.mark.parametrize("cap", [0, 5, 4, 6, 16], ids=["zero", "one_short", "inside_a_read", "exact", "above"])
def test_gap_capacity_zero_short_exact_and_above(gpu, text, text_index, cap):
    arrays = _capacity_batch(text)
    want, w_ooffs, w_ops, w_ends = extend_reference(arrays[0], arrays[1], text, arrays[3], arrays[2], arrays[4], arrays[5])
    goffs = np.r_[0, np.cumsum(want["anchors"].astype(np.int64) - 1)]
    assert goffs.tolist() == [0, 2, 2, 3, 6]
    got, ooffs, ops, ends = _run(text_index, arrays, cap=cap)
    fits = (goffs[1:] <= cap) | (np.diff(goffs) == 0)  # (a chain of one anchor has no gaps: it always fits)
    assert np.array_equal(got[fits], want[fits]) and all(r.tolist() == UNALIGNED_REC for r in got[~fits])
    assert np.array_equal(ends, np.where(np.repeat(fits, 2), w_ends, np.zeros(1, dtype=END_DTYPE)))
    counts = np.where(fits, np.diff(w_ooffs.astype(np.int64)), 0)  # a read that comes back unaligned has no entries
    assert ooffs.tolist() == np.r_[0, np.cumsum(counts)].tolist()
    assert np.array_equal(ops, np.concatenate([w_ops[int(w_ooffs[q]):int(w_ooffs[q + 1])] for q in np.flatnonzero(fits)] + [w_ops[:0]]))
    st = text_index.extend_stats()
    assert st["overflow"] == int(not fits.all()) and st["error"] == 0 and st["aligned_reads"] == int(fits.sum()), st


def test_repeated_calls_a_batch_in_two_calls_and_a_clone(gpu, text, text_index):
    rng = np.random.default_rng(7)
    B = Ends(front=1)
    for q in range(300):
        h = int(rng.integers(0, 6))
        if h:
            B.add_ends(text, rng, int(rng.integers(1000, 900_000)), [(int(a), int(b)) for a, b in rng.integers(0, 30, (h - 1, 2))],
                       int(rng.integers(0, 40)), int(rng.integers(0, 40)), rate=0.1)
        else:
            B.add_empty()
    arrays = B.arrays()
    a = _run(text_index, arrays)
    b = _run(text_index, arrays)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a, b))
    other = text_index.clone(0)
    c = _run(other, arrays)
    R, roffs, rec, moffs, chains, pred = arrays
    half = 150
    first = _run(text_index, (R, roffs[:half + 1], rec, moffs[:half + 1], chains[:half], pred))  # (the first handle goes on meanwhile)
    second = _run(text_index, (R, roffs[half:], rec, moffs[half:], chains[half:], pred))
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a, c))
    for k in (0, 2, 3):
        assert np.array_equal(np.concatenate([first[k], second[k]]), a[k]), k
    want = extend_reference(R, roffs, text, moffs, rec, chains, pred)
    assert all(np.array_equal(p, q) for p, q in zip(a, want))
    assert other.extend_stats()["entries"] == want[2].size and text_index.extend_stats()["reads"] == 150
    other.close()


def test_argument_errors(gpu, text, text_index):
    rng = np.random.default_rng(8)
    B = Ends()
    B.add_ends(text, rng, 1000, [(3, 3)], 5, 5)
    arrays = B.arrays()
    seqs, one = np.frombuffer(b"ACGT", dtype=np.uint8), [0, 4]
    for bad, message in (((0, 16, 4, 6), "max_extend must be 1 .. 4096"), ((4097, 16, 4, 6), "max_extend must be 1 .. 4096"),
                         ((512, 64, 4, 6), "band must be 0 .. 63"), ((512, 16, 65536, 6), "mismatch and indel must be 0 .. 65535"),
                         ((512, 16, 4, 65536), "mismatch and indel must be 0 .. 65535")):
        with pytest.raises(capi.SpxError, match="spx error -1: " + message):
            _run(text_index, arrays, None, bad)
        with pytest.raises(capi.SpxError, match="spx error -1: " + message):
            text_index.extend_host(seqs, one, 1, extend_params=bad)
    with pytest.raises(capi.SpxError, match="spx error -1: max_fill must be 1 .. 4096"):
        _run(text_index, arrays, (0,))
    with pytest.raises(capi.SpxError, match="spx error -1: lookback must be 1 .. 64"):
        text_index.extend_host(seqs, one, 1, chain_params=(0, 5000, 500, 1))
    z = torch.zeros(64, dtype=torch.int64, device="cuda")
    for caps in (dict(gap_capacity=2**32, op_capacity=4), dict(gap_capacity=4, op_capacity=2**32)):
        with pytest.raises(capi.SpxError, match="gap_capacity and op_capacity must be at most"):
            text_index.extend_device(z, z, z, z, z, z, None, None, d_out=z, d_out_op_offsets=z, d_out_ops=z, d_out_ends=z, **caps)
    S = capi._spe()
    p, ep = capi.SpaParams(512), capi.SpeParams(512, 16, 4, 6)
    t = [torch.zeros(64, dtype=torch.int64, device="cuda") for _ in range(10)]
    ptr = [x.data_ptr() for x in t]
    args = lambda **kw: [kw.get("ix", text_index._h), kw.get("R", ptr[0]), kw.get("ro", ptr[1]), kw.get("M", ptr[2]), kw.get("mo", ptr[3]), 1,
                         kw.get("ch", ptr[4]), kw.get("pred", ptr[5]), kw.get("p", p), kw.get("ep", ep), 4, 4, kw.get("out", ptr[6]),
                         kw.get("oo", ptr[7]), kw.get("ops", ptr[8]), kw.get("ends", ptr[9]), None]
    for kw in (dict(ix=None), dict(p=None), dict(ep=None), dict(R=None), dict(ro=None), dict(M=None), dict(mo=None), dict(ch=None),
               dict(pred=None), dict(out=None), dict(oo=None), dict(ops=None)):
        assert S.spe_extend_device(*args(**kw)) == -1, kw
    assert b"must be non-null" in capi.lib().spx_last_error()
    for kw in (dict(M=ptr[2] + 8), dict(ch=ptr[4] + 8), dict(out=ptr[6] + 4), dict(ends=ptr[9] + 8), dict(ro=ptr[1] + 4), dict(mo=ptr[3] + 4),
               dict(pred=ptr[5] + 2), dict(oo=ptr[7] + 4), dict(ops=ptr[8] + 2)):
        assert S.spe_extend_device(*args(**kw)) == -1, kw
        assert b"16-byte aligned" in capi.lib().spx_last_error()
    assert S.spe_last_extend_stats(text_index._h, None) == -1 and S.spe_last_extend_stats(None, None) == -1
    assert S.spe_extend_fetch(None, None, None) == -1
    bare = capi.Index.from_raw(synth.statistical_rlbwt(2000, 20, 3.0, seed=1, with_samples=True, n_docs=4), 0)
    with pytest.raises(capi.SpxError, match="the extended CIGARs need the text .spx_index_set_text / spx_index_rebuild_text"):
        _run(bare, arrays)
    with pytest.raises(capi.SpxError, match="the extended CIGARs need an index built with SA samples and the text"):
        bare.extend_host(seqs, one, 1)
    with pytest.raises(capi.SpxError, match="no extended CIGARs have been computed"):
        bare.extend_stats()
    with pytest.raises(capi.SpxError, match="spe_extend_fetch without a successful spe_extend_begin"):
        capi._check(S.spe_extend_fetch(bare._h, ptr[0], ptr[1]))
    bare.set_text(torch.from_numpy(np.full(5000, 65, dtype=np.uint8)), unchecked=True)
    with pytest.raises(capi.SpxError, match="spx error -1: min_length must be at least 1"):
        bare.extend_host(seqs, one, 0)
    with pytest.raises(capi.SpxError, match="spx error -1: one piece per call"):
        bare.extend_host(seqs, np.zeros((4 << 20) + 2, dtype=np.uint64), 1)
    with pytest.raises(capi.SpxError, match="spx error -1: one piece per call"):
        bare.extend_host(seqs, [0, (32 << 20) + 1], 1)
    bare.close()


@pytest.mark.parametrize("kind", ["pred_does_not_decrease", "pred_leaves_first_last", "more_anchors_than_steps", "a_link_of_negative_length",
                                  "chain_anchor_leaves_the_read", "a_gap_leaves_the_text", "read_end_beyond_the_read", "read_start_behind_read_end",
                                  "ref_end_beyond_the_text", "ref_start_behind_ref_end"])
def test_bad_inputs_are_refused(gpu, text, text_index, kind):
    """cigar's bad inputs, and chain records whose spans do not lie in the read and in the text in order: the spoiled read
    comes back unaligned without entries and ends, the others as the reference has them."""
    arrays = _bad_batch(text).arrays()
    chains = arrays[4]
    if kind == "read_end_beyond_the_read":
        chains["read_end"][1] = int(arrays[1][2] - arrays[1][1]) + 1
    elif kind == "read_start_behind_read_end":
        chains["read_start"][1] = int(chains["read_end"][1]) + 1
    elif kind == "ref_end_beyond_the_text":
        chains["ref_end"][1] = N_TEXT + 1
    elif kind == "ref_start_behind_ref_end":
        chains["ref_start"][1] = int(chains["ref_end"][1]) + 1
    else:
        _spoil(arrays, kind)
    got, ooffs, ops, ends = _run(text_index, arrays)  # (the fences are _run's)
    with pytest.raises(capi.SpxError, match="spx error -5: a read's chain failed the walk's checks"):
        text_index.extend_stats()
    good = _bad_batch(text).arrays()
    want, w_ooffs, w_ops, w_ends = extend_reference(good[0], good[1], text, good[3], good[2], good[4], good[5])
    assert got[1].tolist() == UNALIGNED_REC and got[0] == want[0] and got[2] == want[2]
    assert ends[2:4].tolist() == [NO_END, NO_END] and np.array_equal(ends[[0, 1, 4, 5]], w_ends[[0, 1, 4, 5]])
    assert int(ooffs[2]) == int(ooffs[1]) == int(w_ooffs[1])
    assert np.array_equal(ops, np.r_[w_ops[:int(w_ooffs[1])], w_ops[int(w_ooffs[2]):]])


# ---- extend_host against the oracle -> mems_reference -> chain_reference -> extend_reference ----------------------------
def _host_check(ix, orc, text, seqs, offs, min_length, chain_params=None, params=None, ep=None, digest=None, want_docs=False, oracle_mod=None):
    kind = digest[0] if digest else 0
    dseqs, doffs = oracle_mod.digest_batch(kind, digest[1], digest[2], seqs, offs) if kind else (seqs, offs)
    ms = orc.ms(dseqs, doffs, want_docs=want_docs, text=text)
    m = mems_reference(ms["lengths"], ms["pointers"], doffs, min_length, ms["docs"] if want_docs else None)
    w_chains, _, pred = chain_reference(m[0], m[1], chain_params, m[2] if want_docs else None)
    count = {}
    want, w_ooffs, w_ops, w_ends = extend_reference(dseqs, doffs, text, m[0], m[1], w_chains, pred, params, ep, count=count)
    got, ooffs, ops, chains, vals, ends = ix.extend_host(seqs, offs, min_length, chain_params, params, ep, digest=digest, want_docs=want_docs)
    st = ix.extend_stats()
    bad = np.flatnonzero(got != want)
    assert got.dtype == ALIGN_DTYPE and bad.size == 0, (min_length, params, bad[:5], got[bad[:5]], want[bad[:5]])
    assert ends.dtype == END_DTYPE and np.array_equal(ends, w_ends)
    assert ooffs.dtype == np.uint64 and np.array_equal(ooffs, w_ooffs) and ops.dtype == np.uint32 and np.array_equal(ops, w_ops)
    assert np.array_equal(chains, w_chains) and np.array_equal(vals, np.diff(doffs.astype(np.int64)))
    assert st["reads"] == len(offs) - 1 and st["entries"] == w_ops.size and st["overflow"] == 0 and st["error"] == 0, st
    assert (st["ends"], st["extended_ends"], st["band_cells"], st["clipped"]) == (count["ends"], count["extended"], count["cells"],
                                                                                   count["clipped"]), (st, count)
    # its middle is cigar_host's on the same call: with the ends' steps and the clips taken off, the same operations
    c_got, c_ooffs, c_ops, _, _ = ix.cigar_host(seqs, offs, min_length, chain_params, params, digest=digest, want_docs=want_docs)
    for q in range(len(offs) - 1):
        mine = [e & 15 for e in map(int, ops[int(ooffs[q]):int(ooffs[q + 1])]) for _ in range(e >> 4) if e & 15 != OP_S]
        core = [e & 15 for e in map(int, c_ops[int(c_ooffs[q]):int(c_ooffs[q + 1])]) for _ in range(e >> 4)]
        l, r = ends[2 * q], ends[2 * q + 1]
        ls = [k for k in range(max(int(l["read_chars"]), int(l["text_chars"])), int(l["read_chars"]) + int(l["text_chars"]) + 1)
              if mine[k:k + len(core)] == core]
        assert ls and int(got[q]["edits"]) == int(c_got[q]["edits"]) + int(l["edits"]) + int(r["edits"]), q
        assert [got[q][f] for f in ("anchors", "unfilled", "skipped", "doc")] == [c_got[q][f] for f in ("anchors", "unfilled", "skipped", "doc")]
    return want, w_ooffs, w_ops, w_ends, dseqs, doffs


@pytest.mark.parametrize("kind", [0, capi.SPX_DIGEST_PROMOTED, capi.SPX_DIGEST_DNA])
def test_extend_host_on_an_index_from_the_oracles_side(gpu, oracle_mod, kind):
    rng = np.random.default_rng(80 + kind)
    genome = cases.repetitive_text(rng, 40_000, DNA)
    text = oracle_mod.digest(kind, K, W, genome) if kind else genome
    cuts = [text.size // 5, text.size // 2, text.size - text.size // 5 - text.size // 2]
    raw = synth.index_from_text(torch.from_numpy(text), doc_lengths=cuts)
    orc = oracle_mod.OracleIndex.from_raw(raw)
    ix = capi.Index.from_raw(raw, 0)
    ix.set_text(torch.from_numpy(text.copy()))
    seqs, offs = cases.reads_mixed(rng, genome, DNA, 300, 500, [ord("N")])
    offs = offs.astype(np.uint64)
    digest = (kind, K, W) if kind else None
    kinds, extended = set(), 0
    for min_length, cp, ap, ep, want_docs in ((6, None, None, None, True),
                                              (12, ChainParams(64, 5000, 500, 0), AlignParams(8), ExtendParams(40, 3, 1, 2), False),
                                              (10**6, None, None, None, True)):
        want, ooffs, ops, ends, dseqs, doffs = _host_check(ix, orc, text, seqs, offs, min_length, cp, ap, ep, digest, want_docs, oracle_mod)
        check_invariants(want, ooffs, ops, dseqs, doffs, text)
        kinds |= {int(e) & 15 for e in ops}
        extended += int((ends["read_chars"] > 0).sum())
        if min_length == 10**6:
            assert (want["ref_start"] == np.uint64(UNALIGNED)).all() and ops.size == 0 and not ooffs.any() and not ends["score"].any()
    assert OP_EQ in kinds and OP_S in kinds and len(kinds) >= 4 and extended > 20
    got = ix.extend_host(np.zeros(0, dtype=np.uint8), [0], 4)
    assert got[0].size == 0 and got[1].tolist() == [0] and got[2].size == 0 and got[5].size == 0 and ix.extend_stats()["reads"] == 0
    ix.close()


def test_extend_host_takes_the_planted_reads_to_their_ends(gpu, oracle_mod):
    text, seqs, offs, cuts = planted_reads()
    raw = capi.build_raw(text)
    ix = capi.Index.from_raw(raw, 0)
    want, ooffs, ops, ends, _, _ = _host_check(ix, oracle_mod.OracleIndex.from_raw(raw), text, seqs, offs, 12, oracle_mod=oracle_mod)
    lens = np.diff(np.asarray(offs).astype(np.int64))
    assert (want["read_start"] == 0).all() and (want["read_end"] == lens).all() and OP_S not in {int(e) & 15 for e in ops}
    ix.close()


def test_the_seven_products_interleaved_on_one_handle(gpu):
    rng = np.random.default_rng(90)
    genome = cases.repetitive_text(rng, 40_000, DNA)
    cuts = [genome.size // 3, genome.size - genome.size // 3]
    raw = capi.build_raw(genome, doc_lengths=cuts)
    seqs, offs = cases.reads_mixed(rng, genome, DNA, 300, 500, [ord("N")])
    A = (seqs, offs.astype(np.uint64))
    long_read = np.tile(genome, 2)[:70_000].copy()
    long_read[rng.integers(0, long_read.size, 300)] = ord("N")
    B = (np.r_[seqs[: int(offs[20])], long_read], np.r_[offs[:21], offs[20] + long_read.size].astype(np.uint64))

    def extend(batch, want_docs=False, ep=None):
        return lambda ix: (list(ix.extend_host(batch[0], batch[1], 6, None, None, ep, want_docs=want_docs)), ix.extend_stats())

    def cigar(batch, want_docs=False):
        return lambda ix: (list(ix.cigar_host(batch[0], batch[1], 6, want_docs=want_docs)), ix.cigar_stats())

    def align(batch, want_docs=False):
        return lambda ix: (list(ix.align_host(batch[0], batch[1], 6, want_docs=want_docs)), ix.align_stats())

    def chain(batch):
        return lambda ix: (list(ix.chain_host(batch[0], batch[1], 6)), ix.chain_stats())

    def mems(batch):
        return lambda ix: (list(ix.mems_host(batch[0], batch[1], 6)), ix.mems_stats())

    def place(batch):
        return lambda ix: (list(ix.place_host(batch[0], batch[1], 6)), ix.place_stats())

    def assign(batch):
        return lambda ix: (list(ix.assign_host(capi.SPX_MODE_MS, batch[0], batch[1], 6)), ix.votes_stats())

    steps = [("align A", align(A)), ("cigar A", cigar(A)), ("extend A", extend(A)), ("mems A", mems(A)), ("extend B docs", extend(B, True)),
             ("cigar A", cigar(A)), ("place A", place(A)), ("chain B", chain(B)), ("extend A narrow", extend(A, False, ExtendParams(20, 2, 1, 1))),
             ("assign A", assign(A)), ("cigar B docs", cigar(B, True)), ("extend A", extend(A)), ("align A", align(A))]
    ix = capi.Index.from_raw(raw, 0)
    seen = {}
    for name, step in steps:
        got, got_stats = step(ix)
        fresh = capi.Index.from_raw(raw, 0)
        want, want_stats = step(fresh)
        fresh.close()
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (name, i)
        for s in (got_stats, want_stats):
            for key in ("kernel_ms", "step_ms", "wave_fill_ticks", "wave_back_ticks"):
                s.pop(key, None)
        assert got_stats == want_stats, (name, got_stats, want_stats)
        if name in seen:  # cigar's, align's and extend's results are the same bytes before and after the others
            assert all(g.tobytes() == w.tobytes() for g, w in zip(got, seen[name])), name
        seen[name] = got
    # the entries of an extend call wait for ITS fetch alone
    ix.extend_host(A[0], A[1], 6)
    with pytest.raises(capi.SpxError, match="spg_cigar_fetch without a successful spg_cigar_begin"):
        capi._check(capi._spg().spg_cigar_fetch(ix._h, None, None))
    with pytest.raises(capi.SpxError, match="spe_extend_fetch without a successful spe_extend_begin"):
        capi._check(capi._spe().spe_extend_fetch(ix._h, None, None))
    ix.close()


# ---- the command -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["dna_multiline_fasta", "dna_fastq", "promoted_alphabet_fasta"])
def test_cli_extend_equals_the_reference_over_the_golden_files(gpu, tmp_path, case):
    work = tmp_path / case
    shutil.copytree(os.path.join(FILES, case), work)
    ref, reads = str(work / "ref"), str(work / "reads.fa")
    env = dict(os.environ, SPUMONI_TEXT=ref + ".fa.rawtext", SPUMONI_SUPER_BATCH="3000")
    gold = os.path.join(FILES, case, "expected_M", "reads.fa")
    ids, L = _parse_values(gold + ".lengths")
    _, P = _parse_values(gold + ".pointers")
    _, D = _parse_values(gold + ".doc_numbers")
    offs = np.r_[0, np.cumsum([v.size for v in L])].astype(np.uint64)
    L, P, D = np.concatenate(L), np.concatenate(P), np.concatenate(D)
    text = np.fromfile(ref + ".fa.rawtext", dtype=np.uint8)
    seqs = _sequences(reads, offs)
    clips = 0
    for extra, min_length, cp, ap, ep, docs in (
            (["-L", "4", "-d"], 4, ChainParams(), AlignParams(), ExtendParams(), True),
            (["-L", "8", "-F", "3", "-E", "5", "-O", "0", "-N", "0", "-I", "65535"], 8, ChainParams(), AlignParams(3), ExtendParams(5, 0, 0, 65535), False),
            (["-L", "4", "-M", "-S", "40", "-G", "3", "-B", "2", "-H", "5", "--max-extend", "4096", "--band", "63", "--mismatch", "1", "--indel", "1"],
             4, ChainParams(5, 40, 3, 2), AlignParams(), ExtendParams(4096, 63, 1, 1), False)):
        if os.path.exists(reads + ".extended"):
            os.remove(reads + ".extended")
        r = _cli(["extend", "-r", ref, "-p", reads, "-n"] + extra, env)
        assert r.returncode == 0, r.stderr.decode()
        m = mems_reference(L, P, offs, min_length, D if docs else None)
        chains, _, pred = chain_reference(m[0], m[1], cp, m[2] if docs else None)
        want, ooffs, ops, ends = extend_reference(seqs, offs, text, m[0], m[1], chains, pred, ap, ep)
        lines = []
        for q in range(len(ids)):
            w = want[q]
            ok = w["ref_start"] != np.uint64(UNALIGNED)
            f = [ids[q]] + [str(int(x)).encode() for x in (offs[q + 1] - offs[q], w["read_start"], w["read_end"])]
            f += [str(int(w["ref_start"])).encode() if ok else b"-1"]
            f += [str(int(w[x])).encode() for x in ("ref_end", "matches", "edits", "anchors", "unfilled", "skipped")]
            f += [str(int(w["doc"])).encode() if ok else b"-1"] if docs else []
            f += [str(int(offs[q + 1] - offs[q])).encode()]
            lines.append(b"\t".join(f + [cigar_text(ops[int(ooffs[q]):int(ooffs[q + 1])]).encode()]) + b"\n")
        assert open(reads + ".extended", "rb").read() == b"".join(lines), (extra, r.stderr.decode())
        aligned = int((want["ref_start"] != np.uint64(UNALIGNED)).sum())
        clipped = sum(int(e) >> 4 for e in ops if int(e) & 15 == OP_S)
        assert f"{len(ids)} reads, {aligned} aligned, {len(ids) - aligned} without a match, {ops.size} CIGAR entries, {clipped} characters clipped".encode() \
            in r.stderr
        clips += clipped
    assert clips  # (soft clips are exercised)
    assert sorted(f for f in os.listdir(work) if f.startswith("reads.fa")) == ["reads.fa", "reads.fa.extended"]


def test_cli_extend_cuts_a_full_super_batch_into_calls_of_one_piece(gpu, tmp_path):
    """A super-batch ends with the read that fills it: 32 Mi characters and a few more are two calls of spe_extend_begin,
    the second one with offsets that do not start at 0 and entries behind the first call's.  The reads' first error sits
    12 characters in and their last 9 before the end: neither is an anchor's at -L 20, both are the extension's."""
    rng = np.random.default_rng(12)
    text = np.asarray(DNA, dtype=np.uint8)[rng.integers(0, 4, 100_000)]
    raw = capi.build_raw(text)
    prefix = str(tmp_path / "ref.fa")
    open(prefix, "w").write(">dummy\n")
    raw.write_raw_files(prefix)
    text.tofile(prefix + ".rawtext")
    nreads, m = 225_000, 150  # 33 750 000 characters: the super-batch of 32 Mi fills inside read 223 696
    at = rng.integers(0, text.size - m, nreads)
    rs = text[at.astype(np.int32)[:, None] + np.arange(m, dtype=np.int32)[None, :]]
    other = np.zeros(256, dtype=np.uint8)
    other[DNA] = DNA[1:] + DNA[:1]
    for col in (12, 140):
        rs[:, col] = other[rs[:, col]]
    reads = str(tmp_path / "reads.fa")
    with open(reads, "wb") as f:
        for i in range(0, nreads, 25_000):
            f.write(b"".join(b">r%d\n%s\n" % (q, rs[q].tobytes()) for q in range(i, i + 25_000)))
    env = dict(os.environ, SPUMONI_GPUS="0", SPUMONI_TEXT=prefix + ".rawtext", SPUMONI_SUPER_BATCH=str(64 << 20))
    r = _cli(["extend", "-r", prefix[:-3], "-p", reads, "-n", "-L", "20"], env)
    assert r.returncode == 0, r.stderr.decode()
    ix = capi.Index.from_raw(raw, 0)
    half = nreads // 2
    offs = np.arange(0, half * m + 1, m).astype(np.uint64)
    parts = [ix.extend_host(rs[:half].reshape(-1), offs, 20), ix.extend_host(rs[half:].reshape(-1), offs, 20)]
    ix.close()
    want = np.concatenate([p[0] for p in parts])
    assert ((want["edits"] == 2) & (want["matches"] == m - 2)).sum() > nreads // 2
    with open(reads + ".extended", "rb") as f:
        rows = [line.split(b"\t") for line in f]
    assert len(rows) == nreads and all(len(row) == 13 for row in rows[:10] + rows[-10:])
    got = np.array([[int(v) for v in row[1:12]] for row in rows], dtype=np.int64)
    for col, field in enumerate(("read_start", "read_end", "ref_start", "ref_end", "matches", "edits", "anchors", "unfilled", "skipped"), start=1):
        assert np.array_equal(got[:, col], want[field].astype(np.int64)), field
    assert (got[:, 0] == m).all() and (got[:, 10] == m).all()
    texts = [cigar_text(p[2][int(p[1][q]):int(p[1][q + 1])]).encode() + b"\n" for p in parts for q in range(half)]
    assert [row[12] for row in rows] == texts
    assert sum(t == b"12=1X127=1X9=\n" for t in texts) > nreads // 2


def test_cli_extend_writes_no_file_when_it_fails(gpu, tmp_path):
    work = tmp_path / "c"
    shutil.copytree(os.path.join(FILES, "dna_multiline_fasta"), work)
    text = open(work / "ref.fa.rawtext", "rb").read()
    with open(work / "reads.fa", "wb") as f:  # a read without characters ends the run, as it ends `run`: behind 40 good ones
        for q in range(40):
            f.write(b">r%d\n" % q + text[17 * q: 17 * q + 60] + b"\n")
        f.write(b">bad_one\n>after\n" + text[:40] + b"\n")
    env = dict(os.environ, SPUMONI_TEXT=str(work / "ref.fa.rawtext"), SPUMONI_SUPER_BATCH="1000")
    before = sorted(os.listdir(work))
    r = _cli(["extend", "-r", str(work / "ref"), "-p", str(work / "reads.fa"), "-n", "-L", "4"], env)
    assert r.returncode == 1 and b"bad_one was empty after digestion" in r.stderr, r.stderr.decode()
    assert sorted(os.listdir(work)) == before
