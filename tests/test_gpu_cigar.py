"""-m gpu: the CIGARs (spumoni_amd/csrc/spx_cigar.hip, include/spumoni_cigar.h) against the definition
(spumoni_amd/cigar.py: cigar_reference), bit for bit: the records, the op offsets and every entry.

cigar_device gets crafted reads, anchors, chains and pred (tests/test_gpu_align.py's Batch) on an index whose text is handed
in; cigar_host is held to the oracle's MS arrays -> mems_reference -> chain_reference -> cigar_reference, and `spumoni cigar`
to the same over the committed golden files.  The tracing fill gives a gap a lane up to 16 x 16 and a wavefront above, in
strips of 64 rows, whose trace stands in LDS up to 2048 words (a * ceil(b / 16)) and in device memory above: the crafted
gaps lie around 1, 16, 64 and 128 on either side and on both sides of 2048 words."""
import os
import shutil

import numpy as np
import pytest
import torch

from spumoni_amd import capi, synth
from spumoni_amd.align import ALIGN_DTYPE, UNALIGNED, AlignParams
from spumoni_amd.chain import CHAIN_DTYPE, ChainParams, chain_reference
from spumoni_amd.cigar import MAX_LENGTH, OP_D, OP_EQ, OP_I, OP_N, OP_X, cigar_reference, cigar_text
from spumoni_amd.mems import MATCH_DTYPE, mems_reference
from tests import cases
from tests.test_align_cpu import clustered_reads
from tests.test_chain_cpu import planted_reads
from tests.test_cigar_cpu import replay
from tests.test_gpu_align import (DNA, FENCE, FILES, K, LETTERS, N_TEXT, RUN_A, UNALIGNED_REC, W, Batch, _bad_batch, _cli, _parse_values,
                                  _sequences)

pytestmark = pytest.mark.gpu


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


@pytest.fixture(scope="module")
def text_index(gpu, text):
    """Any index, with the crafted text handed in: the cigar kernels read the text and nothing else of the index."""
    ix = capi.Index.from_raw(synth.statistical_rlbwt(5000, 60, 4.0, seed=3, with_samples=True, n_docs=8), 0)
    ix.set_text(torch.from_numpy(text.copy()), unchecked=True)
    yield ix
    ix.close()


def _generous(arrays):
    R, roffs, rec, moffs, chains, pred = arrays
    return 2 * R.size + 2 * rec.size + moffs.size + 64


def _run(ix, arrays, params=None, cap=None, op_cap=None):
    """cigar_device with every output fenced; returns (records, op_offsets, entries) -- entries up to min(total, op_cap)."""
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
    out, _, _ = ix.cigar_device(d_R, d_roffs, d_rec, d_moffs, d_chains, d_pred, params, gap_capacity=cap, op_capacity=op_cap,
                                d_out=fenced[:nreads], d_out_op_offsets=d_ooffs, d_out_ops=d_ops)
    torch.cuda.synchronize()
    assert (fenced[nreads:] == FENCE).all().item()
    records = out.cpu().numpy().view(ALIGN_DTYPE).reshape(-1)
    ooffs = d_ooffs.cpu().numpy()
    assert (ooffs[nreads + 1:] == FENCE).all()
    ooffs = ooffs[:nreads + 1].view(np.uint64)
    ends = ooffs[1:][ooffs[1:] <= op_cap]
    written = int(ends.max(initial=0))
    ops = d_ops.cpu().numpy()
    assert (ops[written:] == FENCE).all()  # nothing is written past the reads that fit (or past the capacity)
    return records, ooffs, ops[:written].copy().view(np.uint32)


def _check(ix, text, arrays, params=None, ref=None):
    R, roffs, rec, moffs, chains, pred = arrays
    if ref is None:
        count = [0]
        ref = cigar_reference(R, roffs, text, moffs, rec, chains, pred, params, count=count) + (count,)
    want, w_ooffs, w_ops, count = ref
    got, ooffs, ops = _run(ix, arrays, params)
    assert np.array_equal(ooffs, w_ooffs), (params, np.flatnonzero(ooffs != w_ooffs)[:5])
    bad = np.flatnonzero(ops != w_ops)
    assert bad.size == 0, (params, bad[:5], ops[bad[:5]], w_ops[bad[:5]])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (params, bad[:5], got[bad[:5]], want[bad[:5]])
    st = ix.cigar_stats()
    ok = want["ref_start"] != np.uint64(UNALIGNED)
    gaps = int((want["anchors"][ok].astype(np.int64) - 1).sum())
    assert st["reads"] == moffs.size - 1 and st["aligned_reads"] == int(ok.sum()) and st["gaps"] == gaps, st
    assert st["filled_gaps"] == gaps - int(want["unfilled"].sum()) and st["cells"] == count[0] and st["entries"] == w_ops.size, (st, count)
    assert st["error"] == 0 and st["overflow"] == 0 and len(st["step_ms"]) == 5, st
    return ref


SIDES = [0, 1, 2, 15, 16, 17, 63, 64, 65, 129]  # every bin (none, 1 x 1, a lane, a wavefront) and both sides of a strip of 64 rows
# a wavefront's trace: 128 x 256 is 2048 words, the last that LDS takes; the others go to device memory
TRACE_EDGE = [(128, 256), (129, 256), (127, 257), (200, 300), (300, 200)]


@pytest.mark.parametrize("alphabet", [b"ACGT", b"AC"], ids=["four_letters", "two_letters"])
def test_every_pair_of_gap_sides_alone_and_mixed_in_one_read(gpu, text, text_index, alphabet):
    """Over two letters the text is a copy with G -> A and T -> C: ties are everywhere."""
    rng = np.random.default_rng(len(alphabet))
    if len(alphabet) == 2:
        fold = np.arange(256, dtype=np.uint8)
        fold[ord("G")], fold[ord("T")] = ord("A"), ord("C")
        text = fold[text]
        ix = capi.Index.from_raw(synth.statistical_rlbwt(5000, 60, 4.0, seed=3, with_samples=True, n_docs=8), 0)
        ix.set_text(torch.from_numpy(text.copy()), unchecked=True)
    else:
        ix = text_index
    combos = [(a, b) for a in SIDES for b in SIDES] + TRACE_EDGE
    B = Batch(front=3)
    for a, b in combos:
        B.add(text, rng, int(rng.integers(0, 900_000)), [(a, b)])
    B.add(text, rng, 5000, [combos[i] for i in rng.permutation(len(combos))])  # one read whose gaps mix all bins
    B.add(text, rng, 70_000, [(40, 40), (33, 35)], mutate=0.0)  # A = B, and A = a prefix of B
    arrays = B.arrays()
    if len(alphabet) == 2:
        arrays = (fold[arrays[0]],) + arrays[1:]
    want, ooffs, ops, _ = _check(ix, text, arrays)
    assert ops.size > 3000 and {int(e) & 15 for e in ops} == {OP_EQ, OP_X, OP_I, OP_D}
    for q in (0, len(combos), len(combos) + 1):  # (the replay is the reference's own test; here it guards the crafted input)
        replay(ops[int(ooffs[q]):int(ooffs[q + 1])], bytes(arrays[0][int(arrays[1][q]):int(arrays[1][q + 1])]), bytes(text), want[q])
    if len(alphabet) == 2:
        ix.close()
    else:
        st = ix.cigar_stats()
        assert st["path_words"] > 500 and st["wave_fill_ticks"] > 0 and st["wave_back_ticks"] > 0, st


@pytest.mark.parametrize("max_fill", [1, 16, 512, 4096])
def test_max_fill_with_gaps_at_the_limit_and_one_above(gpu, text, text_index, max_fill):
    rng = np.random.default_rng(2)
    B = Batch()
    m = max_fill
    other = min(m, 20)
    B.add(text, rng, 1000, [(m, other), (m + 1, other), (other, m), (other, m + 1), (1, 1), (0, m), (0, m + 1), (m + 1, 0), (m, 0), (2, 1)])
    B.add(text, rng, 50_000, [(m + 1, m + 1), (3, 3)])
    if m == 512:
        B.add(text, rng, 100_000, [(m, m - 70)])  # 512 x 28 words: a trace in device memory, at the limit
    want, ooffs, ops, _ = _check(text_index, text, B.arrays(), AlignParams(max_fill))
    assert int(want["unfilled"][0]) == 4 + (m < 2) and int(want["skipped"][0]) == 4 * (m + 1) + 2 * (m < 2)
    kinds = [int(e) & 15 for e in ops[int(ooffs[1]):int(ooffs[2])]]
    assert kinds[:3] == [OP_EQ, OP_I, OP_N] and int(ops[int(ooffs[1]) + 1]) >> 4 == m + 1  # an unfilled gap: a x I, b x N


def test_the_largest_gaps_have_their_closed_forms(gpu, text, text_index):
    """4096 x 4096 with A = B: 4096=.  4096 x 4096 over disjoint letters: 4096X.  P followed by 496 letters that P lacks,
    against P alone (4096 x 3600): the last 496 rows can only go up, then the strings are equal: 3600=496I.  Beside them a
    gap one above the limit.  The anchors on either side are 10 characters each and merge with the gap's matches."""
    S = text[200_000:204_096]
    B = Batch()
    B.reads = [np.r_[text[199_990:200_000], S, text[204_096:204_106]],
               np.r_[text[RUN_A - 10:RUN_A], np.full(4096, ord("C"), dtype=np.uint8), text[RUN_A + 4096:RUN_A + 4106]],
               np.r_[text[RUN_A - 10:RUN_A], np.full(3600, ord("A"), dtype=np.uint8), np.full(496, ord("C"), dtype=np.uint8),
                     text[RUN_A + 3600:RUN_A + 3610]],
               np.r_[text[300_000:300_010], text[300_010:304_107], text[304_107:304_117]]]
    B.anchors = [(0, 199_990, 10), (4106, 204_096, 10), (0, RUN_A - 10, 10), (4106, RUN_A + 4096, 10),
                 (0, RUN_A - 10, 10), (4106, RUN_A + 3600, 10), (0, 300_000, 10), (4107, 304_107, 10)]
    B.counts = [2, 2, 2, 2]
    got, ooffs, ops = _run(text_index, B.arrays(), AlignParams(4096))
    cigars = [cigar_text(ops[int(ooffs[q]):int(ooffs[q + 1])]) for q in range(4)]
    assert cigars == ["4116=", "10=4096X10=", "3610=496I10=", "10=4097I4097N10="], cigars
    assert [(int(r["matches"]), int(r["edits"]), int(r["unfilled"]), int(r["skipped"])) for r in got] == \
        [(4116, 0, 0, 0), (20, 4096, 0, 0), (3620, 496, 0, 0), (20, 0, 1, 4097)]
    st = text_index.cigar_stats()
    assert st["cells"] == 2 * 4096 * 4096 + 4096 * 3600 and st["filled_gaps"] == 3 and st["gaps"] == 4 and st["entries"] == 11, st
    assert st["path_words"] == 2 * 512 + 481 and st["overflow"] == 0, st


def test_chains_of_every_length_and_runs_of_unchained_reads(gpu, text, text_index):
    rng = np.random.default_rng(3)
    B = Batch(front=5)
    small = lambda h: [(int(a), int(b)) for a, b in rng.integers(0, 6, (h - 1, 2))]
    for _ in range(3):
        B.add_empty()
    for h in (1, 2, 16, 17, 64, 65, 1000, 1, 3):
        B.add(text, rng, int(rng.integers(0, 900_000)), small(h))
        if h in (2, 65):
            for _ in range(4):
                B.add_empty()
    B.add_empty()
    want, ooffs, ops, _ = _check(text_index, text, B.arrays())
    assert sorted(want["anchors"].tolist())[-3:] == [64, 65, 1000] and (want["ref_start"] == np.uint64(UNALIGNED)).sum() == 12
    assert ops[int(ooffs[3]):int(ooffs[4])].tolist() == [B.anchors[5][2] << 4 | OP_EQ]  # a chain of one anchor: l x '='
    assert (np.diff(ooffs.astype(np.int64))[want["ref_start"] == np.uint64(UNALIGNED)] == 0).all()


def test_one_chain_of_100000_anchors_among_short_reads(gpu, text, text_index):
    rng = np.random.default_rng(4)
    B = Batch()
    for q in range(601):
        if q == 300:
            B.add(text, rng, 10_000, [(int(a), int(b)) for a, b in rng.integers(0, 4, (99_999, 2))], lengths=rng.integers(3, 9, 100_000))
        else:
            h = int(rng.integers(0, 6))
            B.add(text, rng, int(rng.integers(0, 900_000)), [(int(a), int(b)) for a, b in rng.integers(0, 20, (h - 1, 2))]) if h else B.add_empty()
    want, ooffs, ops, _ = _check(text_index, text, B.arrays())
    assert int(want["anchors"][300]) == 100_000 and int(ooffs[301] - ooffs[300]) > 100_000


@pytest.mark.parametrize("nreads", [0, 1, 63, 64, 65, 3000])
def test_read_counts_around_the_wavefront(gpu, text, text_index, nreads):
    rng = np.random.default_rng(nreads)
    B = Batch(front=nreads % 3)
    for q in range(nreads):
        h = int(rng.integers(0, 5))
        if h:
            B.add(text, rng, int(rng.integers(0, 900_000)), [(int(a), int(b)) for a, b in rng.integers(0, 24, (h - 1, 2))])
        else:
            B.add_empty()
    _check(text_index, text, B.arrays())
    if nreads in (65, 3000):
        _check(text_index, text, B.arrays(), AlignParams(8))


def test_overlapping_anchors_the_texts_last_character_and_wide_positions(gpu, text, text_index):
    rng = np.random.default_rng(5)
    B = Batch()
    # anchors that begin inside their predecessor, in the read (a = 0) and in the text (b = 0)
    B.reads.append(text[1000:1060].copy())
    B.anchors += [(0, 1000, 20), (14, 1016, 20), (30, 1030, 12), (40, 1050, 20)]
    B.counts.append(4)
    # a gap that ends at the text's last character: the anchor behind it stands where the text ends
    B.reads.append(np.r_[text[N_TEXT - 30:N_TEXT - 20], LETTERS[rng.integers(0, 4, 18)], LETTERS[rng.integers(0, 4, 6)]])
    B.anchors += [(0, N_TEXT - 30, 10), (28, N_TEXT, 6)]
    B.counts.append(2)
    # y near 2^40: nothing of the text is read where the gaps have b = 0, and positions are 64 bits wide
    Y = (1 << 40) - 7
    B.reads.append(LETTERS[rng.integers(0, 4, 60)])
    B.anchors += [(0, Y, 10), (15, Y + 10, 10), (40, Y + 20, 20)]
    B.counts.append(3)
    want, ooffs, ops, _ = _check(text_index, text, B.arrays())
    assert cigar_text(ops[:int(ooffs[1])]) == "20=2D14=2I6=10D18="
    assert cigar_text(ops[int(ooffs[2]):]) == "10=5I10=15I20="
    assert int(want["ref_end"][1]) == N_TEXT + 6


def test_an_unfilled_gap_of_more_than_2_to_the_28_text_characters_is_split(gpu):
    """The walk refuses a gap outside the text, so the text is 2^28 and some characters long (one letter: only its length
    matters, an unfilled gap reads nothing)."""
    far = 2**28 + 5
    big = np.full(far + 1000, ord("A"), dtype=np.uint8)
    ix = capi.Index.from_raw(synth.statistical_rlbwt(5000, 60, 4.0, seed=3, with_samples=True, n_docs=8), 0)
    ix.set_text(torch.from_numpy(big), unchecked=True)
    B = Batch()
    B.reads = [np.full(23, ord("A"), dtype=np.uint8), np.full(20, ord("A"), dtype=np.uint8)]
    B.anchors = [(0, 100, 10), (13, 110 + far, 10), (0, 50, 10), (10, 60 + MAX_LENGTH, 10)]
    B.counts = [2, 2]
    got, ooffs, ops = _run(ix, B.arrays())
    assert ooffs.tolist() == [0, 5, 8]
    assert cigar_text(ops[:5]) == f"10=3I{MAX_LENGTH}N6N10=" and cigar_text(ops[5:]) == f"10={MAX_LENGTH}N10="  # (a full entry alone)
    assert got[0].tolist()[4:9] == (20, 0, 2, 1, far) and int(got[1]["skipped"]) == MAX_LENGTH
    st = ix.cigar_stats()
    assert st["entries"] == 8 and st["overflow"] == 0 and st["error"] == 0, st
    ix.close()


def _capacity_batch(text):
    rng = np.random.default_rng(6)
    B = Batch()
    for gaps in ([(3, 4), (20, 20)], [], [(5, 5)], [(2, 2), (1, 1), (0, 3)]):
        B.add(text, rng, int(rng.integers(0, 900_000)), gaps)
    return B.arrays()


def test_op_capacity_zero_short_exact_and_above(gpu, text, text_index):
    """A read whose entries do not all fit writes none and comes back unaligned, nothing is written past the capacity, the
    offsets still count every read, and the stats say so."""
    arrays = _capacity_batch(text)
    want, w_ooffs, w_ops = cigar_reference(arrays[0], arrays[1], text, arrays[3], arrays[2], arrays[4], arrays[5])
    total = int(w_ooffs[-1])
    assert (np.diff(w_ooffs.astype(np.int64)) >= 1).all() and total > 12
    for op_cap in (0, total - 1, int(w_ooffs[2]) + 1, int(w_ooffs[1]), total, total + 9):
        got, ooffs, ops = _run(text_index, arrays, op_cap=op_cap)
        assert np.array_equal(ooffs, w_ooffs), op_cap
        fits = w_ooffs[1:] <= op_cap
        assert np.array_equal(got[fits], want[fits]) and all(r.tolist() == UNALIGNED_REC for r in got[~fits]), op_cap
        whole = int(w_ooffs[1:][fits].max(initial=0))
        assert ops.size == whole and np.array_equal(ops, w_ops[:whole]), op_cap
        st = text_index.cigar_stats()
        assert st["overflow"] == int(not fits.all()) and st["error"] == 0 and st["aligned_reads"] == int(fits.sum()), (op_cap, st)
        assert st["entries"] == whole, (op_cap, st)


@pytest.mark.parametrize("cap", [0, 5, 4, 6, 16], ids=["zero", "one_short", "inside_a_read", "exact", "above"])
def test_gap_capacity_zero_short_exact_and_above(gpu, text, text_index, cap):
    arrays = _capacity_batch(text)
    want, w_ooffs, w_ops = cigar_reference(arrays[0], arrays[1], text, arrays[3], arrays[2], arrays[4], arrays[5])
    goffs = np.r_[0, np.cumsum(want["anchors"].astype(np.int64) - 1)]
    assert goffs.tolist() == [0, 2, 2, 3, 6]
    got, ooffs, ops = _run(text_index, arrays, cap=cap)
    fits = (goffs[1:] <= cap) | (np.diff(goffs) == 0)  # (a chain of one anchor has no gaps: it always fits)
    assert np.array_equal(got[fits], want[fits]) and all(r.tolist() == UNALIGNED_REC for r in got[~fits])
    counts = np.where(fits, np.diff(w_ooffs.astype(np.int64)), 0)  # a read that comes back unaligned has no entries
    assert ooffs.tolist() == np.r_[0, np.cumsum(counts)].tolist()
    assert np.array_equal(ops, np.concatenate([w_ops[int(w_ooffs[q]):int(w_ooffs[q + 1])] for q in np.flatnonzero(fits)] + [w_ops[:0]]))
    st = text_index.cigar_stats()
    assert st["overflow"] == int(not fits.all()) and st["error"] == 0 and st["aligned_reads"] == int(fits.sum()), st


def test_repeated_calls_a_batch_in_two_calls_and_a_clone(gpu, text, text_index):
    rng = np.random.default_rng(7)
    B = Batch(front=1)
    for q in range(300):
        h = int(rng.integers(0, 8))
        B.add(text, rng, int(rng.integers(0, 900_000)), [(int(a), int(b)) for a, b in rng.integers(0, 40, (h - 1, 2))]) if h else B.add_empty()
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
    assert np.array_equal(np.concatenate([first[0], second[0]]), a[0]) and np.array_equal(np.concatenate([first[2], second[2]]), a[2])
    want = cigar_reference(R, roffs, text, moffs, rec, chains, pred)
    assert all(np.array_equal(p, q) for p, q in zip(a, want))
    assert other.cigar_stats()["entries"] == want[2].size and text_index.cigar_stats()["reads"] == 150
    other.close()


def test_argument_errors(gpu, text, text_index):
    rng = np.random.default_rng(8)
    B = Batch()
    B.add(text, rng, 100, [(3, 3)])
    arrays = B.arrays()
    for bad in ((0,), (4097,)):
        with pytest.raises(capi.SpxError, match="spx error -1: max_fill must be 1 .. 4096"):
            _run(text_index, arrays, bad)
        with pytest.raises(capi.SpxError, match="spx error -1: max_fill must be 1 .. 4096"):
            text_index.cigar_host(np.frombuffer(b"ACGT", dtype=np.uint8), [0, 4], 1, params=bad)
    with pytest.raises(capi.SpxError, match="spx error -1: lookback must be 1 .. 64"):
        text_index.cigar_host(np.frombuffer(b"ACGT", dtype=np.uint8), [0, 4], 1, chain_params=(0, 5000, 500, 1))
    z = torch.zeros(64, dtype=torch.int64, device="cuda")
    for caps in (dict(gap_capacity=2**32, op_capacity=4), dict(gap_capacity=4, op_capacity=2**32)):
        with pytest.raises(capi.SpxError, match="gap_capacity and op_capacity must be at most"):
            text_index.cigar_device(z, z, z, z, z, z, None, d_out=z, d_out_op_offsets=z, d_out_ops=z, **caps)
    S = capi._spg()
    p = capi.SpaParams(512)
    t = [torch.zeros(64, dtype=torch.int64, device="cuda") for _ in range(9)]
    ptr = [x.data_ptr() for x in t]
    args = lambda **kw: [kw.get("ix", text_index._h), kw.get("R", ptr[0]), kw.get("ro", ptr[1]), kw.get("M", ptr[2]), kw.get("mo", ptr[3]), 1,
                         kw.get("ch", ptr[4]), kw.get("pred", ptr[5]), kw.get("p", p), 4, 4, kw.get("out", ptr[6]), kw.get("oo", ptr[7]),
                         kw.get("ops", ptr[8]), None]
    for kw in (dict(ix=None), dict(p=None), dict(R=None), dict(ro=None), dict(M=None), dict(mo=None), dict(ch=None), dict(pred=None), dict(out=None),
               dict(oo=None), dict(ops=None)):
        assert S.spg_cigar_device(*args(**kw)) == -1, kw
    assert b"must be non-null" in capi.lib().spx_last_error()
    for kw in (dict(M=ptr[2] + 8), dict(ch=ptr[4] + 8), dict(out=ptr[6] + 4), dict(ro=ptr[1] + 4), dict(mo=ptr[3] + 4), dict(pred=ptr[5] + 2),
               dict(oo=ptr[7] + 4), dict(ops=ptr[8] + 2)):
        assert S.spg_cigar_device(*args(**kw)) == -1, kw
        assert b"16-byte aligned" in capi.lib().spx_last_error()
    assert S.spg_last_cigar_stats(text_index._h, None) == -1 and S.spg_last_cigar_stats(None, None) == -1
    assert S.spg_cigar_fetch(None, None, None) == -1
    # an index without the text; the host form's own checks and the limits of one piece
    bare = capi.Index.from_raw(synth.statistical_rlbwt(2000, 20, 3.0, seed=1, with_samples=True, n_docs=4), 0)
    with pytest.raises(capi.SpxError, match="spx_index_set_text / spx_index_rebuild_text"):
        _run(bare, arrays)
    seqs, one = np.frombuffer(b"ACGT", dtype=np.uint8), [0, 4]
    with pytest.raises(capi.SpxError, match="spx_index_set_text / spx_index_rebuild_text"):
        bare.cigar_host(seqs, one, 1)
    with pytest.raises(capi.SpxError, match="no CIGARs have been computed"):
        bare.cigar_stats()
    with pytest.raises(capi.SpxError, match="spg_cigar_fetch without a successful spg_cigar_begin"):
        capi._check(S.spg_cigar_fetch(bare._h, ptr[0], ptr[1]))
    bare.set_text(torch.from_numpy(np.full(5000, 65, dtype=np.uint8)), unchecked=True)
    with pytest.raises(capi.SpxError, match="spx error -1: min_length must be at least 1"):
        bare.cigar_host(seqs, one, 0)
    with pytest.raises(capi.SpxError, match="digest_kind must be"):
        bare.cigar_host(seqs, one, 1, digest=(7, 4, 11))
    with pytest.raises(capi.SpxError, match="spx error -1: one piece per call"):
        bare.cigar_host(seqs, np.zeros((4 << 20) + 2, dtype=np.uint64), 1)
    with pytest.raises(capi.SpxError, match="spx error -1: one piece per call"):
        bare.cigar_host(seqs, [0, (32 << 20) + 1], 1)
    bare.close()


# ---- bad input: refused by the walk's checks, unaligned, SPX_E_FORMAT, fences intact -----------------------------------
def _spoil(arrays, kind):
    """The five bad inputs of spa_align_device, on the middle read of _bad_batch."""
    R, roffs, rec, moffs, chains, pred = arrays
    o = int(moffs[1])
    if kind == "pred_does_not_decrease":
        pred[o + 3] = 3
    elif kind == "pred_leaves_first_last":
        chains["first"][1], chains["anchors"][1], pred[o + 3] = 2, 3, 1
    elif kind == "more_anchors_than_steps":
        pred[o + 2] = 0xFFFFFFFF
    elif kind == "a_link_of_negative_length":
        rec["read_pos"][o + 2], rec["length"][o + 2] = 1, 2
    elif kind == "chain_anchor_leaves_the_read":
        rec["length"][o + 4] = 10_000
    else:
        assert kind == "a_gap_leaves_the_text"
        rec["ref_pos"][o + 4] = N_TEXT + 1
        chains["ref_end"][1] = N_TEXT + 1 + int(rec["length"][o + 4])


@pytest.mark.parametrize("kind", ["pred_does_not_decrease", "pred_leaves_first_last", "more_anchors_than_steps", "a_link_of_negative_length",
                                  "chain_anchor_leaves_the_read", "a_gap_leaves_the_text"])
def test_bad_inputs_are_refused(gpu, text, text_index, kind):
    """The spoiled read comes back unaligned without entries, the others as the reference has them."""
    arrays = _bad_batch(text).arrays()
    _spoil(arrays, kind)
    got, ooffs, ops = _run(text_index, arrays)  # (the fences are _run's)
    with pytest.raises(capi.SpxError, match="spx error -5: a read's chain failed the walk's checks"):
        text_index.cigar_stats()
    good = _bad_batch(text).arrays()
    want, w_ooffs, w_ops = cigar_reference(good[0], good[1], text, good[3], good[2], good[4], good[5])
    assert got[1].tolist() == UNALIGNED_REC and got[0] == want[0] and got[2] == want[2]
    assert int(ooffs[2]) == int(ooffs[1]) == int(w_ooffs[1])
    assert np.array_equal(ops, np.r_[w_ops[:int(w_ooffs[1])], w_ops[int(w_ooffs[2]):]])


# ---- cigar_host against the oracle -> mems_reference -> chain_reference -> cigar_reference ------------------------------
def _host_check(ix, orc, text, seqs, offs, min_length, chain_params=None, params=None, digest=None, want_docs=False, oracle_mod=None):
    kind = digest[0] if digest else 0
    dseqs, doffs = oracle_mod.digest_batch(kind, digest[1], digest[2], seqs, offs) if kind else (seqs, offs)
    ms = orc.ms(dseqs, doffs, want_docs=want_docs, text=text)
    m = mems_reference(ms["lengths"], ms["pointers"], doffs, min_length, ms["docs"] if want_docs else None)
    w_chains, _, pred = chain_reference(m[0], m[1], chain_params, m[2] if want_docs else None)
    count = [0]
    want, w_ooffs, w_ops = cigar_reference(dseqs, doffs, text, m[0], m[1], w_chains, pred, params, count=count)
    got, ooffs, ops, chains, vals = ix.cigar_host(seqs, offs, min_length, chain_params, params, digest=digest, want_docs=want_docs)
    st = ix.cigar_stats()
    bad = np.flatnonzero(got != want)
    assert got.dtype == ALIGN_DTYPE and bad.size == 0, (min_length, params, bad[:5], got[bad[:5]], want[bad[:5]])
    assert ooffs.dtype == np.uint64 and np.array_equal(ooffs, w_ooffs) and ops.dtype == np.uint32 and np.array_equal(ops, w_ops)
    assert np.array_equal(chains, w_chains) and np.array_equal(vals, np.diff(doffs.astype(np.int64)))
    assert st["reads"] == len(offs) - 1 and st["cells"] == count[0] and st["entries"] == w_ops.size and st["overflow"] == 0, (st, count)
    assert st["aligned_reads"] == int((want["anchors"] > 0).sum()), st
    # its records are align_host's on the same call
    assert got.tobytes() == ix.align_host(seqs, offs, min_length, chain_params, params, digest=digest, want_docs=want_docs)[0].tobytes()
    return want, w_ooffs, w_ops


@pytest.mark.parametrize("kind", [0, capi.SPX_DIGEST_PROMOTED, capi.SPX_DIGEST_DNA])
def test_cigar_host_on_an_index_from_the_oracles_side(gpu, oracle_mod, kind):
    """Several documents; DNA reads through digestion, walk, MS extension, the matches, the chaining, the tables and their
    walk back in two calls of the library, with and without ids."""
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
    kinds = set()
    for min_length, cp, ap, want_docs in ((6, None, None, True), (12, ChainParams(64, 5000, 500, 0), AlignParams(8), False),
                                          (10**6, None, None, True)):
        want, ooffs, ops = _host_check(ix, orc, text, seqs, offs, min_length, cp, ap, digest, want_docs, oracle_mod)
        kinds |= {int(e) & 15 for e in ops}
        if min_length == 10**6:
            assert (want["ref_start"] == np.uint64(UNALIGNED)).all() and ops.size == 0 and not ooffs.any()
    assert OP_EQ in kinds and len(kinds) >= 3
    got = ix.cigar_host(np.zeros(0, dtype=np.uint8), [0], 4)
    assert got[0].size == 0 and got[1].tolist() == [0] and got[2].size == 0 and ix.cigar_stats()["reads"] == 0
    ix.close()


def test_cigar_host_on_both_planted_sets(gpu, oracle_mod):
    text, seqs, offs, cuts = planted_reads()
    raw = capi.build_raw(text)
    ix = capi.Index.from_raw(raw, 0)
    want, ooffs, ops = _host_check(ix, oracle_mod.OracleIndex.from_raw(raw), text, seqs, offs, 12, oracle_mod=oracle_mod)
    assert all((int(r["edits"]), int(r["matches"]), int(r["unfilled"])) == (7, 298, 0) for r in want)
    assert [int(e) & 15 for e in ops[:int(ooffs[1])]] == [OP_EQ, OP_X, OP_EQ, OP_D, OP_EQ, OP_X, OP_EQ, OP_I, OP_EQ]
    ix.close()
    text, seqs, offs = clustered_reads()
    raw = capi.build_raw(text)
    ix = capi.Index.from_raw(raw, 0)
    want, ooffs, ops = _host_check(ix, oracle_mod.OracleIndex.from_raw(raw), text, seqs, offs, 12, oracle_mod=oracle_mod)
    assert ops.size > 12 * 20 and ix.cigar_stats()["path_words"] > 12
    ix.close()


def test_the_six_products_interleaved_on_one_handle(gpu):
    rng = np.random.default_rng(90)
    genome = cases.repetitive_text(rng, 40_000, DNA)
    cuts = [genome.size // 3, genome.size - genome.size // 3]
    raw = capi.build_raw(genome, doc_lengths=cuts)
    seqs, offs = cases.reads_mixed(rng, genome, DNA, 300, 500, [ord("N")])
    A = (seqs, offs.astype(np.uint64))
    long_read = np.tile(genome, 2)[:70_000].copy()
    long_read[rng.integers(0, long_read.size, 300)] = ord("N")
    B = (np.r_[seqs[: int(offs[20])], long_read], np.r_[offs[:21], offs[20] + long_read.size].astype(np.uint64))

    def cigar(batch, want_docs=False, params=None):
        return lambda ix: (list(ix.cigar_host(batch[0], batch[1], 6, None, params, want_docs=want_docs)), ix.cigar_stats())

    def align(batch, want_docs=False, params=None):
        return lambda ix: (list(ix.align_host(batch[0], batch[1], 6, None, params, want_docs=want_docs)), ix.align_stats())

    def chain(batch):
        return lambda ix: (list(ix.chain_host(batch[0], batch[1], 6)), ix.chain_stats())

    def mems(batch):
        return lambda ix: (list(ix.mems_host(batch[0], batch[1], 6)), ix.mems_stats())

    def place(batch):
        return lambda ix: (list(ix.place_host(batch[0], batch[1], 6)), ix.place_stats())

    def assign(batch):
        return lambda ix: (list(ix.assign_host(capi.SPX_MODE_MS, batch[0], batch[1], 6)), ix.votes_stats())

    steps = [("align A", align(A)), ("cigar A", cigar(A)), ("mems A", mems(A)), ("cigar B docs", cigar(B, True)), ("place A", place(A)),
             ("chain B", chain(B)), ("cigar A narrow", cigar(A, False, AlignParams(4))), ("assign A", assign(A)), ("align B docs", align(B, True)),
             ("cigar A docs", cigar(A, True)), ("align A", align(A))]
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
        if name in seen:  # align's result is the same before and after the cigars
            assert all(g.tobytes() == w.tobytes() for g, w in zip(got, seen[name])), name
        seen[name] = got
    # the entries of a cigar call wait for ITS fetch alone, and nothing waits for spm_mems_fetch behind it
    ix.cigar_host(A[0], A[1], 6)
    with pytest.raises(capi.SpxError, match="spm_mems_fetch without a successful spm_mems_begin"):
        capi._check(capi._spm().spm_mems_fetch(ix._h, None, None))
    with pytest.raises(capi.SpxError, match="spg_cigar_fetch without a successful spg_cigar_begin"):
        capi._check(capi._spg().spg_cigar_fetch(ix._h, None, None))
    ix.close()


# ---- the command -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["dna_multiline_fasta", "dna_fastq", "promoted_alphabet_fasta"])
def test_cli_cigar_equals_the_reference_over_the_golden_files(gpu, tmp_path, case):
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
    several = 0
    for extra, min_length, cp, ap, docs in ((["-L", "4", "-d"], 4, ChainParams(), AlignParams(), True),
                                            (["-L", "8", "-F", "3"], 8, ChainParams(), AlignParams(3), False),
                                            (["-L", "4", "-M", "-S", "40", "-G", "3", "-B", "2", "-H", "5", "-F", "4096"], 4, ChainParams(5, 40, 3, 2),
                                             AlignParams(4096), False)):
        if os.path.exists(reads + ".cigars"):
            os.remove(reads + ".cigars")
        r = _cli(["cigar", "-r", ref, "-p", reads, "-n"] + extra, env)
        assert r.returncode == 0, r.stderr.decode()
        m = mems_reference(L, P, offs, min_length, D if docs else None)
        chains, _, pred = chain_reference(m[0], m[1], cp, m[2] if docs else None)
        want, ooffs, ops = cigar_reference(seqs, offs, text, m[0], m[1], chains, pred, ap)
        lines = []
        for q in range(len(ids)):
            w = want[q]
            ok = w["ref_start"] != np.uint64(UNALIGNED)
            f = [ids[q]] + [str(int(x)).encode() for x in (offs[q + 1] - offs[q], w["read_start"], w["read_end"])]
            f += [str(int(w["ref_start"])).encode() if ok else b"-1"]
            f += [str(int(w[x])).encode() for x in ("ref_end", "matches", "edits", "anchors", "unfilled", "skipped")]
            f += [str(int(w["doc"])).encode() if ok else b"-1"] if docs else []
            lines.append(b"\t".join(f + [cigar_text(ops[int(ooffs[q]):int(ooffs[q + 1])]).encode()]) + b"\n")
        assert open(reads + ".cigars", "rb").read() == b"".join(lines), (extra, r.stderr.decode())
        aligned = int((want["ref_start"] != np.uint64(UNALIGNED)).sum())
        assert f"{len(ids)} reads, {aligned} aligned, {len(ids) - aligned} without a match, {ops.size} CIGAR entries".encode() in r.stderr
        several += int((np.diff(ooffs.astype(np.int64)) > 1).sum())
    assert several  # (CIGARs of more than one entry are exercised)
    assert sorted(f for f in os.listdir(work) if f.startswith("reads.fa")) == ["reads.fa", "reads.fa.cigars"]


def test_cli_cigar_cuts_a_full_super_batch_into_calls_of_one_piece(gpu, tmp_path):
    """A super-batch ends with the read that fills it: 32 Mi characters and a few more are two calls of spg_cigar_begin,
    the second one with offsets that do not start at 0 and entries behind the first call's."""
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
    rs[:, 70] = other[rs[:, 70]]  # one substitution: two anchors on one diagonal and a gap of 1 x 1
    reads = str(tmp_path / "reads.fa")
    with open(reads, "wb") as f:
        for i in range(0, nreads, 25_000):
            f.write(b"".join(b">r%d\n%s\n" % (q, rs[q].tobytes()) for q in range(i, i + 25_000)))
    env = dict(os.environ, SPUMONI_GPUS="0", SPUMONI_TEXT=prefix + ".rawtext", SPUMONI_SUPER_BATCH=str(64 << 20))
    r = _cli(["cigar", "-r", prefix[:-3], "-p", reads, "-n", "-L", "20"], env)
    assert r.returncode == 0, r.stderr.decode()
    ix = capi.Index.from_raw(raw, 0)
    half = nreads // 2
    offs = np.arange(0, half * m + 1, m).astype(np.uint64)
    parts = [ix.cigar_host(rs[:half].reshape(-1), offs, 20), ix.cigar_host(rs[half:].reshape(-1), offs, 20)]
    ix.close()
    want = np.concatenate([p[0] for p in parts])
    assert ((want["edits"] == 1) & (want["matches"] == m - 1)).sum() > nreads // 2
    with open(reads + ".cigars", "rb") as f:
        rows = [line.split(b"\t") for line in f]
    assert len(rows) == nreads and all(len(row) == 12 for row in rows[:10] + rows[-10:])
    got = np.array([[int(v) for v in row[1:11]] for row in rows], dtype=np.int64)
    for col, field in enumerate(("read_start", "read_end", "ref_start", "ref_end", "matches", "edits", "anchors", "unfilled", "skipped"), start=1):
        assert np.array_equal(got[:, col], want[field].astype(np.int64)), field
    assert (got[:, 0] == m).all()
    texts = [cigar_text(p[2][int(p[1][q]):int(p[1][q + 1])]).encode() + b"\n" for p in parts for q in range(half)]
    assert [row[11] for row in rows] == texts
    assert sum(t == b"70=1X79=\n" for t in texts) > nreads // 2


def test_cli_cigar_writes_no_file_when_it_fails(gpu, tmp_path):
    work = tmp_path / "c"
    shutil.copytree(os.path.join(FILES, "dna_multiline_fasta"), work)
    text = open(work / "ref.fa.rawtext", "rb").read()
    with open(work / "reads.fa", "wb") as f:  # a read without characters ends the run, as it ends `run`: behind 40 good ones
        for q in range(40):
            f.write(b">r%d\n" % q + text[17 * q: 17 * q + 60] + b"\n")
        f.write(b">bad_one\n>after\n" + text[:40] + b"\n")
    env = dict(os.environ, SPUMONI_TEXT=str(work / "ref.fa.rawtext"), SPUMONI_SUPER_BATCH="1000")
    before = sorted(os.listdir(work))
    r = _cli(["cigar", "-r", str(work / "ref"), "-p", str(work / "reads.fa"), "-n", "-L", "4"], env)
    assert r.returncode == 1 and b"bad_one was empty after digestion" in r.stderr, r.stderr.decode()
    assert sorted(os.listdir(work)) == before
