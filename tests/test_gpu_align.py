"""-m gpu: the alignments (spumoni_amd/csrc/spx_align.hip, include/spumoni_align.h) against the definition
(spumoni_amd/align.py: align_reference), bit for bit: the records, the gap offsets and the whole per-gap table.

align_device gets crafted reads, anchors, chains and pred on an index whose text is handed in; align_host is held to the
oracle's MS arrays -> mems_reference -> chain_reference -> align_reference, and `spumoni align` to the same over the
committed golden files.  The fill gives a gap a lane up to 16 x 16 and a wavefront above, in strips of 64 rows: the
crafted gaps lie around 1, 16, 64 and 128 on either side."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from spumoni_amd import capi, synth
from spumoni_amd.align import ALIGN_DTYPE, GAP_DTYPE, UNALIGNED, UNFILLED, AlignParams, align_reference
from spumoni_amd.chain import CHAIN_DTYPE, NO_DOC, NO_PRED, UNCHAINED, ChainParams, chain_reference
from spumoni_amd.mems import MATCH_DTYPE, mems_reference
from tests import cases
from tests.test_align_cpu import clustered_reads
from tests.test_chain_cpu import planted_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
FILES = os.path.join(ROOT, "tests", "golden", "files")
DNA = list(b"ACGT")
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)
FENCE = -7
K, W = 4, 11
N_TEXT = 2_000_000
RUN_A = 1_000_000  # TEXT[RUN_A : RUN_A + 5000] is a run of 'A'
UNALIGNED_REC = (UNALIGNED, 0, 0, 0, 0, 0, 0, 0, 0, NO_DOC)


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
    """Any index, with the crafted text handed in: the align kernels read the text and nothing else of the index."""
    ix = capi.Index.from_raw(synth.statistical_rlbwt(5000, 60, 4.0, seed=3, with_samples=True, n_docs=8), 0)
    ix.set_text(torch.from_numpy(text.copy()), unchecked=True)
    yield ix
    ix.close()


class Batch:
    """Crafted reads: characters, offsets, anchors, and for every read a chain over ALL of its anchors in order."""

    def __init__(self, front=0):
        self.front = front
        self.reads, self.anchors, self.counts = [], [(7, 7, 7)] * front, []

    def add(self, text, rng, y0, gaps, lengths=None, mutate=0.3):
        """A read of len(gaps) + 1 anchors from text position y0 on; gap t has sides gaps[t] = (a, b): A is B cut or grown to
        a characters with a share of its characters replaced."""
        parts, x, y = [], 0, y0
        for t in range(len(gaps) + 1):
            l = int(lengths[t]) if lengths is not None else int(rng.integers(3, 12))
            parts.append(text[y:y + l])
            self.anchors.append((x, y, l))
            x, y = x + l, y + l
            if t < len(gaps):
                a, b = gaps[t]
                A = np.resize(text[y:y + b], a) if b else LETTERS[rng.integers(0, 4, a)]
                A = np.where(rng.random(a) < mutate, LETTERS[rng.integers(0, 4, a)], A).astype(np.uint8)
                parts.append(A)
                x, y = x + a, y + b
        assert y <= text.size
        self.reads.append(np.concatenate(parts))
        self.counts.append(len(gaps) + 1)

    def add_empty(self, nchars=5):
        self.reads.append(np.full(nchars, ord("N"), dtype=np.uint8))
        self.counts.append(0)

    def arrays(self):
        counts = np.asarray(self.counts, dtype=np.int64)
        moffs = (self.front + np.r_[0, np.cumsum(counts)]).astype(np.uint64)
        roffs = np.r_[0, np.cumsum([r.size for r in self.reads])].astype(np.uint64)
        rec = np.zeros(len(self.anchors) + 2, dtype=MATCH_DTYPE)  # (two records behind the batch)
        if self.anchors:
            rec["read_pos"][:len(self.anchors)], rec["ref_pos"][:len(self.anchors)], rec["length"][:len(self.anchors)] = zip(*self.anchors)
        R = np.concatenate(self.reads) if self.reads else np.zeros(0, dtype=np.uint8)
        chains = np.zeros(counts.size, dtype=CHAIN_DTYPE)
        chains["ref_start"], chains["doc"] = UNCHAINED, NO_DOC
        pred = np.full(rec.size, NO_PRED, dtype=np.uint32)
        for q, h in enumerate(counts):
            if h == 0:
                continue
            o = int(moffs[q])
            first, last = rec[o], rec[o + h - 1]
            chains[q] = (first["ref_pos"], int(last["ref_pos"]) + int(last["length"]), first["read_pos"], int(last["read_pos"]) + int(last["length"]),
                         0, h, 0, h - 1, 0, q % 5)
            pred[o + 1:o + h] = np.arange(h - 1)
        return R, roffs, rec, moffs, chains, pred


def _run(ix, arrays, params=None, cap=None, table=True):
    """align_device with every output fenced; returns (records, gap_offsets, gaps) -- gaps up to min(total, cap)."""
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
    fenced = torch.full((nreads + 3, 12), FENCE, dtype=torch.int32, device="cuda")
    d_goffs = torch.full((nreads + 1 + 4,), FENCE, dtype=torch.int64, device="cuda") if table else None
    d_gaps = torch.full((cap + 4, 4), FENCE, dtype=torch.int32, device="cuda") if table else None
    if table:
        out, _, _ = ix.align_device(d_R, d_roffs, d_rec, d_moffs, d_chains, d_pred, params, gap_capacity=cap, d_out=fenced[:nreads],
                                    d_out_gap_offsets=d_goffs, d_out_gaps=d_gaps)
    else:  # the table lives in the index's scratch
        capi._check(capi._spa().spa_align_device(ix._h, d_R.data_ptr(), d_roffs.data_ptr(), d_rec.data_ptr(), d_moffs.data_ptr(), nreads,
                                                 d_chains.data_ptr(), d_pred.data_ptr(), capi.C.byref(capi.SpaParams(*(params or AlignParams()))),
                                                 cap, fenced.data_ptr(), None, None, None))
        out = fenced[:nreads]
    torch.cuda.synchronize()
    assert (fenced[nreads:] == FENCE).all().item()
    records = out.cpu().numpy().view(ALIGN_DTYPE).reshape(-1)
    if not table:
        return records, None, None
    goffs = d_goffs.cpu().numpy()
    assert (goffs[nreads + 1:] == FENCE).all()
    goffs = goffs[:nreads + 1].view(np.uint64)
    written = min(int(goffs[-1]), cap)
    gaps = d_gaps.cpu().numpy()
    assert (gaps[written:] == FENCE).all()  # nothing is written past the table (or past the capacity)
    return records, goffs, gaps[:written].copy().view(GAP_DTYPE).reshape(-1)


def _check(ix, text, arrays, params=None, table=True, ref=None):
    """ref: what an earlier _check of the same arrays and params returned (the reference is computed once)."""
    R, roffs, rec, moffs, chains, pred = arrays
    if ref is None:
        count = [0]
        ref = align_reference(R, roffs, text, moffs, rec, chains, pred, params, count=count) + (count,)
    want, w_goffs, w_gaps, count = ref
    got, goffs, gaps = _run(ix, arrays, params, table=table)
    if table:
        assert np.array_equal(goffs, w_goffs)
        bad = np.flatnonzero(gaps != w_gaps)
        assert bad.size == 0, (params, bad[:5], gaps[bad[:5]], w_gaps[bad[:5]])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (params, bad[:5], got[bad[:5]], want[bad[:5]])
    st = ix.align_stats()
    ok = want["ref_start"] != np.uint64(UNALIGNED)
    assert st["reads"] == moffs.size - 1 and st["aligned_reads"] == int(ok.sum()) and st["gaps"] == w_gaps.size, st
    assert st["filled_gaps"] == int((w_gaps["edits"] != UNFILLED).sum()) and st["cells"] == count[0], (st, count)
    assert st["error"] == 0 and st["overflow"] == 0 and len(st["step_ms"]) == 4, st
    return ref


SIDES = [0, 1, 2, 16, 17, 63, 64, 65, 129]  # every bin (none, 1 x 1, a lane, a wavefront) and both sides of a strip of 64 rows


def test_every_combination_of_gap_sides_alone_and_mixed_in_one_read(gpu, text, text_index):
    rng = np.random.default_rng(1)
    combos = [(a, b) for a in SIDES for b in SIDES] + [(15, 15), (128, 128), (15, 128), (128, 15)]
    B = Batch(front=3)
    for a, b in combos:
        B.add(text, rng, int(rng.integers(0, 900_000)), [(a, b)])
    mixed = [combos[i] for i in rng.permutation(len(combos))]
    B.add(text, rng, 5000, mixed)  # one read whose gaps mix all bins
    B.add(text, rng, 70_000, [(40, 40), (33, 35)], mutate=0.0)  # A = B, and A = a prefix of B
    arrays = B.arrays()
    ref = _check(text_index, text, arrays)
    want, goffs, gaps, _ = ref
    assert (gaps["matches"] > 0).sum() > 60
    assert gaps[-2].tolist() == (40, 40, 0, 40) and gaps[-1].tolist() == (33, 35, 2, 33)
    assert text_index.align_stats()["cells"] > 200_000
    _check(text_index, text, arrays, table=False, ref=ref)


@pytest.mark.parametrize("max_fill", [1, 16, 512, 4096])
def test_max_fill_with_gaps_at_the_limit_and_one_above(gpu, text, text_index, max_fill):
    rng = np.random.default_rng(2)
    B = Batch()
    m = max_fill
    other = min(m, 20)
    B.add(text, rng, 1000, [(m, other), (m + 1, other), (other, m), (other, m + 1), (1, 1), (0, m), (0, m + 1), (m + 1, 0), (m, 0), (2, 1)])
    B.add(text, rng, 50_000, [(m + 1, m + 1), (3, 3)])
    want, goffs, gaps, _ = _check(text_index, text, B.arrays(), AlignParams(max_fill))
    assert (gaps["edits"] == UNFILLED).tolist()[:10] == [False, True, False, True, False, False, True, True, False, m < 2]
    assert int(want["unfilled"][0]) == 4 + (m < 2) and int(want["skipped"][0]) == 4 * (m + 1) + 2 * (m < 2)
    assert int(want["unfilled"][1]) == 1 + (m < 3)


def test_the_largest_gaps_have_their_closed_forms(gpu, text, text_index):
    """4096 x 4096 with A = B: (0, 4096).  4096 x 3600 within a run of one letter: (496, 3600).  Beside them 4096 x 4096
    of two different letters, (4096, 0), and a gap one above the limit."""
    S = text[200_000:204_096]
    B = Batch()
    B.reads = [np.r_[text[199_990:200_000], S, text[204_096:204_106]],
               np.r_[text[RUN_A - 10:RUN_A], np.full(4096, ord("A"), dtype=np.uint8), text[RUN_A + 3600:RUN_A + 3610]],
               np.r_[text[RUN_A - 10:RUN_A], np.full(4096, ord("C"), dtype=np.uint8), text[RUN_A + 4096:RUN_A + 4106]],
               np.r_[text[300_000:300_010], text[300_010:304_107], text[304_107:304_117]]]
    B.anchors = [(0, 199_990, 10), (4106, 204_096, 10), (0, RUN_A - 10, 10), (4106, RUN_A + 3600, 10),
                 (0, RUN_A - 10, 10), (4106, RUN_A + 4096, 10), (0, 300_000, 10), (4107, 304_107, 10)]
    B.counts = [2, 2, 2, 2]
    got, goffs, gaps = _run(text_index, B.arrays(), AlignParams(4096))
    assert goffs.tolist() == [0, 1, 2, 3, 4]
    assert gaps.tolist() == [(4096, 4096, 0, 4096), (4096, 3600, 496, 3600), (4096, 4096, 4096, 0), (4097, 4097, UNFILLED, 0)]
    assert [(int(r["matches"]), int(r["edits"]), int(r["unfilled"]), int(r["skipped"])) for r in got] == \
        [(4116, 0, 0, 0), (3620, 496, 0, 0), (20, 4096, 0, 0), (20, 0, 1, 4097)]
    st = text_index.align_stats()
    assert st["cells"] == 2 * 4096 * 4096 + 4096 * 3600 and st["filled_gaps"] == 3 and st["gaps"] == 4, st


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
    want, goffs, gaps, _ = _check(text_index, text, B.arrays())
    assert sorted(want["anchors"].tolist())[-3:] == [64, 65, 1000] and (want["ref_start"] == np.uint64(UNALIGNED)).sum() == 12
    assert want[3].tolist()[4:8] == (B.anchors[5][2], 0, 1, 0)  # a chain of one anchor: matches = l, edits = 0


def test_one_chain_of_100000_anchors_among_short_reads(gpu, text, text_index):
    rng = np.random.default_rng(4)
    B = Batch()
    for q in range(2001):
        if q == 1000:
            B.add(text, rng, 10_000, [(int(a), int(b)) for a, b in rng.integers(0, 4, (99_999, 2))], lengths=rng.integers(3, 9, 100_000))
        else:
            h = int(rng.integers(0, 6))
            B.add(text, rng, int(rng.integers(0, 900_000)), [(int(a), int(b)) for a, b in rng.integers(0, 20, (h - 1, 2))]) if h else B.add_empty()
    want, goffs, gaps, _ = _check(text_index, text, B.arrays())
    assert int(want["anchors"][1000]) == 100_000 and int(goffs[1001] - goffs[1000]) == 99_999


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
    _check(text_index, text, B.arrays(), AlignParams(8), table=False)


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
    want, goffs, gaps, _ = _check(text_index, text, B.arrays())
    assert gaps.tolist()[:3] == [(0, 2, 2, 0), (2, 0, 2, 0), (0, 10, 10, 0)], gaps[:3]
    assert want[0].tolist()[:7] == (1000, 1070, 0, 60, 20 + 14 + 6 + 18, 14, 4)
    assert gaps[3]["a"] == 18 and gaps[3]["b"] == 20 and gaps[3]["edits"] != UNFILLED
    assert gaps.tolist()[4:] == [(5, 0, 5, 0), (15, 0, 15, 0)] and int(want["ref_end"][2]) == Y + 40 and int(want["ref_start"][2]) == Y


@pytest.mark.parametrize("cap", [0, 5, 4, 6, 16], ids=["zero", "one_short", "inside_a_read", "exact", "above"])
def test_gap_capacity_zero_short_exact_and_above(gpu, text, text_index, cap):
    """A read whose gaps do not all fit comes back unaligned, nothing is written past the capacity, and the stats say so."""
    rng = np.random.default_rng(6)
    B = Batch()
    for gaps in ([(3, 4), (20, 20)], [], [(5, 5)], [(2, 2), (1, 1), (0, 3)]):
        B.add(text, rng, int(rng.integers(0, 900_000)), gaps)
    arrays = B.arrays()
    want, w_goffs, w_gaps = align_reference(arrays[0], arrays[1], text, arrays[3], arrays[2], arrays[4], arrays[5])
    total = int(w_goffs[-1])
    assert w_goffs.tolist() == [0, 2, 2, 3, 6]
    got, goffs, gaps = _run(text_index, arrays, cap=cap)
    assert np.array_equal(goffs, w_goffs)
    fits = (w_goffs[1:] <= cap) | (np.diff(w_goffs.astype(np.int64)) == 0)  # (a chain of one anchor has no gaps: it always fits)
    assert np.array_equal(got[fits], want[fits]) and all(r.tolist() == UNALIGNED_REC for r in got[~fits])
    whole = int(w_goffs[1:][w_goffs[1:] <= cap].max(initial=0))
    assert np.array_equal(gaps[:whole], w_gaps[:whole]) and gaps.size == min(cap, total)
    assert not gaps[whole:].view(np.uint32).any()  # (the places of a read that does not fit, below the capacity: empty gaps)
    st = text_index.align_stats()
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
    want = align_reference(R, roffs, text, moffs, rec, chains, pred)
    assert np.array_equal(a[0], want[0]) and np.array_equal(a[2], want[2])
    assert other.align_stats()["gaps"] == want[2].size and text_index.align_stats()["reads"] == 150
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
            text_index.align_host(np.frombuffer(b"ACGT", dtype=np.uint8), [0, 4], 1, params=bad)
    with pytest.raises(capi.SpxError, match="spx error -1: lookback must be 1 .. 64"):
        text_index.align_host(np.frombuffer(b"ACGT", dtype=np.uint8), [0, 4], 1, chain_params=(0, 5000, 500, 1))
    with pytest.raises(capi.SpxError, match="gap_capacity must be at most"):
        _run_raw(text_index, arrays, cap=2**32)
    S = capi._spa()
    p = capi.SpaParams(512)
    t = [torch.zeros(64, dtype=torch.int64, device="cuda") for _ in range(7)]
    ptr = [x.data_ptr() for x in t]
    args = lambda **kw: [kw.get("ix", text_index._h), kw.get("R", ptr[0]), kw.get("ro", ptr[1]), kw.get("M", ptr[2]), kw.get("mo", ptr[3]), 1,
                         kw.get("ch", ptr[4]), kw.get("pred", ptr[5]), kw.get("p", p), 4, kw.get("out", ptr[6]), None, None, None]
    for kw in (dict(ix=None), dict(p=None), dict(R=None), dict(ro=None), dict(M=None), dict(mo=None), dict(ch=None), dict(pred=None), dict(out=None)):
        assert S.spa_align_device(*args(**kw)) == -1, kw
    assert b"must be non-null" in capi.lib().spx_last_error()
    for kw in (dict(M=ptr[2] + 8), dict(ch=ptr[4] + 8), dict(out=ptr[6] + 4), dict(ro=ptr[1] + 4), dict(mo=ptr[3] + 4), dict(pred=ptr[5] + 2)):
        assert S.spa_align_device(*args(**kw)) == -1, kw
        assert b"16-byte aligned" in capi.lib().spx_last_error()
    assert S.spa_last_align_stats(text_index._h, None) == -1 and S.spa_last_align_stats(None, None) == -1
    # an index without the text; the host form's own checks and the limits of one piece
    bare = capi.Index.from_raw(synth.statistical_rlbwt(2000, 20, 3.0, seed=1, with_samples=True, n_docs=4), 0)
    with pytest.raises(capi.SpxError, match="spx_index_set_text / spx_index_rebuild_text"):
        _run(bare, arrays)
    seqs, one = np.frombuffer(b"ACGT", dtype=np.uint8), [0, 4]
    with pytest.raises(capi.SpxError, match="spx_index_set_text / spx_index_rebuild_text"):
        bare.align_host(seqs, one, 1)
    with pytest.raises(capi.SpxError, match="no alignments have been computed"):
        bare.align_stats()
    bare.set_text(torch.from_numpy(np.full(5000, 65, dtype=np.uint8)), unchecked=True)
    with pytest.raises(capi.SpxError, match="spx error -1: min_length must be at least 1"):
        bare.align_host(seqs, one, 0)
    with pytest.raises(capi.SpxError, match="digest_kind must be"):
        bare.align_host(seqs, one, 1, digest=(7, 4, 11))
    with pytest.raises(capi.SpxError, match="spx error -1: one piece per call"):
        bare.align_host(seqs, np.zeros((4 << 20) + 2, dtype=np.uint64), 1)
    with pytest.raises(capi.SpxError, match="spx error -1: one piece per call"):
        bare.align_host(seqs, [0, (32 << 20) + 1], 1)
    bare.close()


def _run_raw(ix, arrays, cap):
    R, roffs, rec, moffs, chains, pred = arrays
    z = torch.zeros(64, dtype=torch.int64, device="cuda")
    return ix.align_device(z, z, z, z, z, z, None, gap_capacity=cap, d_out=z, d_out_gap_offsets=z, d_out_gaps=z)


# ---- bad input: refused by the walk's checks, unaligned, SPX_E_FORMAT, fences intact -----------------------------------
def _bad_batch(text):
    """Three reads; the middle one is the one a test spoils."""
    rng = np.random.default_rng(9)
    B = Batch(front=2)
    B.add(text, rng, 1000, [(2, 3), (20, 20)])
    B.add(text, rng, 5000, [(3, 3), (1, 1), (0, 2), (18, 17)])
    B.add(text, rng, 9000, [(5, 5)])
    return B


def _refused(ix, text, arrays):
    """The spoiled read comes back unaligned with its places in the table empty, the others as the reference has them."""
    R, roffs, rec, moffs, chains, pred = arrays
    got, goffs, gaps = _run(ix, arrays)  # (the fences are _run's)
    with pytest.raises(capi.SpxError, match="spx error -5: a read's chain failed the walk's checks"):
        ix.align_stats()
    good = _bad_batch(text).arrays()
    want, w_goffs, w_gaps = align_reference(good[0], good[1], text, good[3], good[2], good[4], good[5])
    assert got[1].tolist() == UNALIGNED_REC and got[0] == want[0] and got[2] == want[2]
    lo, hi = int(goffs[1]), int(goffs[2])
    assert np.array_equal(gaps[:lo], w_gaps[:int(w_goffs[1])]) and np.array_equal(gaps[hi:], w_gaps[int(w_goffs[2]):])
    assert not gaps[lo:hi].view(np.uint32).any()


def test_a_pred_that_does_not_decrease_is_refused(gpu, text, text_index):
    arrays = _bad_batch(text).arrays()
    o = int(arrays[3][1])
    arrays[5][o + 3] = 3  # anchor 3 names itself
    _refused(text_index, text, arrays)
    arrays[5][o + 3] = 4  # ... and its successor
    _refused(text_index, text, arrays)


def test_a_pred_outside_the_read_is_refused(gpu, text, text_index):
    arrays = _bad_batch(text).arrays()
    o = int(arrays[3][1])
    arrays[5][o + 2] = 2**31 + 5
    _refused(text_index, text, arrays)
    arrays = _bad_batch(text).arrays()
    arrays[4]["first"][1] = 2  # pred walks below `first`
    arrays[4]["anchors"][1] = 3
    arrays[5][o + 3] = 1
    _refused(text_index, text, arrays)
    arrays = _bad_batch(text).arrays()
    arrays[4]["last"][1] = 5  # `last` is not one of the read's anchors
    _refused(text_index, text, arrays)


def test_more_anchors_than_the_walk_finds_are_refused(gpu, text, text_index):
    arrays = _bad_batch(text).arrays()
    o = int(arrays[3][1])
    arrays[5][o + 2] = NO_PRED  # the chain ends after three of its five anchors
    _refused(text_index, text, arrays)
    arrays = _bad_batch(text).arrays()
    arrays[4]["anchors"][1] = 4  # ... or goes on beyond them: the walk does not end at `first`
    _refused(text_index, text, arrays)
    arrays = _bad_batch(text).arrays()
    arrays[4]["anchors"][1] = 6  # more anchors than the read has records
    got, goffs, gaps = _run(text_index, arrays)
    with pytest.raises(capi.SpxError, match="spx error -5"):
        text_index.align_stats()
    assert got[1].tolist() == UNALIGNED_REC and int(goffs[2] - goffs[1]) == 0 and int(goffs[-1]) == 3


def test_a_link_of_negative_length_is_refused(gpu, text, text_index):
    """Anchor 2 ends in the read before anchor 1 does: ex < 1, the gap in the read would have a negative length."""
    arrays = _bad_batch(text).arrays()
    o = int(arrays[3][1])
    arrays[2]["read_pos"][o + 2] = 1
    arrays[2]["length"][o + 2] = 2
    _refused(text_index, text, arrays)
    arrays = _bad_batch(text).arrays()
    arrays[2]["ref_pos"][o + 2] = 4000  # ... and the same in the text
    _refused(text_index, text, arrays)
    arrays = _bad_batch(text).arrays()
    arrays[2]["length"][o + 4] = 10_000  # the chain's last anchor ends outside the read
    _refused(text_index, text, arrays)


def test_a_gap_past_the_texts_end_is_refused(gpu, text, text_index):
    arrays = _bad_batch(text).arrays()
    o = int(arrays[3][1])
    arrays[2]["ref_pos"][o + 4] = N_TEXT + 1  # the gap in front of it would end one character past the text
    arrays[4]["ref_end"][1] = N_TEXT + 1 + int(arrays[2]["length"][o + 4])
    _refused(text_index, text, arrays)
    arrays = _bad_batch(text).arrays()
    arrays[2]["ref_pos"][o + 3:o + 5] += np.uint64(1 << 41)  # ... or begin far behind it
    _refused(text_index, text, arrays)


# ---- align_host against the oracle -> mems_reference -> chain_reference -> align_reference ------------------------------
def _host_check(ix, orc, text, seqs, offs, min_length, chain_params=None, params=None, digest=None, want_docs=False, oracle_mod=None):
    kind = digest[0] if digest else 0
    dseqs, doffs = oracle_mod.digest_batch(kind, digest[1], digest[2], seqs, offs) if kind else (seqs, offs)
    ms = orc.ms(dseqs, doffs, want_docs=want_docs, text=text)
    m = mems_reference(ms["lengths"], ms["pointers"], doffs, min_length, ms["docs"] if want_docs else None)
    w_chains, _, pred = chain_reference(m[0], m[1], chain_params, m[2] if want_docs else None)
    count = [0]
    want, w_goffs, w_gaps = align_reference(dseqs, doffs, text, m[0], m[1], w_chains, pred, params, count=count)
    got, chains, vals = ix.align_host(seqs, offs, min_length, chain_params, params, digest=digest, want_docs=want_docs)
    bad = np.flatnonzero(got != want)
    assert got.dtype == ALIGN_DTYPE and bad.size == 0, (min_length, params, bad[:5], got[bad[:5]], want[bad[:5]])
    assert np.array_equal(chains, w_chains) and np.array_equal(vals, np.diff(doffs.astype(np.int64)))
    assert np.array_equal(chains, ix.chain_host(seqs, offs, min_length, chain_params, digest=digest, want_docs=want_docs)[0])
    st = ix.align_stats()
    assert st["reads"] == len(offs) - 1 and st["gaps"] == w_gaps.size and st["cells"] == count[0], (st, count)
    assert st["aligned_reads"] == int((want["anchors"] > 0).sum()) and st["filled_gaps"] == int((w_gaps["edits"] != UNFILLED).sum()), st
    return want, w_gaps


@pytest.mark.parametrize("kind", [0, capi.SPX_DIGEST_PROMOTED, capi.SPX_DIGEST_DNA])
def test_align_host_on_an_index_from_the_oracles_side(gpu, oracle_mod, kind):
    """Several documents; DNA reads through digestion, walk, MS extension, the matches, the chaining and the gaps in one
    call, 16-bit arrays and -- with a read of 70 000 characters -- 32-bit."""
    rng = np.random.default_rng(80 + kind)
    genome = cases.repetitive_text(rng, 40_000, DNA)
    text = oracle_mod.digest(kind, K, W, genome) if kind else genome
    cuts = [text.size // 5, text.size // 2, text.size - text.size // 5 - text.size // 2]
    raw = synth.index_from_text(torch.from_numpy(text), doc_lengths=cuts)
    orc = oracle_mod.OracleIndex.from_raw(raw)
    ix = capi.Index.from_raw(raw, 0)
    ix.set_text(torch.from_numpy(text.copy()))
    seqs, offs = cases.reads_mixed(rng, genome, DNA, 300, 500, [ord("N")])
    long_read = np.concatenate([genome[s:s + 7000] for s in np.sort(rng.integers(0, 30_000, 10))])
    long_read[rng.integers(0, long_read.size, 700)] = ord("N")
    wide = (np.r_[seqs[: int(offs[50])], long_read], np.r_[offs[:51], offs[50] + long_read.size])
    digest = (kind, K, W) if kind else None
    gaps_seen = tables = 0
    for s, o in ((seqs, offs), wide):
        o = o.astype(np.uint64)
        for min_length, cp, ap, want_docs in ((6, None, None, True), (12, ChainParams(64, 5000, 500, 0), AlignParams(8), False),
                                              (10**6, None, None, True)):
            want, gaps = _host_check(ix, orc, text, s, o, min_length, cp, ap, digest, want_docs, oracle_mod)
            gaps_seen += gaps.size
            tables += int(((gaps["a"] > 1) & (gaps["b"] > 1) & (gaps["edits"] != UNFILLED)).sum())
            if min_length == 10**6:
                assert (want["ref_start"] == np.uint64(UNALIGNED)).all()
    assert gaps_seen > 100 and tables > 5
    got, chains, vals = ix.align_host(np.zeros(0, dtype=np.uint8), [0], 4)
    assert got.size == 0 and ix.align_stats()["reads"] == 0
    ix.close()


def test_align_host_on_a_text_built_on_the_device_and_both_planted_sets(gpu, oracle_mod):
    text, seqs, offs, cuts = planted_reads()
    raw = capi.build_raw(text)
    ix = capi.Index.from_raw(raw, 0)
    want, gaps = _host_check(ix, oracle_mod.OracleIndex.from_raw(raw), text, seqs, offs, 12, oracle_mod=oracle_mod)
    assert all((int(r["edits"]), int(r["matches"]), int(r["unfilled"])) == (7, 298, 0) for r in want)
    ix.close()
    text, seqs, offs = clustered_reads()
    raw = capi.build_raw(text)
    ix = capi.Index.from_raw(raw, 0)
    want, gaps = _host_check(ix, oracle_mod.OracleIndex.from_raw(raw), text, seqs, offs, 12, oracle_mod=oracle_mod)
    assert ((gaps["a"] >= 8) & (gaps["b"] >= 8) & (gaps["a"] != gaps["b"])).any() and (gaps["matches"] > 0).any()
    ix.close()


def test_the_five_products_interleaved_on_one_handle(gpu):
    rng = np.random.default_rng(90)
    genome = cases.repetitive_text(rng, 40_000, DNA)
    cuts = [genome.size // 3, genome.size - genome.size // 3]
    raw = capi.build_raw(genome, doc_lengths=cuts)
    seqs, offs = cases.reads_mixed(rng, genome, DNA, 300, 500, [ord("N")])
    A = (seqs, offs.astype(np.uint64))
    long_read = np.tile(genome, 2)[:70_000].copy()
    long_read[rng.integers(0, long_read.size, 300)] = ord("N")
    B = (np.r_[seqs[: int(offs[20])], long_read], np.r_[offs[:21], offs[20] + long_read.size].astype(np.uint64))

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

    steps = [("align A", align(A)), ("mems A", mems(A)), ("align B docs", align(B, True)), ("place A", place(A)), ("chain B", chain(B)),
             ("align A narrow", align(A, False, AlignParams(4))), ("assign A", assign(A)), ("mems B", mems(B)), ("align A docs", align(A, True))]
    ix = capi.Index.from_raw(raw, 0)
    for name, step in steps:
        got, got_stats = step(ix)
        fresh = capi.Index.from_raw(raw, 0)
        want, want_stats = step(fresh)
        fresh.close()
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (name, i)
        for s in (got_stats, want_stats):
            s.pop("kernel_ms", None)
            s.pop("step_ms", None)
        assert got_stats == want_stats, (name, got_stats, want_stats)
    # the records of an align call are that call's own: nothing waits for spm_mems_fetch behind it
    ix.align_host(A[0], A[1], 6)
    with pytest.raises(capi.SpxError, match="spm_mems_fetch without a successful spm_mems_begin"):
        capi._check(capi._spm().spm_mems_fetch(ix._h, None, None))
    ix.close()


# ---- the command -------------------------------------------------------------------------------------------------------
def _parse_values(path):
    ids, vals = [], []
    with open(path, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                ids.append(line[1:-1])
            else:
                vals.append(np.array(line.split(), dtype=np.uint64))
    return ids, vals


def _cli(args, env):
    return subprocess.run([HOST_BIN] + args, capture_output=True, env=env, timeout=300)  # (every child has its time limit)


@pytest.mark.parametrize("case", ["dna_multiline_fasta", "dna_fastq", "promoted_alphabet_fasta"])
def test_cli_align_equals_the_reference_over_the_golden_files(gpu, tmp_path, case):
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
    filled_any = 0
    for extra, min_length, cp, ap, docs in ((["-L", "4", "-d"], 4, ChainParams(), AlignParams(), True),
                                            (["-L", "8", "-F", "3"], 8, ChainParams(), AlignParams(3), False),
                                            (["-L", "4", "-M", "-S", "40", "-G", "3", "-B", "2", "-H", "5", "-F", "4096"], 4, ChainParams(5, 40, 3, 2),
                                             AlignParams(4096), False)):
        if os.path.exists(reads + ".alignments"):
            os.remove(reads + ".alignments")
        r = _cli(["align", "-r", ref, "-p", reads, "-n"] + extra, env)
        assert r.returncode == 0, r.stderr.decode()
        m = mems_reference(L, P, offs, min_length, D if docs else None)
        chains, _, pred = chain_reference(m[0], m[1], cp, m[2] if docs else None)
        want, _, gaps = align_reference(seqs, offs, text, m[0], m[1], chains, pred, ap)
        lines = []
        for q in range(len(ids)):
            w = want[q]
            ok = w["ref_start"] != np.uint64(UNALIGNED)
            f = [ids[q]] + [str(int(x)).encode() for x in (offs[q + 1] - offs[q], w["read_start"], w["read_end"])]
            f += [str(int(w["ref_start"])).encode() if ok else b"-1"]
            f += [str(int(w[x])).encode() for x in ("ref_end", "matches", "edits", "anchors", "unfilled", "skipped")]
            lines.append(b"\t".join(f + ([str(int(w["doc"])).encode() if ok else b"-1"] if docs else [])) + b"\n")
        assert open(reads + ".alignments", "rb").read() == b"".join(lines), (extra, r.stderr.decode())
        aligned = int((want["ref_start"] != np.uint64(UNALIGNED)).sum())
        assert f"{len(ids)} reads, {aligned} aligned, {len(ids) - aligned} without a match".encode() in r.stderr
        filled_any += int((gaps["edits"] != UNFILLED).sum())
    assert filled_any  # (chains of more than one anchor are exercised)
    assert sorted(f for f in os.listdir(work) if f.startswith("reads.fa")) == ["reads.fa", "reads.fa.alignments"]


def _sequences(path, offs):
    """The reads of a FASTA or FASTQ file as the walk sees them: the sequence lines joined, upper-cased and concatenated
    (FASTQ: the reference drops the file's last batch, and so does the command)."""
    lines = open(path, "rb").read().split(b"\n")
    reads = []
    if lines[0].startswith(b"@"):
        reads = [lines[i + 1].upper() for i in range(0, len(lines) - 3, 4)]
    else:
        for line in lines:
            if line.startswith(b">"):
                reads.append(b"")
            elif reads:
                reads[-1] += line.upper()
    reads = reads[: offs.size - 1]
    assert [len(r) for r in reads] == np.diff(offs.astype(np.int64)).tolist()
    return np.frombuffer(b"".join(reads), dtype=np.uint8)


def test_cli_align_cuts_a_full_super_batch_into_calls_of_one_piece(gpu, tmp_path):
    """A super-batch ends with the read that fills it: 32 Mi characters and a few more are two calls of spa_align_batch,
    the second one with offsets that do not start at 0."""
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
    r = _cli(["align", "-r", prefix[:-3], "-p", reads, "-n", "-L", "20"], env)
    assert r.returncode == 0, r.stderr.decode()
    ix = capi.Index.from_raw(raw, 0)
    half = nreads // 2
    offs = np.arange(0, half * m + 1, m).astype(np.uint64)
    want = np.concatenate([ix.align_host(rs[:half].reshape(-1), offs, 20)[0], ix.align_host(rs[half:].reshape(-1), offs, 20)[0]])
    ix.close()
    assert ((want["edits"] == 1) & (want["matches"] == m - 1)).sum() > nreads // 2
    got = np.loadtxt(reads + ".alignments", dtype=np.int64, usecols=range(1, 11))
    assert got.shape == (nreads, 10)
    for col, field in enumerate(("read_start", "read_end", "ref_start", "ref_end", "matches", "edits", "anchors", "unfilled", "skipped"), start=1):
        assert np.array_equal(got[:, col], want[field].astype(np.int64)), field
    assert (got[:, 0] == m).all()


def test_cli_align_writes_no_file_when_it_fails(gpu, tmp_path):
    work = tmp_path / "c"
    shutil.copytree(os.path.join(FILES, "dna_multiline_fasta"), work)
    text = open(work / "ref.fa.rawtext", "rb").read()
    with open(work / "reads.fa", "wb") as f:  # a read without characters ends the run, as it ends `run`: behind 40 good ones
        for q in range(40):
            f.write(b">r%d\n" % q + text[17 * q: 17 * q + 60] + b"\n")
        f.write(b">bad_one\n>after\n" + text[:40] + b"\n")
    env = dict(os.environ, SPUMONI_TEXT=str(work / "ref.fa.rawtext"), SPUMONI_SUPER_BATCH="1000")
    before = sorted(os.listdir(work))
    r = _cli(["align", "-r", str(work / "ref"), "-p", str(work / "reads.fa"), "-n", "-L", "4"], env)
    assert r.returncode == 1 and b"bad_one was empty after digestion" in r.stderr, r.stderr.decode()
    assert sorted(os.listdir(work)) == before
