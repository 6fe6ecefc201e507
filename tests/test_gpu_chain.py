"""-m gpu: the chains (spumoni_amd/csrc/spx_chain.hip, include/spumoni_chain.h) against the definition
(spumoni_amd/chain.py: chain_reference), bit for bit: the records, and f and pred of every anchor.

chain_device gets crafted anchors (the rule is one on the records, and no index array is read: any handle will do);
chain_host is held to chain_reference over what mems_host returns for the same reads, and `spumoni chain` to
chain_reference over mems_reference of the committed golden files.  The kernel gives a read of up to 16 anchors a group
of 16 lanes and a longer one the whole wavefront with a ring of 64: the crafted reads, ties and limits lie around each."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from spumoni_amd import capi, synth
from spumoni_amd.chain import CHAIN_DTYPE, NO_DOC, NO_PRED, UNCHAINED, ChainParams, chain_reference
from spumoni_amd.mems import MATCH_DTYPE, mems_reference
from tests import cases
from tests.test_chain_cpu import planted_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
FILES = os.path.join(ROOT, "tests", "golden", "files")
DNA = list(b"ACGT")
FENCE = -7
K, W = 4, 11


@pytest.fixture(scope="module")
def gpu(built_all):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    capi.lib()
    return 0


@pytest.fixture(scope="module")
def any_index(gpu):
    ix = capi.Index.from_raw(synth.statistical_rlbwt(5000, 60, 4.0, seed=3, with_samples=True, n_docs=8), 0)
    yield ix
    ix.close()


def _recs(x, y, l):
    rec = np.zeros(len(x), dtype=MATCH_DTYPE)
    rec["read_pos"], rec["ref_pos"], rec["length"] = x, y, l
    return rec


def _run(ix, offs, rec, params=None, D=None, table=True):
    """chain_device with every output fenced; returns (chains, score, pred) with score / pred None when not asked for."""
    offs = np.asarray(offs, dtype=np.uint64)
    nreads, n = offs.size - 1, rec.size
    d_rec = torch.from_numpy(np.concatenate([rec, np.zeros(1, dtype=MATCH_DTYPE)]).view(np.int32).reshape(-1, 4).copy()).cuda()[:n]
    d_offs = torch.from_numpy(offs.view(np.int64).copy()).cuda()
    d_D = None if D is None else torch.from_numpy(np.concatenate([np.asarray(D, dtype=np.uint32), np.zeros(1, dtype=np.uint32)]).view(np.int32).copy()).cuda()[:n]
    fenced = torch.full((nreads + 3, 12), FENCE, dtype=torch.int32, device="cuda")
    d_score = torch.full((n + 5,), FENCE, dtype=torch.int32, device="cuda") if table else None
    d_pred = torch.full((n + 5,), FENCE, dtype=torch.int32, device="cuda") if table else None
    out = ix.chain_device(d_rec, d_offs, params, d_match_docs=d_D, d_out=fenced[:nreads], d_out_score=d_score, d_out_pred=d_pred)
    torch.cuda.synchronize()
    assert (fenced[nreads:] == FENCE).all().item()
    chains = out.cpu().numpy().view(CHAIN_DTYPE).reshape(-1)
    if not table:
        return chains, None, None
    lo, hi = (int(offs[0]), int(offs[-1])) if nreads > 0 else (0, 0)
    score, pred = d_score.cpu().numpy(), d_pred.cpu().numpy()
    for a in (score, pred):  # nothing is written outside the batch's anchors
        assert (a[:lo] == FENCE).all() and (a[hi:] == FENCE).all()
    return chains, score[lo:hi].view(np.uint32), pred[lo:hi].view(np.uint32)


def _check(ix, offs, rec, params=None, D=None, table=True):
    count = [0]
    want, w_score, w_pred = chain_reference(offs, rec, params, D, count=count)
    got, score, pred = _run(ix, offs, rec, params, D, table)
    offs = np.asarray(offs, dtype=np.int64)
    lo, hi = (int(offs[0]), int(offs[-1])) if offs.size > 1 else (0, 0)
    if table:
        bad = np.flatnonzero((score != w_score[lo:hi]) | (pred != w_pred[lo:hi]))
        assert bad.size == 0, (params, bad[:5] + lo, score[bad[:5]], w_score[lo:hi][bad[:5]], pred[bad[:5]], w_pred[lo:hi][bad[:5]])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (params, bad[:5], np.diff(offs)[bad[:5]], got[bad[:5]], want[bad[:5]])
    st = ix.chain_stats()
    assert st["reads"] == offs.size - 1 and st["anchors"] == hi - lo, st
    assert st["chained_reads"] == int((want["anchors"] > 0).sum()) and st["chain_anchors"] == int(want["anchors"].sum()), st
    assert st["candidates"] == count[0], (st, count)
    return want, w_score, w_pred


def _batch(rng, counts, front=0, step=40, spread=3, y0=1000, n_docs=0):
    """Reads of counts[q] anchors that mostly follow a diagonal with small indels: some anchors out of order, some overlapping,
    some equal lengths (ties); `front` records in front of the batch and 3 behind it."""
    counts = np.asarray(counts, dtype=np.int64)
    offs = (front + np.r_[0, np.cumsum(counts)]).astype(np.uint64)
    n = int(offs[-1]) + 3
    x, y, l = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), rng.integers(1, 60, n)
    l[rng.random(n) < 0.5] = 20
    for o, h in zip(offs[:-1].astype(np.int64), counts):
        xs = np.sort(rng.integers(0, step * max(int(h), 1), int(h)))
        ys = y0 + int(rng.integers(0, 1000)) + xs + np.cumsum(rng.integers(-spread, spread + 1, int(h)))
        swap = rng.random(int(h)) < 0.08
        ys[swap] = y0 + rng.integers(0, 3000, int(swap.sum()))
        x[o:o + h], y[o:o + h] = xs, ys
    D = rng.integers(0, n_docs, n) if n_docs else None
    return offs, _recs(x, y, l), D


EDGES = [0, 1, 2, 15, 16, 17, 63, 64, 65, 66, 128, 129, 1000]
PARAMS = [ChainParams(), ChainParams(1, 5000, 500, 1), ChainParams(2, 5000, 500, 0), ChainParams(63, 300, 4, 2),
          ChainParams(64, 2**31 - 1, 2**31 - 1, 65535), ChainParams(64, 5000, 0, 1)]


def test_reads_of_every_anchor_count(gpu, any_index):
    rng = np.random.default_rng(1)
    counts = np.array(EDGES * 2 + list(range(3, 15)))
    counts = counts[rng.permutation(counts.size)]
    counts = np.r_[[0, 0, 0], counts[:15], [0] * 5, counts[15:], [5, 0, 0, 61, 0, 0, 0, 0]]  # anchor-less runs: front, middle, end
    offs, rec, D = _batch(rng, counts, front=7, n_docs=3)
    for i, params in enumerate(PARAMS):
        want, score, pred = _check(any_index, offs, rec, params, D if i % 2 == 0 else None, table=i != 3)
        assert (want["ref_start"] == np.uint64(UNCHAINED)).sum() == (counts == 0).sum()
        if params == ChainParams():
            assert int(want["anchors"].max()) > 64  # the ring wrapped inside one chain
    assert set(want["doc"][counts > 0].tolist()) == {NO_DOC}


def test_one_read_of_100000_anchors_among_short_ones(gpu, any_index):
    rng = np.random.default_rng(2)
    counts = rng.integers(0, 7, 2001)
    counts[1000] = 100_000
    offs, rec, _ = _batch(rng, counts, step=1000)  # (x steps of about 1000: five predecessors or so in reach of max_dist)
    want, _, _ = _check(any_index, offs, rec)
    total = any_index.chain_stats()["candidates"]  # (equal to the reference's count: _check)
    o, e = int(offs[1000]), int(offs[1001])
    count_short = [0]
    chain_reference(np.r_[offs[:1001], offs[1001:] - np.uint64(e - o)], np.concatenate([rec[:o], rec[e:]]), None, count=count_short)
    assert 0 < count_short[0] < total  # both paths took reads, and their pairs add up
    assert int(want["anchors"][1000]) > 64


@pytest.mark.parametrize("nreads", [0, 1, 3, 4, 5, 63, 64, 65, 3000])
def test_read_counts_around_the_group_count(gpu, any_index, nreads):
    rng = np.random.default_rng(nreads)
    offs, rec, D = _batch(rng, rng.integers(0, 40, nreads), front=nreads % 3, n_docs=2)
    _check(any_index, offs, rec, None, D)
    _check(any_index, offs, rec, ChainParams(7, 100, 2, 3), None, table=False)


def _embedded(pairs, pad):
    """Every pair of anchors as a read of its own, `pad` anchors in front that nothing chains with (y falls)."""
    x, y, l, counts = [], [], [], []
    for (a, b) in pairs:
        for t in range(pad):
            x.append(t)
            y.append(10**9 - 10 * t)
            l.append(3)
        for (ax, ay, al) in (a, b):
            x.append(pad + 10 + ax)
            y.append(ay)
            l.append(al)
        counts.append(pad + 2)
    return np.r_[0, np.cumsum(counts)].astype(np.uint64), _recs(x, y, l)


@pytest.mark.parametrize("pad", [0, 14, 15, 40, 70], ids=["group", "group16", "wavefront17", "wavefront", "wrapped"])
def test_limits_of_distance_and_gap(gpu, any_index, pad):
    """dx and dy at max_dist and one above, d at max_gap and one above, max_gap 0; with a penalty of 0 and of 65535 and
    d near 2^31; y near 2^40."""
    Y = 1 << 40
    a = (0, Y, 10)
    pairs = [(a, (5000, Y + 5000, 10)), (a, (5001, Y + 5001, 10)), (a, (5000, Y + 4990, 10)), (a, (4990, Y + 5001, 10)),
             (a, (20, Y + 520, 10)), (a, (20, Y + 521, 10)), (a, (520, Y + 20, 10)), (a, (521, Y + 20, 10)),
             (a, (20, Y + 20, 10)), (a, (20, Y + 21, 10)), (a, (20, Y + 19, 10))]
    offs, rec = _embedded(pairs, pad)
    want, score, _ = _check(any_index, offs, rec, ChainParams(gap_penalty=0))
    assert score[pad + 1::pad + 2].tolist() == [20, 10, 20, 10, 20, 10, 20, 10, 20, 20, 20]
    want, score, _ = _check(any_index, offs, rec, ChainParams(max_gap=0))
    assert score[pad + 1::pad + 2].tolist() == [20, 10, 10, 10, 10, 10, 10, 10, 20, 10, 10]
    # d near 2^31: free of charge it chains and the gaps add up past 2^32 (the sum saturates); at 65535 a unit nothing chains
    wide = 2**31 - 1
    x = np.arange(4) * 5 + 1
    y = Y + np.arange(4) * wide
    far_offs, far = np.array([0, 4], dtype=np.uint64), _recs(x, y, [5, 5, 5, 5])
    if pad:
        far_offs, far = np.array([0, pad + 4], dtype=np.uint64), np.concatenate([rec[:pad], far])
        far["read_pos"][pad:] += pad + 10
    want, score, pred = _check(any_index, far_offs, far, ChainParams(64, wide, wide, 0))
    assert score[pad:].tolist() == [5, 10, 15, 20] and int(want["gap"][0]) == 2**32 - 1 and int(want["anchors"][0]) == 4
    want, score, pred = _check(any_index, far_offs, far, ChainParams(64, wide, wide, 65535))
    assert score[pad:].tolist() == [5, 5, 5, 5] and (pred == NO_PRED).all() and int(want["first"][0]) == pad


def test_ids_equal_alternating_and_absent(gpu, any_index):
    rng = np.random.default_rng(4)
    offs, rec, _ = _batch(rng, [3, 16, 17, 40, 0, 100, 8], front=2)
    n = rec.size
    same, _, _ = _check(any_index, offs, rec, None, np.full(n, 65535))
    none, _, _ = _check(any_index, offs, rec, None, None)
    alt, _, _ = _check(any_index, offs, rec, None, np.arange(n) % 2)
    full = np.diff(offs.astype(np.int64)) > 0
    assert np.array_equal(same["score"], none["score"]) and (same["doc"][full] == 65535).all() and (none["doc"] == NO_DOC).all()
    assert (alt["score"] <= none["score"]).all() and (alt["score"] < none["score"]).any() and set(alt["doc"][full].tolist()) <= {0, 1}


def test_ties_go_to_the_larger_predecessor_on_both_paths(gpu, any_index):
    """Anchors of one length on one diagonal and a second, parallel one, free gaps: every anchor has many predecessors with
    the same candidate.  The same 12 anchors as a read of their own (16 lanes) and in front of 8 more (the wavefront) must
    give the same table; 200 of them tie across the ring's wrap."""
    def lattice(h):
        t = np.arange(h)
        return 30 * (t // 2), 5000 + 30 * (t // 2) + 7 * (t % 2), np.full(h, 10)
    x12, y12, l12 = lattice(12)
    x20, y20, l20 = lattice(20)
    x200, y200, l200 = lattice(200)
    rec = _recs(np.r_[x12, x20, x200], np.r_[y12, y20, y200], np.r_[l12, l20, l200])
    offs = np.array([0, 12, 32, 232], dtype=np.uint64)
    for params in (ChainParams(gap_penalty=0), ChainParams(lookback=5, gap_penalty=0), ChainParams()):
        want, score, pred = _check(any_index, offs, rec, params)
        assert score[:12].tolist() == score[12:24].tolist() == score[32:44].tolist()
        assert pred[:12].tolist() == pred[12:24].tolist() == pred[32:44].tolist()
    want, score, pred = _check(any_index, offs, rec, ChainParams(gap_penalty=0))
    # anchors 2t and 2t + 1 share x: from 2t + 2 both are eligible with the same candidate, and the larger one is taken
    assert pred[2:12].tolist() == [1, 1, 3, 3, 5, 5, 7, 7, 9, 9] and pred[32 + 198] == 197


def test_repeated_call_gives_the_same_bytes_and_a_clone_has_its_own_scratch(gpu, any_index):
    rng = np.random.default_rng(6)
    offs, rec, D = _batch(rng, np.r_[rng.integers(0, 30, 500), 5000], front=1, n_docs=2)
    a = _run(any_index, offs, rec, None, D)
    b = _run(any_index, offs, rec, None, D)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a, b))
    other = any_index.clone(0)
    c = _run(other, offs, rec, None, D)
    d = _run(any_index, offs[:100], rec, ChainParams(3, 50, 5, 1), None, table=False)  # (the first handle goes on meanwhile)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a, c))
    want = chain_reference(offs, rec, None, D)
    assert np.array_equal(a[0], want[0])
    assert other.chain_stats()["chain_anchors"] == int(want[0]["anchors"].sum())
    assert any_index.chain_stats()["reads"] == 99 and np.array_equal(d[0], chain_reference(offs[:100], rec, ChainParams(3, 50, 5, 1))[0])
    other.close()


def test_argument_errors(gpu, any_index):
    offs, rec, D = _batch(np.random.default_rng(7), [4, 20])
    d_rec = torch.from_numpy(rec.view(np.int32).reshape(-1, 4).copy()).cuda()
    d_offs = torch.from_numpy(offs.view(np.int64).copy()).cuda()
    for bad, message in (((0, 5000, 500, 1), "lookback must be 1 .. 64"), ((65, 5000, 500, 1), "lookback must be 1 .. 64"),
                         ((64, 0, 500, 1), "max_dist must be 1 .. 2\\^31 - 1"), ((64, 2**31, 500, 1), "max_dist must be 1 .. 2\\^31 - 1"),
                         ((64, 5000, 2**31, 1), "max_gap must be 0 .. 2\\^31 - 1"), ((64, 5000, 500, 65536), "gap_penalty must be 0 .. 65535")):
        with pytest.raises(capi.SpxError, match="spx error -1: " + message):
            any_index.chain_device(d_rec, d_offs, bad)
        with pytest.raises(capi.SpxError, match="spx error -1: " + message):
            any_index.chain_host(np.frombuffer(b"ACGT", dtype=np.uint8), [0, 4], 1, bad)
    with pytest.raises(capi.SpxError, match="16-byte aligned"):
        any_index.chain_device(d_rec.view(-1)[2:-2].view(-1, 4), d_offs)
    with pytest.raises(capi.SpxError, match="16-byte aligned"):
        any_index.chain_device(d_rec, d_offs, d_out=torch.empty(30, dtype=torch.int32, device="cuda")[1:25].view(2, 12))
    with pytest.raises(capi.SpxError, match="8-byte"):
        any_index.chain_device(d_rec, _odd_words(d_offs))
    S = capi._spc()
    p = capi.SpcParams(64, 5000, 500, 1)
    out = torch.full((3, 12), FENCE, dtype=torch.int32, device="cuda")
    assert S.spc_chain_device(None, d_rec.data_ptr(), None, d_offs.data_ptr(), 2, p, out.data_ptr(), None, None, None) == -1
    assert S.spc_chain_device(any_index._h, d_rec.data_ptr(), None, d_offs.data_ptr(), 2, None, out.data_ptr(), None, None, None) == -1
    assert b"params must be non-null" in capi.lib().spx_last_error()
    assert S.spc_chain_device(any_index._h, None, None, d_offs.data_ptr(), 2, p, out.data_ptr(), None, None, None) == -1
    assert S.spc_chain_device(any_index._h, d_rec.data_ptr(), None, None, 2, p, out.data_ptr(), None, None, None) == -1
    assert S.spc_chain_device(any_index._h, d_rec.data_ptr(), None, d_offs.data_ptr(), 2, p, None, None, None, None) == -1
    assert b"must be non-null" in capi.lib().spx_last_error()
    assert S.spc_last_chain_stats(any_index._h, None) == -1 and S.spc_last_chain_stats(None, None) == -1
    torch.cuda.synchronize()
    assert (out == FENCE).all().item()
    # decreasing match offsets: the read counts as one without anchors, and the stats say so
    bad_offs = np.array([0, 4, 2, 24], dtype=np.uint64)
    got, _, _ = _run(any_index, bad_offs, rec, table=False)
    with pytest.raises(capi.SpxError, match="spx error -5: a read has 2\\^32 anchors or more"):
        any_index.chain_stats()
    assert got[1].tolist() == (UNCHAINED, 0, 0, 0, 0, 0, 0, 0, 0, NO_DOC) and got[0] == chain_reference([0, 4], rec)[0][0]
    # the host form: what spm_mems_begin refuses, and the limits of one piece
    seqs, one = np.frombuffer(b"ACGT", dtype=np.uint8), [0, 4]
    with pytest.raises(capi.SpxError, match="spx error -1: min_length must be at least 1"):
        any_index.chain_host(seqs, one, 0)
    with pytest.raises(capi.SpxError, match="spx_index_set_text / spx_index_rebuild_text"):
        any_index.chain_host(seqs, one, 1)
    with pytest.raises(capi.SpxError, match="digest_kind must be"):
        any_index.chain_host(seqs, one, 1, digest=(7, 4, 11))
    fresh = capi.Index.from_raw(synth.statistical_rlbwt(2000, 20, 3.0, seed=1, with_samples=True, n_docs=4), 0)
    fresh.set_text(torch.from_numpy(np.full(5000, 65, dtype=np.uint8)), unchecked=True)
    with pytest.raises(capi.SpxError, match="spx error -1: one piece per call"):
        fresh.chain_host(seqs, np.zeros((4 << 20) + 2, dtype=np.uint64), 1)
    with pytest.raises(capi.SpxError, match="spx error -1: one piece per call"):
        fresh.chain_host(seqs, [0, (32 << 20) + 1], 1)
    with pytest.raises(capi.SpxError, match="no chains have been computed"):
        fresh.chain_stats()
    fresh.close()


def _odd_words(d_offs):
    """The same offsets at an address that is 4 modulo 8."""
    w = torch.empty(d_offs.numel() * 2 + 2, dtype=torch.int32, device="cuda")
    w[1:-1] = d_offs.view(torch.int32)
    return _Shifted(w, d_offs.numel())


class _Shifted:
    """What chain_device asks of a tensor, over words 1 .. of `w`."""
    def __init__(self, w, n):
        self.w, self.n, self.device = w, n, w.device

    def numel(self):
        return self.n

    def data_ptr(self):
        return self.w.data_ptr() + 4


# ---- chain_host against mems_host -> chain_reference -------------------------------------------------------------------
def _host_check(ix, seqs, offs, min_length, params=None, digest=None, want_docs=False):
    out = ix.mems_host(seqs, offs, min_length, digest=digest, want_docs=want_docs)
    mo, rec, docs, values = (out[0], out[1], out[2], out[3]) if want_docs else (out[0], out[1], None, out[2])
    count = [0]
    want, _, _ = chain_reference(mo, rec, params, docs, count=count)
    got, vals = ix.chain_host(seqs, offs, min_length, params, digest=digest, want_docs=want_docs)
    bad = np.flatnonzero(got != want)
    assert got.dtype == CHAIN_DTYPE and bad.size == 0, (min_length, params, bad[:5], got[bad[:5]], want[bad[:5]])
    assert np.array_equal(vals, values)
    st = ix.chain_stats()
    assert st["reads"] == len(offs) - 1 and st["anchors"] == rec.size and st["candidates"] == count[0], st
    assert st["chained_reads"] == int((want["anchors"] > 0).sum()) and st["chain_anchors"] == int(want["anchors"].sum()), st
    return want


@pytest.mark.parametrize("kind", [0, capi.SPX_DIGEST_PROMOTED, capi.SPX_DIGEST_DNA])
def test_chain_host_on_an_index_from_the_oracles_side(gpu, oracle_mod, kind):
    """Several documents, indexed by synth.index_from_text (digested first for -m / -a); DNA reads through digestion, walk,
    MS extension, the matches and the chaining in one call, 16-bit arrays and -- with a read of 70 000 characters -- 32-bit."""
    rng = np.random.default_rng(80 + kind)
    genome = cases.repetitive_text(rng, 40_000, DNA)
    text = oracle_mod.digest(kind, K, W, genome) if kind else genome
    cuts = [text.size // 5, text.size // 2, text.size - text.size // 5 - text.size // 2]
    raw = synth.index_from_text(torch.from_numpy(text), doc_lengths=cuts)
    ix = capi.Index.from_raw(raw, 0)
    ix.set_text(torch.from_numpy(text.copy()))
    seqs, offs = cases.reads_mixed(rng, genome, DNA, 600, 500, [ord("N")])
    long_read = np.concatenate([genome[s:s + 7000] for s in np.sort(rng.integers(0, 30_000, 10))])
    long_read[rng.integers(0, long_read.size, 700)] = ord("N")
    wide = (np.r_[seqs[: int(offs[100])], long_read], np.r_[offs[:101], offs[100] + long_read.size])
    digest = (kind, K, W) if kind else None
    chained = longest = 0
    for s, o in ((seqs, offs), wide):
        o = o.astype(np.uint64)
        for min_length, params, want_docs in ((1, None, True), (6, None, False), (4, ChainParams(8, 300, 20, 2), True),
                                              (10**6, None, True)):
            want = _host_check(ix, s, o, min_length, params, digest, want_docs)
            chained += int((want["anchors"] > 1).sum())
            longest = max(longest, int(want["anchors"].max(initial=0)))
            if min_length == 10**6:
                assert (want["ref_start"] == np.uint64(UNCHAINED)).all()
            elif want_docs:
                assert len(set(want["doc"][want["anchors"] > 0].tolist())) >= 2
    assert chained > 100 and longest > 16  # both paths of the kernel, and chains that are more than one anchor
    got, vals = ix.chain_host(np.zeros(0, dtype=np.uint8), [0], 4)
    assert got.size == 0 and ix.chain_stats()["reads"] == 0
    ix.close()


def test_chain_host_on_a_text_built_on_the_device_and_the_planted_reads(gpu):
    text, seqs, offs, cuts = planted_reads()
    ix = capi.Index.from_raw(capi.build_raw(text), 0)
    want = _host_check(ix, seqs, offs, 12)
    for q, c in enumerate(cuts):
        got = want[q]
        assert (int(got["read_start"]), int(got["read_end"]), int(got["ref_start"]), int(got["ref_end"]), int(got["anchors"]),
                int(got["gap"]), int(got["score"])) == (0, 302, int(c), int(c) + 303, 5, 5, 293), (q, got)
    # one gap more than -G allows, or a gap that costs more than it joins: the chain breaks at the indels
    split = _host_check(ix, seqs, offs, 12, ChainParams(max_gap=2))
    assert (split["anchors"] < 5).all() and (split["score"] < 293).all()
    ix.close()


def test_chains_interleaved_with_matches_and_placements_on_one_handle(gpu):
    rng = np.random.default_rng(90)
    genome = cases.repetitive_text(rng, 40_000, DNA)
    cuts = [genome.size // 3, genome.size - genome.size // 3]
    raw = capi.build_raw(genome, doc_lengths=cuts)
    seqs, offs = cases.reads_mixed(rng, genome, DNA, 400, 500, [ord("N")])
    A = (seqs, offs.astype(np.uint64))
    long_read = np.tile(genome, 2)[:70_000].copy()
    long_read[rng.integers(0, long_read.size, 300)] = ord("N")
    B = (np.r_[seqs[: int(offs[20])], long_read], np.r_[offs[:21], offs[20] + long_read.size].astype(np.uint64))

    def chain(batch, want_docs=False, params=None):
        return lambda ix: (list(ix.chain_host(batch[0], batch[1], 4, params, want_docs=want_docs)), ix.chain_stats())

    def mems(batch):
        return lambda ix: (list(ix.mems_host(batch[0], batch[1], 4)), ix.mems_stats())

    def place(batch):
        return lambda ix: (list(ix.place_host(batch[0], batch[1], 4)), ix.place_stats())

    steps = [("chain A", chain(A)), ("mems A", mems(A)), ("chain B docs", chain(B, True)), ("place A", place(A)),
             ("chain A narrow", chain(A, False, ChainParams(4, 100, 3, 5))), ("mems B", mems(B)), ("place B", place(B)),
             ("chain A docs", chain(A, True))]
    ix = capi.Index.from_raw(raw, 0)
    for name, step in steps:
        got, got_stats = step(ix)
        fresh = capi.Index.from_raw(raw, 0)
        want, want_stats = step(fresh)
        fresh.close()
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (name, i)
        got_stats.pop("kernel_ms")
        want_stats.pop("kernel_ms")
        assert got_stats == want_stats, (name, got_stats, want_stats)
    # the records of a chain call are that call's own: nothing waits for spm_mems_fetch behind it
    ix.chain_host(A[0], A[1], 4)
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
def test_cli_chain_equals_the_reference_over_the_golden_files(gpu, tmp_path, case):
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
    chained_any = 0
    for extra, min_length, params, docs in ((["-L", "4", "-d"], 4, ChainParams(), True), (["-L", "8"], 8, ChainParams(), False),
                                            (["-L", "4", "-M", "-S", "40", "-G", "3", "-B", "2", "-H", "5"], 4, ChainParams(5, 40, 3, 2), False)):
        if os.path.exists(reads + ".chains"):
            os.remove(reads + ".chains")
        r = _cli(["chain", "-r", ref, "-p", reads, "-n"] + extra, env)
        assert r.returncode == 0, r.stderr.decode()
        m = mems_reference(L, P, offs, min_length, D if docs else None)
        want, _, _ = chain_reference(m[0], m[1], params, m[2] if docs else None)
        lines = []
        for q in range(len(ids)):
            w = want[q]
            ok = w["ref_start"] != np.uint64(UNCHAINED)
            f = [ids[q]] + [str(int(x)).encode() for x in (offs[q + 1] - offs[q], w["score"], w["anchors"], w["read_start"], w["read_end"])]
            f += [str(int(w["ref_start"])).encode() if ok else b"-1"] + [str(int(w[x])).encode() for x in ("ref_end", "gap")]
            lines.append(b"\t".join(f + ([str(int(w["doc"])).encode() if ok else b"-1"] if docs else [])) + b"\n")
        assert open(reads + ".chains", "rb").read() == b"".join(lines), (extra, r.stderr.decode())
        chained = int((want["ref_start"] != np.uint64(UNCHAINED)).sum())
        assert f"{len(ids)} reads, {chained} chained, {len(ids) - chained} without a match".encode() in r.stderr
        chained_any += int((want["anchors"] > 1).sum())
    assert chained_any  # (chains of more than one anchor are exercised)
    assert sorted(f for f in os.listdir(work) if f.startswith("reads.fa")) == ["reads.fa", "reads.fa.chains"]


def test_cli_chain_cuts_a_full_super_batch_into_calls_of_one_piece(gpu, tmp_path):
    """A super-batch ends with the read that fills it: 32 Mi characters and a few more are two calls of spc_chain_batch,
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
    rs[:, 70] = other[rs[:, 70]]  # one substitution: two anchors on one diagonal
    reads = str(tmp_path / "reads.fa")
    with open(reads, "wb") as f:
        for i in range(0, nreads, 25_000):
            f.write(b"".join(b">r%d\n%s\n" % (q, rs[q].tobytes()) for q in range(i, i + 25_000)))
    env = dict(os.environ, SPUMONI_GPUS="0", SPUMONI_TEXT=prefix + ".rawtext", SPUMONI_SUPER_BATCH=str(64 << 20))
    r = _cli(["chain", "-r", prefix[:-3], "-p", reads, "-n", "-L", "20"], env)
    assert r.returncode == 0, r.stderr.decode()
    ix = capi.Index.from_raw(raw, 0)
    half = nreads // 2
    offs = np.arange(0, half * m + 1, m).astype(np.uint64)
    want = np.concatenate([ix.chain_host(rs[:half].reshape(-1), offs, 20)[0], ix.chain_host(rs[half:].reshape(-1), offs, 20)[0]])
    ix.close()
    assert (want["anchors"] == 2).sum() > nreads // 2 and (want["ref_start"] == at.astype(np.uint64)).sum() > nreads // 2
    got = np.loadtxt(reads + ".chains", dtype=np.int64, usecols=range(1, 9))
    assert got.shape == (nreads, 8)
    for col, field in enumerate(("score", "anchors", "read_start", "read_end", "ref_start", "ref_end", "gap"), start=1):
        assert np.array_equal(got[:, col], want[field].astype(np.int64)), field
    assert (got[:, 0] == m).all()


def test_cli_chain_writes_no_file_when_it_fails(gpu, tmp_path):
    work = tmp_path / "c"
    shutil.copytree(os.path.join(FILES, "dna_multiline_fasta"), work)
    text = open(work / "ref.fa.rawtext", "rb").read()
    with open(work / "reads.fa", "wb") as f:  # a read without characters ends the run, as it ends `run`: behind 40 good ones
        for q in range(40):
            f.write(b">r%d\n" % q + text[17 * q: 17 * q + 60] + b"\n")
        f.write(b">bad_one\n>after\n" + text[:40] + b"\n")
    env = dict(os.environ, SPUMONI_TEXT=str(work / "ref.fa.rawtext"), SPUMONI_SUPER_BATCH="1000")
    before = sorted(os.listdir(work))
    r = _cli(["chain", "-r", str(work / "ref"), "-p", str(work / "reads.fa"), "-n", "-L", "4"], env)
    assert r.returncode == 1 and b"bad_one was empty after digestion" in r.stderr, r.stderr.decode()
    assert sorted(os.listdir(work)) == before
