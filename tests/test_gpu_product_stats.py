"""-m gpu: what the stats of the six products behind the walk hold -- counters, kernel_ms and step_ms -- over a sequence of
batches on ONE handle: mems, chain, align, cigar, extend and map, each in its host form and in its device form, over
B0 (40 reads), B1 (one read without a match), B2 (no read) and B0 again.

The other modules hold the records to the definitions and the counters to the references' counts; nothing there looks at
the times.  Here: every step time is finite, not negative and no larger than kernel_ms (each step lies inside the interval
or intervals kernel_ms sums, and both come from the same event timestamps: no tolerance), a step that did not run says
0.0, a second *_stats() call collects nothing, the counters of the second B0 are those of the first, and a map_host has
taken the whole chain of waiting records with it."""
import math

import numpy as np
import pytest
import torch

from spumoni_amd import capi, synth
from spumoni_amd.align import UNFILLED, align_reference
from spumoni_amd.chain import chain_reference
from spumoni_amd.extend import extend_reference
from spumoni_amd.mems import mems_reference

pytestmark = pytest.mark.gpu
MIN_LENGTH = 12
TIMES = ("kernel_ms", "step_ms", "wave_fill_ticks", "wave_back_ticks")  # (the ticks are clock readings: no counters)
STEPS = {"mems": 0, "chain": 0, "align": 4, "cigar": 5, "extend": 6, "map": 2}
FETCH = {"mems": (capi._spm, "spm_mems_fetch", "spm_mems_begin"), "cigar": (capi._spg, "spg_cigar_fetch", "spg_cigar_begin"),
         "extend": (capi._spe, "spe_extend_fetch", "spe_extend_begin"), "map": (capi._spn, "spn_map_fetch", "spn_map_begin")}


def _batch(reads):
    offs = np.cumsum([0] + [r.size for r in reads]).astype(np.uint64)
    return np.concatenate(list(reads) + [np.zeros(0, dtype=np.uint8)]).astype(np.uint8), offs


@pytest.fixture(scope="module")
def world(built_all, oracle_mod):
    """A text of 1 500 characters in two sequences with its index, the three batches, the oracle's MS arrays of each (for
    the device forms and for the preconditions) and one handle for the whole module."""
    assert torch.cuda.is_available(), "these tests need the MI355X"
    text = synth.random_genome(1500, seed=41)
    raw = synth.index_from_text(torch.from_numpy(text), doc_lengths=[900, 600])
    orc = oracle_mod.OracleIndex.from_raw(raw)
    rng = np.random.default_rng(42)
    long, _ = synth.sample_reads(text, 40, 150, seed=43, err=0.05, null_fraction=0.1)
    b0 = _batch([long[150 * q:150 * q + int(m)] for q, m in enumerate(rng.integers(60, 151, 40))])
    batches = [b0, _batch([np.full(20, ord("N"), dtype=np.uint8)]), _batch([])]
    ms = [orc.ms(s, o, want_docs=True, text=text) if o.size > 1 else {"lengths": np.zeros(0, np.uint32), "pointers": np.zeros(0, np.uint64)}
          for s, o in batches]
    ix = capi.Index.from_raw(raw, 0)
    ix.set_text(torch.from_numpy(text.copy()))
    ix.set_sequences([900, 600], 1)
    yield dict(ix=ix, text=text, batches=batches, ms=ms)
    ix.close()


def test_the_batches_reach_every_step(world):
    """B0: a read with a gap filled by a table and an extended end, and a read without a match of MIN_LENGTH; B1: no match."""
    text, (seqs, offs), ms = world["text"], world["batches"][0], world["ms"][0]
    assert offs.size == 41 and 60 <= np.diff(offs.astype(np.int64)).min() and np.diff(offs.astype(np.int64)).max() <= 150
    moffs, rec = mems_reference(ms["lengths"], ms["pointers"], offs, MIN_LENGTH)
    chains, _, pred = chain_reference(moffs, rec)
    _, goffs, gaps = align_reference(seqs, offs, text, moffs, rec, chains, pred)
    _, _, _, ends = extend_reference(seqs, offs, text, moffs, rec, chains, pred)
    table = (gaps["a"] >= 2) & (gaps["b"] >= 2) & (gaps["edits"] != UNFILLED)
    extended = (ends["read_chars"] + ends["text_chars"]).reshape(-1, 2).max(axis=1) > 0
    per_read = np.add.reduceat(np.r_[table, False], goffs[:-1].astype(np.int64)) * (np.diff(goffs.astype(np.int64)) > 0)
    assert ((per_read > 0) & extended).any()
    assert (np.diff(moffs.astype(np.int64)) == 0).any()
    one = world["batches"][1]
    assert mems_reference(world["ms"][1]["lengths"], world["ms"][1]["pointers"], one[1], 1)[0].tolist() == [0, 0]
    assert world["batches"][2][1].tolist() == [0]


def _host(ix, product, batch):
    """The product's host form; returns (its stats, the offsets its fetch gave or None)."""
    out = getattr(ix, product + "_host")(*batch, MIN_LENGTH)
    offsets = {"mems": 0, "cigar": 1, "extend": 1, "map": 1}.get(product)
    return getattr(ix, product + "_stats"), None if offsets is None else out[offsets]


def _i64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def _device(ix, product, batch, ms):
    """The device forms up to the product's, each on what the one before left on the device."""
    seqs, offs = batch
    d_len = torch.from_numpy(np.r_[ms["lengths"].astype(np.uint32), np.zeros(8, np.uint32)].view(np.int32).copy()).cuda()[:seqs.size]
    d_offs, d_reads = _i64(offs), torch.from_numpy(np.r_[seqs, np.zeros(8, dtype=np.uint8)]).cuda()
    d_moffs, d_rec = ix.mems_device(d_len, _i64(np.r_[ms["pointers"], np.zeros(1, np.uint64)])[:seqs.size], d_offs, MIN_LENGTH)
    n = d_rec.shape[0]
    if product != "mems":
        if n == 0:
            d_rec = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
        d_pred = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
        d_chains = ix.chain_device(d_rec, d_moffs, d_out_pred=d_pred)
        args = (d_reads, d_offs, d_rec, d_moffs, d_chains, d_pred)
        if product == "align":
            ix.align_device(*args, gap_capacity=n)
        elif product == "cigar":
            ix.cigar_device(*args, gap_capacity=n)
        elif product in ("extend", "map"):
            d_out, d_ooffs, d_ops, _ = ix.extend_device(*args, gap_capacity=n)
            if product == "map":
                ix.map_device(d_out, d_ooffs, d_ops, d_offs)
    torch.cuda.synchronize()
    return getattr(ix, product + "_stats"), None


def _counters(st):
    return {k: v for k, v in st.items() if k not in TIMES}


def _check_times(product, st, ran):
    steps = st.get("step_ms", [])
    assert len(steps) == STEPS[product], st
    assert math.isfinite(st["kernel_ms"]) and st["kernel_ms"] >= 0, st
    assert all(math.isfinite(t) and 0 <= t <= st["kernel_ms"] for t in steps), st
    if ran:
        assert st["kernel_ms"] > 0 and (not steps or max(steps) > 0), st


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("product", ["mems", "chain", "align", "cigar", "extend", "map"])
def test_counters_and_times_over_b0_b1_b2_b0(world, product, form):
    ix, batches = world["ix"], world["batches"]
    run = (lambda b: _host(ix, product, batches[b])) if form == "host" else (lambda b: _device(ix, product, batches[b], world["ms"][b]))
    stats, _ = run(0)
    first = stats()
    print(product, form, "B0", first)
    _check_times(product, first, ran=True)
    assert stats() == first  # (the second call collects nothing)
    assert first.get("reads", 40) == 40 and first.get("error", 0) == 0 and first.get("overflow", 0) == 0, first
    stats, _ = run(1)
    one = stats()
    print(product, form, "B1", one)
    _check_times(product, one, ran=False)
    assert one.get("reads", 1) == 1 and one.get("matches", 0) == 0 and one.get("gaps", 0) == 0 and one.get("mapped", 0) == 0, one
    stats, offsets = run(2)
    none = stats()
    print(product, form, "B2", none)
    _check_times(product, none, ran=False)
    assert not any(_counters(none).values()), none
    assert not any(none.get("step_ms", [])), none
    if form == "host" or product == "mems":
        assert none["kernel_ms"] == 0.0, none  # (nothing was enqueued)
    else:
        # the other device forms zero their counters between the two events whatever the batch holds: kernel_ms is that
        # memset of under 200 bytes and no kernel, a few microseconds.  0.1 ms is some twenty times that, and well below
        # the first launch of a real kernel plus a device scan
        assert none["kernel_ms"] < 0.1, none
    if form == "host" and product in FETCH:
        lib, fetch, begin = FETCH[product]
        assert offsets.tolist() == [0]
        with pytest.raises(capi.SpxError, match=f"{fetch} without a successful {begin}"):
            capi._check(getattr(lib(), fetch)(ix._h, None, None))
    stats, _ = run(0)
    again = stats()
    _check_times(product, again, ran=True)
    assert _counters(again) == _counters(first), (again, first)  # (nothing leaks across calls)


def test_map_host_takes_the_whole_chain_of_waiting_records(world):
    ix = world["ix"]
    ix.map_host(*world["batches"][0], MIN_LENGTH)
    for lib, fetch, begin in (FETCH["extend"], FETCH["mems"]):
        with pytest.raises(capi.SpxError, match=f"{fetch} without a successful {begin}"):
            capi._check(getattr(lib(), fetch)(ix._h, None, None))
