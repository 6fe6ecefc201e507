"""-m gpu: chain, place, align and cigar at batches where a wavefront does a second unit of work, bit for bit against
chain_reference, place_reference, align_reference and cigar_reference.

tests/grid_cases.py builds the batches and their expectations and asserts, on the references' answers, the regime each is
in: chunk_reads 4 / 8 / 12 of k_chain, one to three trips of k_place's grid stride, every wavefront of k_fill_wave and
k_trace_wave<false> with two gaps or more, the trace buffers in device memory taken for a second and a third gap at two
strides, the list whose two ends meet, k_align_reduce and k_cigar_plan past their 1024 blocks, and the host forms past the
chain's cap.  The device forms run through the _run helpers of the four neighbouring modules (fenced outputs, padded
uploads); every record, table entry, offset, entry and the stats are compared."""
import numpy as np
import pytest
import torch

from spumoni_amd import capi, synth
from spumoni_amd.align import UNALIGNED, UNFILLED
from spumoni_amd.place import UNPLACED
from tests import grid_cases as gc
from tests import test_gpu_align as t_align
from tests import test_gpu_chain as t_chain
from tests import test_gpu_cigar as t_cigar
from tests import test_gpu_place as t_place

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def text_index(built_all):
    """Any index with the crafted text handed in: chain reads no index array, place, align and cigar the text alone."""
    assert torch.cuda.is_available(), "these tests need the MI355X"
    capi.lib()
    ix = capi.Index.from_raw(synth.statistical_rlbwt(5000, 60, 4.0, seed=3, with_samples=True, n_docs=8), 0)
    ix.set_text(torch.from_numpy(gc.text().copy()), unchecked=True)
    yield ix
    ix.close()


def _same(what, got, want):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("nreads", list(gc.CHAIN_SIZES))
def test_chain_with_chunks_of_one_two_and_three_quads(text_index, nreads):
    c = gc.case(f"chain-{nreads}")
    c.reaches()
    chains, score, pred = t_chain._run(text_index, c.offs, c.rec, None, c.D, table=True)
    lo, hi = int(c.offs[0]), int(c.offs[-1])
    _same("score", score, c.want[1][lo:hi])
    _same("pred", pred, c.want[2][lo:hi])
    _same("chains", chains, c.want[0])
    st = text_index.chain_stats()
    assert st["reads"] == nreads and st["anchors"] == hi - lo, st
    assert st["chained_reads"] == int((c.want[0]["anchors"] > 0).sum()) and st["chain_anchors"] == int(c.want[0]["anchors"].sum()), st
    assert st["candidates"] == c.count[0], (st, c.count)


@pytest.mark.parametrize("nreads", list(gc.PLACE_SIZES))
def test_place_in_one_two_and_three_trips_of_the_grid(text_index, nreads):
    c = gc.case(f"place-{nreads}")
    c.reaches()
    got = t_place._run(text_index, c.R, c.L, c.P, c.offs, c.params, c.bits, c.D)
    _same("placements", got, c.want)
    st = text_index.place_stats()
    ok = c.want["ref_start"] != np.uint64(UNPLACED)
    span = c.want["read_end"][ok].astype(np.int64) - c.want["read_start"][ok] - c.want["seed_len"][ok]
    assert st["values"] == int(c.offs[-1]) - int(c.offs[0]) and st["placed"] == int(ok.sum()), st
    assert st["seed_values"] == int(c.want["seed_len"][ok].sum()) and st["extended_values"] == int(span.sum()), st


def _align(ix, c, table):
    want, w_goffs, w_gaps = c.align
    got, goffs, gaps = t_align._run(ix, c.arrays, c.params, cap=c.cap, table=table)
    if table:
        _same("gap offsets", goffs, w_goffs)
        _same("gaps", gaps, w_gaps)
    _same("alignments", got, want)
    st = ix.align_stats()
    ok = want["ref_start"] != np.uint64(UNALIGNED)
    assert st["reads"] == want.size and st["aligned_reads"] == int(ok.sum()) and st["gaps"] == w_gaps.size, st
    assert st["filled_gaps"] == int((w_gaps["edits"] != UNFILLED).sum()) and st["cells"] == c.cells, (st, c.cells)
    assert st["error"] == 0 and st["overflow"] == 0, st


def _cigar(ix, c):
    want, w_ooffs, w_ops = c.cigar
    got, ooffs, ops = t_cigar._run(ix, c.arrays, c.params, cap=c.cap)
    _same("op offsets", ooffs, w_ooffs)
    _same("entries", ops, w_ops)
    _same("alignments", got, want)
    st = ix.cigar_stats()
    w_gaps = c.align[2]
    ok = want["ref_start"] != np.uint64(UNALIGNED)
    assert st["reads"] == want.size and st["aligned_reads"] == int(ok.sum()) and st["gaps"] == w_gaps.size, st
    assert st["filled_gaps"] == int((w_gaps["edits"] != UNFILLED).sum()) and st["cells"] == c.cells, (st, c.cells)
    assert st["entries"] == w_ops.size and st["path_words"] == c.path_words, (st, w_ops.size, c.path_words)
    assert st["overflow"] == 0 and st["error"] == 0, st


@pytest.mark.parametrize("form", ["align, table in caller buffers", "align, table in the scratch", "cigar"])
def test_every_wavefront_of_the_lds_launches_fills_two_gaps_or_more(text_index, form):
    c = gc.case("wave-two-gaps")
    c.reaches()
    if form == "cigar":
        _cigar(text_index, c)
    else:
        _align(text_index, c, table="caller" in form)


@pytest.mark.parametrize("max_fill", [4096, 2048])
def test_cigar_reuses_its_trace_buffers_in_device_memory(text_index, max_fill):
    c = gc.case(f"trace-{max_fill}")
    c.reaches()
    _cigar(text_index, c)


@pytest.mark.parametrize("n_lds,n_dev", gc.ENDS)
def test_the_two_ends_of_the_list_meet(text_index, n_lds, n_dev):
    c = gc.case(f"ends-{n_lds}-{n_dev}")
    assert c.reaches() == (n_lds, n_dev)
    _cigar(text_index, c)
    _align(text_index, c, table=True)
    _align(text_index, c, table=False)


@pytest.mark.parametrize("nreads", gc.REDUCE_SIZES)
def test_reduce_and_plan_past_their_1024_blocks(text_index, nreads):
    c = gc.case(f"reduce-{nreads}")
    c.reaches()
    _align(text_index, c, table=True)
    _cigar(text_index, c)


def test_the_plan_spans_the_gap_capacity_when_that_is_larger_than_the_reads(text_index):
    c = gc.case("plan-span")
    c.reaches()
    _cigar(text_index, c)


def test_host_forms_on_70000_reads(built_all, oracle_mod):
    """chain_host, align_host, cigar_host and place_host past the chain's cap (chunk_reads 8), on an index from
    capi.build_raw, against oracle MS -> mems_reference -> chain_reference -> align_reference / cigar_reference, and
    place_reference."""
    T, seqs, offs = gc.host_batch()
    raw = capi.build_raw(T)
    c = gc.host_expectation(oracle_mod, raw, T, seqs, offs)
    c.reaches()
    print(f"host forms: oracle and references {c.seconds:.2f} s")
    ix = capi.Index.from_raw(raw, 0)
    values = np.diff(offs.astype(np.int64))
    n_anchors = c.m[1].size
    got, vals = ix.chain_host(seqs, offs, gc.HOST_MIN_LENGTH)
    _same("chains", got, c.chains)
    assert np.array_equal(vals, values)
    st = ix.chain_stats()
    assert st["reads"] == gc.HOST_READS and st["anchors"] == n_anchors and st["candidates"] == c.chain_count[0], st
    assert st["chained_reads"] == int((c.chains["anchors"] > 0).sum()) and st["chain_anchors"] == int(c.chains["anchors"].sum()), st
    want, _, w_gaps = c.align
    ok = want["ref_start"] != np.uint64(UNALIGNED)
    got, chains, vals = ix.align_host(seqs, offs, gc.HOST_MIN_LENGTH)
    _same("alignments", got, want)
    _same("chains of align_host", chains, c.chains)
    assert np.array_equal(vals, values)
    st = ix.align_stats()
    assert st["reads"] == gc.HOST_READS and st["aligned_reads"] == int(ok.sum()) and st["gaps"] == w_gaps.size and st["cells"] == c.cells, st
    assert st["filled_gaps"] == int((w_gaps["edits"] != UNFILLED).sum()), st
    want, w_ooffs, w_ops = c.cigar
    got, ooffs, ops, chains, vals = ix.cigar_host(seqs, offs, gc.HOST_MIN_LENGTH)
    st = ix.cigar_stats()
    _same("alignments of cigar_host", got, want)
    _same("op offsets", ooffs, w_ooffs)
    _same("entries", ops, w_ops)
    _same("chains of cigar_host", chains, c.chains)
    assert np.array_equal(vals, values)
    assert st["reads"] == gc.HOST_READS and st["cells"] == c.cells and st["entries"] == w_ops.size, st
    assert st["path_words"] == gc.path_words(w_gaps, 512) and st["overflow"] == 0 and st["error"] == 0, st
    got, vals = ix.place_host(seqs, offs, gc.HOST_MIN_SEED)
    _same("placements", got, c.place)
    assert np.array_equal(vals, values)
    placed = c.place["ref_start"] != np.uint64(UNPLACED)
    st = ix.place_stats()
    assert st["placed"] == int(placed.sum()) and st["values"] == int(values.sum()) and st["seed_values"] == int(c.place["seed_len"].sum()), st
    ix.close()
