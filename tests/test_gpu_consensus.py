"""The consensus on the GPU (include/spumoni_consensus.h): crafted arrays through the device form against
spumoni_amd/consensus.py in every record, every byte of the body, the count and the stats, with every buffer fenced on both
sides and the body at every alignment; the host forms on the planted genome of tests/consensus_cases.py against the
reference on the handle's own arrays and against what the reads were cut from, beside the ten products before it on one
handle; and `spumoni consensus` against both."""
import os

import numpy as np
import pytest
import torch

from spumoni_amd import capi
from spumoni_amd.consensus import MAX_LINE_WIDTH, SEQ_DTYPE, consensus_reference, fasta_of, tsv_of
from spumoni_amd.cover import seq_starts
from spumoni_amd.extend import ExtendParams
from tests import cases
from tests import consensus_cases as cc
from tests.test_gpu_align import DNA, FENCE, _cli
from tests.test_gpu_call import PARAMS, TEXT_LETTERS, _host_state
from tests.test_gpu_cover import _fenced, _unfence
from tests.test_gpu_map import _index_of, gpu, table  # noqa: F401 (gpu: a fixture)

pytestmark = pytest.mark.gpu
TILE, PER_THREAD = 4096, 16  # positions of a tile and of one of its threads (spx_consensus.hip)
BYTE_FENCE = 0xF9
WIDTHS = [0, 1, 7, 60, 4096, MAX_LINE_WIDTH]
MASKS = [ord("N"), ord("n"), 0]


@pytest.fixture(scope="module")
def ix(gpu):
    """Any index: the kernels read the table, the text and nothing else of it.  Every case sets its own text."""
    index = _index_of(16)
    yield index
    index.close()


def _set(ix, lengths, strands, seed=0):
    """The table and a text of a few lower-case letters and N among ACGT; returns the text."""
    n_text = int(np.sum(lengths)) * strands
    text = TEXT_LETTERS[np.random.default_rng(3000 + seed).integers(0, TEXT_LETTERS.size, n_text)]
    ix.set_text(torch.from_numpy(text.copy()), unchecked=True)
    ix.set_sequences(lengths, strands)
    return text


def _arrays(rng, G):
    """Dense random counts: every rule decides a good share of the positions at every parameter set of PARAMS."""
    depth = rng.integers(0, 9, G).astype(np.uint32)
    dele = (rng.integers(0, 6, G) * (rng.random(G) < 0.35)).astype(np.uint32)
    alt = rng.integers(0, 5, 4 * G).astype(np.uint32)
    ins = rng.integers(0, 4, G).astype(np.uint32)
    return depth, alt, ins, dele


def _run(ix, n_seqs, depth, alt, ins, dele, cap, pad=8, **kw):
    """consensus_device with the records, the body and the count fenced, the inputs too; the body starts `pad` bytes into
    its allocation.  Returns (records, the bytes that fit, the count)."""
    ins_ = [_fenced(a, np.uint32) for a in (depth, alt, ins, dele)]
    w_rec, d_rec = _fenced(np.full(6 * n_seqs, 0x1234567, dtype=np.uint64), np.uint64)  # (the records are zeroed by the call)
    w_count, d_count = _fenced(1, np.uint64)
    whole = torch.full((cap + pad + 9,), BYTE_FENCE, dtype=torch.uint8, device="cuda")
    ix.consensus_device(*(view for _, view in ins_), body_capacity=cap, d_records=d_rec, d_body=whole[pad:pad + cap] if cap else None,
                        d_count=d_count, **kw)
    torch.cuda.synchronize()
    for (w, _), a in zip(ins_, (depth, alt, ins, dele)):
        assert np.array_equal(_unfence(w, a.size, np.uint32), a), "an input changed"
    total = int(_unfence(w_count, 1, np.uint64)[0])
    body = whole.cpu().numpy()
    fit = min(total, cap)
    assert (body[:pad] == BYTE_FENCE).all() and (body[pad + fit:] == BYTE_FENCE).all(), "a byte outside the body that fits"
    return _unfence(w_rec, 6 * n_seqs, np.uint64).view(SEQ_DTYPE), body[pad:pad + fit].copy(), total


def _check(ix, text, lengths, strands, depth, alt, ins, dele, combos, slack=3):
    """Every (params, line_width, mask) of `combos` against the reference: records, body, count and stats."""
    n_seqs = len(lengths)
    G = int(np.sum(lengths))
    seen = {"substituted": 0, "deleted": 0, "masked": 0, "ins_sites": 0, "letters": 0}
    for i, (params, width, mask) in enumerate(combos):
        want_rec, want_body = consensus_reference(depth, alt, ins, dele, text, lengths, strands, *params, mask=mask, line_width=width)
        rec, body, total = _run(ix, n_seqs, depth, alt, ins, dele, want_body.size + slack, pad=5 + i % 4, min_depth=params[0],
                                min_alt=params[1], min_permille=params[2], mask=mask, line_width=width)
        bad = [s for s in range(n_seqs) if rec[s].tobytes() != want_rec[s].tobytes()]
        assert not bad, (params, width, mask, bad[:5], rec[bad[:5]], want_rec[bad[:5]])
        assert total == want_body.size, (params, width, mask, total, want_body.size)
        diff = np.flatnonzero(body != want_body)
        assert diff.size == 0, (params, width, mask, diff[:5], body[diff[:5]], want_body[diff[:5]])
        st = ix.consensus_stats()
        sums = {k: int(want_rec[k].sum()) for k in seen}
        assert (st["positions"], st["bytes"], st["overflow"]) == (G, want_body.size, 0) and all(st[k] == v for k, v in sums.items()), (st, sums)
        assert st["kept"] == sums["letters"] - sums["substituted"] - sums["masked"] and len(st["step_ms"]) == 3
        for k, v in sums.items():
            seen[k] += v
    return seen


def _rotate(n):
    """n combinations that take every parameter set, every width and every mask in turn."""
    return [(PARAMS[i % 4], WIDTHS[i % 6], MASKS[i % 3]) for i in range(n)]


@pytest.mark.parametrize("strands", [1, 2])
@pytest.mark.parametrize("G", [1, 15, 16, 17, 4095, 4096, 4097, 8193, 10_000])
def test_genome_sizes_around_the_thread_and_the_tile(gpu, ix, G, strands):
    """One sequence, and the same genome cut into a few: below, at and above a thread's 16 positions and a tile's 4 096."""
    rng = np.random.default_rng(G * 2 + strands)
    depth, alt, ins, dele = _arrays(rng, G)
    for n_seqs in (1, min(G, 5)):
        lengths = table(rng, n_seqs, 1, G)
        text = _set(ix, lengths, strands, seed=G)
        seen = _check(ix, text, lengths, strands, depth, alt, ins, dele, [(PARAMS[0], 60, MASKS[0]), (PARAMS[1], 7, MASKS[2]), (PARAMS[3], 0, MASKS[1])])
    assert G < 1000 or all(v > 0 for v in seen.values()), seen


LAYOUTS = {
    "one_sequence": [10_000],
    "4100_of_one_base": [1] * 4100 + [5900],
    "borders_at_threads_and_tiles": np.diff([0, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 8191, 8192, 8193, 10_000]).tolist(),
    "one_base_around_the_tile_border": [4090] + [1] * 12 + [5898],
}


@pytest.mark.parametrize("strands", [1, 2])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_sequence_layouts_at_every_parameter_set_width_and_mask(gpu, ix, layout, strands):
    """10 000 positions under four tables; every one of PARAMS, every line width and every mask in turn."""
    lengths = np.array(LAYOUTS[layout], dtype=np.uint64)
    rng = np.random.default_rng(len(lengths) + strands)
    text = _set(ix, lengths, strands, seed=len(lengths))
    seen = _check(ix, text, lengths, strands, *_arrays(rng, 10_000), _rotate(12))
    assert all(v > 100 for v in seen.values()), seen


def test_sequences_deleted_whole_and_deleted_runs_across_a_tile_border(gpu, ix):
    """A sequence without a letter between two others takes no byte and the next starts where the one before ended -- as one
    sequence of 300 bases, as 50 of one base across a thread's border, and as the sequence that holds a tile's border; a
    deleted run from 20 bases in front of the second border to 20 behind it; and a genome deleted whole."""
    lengths = np.array([1000, 300, 700] + [1] * 50 + [2000, 200, 5750], dtype=np.uint64)
    F = seq_starts(lengths)
    rng = np.random.default_rng(77)
    text = _set(ix, lengths, 2, seed=77)
    depth, alt, ins, dele = _arrays(rng, 10_000)
    gone = np.zeros(10_000, dtype=bool)
    gone[F[1]:F[2]] = gone[F[3]:F[53]] = gone[F[54]:F[55]] = True
    assert F[54] < TILE < F[55]
    gone[2 * TILE - 20:2 * TILE + 20] = True
    depth[gone], dele[gone] = 0, 7
    for params, width, mask in _rotate(6):
        rec, _ = consensus_reference(depth, alt, ins, dele, text, lengths, 2, *params, mask=mask, line_width=width)
        assert not rec["letters"][1] and not rec["letters"][3:53].any() and not rec["letters"][54] and rec["letters"][55] and rec["letters"][2]
        assert rec["body_start"][1] == rec["body_start"][2] and rec["body_start"][54] == rec["body_start"][55]
    _check(ix, text, lengths, 2, depth, alt, ins, dele, _rotate(6))
    depth[:], dele[:] = 0, 9
    seen = _check(ix, text, lengths, 2, depth, alt, ins, dele, _rotate(3))
    assert seen["letters"] == 0 and seen["deleted"] == 3 * 10_000


def test_letter_counts_at_exact_multiples_of_every_width(gpu, ix):
    """Sequences of 1, 7, 14, 60, 120 and 4 096 letters and one of 8 192 less a deleted base: at widths 1, 7, 60 and 4 096
    their last line is full, and the newline that ends the line is the newline that ends the sequence."""
    lengths = np.array([7, 14, 60, 1, 120, 4096, 8193, 9], dtype=np.uint64)
    G = int(lengths.sum())
    text = _set(ix, lengths, 1, seed=5)
    depth, dele = np.full(G, 5, dtype=np.uint32), np.zeros(G, dtype=np.uint32)
    at = seq_starts(lengths)[6] + 4000
    depth[at], dele[at] = 0, 5
    alt, ins = np.zeros(4 * G, dtype=np.uint32), np.zeros(G, dtype=np.uint32)
    rec, _ = consensus_reference(depth, alt, ins, dele, text, lengths, 1)
    assert rec["letters"].tolist() == [7, 14, 60, 1, 120, 4096, 8192, 9]
    _check(ix, text, lengths, 1, depth, alt, ins, dele, [((2, 2, 500), w, ord("N")) for w in WIDTHS])


def test_counts_that_need_64_bits(gpu, ix):
    """del * 1000 beyond 2^32, and depth + del beyond 2^32: one position each way on either side of the share, in two tiles."""
    lengths = np.array([3000, 3000], dtype=np.uint64)
    G = 6000
    text = _set(ix, lengths, 1, seed=64)
    depth, dele = np.full(G, 4, dtype=np.uint32), np.zeros(G, dtype=np.uint32)
    alt, ins = np.zeros(4 * G, dtype=np.uint32), np.zeros(G, dtype=np.uint32)
    for at, d, dl, i in ((10, 5_000_000, 5_000_000, 0), (11, 5_000_001, 5_000_000, 0), (4500, 2**31 + 1, 2**31 + 1, 2**31 + 1),
                         (4501, 2**31 + 2, 2**31 + 1, 2**31 + 1), (4502, 2**32 - 1, 2**32 - 1, 2**32 - 1), (4503, 1, 2**32 - 1, 0)):
        depth[at], dele[at], ins[at] = d, dl, i
    rec, _ = consensus_reference(depth, alt, ins, dele, text, lengths, 1)
    assert rec["deleted"].tolist() == [1, 3] and rec["ins_sites"].tolist() == [0, 2]
    for params in ((2, 2, 500), (2**32 - 1, 2, 500), (2, 2**32 - 1, 1000)):
        _check(ix, text, lengths, 1, depth, alt, ins, dele, [(params, 60, ord("N"))])


def test_body_capacity_at_below_and_zero(gpu, ix):
    rng = np.random.default_rng(8)
    lengths = table(rng, 50, 1, 9000)
    text = _set(ix, lengths, 1, seed=8)
    depth, alt, ins, dele = _arrays(rng, 9000)
    want_rec, want = consensus_reference(depth, alt, ins, dele, text, lengths, 1, line_width=7)
    assert want.size > 9000
    for cap in (want.size, want.size - 1, 4097, 1, 0, want.size + 5):
        for pad in (8, 7):
            rec, body, total = _run(ix, 50, depth, alt, ins, dele, cap, pad=pad, line_width=7)
            st = ix.consensus_stats()
            assert total == want.size == st["bytes"] and body.tobytes() == want[:cap].tobytes(), cap  # the count is kept
            assert rec.tobytes() == want_rec.tobytes() and st["overflow"] == int(cap < want.size), (cap, st)


def test_refusals_of_the_device_form(gpu, ix):
    lengths = np.array([100], dtype=np.uint64)
    _set(ix, lengths, 1)
    t = torch.zeros(1024, dtype=torch.int64, device="cuda")
    for kw in (dict(min_depth=0), dict(min_alt=0), dict(min_permille=1001)):
        with pytest.raises(capi.SpxError, match="spx error -1: min_depth and min_alt must be at least 1 and min_permille between 0 and 1000"):
            ix.consensus_device(t, t, t, t, body_capacity=8, d_records=t, d_body=t, d_count=t, **kw)
    with pytest.raises(capi.SpxError, match="spx error -1: line_width must be between 0 and 2147483647"):
        ix.consensus_device(t, t, t, t, body_capacity=8, d_records=t, d_body=t, d_count=t, line_width=2**31)
    S = capi._sps()
    p = t.data_ptr()
    prm = capi.C.byref(capi.SpsParams(2, 2, 500, 60, ord("N")))
    err = capi.lib().spx_last_error
    for args in ((None, p, p, p, prm, 8, p, p, p), (p, None, p, p, prm, 8, p, p, p), (p, p, None, p, prm, 8, p, p, p), (p, p, p, None, prm, 8, p, p, p),
                 (p, p, p, p, prm, 8, None, p, p), (p, p, p, p, prm, 8, p, None, p), (p, p, p, p, prm, 8, p, p, None)):
        assert S.sps_consensus_device(ix._h, *args, None) == -1 and b"must be non-null" in err(), args
    assert S.sps_consensus_device(ix._h, p, p, p, p, None, 8, p, p, p, None) == -1 and b"params must be non-null" in err()
    assert S.sps_consensus_device(ix._h, p, p + 8, p, p, prm, 8, p, p, p, None) == -1 and b"d_alt must be 16-byte aligned" in err()
    assert S.sps_consensus_device(ix._h, p, p, p, p, prm, 8, p + 4, p, p, None) == -1 and b"8-byte" in err()
    assert S.sps_consensus_device(ix._h, p, p, p, p, prm, 8, p, p, p + 4, None) == -1 and b"8-byte" in err()
    assert S.sps_consensus_device(ix._h, p + 2, p, p, p, prm, 8, p, p, p, None) == -1 and b"4-byte aligned" in err()
    assert S.sps_consensus_device(ix._h, p, p, p, p, prm, 0, p + 4096, None, p + 8000, None) == 0  # (no body is asked for: none is needed)
    torch.cuda.synchronize()
    bare = _index_of(16)
    with pytest.raises(capi.SpxError, match="spx error -1: sps_consensus_device needs the sequence table: the index has none"):
        bare.consensus_device(t, t, t, t, body_capacity=8, d_records=t, d_body=t, d_count=t)
    with pytest.raises(capi.SpxError, match="spx error -1: sps_consensus_begin needs the sequence table: the index has none"):
        bare.consensus()
    with pytest.raises(capi.SpxError, match="no consensus has been computed"):
        bare.consensus_stats()
    bare.close()


# ---- the host forms ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plant():
    return cc.planted()


@pytest.fixture(scope="module")
def planted_raw(gpu, plant):
    return capi.build_raw(plant["text"])


def _handle(raw):
    index = capi.Index.from_raw(raw, 0)
    index.set_sequences(cc.LENGTHS, cc.STRANDS)
    index.call_reset()
    return index


def _reference_on_the_handle(index, text, **kw):
    G = sum(cc.LENGTHS)
    depth, _ = index.cover_depth(0, G)
    alt, _, ins, dele = index.pileup_counts(0, G)
    return consensus_reference(depth, alt.reshape(-1), ins, dele, text, cc.LENGTHS, cc.STRANDS, **kw)


def _same(got, want):
    assert got[0].dtype == SEQ_DTYPE and got[1].dtype == np.uint8
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def test_the_planted_genome_through_the_host_forms(gpu, plant, planted_raw):
    text = plant["text"]
    seqs, offs = plant["seqs_offs"]
    index = _handle(planted_raw)
    index.call_add_host(seqs, offs, cc.MIN_LENGTH)
    calls, summary = index.calls(), index.cover_summary(2)
    got = index.consensus(min_depth=cc.MIN_DEPTH)
    _same(got, _reference_on_the_handle(index, text, min_depth=cc.MIN_DEPTH))
    # what the reads were cut from, and what tests/test_consensus_cpu.py gets from the Python chain
    assert got[1].tobytes() == cc.expected_body(plant)
    assert fasta_of(cc.NAMES, *got) == b"".join(b">" + n + b"\n" + cc.wrap(e, 60) for n, e in zip(cc.NAMES, plant["expected"]))
    assert got[0]["substituted"].tolist() == [7, 3] and got[0]["deleted"].tolist() == [3, 0]
    st = index.consensus_stats()
    assert (st["positions"], st["substituted"], st["deleted"], st["bytes"], st["overflow"]) == (sum(cc.LENGTHS), 10, 3, got[1].size, 0)
    assert st["masked"] == int(got[0]["masked"].sum()) and st["letters"] == int(got[0]["letters"].sum())
    for kw in (dict(), dict(min_depth=1, min_alt=1, min_permille=0, line_width=0), dict(min_depth=cc.MIN_DEPTH, mask=0, line_width=7),
               dict(min_depth=30, mask=b"n", line_width=MAX_LINE_WIDTH)):
        _same(index.consensus(**kw), _reference_on_the_handle(index, text, **kw))
    assert index.consensus(min_depth=cc.MIN_DEPTH, mask=0, line_width=0)[1].tobytes() == b"".join(c + b"\n" for c in plant["copies"])
    # the calls and the coverage are the same bytes before and after
    assert index.calls().tobytes() == calls.tobytes() and index.cover_summary(2).tobytes() == summary.tobytes()
    # a second add changes the result as the reference says: a third of the reads once more, and the ends are deep enough
    third = (offs.size - 1) // 3
    index.call_add_host(seqs[:int(offs[third])].copy(), offs[:third + 1].copy(), cc.MIN_LENGTH)
    again = index.consensus(min_depth=cc.MIN_DEPTH)
    _same(again, _reference_on_the_handle(index, text, min_depth=cc.MIN_DEPTH))
    assert int(again[0]["masked"][0]) < int(got[0]["masked"][0]) and again[1].tobytes() != got[1].tobytes()
    with pytest.raises(capi.SpxError, match="min_depth and min_alt must be at least 1"):
        index.consensus(min_depth=0)
    with pytest.raises(capi.SpxError, match="line_width must be between 0 and 2147483647"):
        index.consensus(line_width=2**31)
    with pytest.raises(capi.SpxError, match="sps_consensus_fetch without a successful sps_consensus_begin"):
        capi._check(capi._sps().sps_consensus_fetch(index._h, None, None))
    index.close()


def test_a_clone_starts_empty_and_a_new_table_drops_the_arrays(gpu, plant, planted_raw):
    text = plant["text"]
    seqs, offs = plant["seqs_offs"]
    index = capi.Index.from_raw(planted_raw, 0)
    index.set_sequences(cc.LENGTHS, cc.STRANDS)
    with pytest.raises(capi.SpxError, match="spx error -1: sps_consensus_begin without a successful spl_call_reset before it"):
        index.consensus()
    index.cover_reset()  # (the coverage alone is not enough)
    with pytest.raises(capi.SpxError, match="spx error -1: sps_consensus_begin without a successful spl_call_reset before it"):
        index.consensus()
    index.call_reset()
    index.call_add_host(seqs, offs, cc.MIN_LENGTH)
    n = capi.C.c_uint64(0)
    prm = capi.SpsParams(cc.MIN_DEPTH, 2, 500, 60, ord("N"))
    capi._check(capi._sps().sps_consensus_begin(index._h, capi.C.byref(prm), capi.C.byref(n)))  # (begun and not fetched)
    assert n.value == len(cc.expected_body(plant))
    # a clone has nothing to fetch and arrays of its own, empty: every base is masked
    other = index.clone(0)
    with pytest.raises(capi.SpxError, match="sps_consensus_fetch without a successful sps_consensus_begin"):
        capi._check(capi._sps().sps_consensus_fetch(other._h, None, None))
    with pytest.raises(capi.SpxError, match="no consensus has been computed"):
        other.consensus_stats()
    rec, body = other.consensus(min_depth=1, line_width=0)
    assert body.tobytes() == b"".join(b"N" * n + b"\n" for n in cc.LENGTHS) and rec["masked"].tolist() == cc.LENGTHS
    half = (offs.size - 1) // 2
    other.call_add_host(seqs[:int(offs[half])].copy(), offs[:half + 1].copy(), cc.MIN_LENGTH)
    _same(other.consensus(), _reference_on_the_handle(other, text))
    other.close()
    # ... and what the first handle began is still there to fetch
    records, body = np.zeros(2, dtype=SEQ_DTYPE), np.zeros(n.value, dtype=np.uint8)
    capi._check(capi._sps().sps_consensus_fetch(index._h, capi._np_ptr(records), capi._np_ptr(body)))
    assert body.tobytes() == cc.expected_body(plant)
    # a new table drops the arrays and what waits for the fetch, and the next call says so
    capi._check(capi._sps().sps_consensus_begin(index._h, capi.C.byref(prm), capi.C.byref(n)))
    index.set_sequences([sum(cc.LENGTHS)], cc.STRANDS)
    with pytest.raises(capi.SpxError, match="spn_set_sequences replaced the sequence table after spl_call_reset and dropped the pileup"):
        index.consensus()
    with pytest.raises(capi.SpxError, match="sps_consensus_fetch without a successful sps_consensus_begin"):
        capi._check(capi._sps().sps_consensus_fetch(index._h, capi._np_ptr(records), capi._np_ptr(body)))
    index.call_reset()
    rec, body = index.consensus(line_width=0)
    assert body.tobytes() == b"N" * sum(cc.LENGTHS) + b"\n" and rec["masked"].tolist() == [sum(cc.LENGTHS)]
    index.close()


def test_the_consensus_between_the_ten_products_on_one_handle(gpu):
    """Every product's answers on a handle that runs a consensus behind each of them are those of a handle that never ran
    one, and the consensus at the end is the same on both."""
    rng = np.random.default_rng(419)
    genome = cases.repetitive_text(rng, 40_000, DNA)
    raw = capi.build_raw(genome, doc_lengths=[genome.size // 3, genome.size - genome.size // 3])
    seqs, offs = cases.reads_mixed(rng, genome, DNA, 300, 500, [ord("N")])
    A = (seqs, offs.astype(np.uint64))
    B = (seqs[:int(offs[120])].copy(), offs[:121].astype(np.uint64))
    lengths = table(rng, 120, 2, genome.size)
    steps = [("call A", lambda ix: ([ix.call_add_host(*A, 6)] + _host_state(ix, lengths), None)),
             ("map A", lambda ix: (list(ix.map_host(*A, 6)), ix.map_stats())),
             ("cover B docs", lambda ix: ([ix.cover_add_host(*B, 6, want_docs=True)] + _host_state(ix, lengths), None)),
             ("extend A", lambda ix: (list(ix.extend_host(*A, 6)), ix.extend_stats())),
             ("cigar A", lambda ix: (list(ix.cigar_host(*A, 6)), ix.cigar_stats())),
             ("align B", lambda ix: (list(ix.align_host(*B, 6)), ix.align_stats())),
             ("chain A", lambda ix: (list(ix.chain_host(*A, 6)), ix.chain_stats())),
             ("mems B", lambda ix: (list(ix.mems_host(*B, 6)), ix.mems_stats())),
             ("place A", lambda ix: (list(ix.place_host(*A, 6)), ix.place_stats())),
             ("assign B", lambda ix: (list(ix.assign_host(capi.SPX_MODE_MS, *B, 6)), ix.votes_stats())),
             ("call B narrow", lambda ix: ([ix.call_add_host(*B, 6, extend_params=ExtendParams(20, 2, 1, 1))] + _host_state(ix, lengths), None))]
    used, plain = capi.Index.from_raw(raw, 0), capi.Index.from_raw(raw, 0)
    for index in (used, plain):
        index.set_sequences(lengths, 2)
        index.call_reset()
    between = []
    for i, (name, step) in enumerate(steps):
        got, got_stats = step(used)
        between.append(used.consensus(*PARAMS[i % 4], mask=MASKS[i % 3], line_width=WIDTHS[i % 6]))
        want, want_stats = step(plain)
        assert len(got) == len(want)
        for j, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (name, j)
        for s in (got_stats, want_stats):
            for key in ("kernel_ms", "step_ms", "wave_fill_ticks", "wave_back_ticks"):
                (s or {}).pop(key, None)
        assert got_stats == want_stats, (name, got_stats, want_stats)
    _same(used.consensus(), plain.consensus())
    assert used.call_stats() == {**plain.call_stats(), "step_ms": used.call_stats()["step_ms"]}
    assert all(rec["letters"].sum() > 0 for rec, _ in between)
    G = int(lengths.sum())
    depth, _ = used.cover_depth(0, G)
    alt, _, ins, dele = used.pileup_counts(0, G)
    want = consensus_reference(depth, alt.reshape(-1), ins, dele, genome, lengths, 2)
    _same(used.consensus(), want)
    assert want[0]["substituted"].sum() > 0 and want[0]["masked"].sum() > 0
    used.close()
    plain.close()


# ---- the command ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built_plant(gpu, plant, tmp_path_factory):
    """The planted reference as `spumoni build -n -M -s` indexes it, and the planted reads as a FASTA file."""
    d = tmp_path_factory.mktemp("consensus")
    (d / "a.fa").write_bytes(b"".join(b">" + n + b"\n" + cc.wrap(s, 70) for n, s in zip(cc.NAMES, plant["seqs"])))
    (d / "list.txt").write_text(f"{d / 'a.fa'}\n")
    r = _cli(["build", "-i", str(d / "list.txt"), "-o", str(d / "ref"), "-n", "-M", "-s"], dict(os.environ))
    assert r.returncode == 0, r.stderr.decode()
    assert (d / "ref.fa.rawtext").read_bytes() == plant["text"].tobytes()
    (d / "reads.fa").write_bytes(b"".join(b">r%d\n%s\n" % (q, r) for q, r in enumerate(plant["reads"])))
    return d


def _consensus_cli(d, extra=(), env=None, name="reads.fa"):
    for suffix in (".consensus.fa", ".consensus.tsv"):
        if os.path.exists(str(d / name) + suffix):
            os.remove(str(d / name) + suffix)
    r = _cli(["consensus", "-r", str(d / "ref"), "-p", str(d / name), "-n", "-L", str(cc.MIN_LENGTH)] + list(extra),
             dict(os.environ, SPUMONI_TEXT=str(d / "ref.fa.rawtext"), **(env or {})))
    assert r.returncode == 0, r.stderr.decode()
    return (d / (name + ".consensus.fa")).read_bytes(), (d / (name + ".consensus.tsv")).read_bytes(), r.stderr.decode()


def test_the_command_writes_what_the_host_forms_give(gpu, plant, planted_raw, built_plant):
    d = built_plant
    seqs, offs = plant["seqs_offs"]
    index = _handle(planted_raw)
    index.call_add_host(seqs, offs, cc.MIN_LENGTH)
    env = dict(os.environ, SPUMONI_TEXT=str(d / "ref.fa.rawtext"))
    assert _cli(["call", "-r", str(d / "ref"), "-p", str(d / "reads.fa"), "-n", "-L", str(cc.MIN_LENGTH)], env).returncode == 0
    vcf = (d / "reads.fa.vcf").read_bytes()
    assert vcf.count(b"\n") > 10
    for extra, kw in ((("-D", "3"), dict(min_depth=3)),
                      (("-D", "3", "-u"), dict(min_depth=3, mask=0)),
                      (("-D", "3", "-U", "n"), dict(min_depth=3, mask=b"n")),
                      (("-D", "3", "-J", "0"), dict(min_depth=3, line_width=0)),
                      ((), dict()),
                      (("-D", "1", "-A", "1", "-Q", "0", "-J", "2147483647", "-U", "x", "-u"), dict(min_depth=1, min_alt=1, min_permille=0,
                                                                                                   line_width=MAX_LINE_WIDTH, mask=0))):
        rec, body = index.consensus(**kw)
        for batch in (None, "1000") if extra == ("-D", "3") else (None,):
            fa, tsv, err = _consensus_cli(d, extra, env=dict(SPUMONI_SUPER_BATCH=batch) if batch else None)
            assert fa == fasta_of(cc.NAMES, rec, body), (extra, batch)
            assert tsv == tsv_of(cc.NAMES, cc.LENGTHS, rec), (extra, batch)
            assert f"{len(plant['reads'])} reads, {len(plant['reads'])} mapped, 0 without a mapping; {int(rec['letters'].sum())} letters, " \
                   f"{int(rec['substituted'].sum())} substituted, {int(rec['deleted'].sum())} deleted, {int(rec['masked'].sum())} masked" in err
            assert ("insertion sites were not applied" in err) == bool(rec["ins_sites"].sum())
    # what the reads were cut from
    fa, tsv, _ = _consensus_cli(d, ("-D", "3"))
    assert fa == b"".join(b">" + n + b"\n" + cc.wrap(e, 60) for n, e in zip(cc.NAMES, plant["expected"]))
    assert tsv.split(b"\n")[0].split(b"\t")[:5] == [b"first", b"1500", b"1497", b"7", b"3"]
    # `spumoni call` on the same file is unchanged
    assert _cli(["call", "-r", str(d / "ref"), "-p", str(d / "reads.fa"), "-n", "-L", str(cc.MIN_LENGTH)], env).returncode == 0
    assert (d / "reads.fa.vcf").read_bytes() == vcf
    index.close()


def test_the_commands_refusals_and_a_failing_run_leave_neither_file(gpu, built_plant):
    d = built_plant
    env = dict(os.environ, SPUMONI_TEXT=str(d / "ref.fa.rawtext"))
    for suffix in (".consensus.fa", ".consensus.tsv"):
        if os.path.exists(str(d / "reads.fa") + suffix):
            os.remove(str(d / "reads.fa") + suffix)
    before = sorted(os.listdir(d))
    for args, message in ((["-r", str(d / "ref"), "-p", str(d / "reads.fa"), "-n", "-P"], "-P cannot be used with `spumoni consensus`"),
                          (["-r", str(d / "ref"), "-p", str(d / "reads.fa"), "-m"], "-m / -a cannot be used with `spumoni consensus`"),
                          (["-r", str(d / "ref"), "-p", str(d / "reads.fa"), "-a"], "-m / -a cannot be used with `spumoni consensus`"),
                          (["-r", str(d / "ref"), "-p", str(d / "reads.fa")], "`spumoni consensus` needs -n"),
                          (["-r", str(d / "ref"), "-p", str(d / "reads.fa"), "-n", "-J", "2147483648"], "the line width (-J) must be between"),
                          (["-r", str(d / "ref"), "-p", str(d / "reads.fa"), "-n", "-U", "NN"], "the mask (-U) must be one byte"),
                          (["-r", str(d / "nosuch"), "-p", str(d / "reads.fa"), "-n"], "The following path is not valid")):
        r = _cli(["consensus"] + args, env)
        assert r.returncode == 1 and message in r.stderr.decode(), r.stderr.decode()
        assert sorted(os.listdir(d)) == before
    # no sequence table; and a read that is empty stops the run behind the adds, in front of the files
    os.rename(d / "ref.fa.seqs", d / "ref.fa.seqs.away")
    r = _cli(["consensus", "-r", str(d / "ref"), "-p", str(d / "reads.fa"), "-n"], env)
    os.rename(d / "ref.fa.seqs.away", d / "ref.fa.seqs")
    assert r.returncode == 1 and "the index has no sequence table" in r.stderr.decode() and sorted(os.listdir(d)) == before
    text = (d / "ref.fa.rawtext").read_bytes()
    (d / "bad.fa").write_bytes(b">good\n" + text[:60] + b"\n>bad_one\n>after\n" + text[5:65] + b"\n")
    r = _cli(["consensus", "-r", str(d / "ref"), "-p", str(d / "bad.fa"), "-n", "-L", "12"], env)
    assert r.returncode == 1 and "bad_one was empty" in r.stderr.decode(), r.stderr.decode()
    os.remove(d / "bad.fa")
    assert sorted(os.listdir(d)) == before
