"""The coverage on the GPU (include/spumoni_cover.h): crafted mappings through the device forms against
spumoni_amd/cover.py in every word of diff, mism, the counts, depth, the summary and the runs, with every buffer fenced on
both sides; the host forms against the oracle's MS arrays -> mems -> chain -> extend -> map -> cover references, alone and
interleaved with the eight products before it on one handle; and `spumoni cover` against depths counted from planted reads."""
import os

import numpy as np
import pytest
import torch

from spumoni_amd import capi, synth
from spumoni_amd.cigar import OP_D, OP_EQ, OP_I, OP_N, OP_X
from spumoni_amd.cover import RUN_DTYPE, SEQ_COVER_DTYPE, cover_reference, depth_of, runs_reference, seq_starts, summary_reference
from spumoni_amd.extend import OP_S, ExtendParams
from spumoni_amd.map import MAPPING_DTYPE, piece_starts
from tests import cases
from tests.test_cover_cpu import BAD, BAD_LENGTHS, TEXT_OPS, mapping, mbatch, spoiled
from tests.test_gpu_align import DNA, FENCE, _cli
from tests.test_gpu_map import _host_reference, _index_of, gpu, planted, revcomp, table  # noqa: F401 (gpu, planted: fixtures)

pytestmark = pytest.mark.gpu
N = 10_000
TILE = 4096  # positions of a finish / runs tile (spx_cover.hip)


@pytest.fixture(scope="module")
def ix(gpu):
    """Any index with a text of N characters: the kernels read the table and nothing else of the index."""
    index = _index_of(N)
    yield index
    index.close()


def _fenced(values, dtype, pad=4):
    """(whole tensor, view of the middle) with `values` (an array, or a count of zeros) between two fences."""
    values = np.zeros(values, dtype=dtype) if isinstance(values, int) else np.ascontiguousarray(values, dtype=dtype)
    whole = torch.full((values.size + 2 * pad,), FENCE, dtype=dtype_t(dtype), device="cuda")
    whole[pad:pad + values.size] = torch.from_numpy(values.view(signed(dtype)).reshape(-1).copy()).cuda()
    return whole, whole[pad:pad + values.size]


def dtype_t(dtype):
    return torch.int32 if np.dtype(dtype).itemsize == 4 else torch.int64


def signed(dtype):
    return np.int32 if np.dtype(dtype).itemsize == 4 else np.int64


def _unfence(whole, n, dtype, pad=4):
    got = whole.cpu().numpy()
    assert (got[:pad] == FENCE).all() and (got[pad + n:] == FENCE).all(), "a write outside the buffer"
    return got[pad:pad + n].copy().view(dtype)


def _add(ix, args, G, n_seqs, into=None, in_entries=None):
    """cover_add_device with the three arrays fenced on both sides; returns (diff, mism, counts[n_seqs, 2])."""
    recs, ooffs, ents = args
    nreads = recs.size
    d_map = torch.from_numpy(np.concatenate([recs, np.zeros(1, dtype=MAPPING_DTYPE)]).view(np.int32).reshape(-1, 12).copy()).cuda()[:nreads]
    d_ooffs = torch.from_numpy(np.asarray(ooffs, dtype=np.uint64).view(np.int64).copy()).cuda()
    d_ents = torch.from_numpy(np.r_[ents, np.zeros(1, dtype=np.uint32)].view(np.int32).copy()).cuda()[:ents.size]
    zero = (G + 1, G, 2 * n_seqs) if into is None else (into[0], into[1], into[2].reshape(-1))
    (w_diff, diff), (w_mism, mism), (w_counts, counts) = _fenced(zero[0], np.uint32), _fenced(zero[1], np.uint32), _fenced(zero[2], np.uint64)
    ix.cover_add_device(d_map, d_ooffs, d_ents, diff, mism, counts, in_entries=ents.size if in_entries is None else in_entries)
    torch.cuda.synchronize()
    return _unfence(w_diff, G + 1, np.uint32), _unfence(w_mism, G, np.uint32), _unfence(w_counts, 2 * n_seqs, np.uint64).reshape(-1, 2)


def _finish(ix, diff, mism, counts):
    """cover_finish_device with depth and the summary fenced; the inputs must come back unchanged."""
    G, n_seqs = mism.size, counts.shape[0]
    (w_diff, d_diff), (w_mism, d_mism), (w_counts, d_counts) = _fenced(diff, np.uint32), _fenced(mism, np.uint32), _fenced(counts.reshape(-1), np.uint64)
    w_depth, d_depth = _fenced(G, np.uint32)
    w_out = torch.full((n_seqs + 2, 6), FENCE, dtype=torch.int64, device="cuda")
    ix.cover_finish_device(d_diff, d_mism, d_counts, d_depth=d_depth, d_out=w_out[1:1 + n_seqs])
    torch.cuda.synchronize()
    assert np.array_equal(_unfence(w_diff, G + 1, np.uint32), diff) and np.array_equal(_unfence(w_mism, G, np.uint32), mism)
    assert np.array_equal(_unfence(w_counts, 2 * n_seqs, np.uint64).reshape(-1, 2), counts)
    out = w_out.cpu().numpy()
    assert (out[0] == FENCE).all() and (out[1 + n_seqs] == FENCE).all()
    return _unfence(w_depth, G, np.uint32), out[1:1 + n_seqs].copy().view(SEQ_COVER_DTYPE).reshape(-1)


def _runs(ix, depth, mism, min_depth, cap):
    """cover_runs_device with the records and the count fenced; returns (the records that fit, the count)."""
    (_, d_depth), (_, d_mism) = _fenced(depth, np.uint32), _fenced(mism, np.uint32)
    w_runs = torch.full((cap + 4, 4), FENCE, dtype=torch.int64, device="cuda")
    w_count, d_count = _fenced(1, np.uint64)
    ix.cover_runs_device(d_depth, d_mism, min_depth, cap, d_runs=w_runs[2:2 + max(cap, 1)] if cap else None, d_count=d_count)
    torch.cuda.synchronize()
    total = int(_unfence(w_count, 1, np.uint64)[0])
    runs = w_runs.cpu().numpy()
    fit = min(total, cap)
    assert (runs[:2] == FENCE).all() and (runs[2 + fit:] == FENCE).all(), "a record outside the runs that fit"
    return runs[2:2 + fit].copy().view(RUN_DTYPE).reshape(-1), total


def _check(ix, args, lengths, strands=1, error=0, in_entries=None, clean=None):
    """Everything of one batch against the references: the add, its stats, the finish and the runs at min_depth 0, 1, 2."""
    ix.set_sequences(lengths, strands)
    F = seq_starts(lengths)
    G, n_seqs = F[-1], len(lengths)
    count = {}
    want = cover_reference(*args, lengths, count=count, in_entries=in_entries)
    if clean is not None:  # the reference that never saw the bad read
        assert all(a.tobytes() == b.tobytes() for a, b in zip(want, cover_reference(*clean, lengths)))
    got = _add(ix, args, G, n_seqs, in_entries=in_entries)
    for name, g, w in zip(("diff", "mism", "counts"), got, want):
        bad = np.flatnonzero((g != w).reshape(-1))
        assert g.dtype == w.dtype and g.shape == w.shape and bad.size == 0, (name, bad[:5], g.reshape(-1)[bad[:5]], w.reshape(-1)[bad[:5]])
    assert count["error"] == error
    if error:
        with pytest.raises(capi.SpxError, match="spx error -5: a read's mapping failed the coverage's checks"):
            ix.cover_stats()
    else:
        st = ix.cover_stats()
        assert (st["reads"], st["mapped"], st["added"], st["skipped"], st["intervals"], st["atomics"], st["error"]) == \
            (args[0].size, count["mapped"], count["added"], 0, count["intervals"], count["atomics"], 0), (st, count)
    depth, out = _finish(ix, *want)
    w_depth, w_out = depth_of(want[0]), summary_reference(*want, lengths)
    bad = np.flatnonzero(depth != w_depth)
    assert bad.size == 0, (bad[:5], depth[bad[:5]], w_depth[bad[:5]])
    bad = np.flatnonzero(out != w_out)
    assert bad.size == 0, (bad[:5], out[bad[:5]], w_out[bad[:5]])
    for min_depth in (0, 1, 2):
        w_runs = runs_reference(w_depth, want[1], lengths, min_depth)
        runs, total = _runs(ix, w_depth, want[1], min_depth, w_runs.size + 3)
        bad = np.flatnonzero(runs != w_runs) if runs.size == w_runs.size else [-1]
        assert total == w_runs.size and len(bad) == 0, (min_depth, total, w_runs.size, bad[:5])
    return want, w_depth, count


def random_mapping(rng, lengths, max_runs=8, max_len=9):
    """A mapping of a few random runs that fits a random sequence (short sequences get short reads)."""
    s = int(rng.integers(0, len(lengths)))
    L = int(lengths[s])
    while True:
        k = int(rng.integers(1, max_runs + 1))
        ents = [int(rng.integers(1, max_len + 1)) << 4 | int(op) for op in rng.choice((OP_EQ, OP_EQ, OP_EQ, OP_X, OP_I, OP_D, OP_N), k)]
        if L < 4:
            ents = [int(rng.integers(1, L + 1)) << 4 | int(rng.choice((OP_EQ, OP_X)))]
        text = sum(e >> 4 for e in ents if e & 15 in TEXT_OPS)
        if text <= L:
            if rng.random() < 0.3:
                ents = [3 << 4 | OP_S] + ents + [2 << 4 | OP_S]
            return mapping(ents, s, int(rng.integers(0, L - text + 1)), strand=int(rng.integers(0, 2)))


@pytest.mark.parametrize("n_seqs,strands", [(1, 1), (1, 2), (2, 2), (3, 1), (64, 2), (65, 1), (5000, 2)])
def test_tables_of_one_to_many_sequences(gpu, ix, n_seqs, strands):
    """One sequence, a few, just over a wavefront's worth, and 5 000 of one base each: there every position is a border,
    every run has one base and a tile of the finish spans 4 096 sequences."""
    rng = np.random.default_rng(n_seqs * 2 + strands)
    lengths = table(rng, n_seqs, strands)
    if n_seqs == 5000:
        assert (lengths == 1).all()
    maps = [random_mapping(rng, lengths, max_len=1 + 400 // n_seqs) if rng.random() < 0.95 else None for _ in range(600)]
    # mappings that fill a sequence from its first to its last base: the first, a middle and the last sequence
    for s in (0, n_seqs // 2, n_seqs - 1):
        maps.append(mapping(f"{lengths[s]}=", s, 0))
    maps += [mapping("1X", n_seqs - 1, int(lengths[-1]) - 1), mapping("1=", 0, 0)]
    want, depth, count = _check(ix, mbatch(maps), lengths, strands)
    assert count["added"] > 500 and depth.max() >= 2 and want[1].any()


def test_sequences_around_the_finish_tile(gpu):
    """Sequences one below, at and one above the tile, so that borders fall on the last position of a tile, on its first
    and one behind it; reads that cover each border's two sides, and whole sequences."""
    lengths = [TILE - 1, TILE, TILE + 1, 1, 2 * TILE - 2, 7]
    index = _index_of(sum(lengths))
    rng = np.random.default_rng(4)
    maps = [random_mapping(rng, lengths, max_runs=12, max_len=40) for _ in range(500)]
    for s, L in enumerate(lengths):
        maps += [mapping(f"{min(L, 5)}=", s, 0), mapping(f"{min(L, 5)}X", s, L - min(L, 5)), mapping(f"{L}=", s, 0)]
    maps += [mapping(f"{TILE - 1}=", 1, 1), mapping("15=1X", 1, TILE - 16), mapping("17=", 2, 0), mapping("16=", 4, TILE - 1)]
    want, depth, count = _check(index, mbatch(maps), lengths)
    assert count["added"] == len(maps) and depth.min() >= 1  # every base is covered: the runs at min_depth 1 partition too
    index.close()


def with_entries(rng, k, L):
    """A mapping of exactly k entries of zero to three columns each on a sequence of L bases."""
    while True:
        ops = rng.choice((OP_EQ, OP_EQ, OP_EQ, OP_X, OP_I, OP_D, OP_N), k)
        ents = [int(rng.integers(0 if k > 4 else 1, 4)) << 4 | int(op) for op in ops]
        text = sum(e >> 4 for e in ents if e & 15 in TEXT_OPS)
        if text <= L:
            return mapping(ents, 0, int(rng.integers(0, L - text + 1)))


def test_reads_of_0_to_1300_entries_on_both_sides_of_the_switch(gpu, ix):
    """Long and short reads mixed in one batch: up to 64 entries a lane walks the read, above a wavefront does.  The same
    batch with every read given a wavefront, and with every read given a lane, adds the same bytes."""
    rng = np.random.default_rng(21)
    lengths = np.array([N], dtype=np.uint64)
    maps = []
    for k in (0, 1, 2, 16, 17, 63, 64, 65, 127, 128, 129, 1300) * 3:
        maps.append(with_entries(rng, k, N))
        if k >= 3:  # the same with both clips among the k entries
            rec, ents = with_entries(rng, k - 2, N)
            maps.append((rec, [5 << 4 | OP_S] + ents + [1 << 4 | OP_S]))
    maps.append(None)
    args = mbatch(maps)
    assert sorted(set(np.diff(args[1].astype(np.int64)).tolist())) == [0, 1, 2, 16, 17, 63, 64, 65, 127, 128, 129, 1300]
    want, _, count = _check(ix, args, lengths)
    assert count["added"] == len(maps) - 1
    try:
        for switch in (0, 1 << 20):
            ix.set_option("cover_switch", switch)
            got = _add(ix, args, N, 1)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), switch
            st = ix.cover_stats()
            assert (st["added"], st["intervals"], st["atomics"]) == (count["added"], count["intervals"], count["atomics"]), (switch, st)
    finally:
        ix.set_option("cover_switch", 64)


@pytest.mark.parametrize("nreads", [0, 1, 63, 64, 65, 3000])
def test_read_counts_around_the_wavefront(gpu, ix, nreads):
    rng = np.random.default_rng(nreads)
    lengths = table(rng, 40, 2)
    maps = [random_mapping(rng, lengths, max_runs=6, max_len=30) if rng.random() < 0.9 else None for _ in range(nreads)]
    _, _, count = _check(ix, mbatch(maps), lengths, 2)
    assert count["mapped"] >= nreads * 3 // 4 and count["reads"] == nreads


def test_all_reads_on_one_sequence_and_on_one_base(gpu, ix):
    """3 000 reads whose counters are one pair of words, and whose depth is one word; then sequences 256 apart, which
    share a slot of a block's table."""
    rng = np.random.default_rng(5)
    lengths = table(rng, 16, 1)
    one = [lengths[5]]
    maps = []
    for _ in range(3000):
        rec, ents = random_mapping(rng, one, max_runs=6, max_len=20)
        rec["seq"] = 5
        maps.append((rec, ents))
    want, depth, _ = _check(ix, mbatch(maps), lengths)
    assert want[2][5, 0] == 3000 and want[2][:, 0].sum() == 3000 and want[2][5, 1] > 1000
    maps = [mapping("1=" if q % 3 else "1X", 9, 2) for q in range(3000)]
    want, depth, _ = _check(ix, mbatch(maps), lengths)
    F = seq_starts(lengths)
    assert depth[F[9] + 2] == 3000 and depth.sum() == 3000 and want[1][F[9] + 2] == 1000
    lengths = table(rng, 600, 1)
    maps = [mapping("1=1I", int(s), 0) for s in rng.choice([3, 259, 515, 4, 260], 2000)]
    want, _, _ = _check(ix, mbatch(maps), lengths)
    assert sorted(np.flatnonzero(want[2][:, 0]).tolist()) == [3, 4, 259, 260, 515] and want[2][:, 1].sum() == 2000


def test_the_strand_field_does_not_enter(gpu, ix):
    rng = np.random.default_rng(6)
    lengths = table(rng, 30, 2)
    maps = [random_mapping(rng, lengths) for _ in range(300)]
    args = mbatch(maps)
    ix.set_sequences(lengths, 2)
    a = _add(ix, args, int(lengths.sum()), 30)
    args[0]["strand"] ^= 1
    b = _add(ix, args, int(lengths.sum()), 30)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    want = cover_reference(*args, lengths)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, want))


@pytest.mark.parametrize("switch", [64, 0], ids=["lane", "wavefront"])
@pytest.mark.parametrize("kind", BAD)
def test_bad_inputs_are_skipped_whole_and_reported(gpu, kind, switch):
    """tests/test_cover_cpu.py's bad reads one by one, by a lane and by a wavefront: the error is reported and the arrays
    are those of the batch without the read."""
    index = _index_of(sum(BAD_LENGTHS))
    index.set_option("cover_switch", switch)
    args, clean, in_entries = spoiled(kind)
    _check(index, args, BAD_LENGTHS, error=1, in_entries=in_entries, clean=clean)
    _check(index, clean, BAD_LENGTHS)  # (and the next call on the handle reports no error)
    index.close()


def test_run_capacity_from_zero_to_above(gpu, ix):
    rng = np.random.default_rng(8)
    lengths = table(rng, 50, 1)
    ix.set_sequences(lengths, 1)
    want = cover_reference(*mbatch([random_mapping(rng, lengths, max_len=30) for _ in range(400)]), lengths)
    depth = depth_of(want[0])
    w_runs = runs_reference(depth, want[1], lengths, 1)
    assert w_runs.size > 100
    for cap in (0, 1, w_runs.size - 1, w_runs.size, w_runs.size + 1):
        runs, total = _runs(ix, depth, want[1], 1, cap)
        st = ix.cover_stats()
        assert total == w_runs.size == st["runs"] and np.array_equal(runs, w_runs[:cap]), cap  # the count is kept
        assert st["overflow"] == int(cap < w_runs.size), (cap, st)


def test_two_adds_equal_one_and_repeated_calls_give_the_same_bytes(gpu, ix):
    rng = np.random.default_rng(9)
    lengths = table(rng, 90, 2)
    ix.set_sequences(lengths, 2)
    G = int(lengths.sum())
    maps = [random_mapping(rng, lengths, max_len=40) if rng.random() < 0.9 else None for _ in range(500)]
    whole = _add(ix, mbatch(maps), G, 90)
    again = _add(ix, mbatch(maps), G, 90)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, again))
    first = _add(ix, mbatch(maps[:200]), G, 90)
    both = _add(ix, mbatch(maps[200:]), G, 90, into=first)
    other = _add(ix, mbatch(maps[:200][::-1]), G, 90, into=_add(ix, mbatch(maps[200:]), G, 90))
    want = cover_reference(*mbatch(maps), lengths)
    for a, b, c, w in zip(whole, both, other, want):
        assert a.tobytes() == b.tobytes() == c.tobytes() == w.tobytes()
    assert ix.cover_stats()["reads"] == 200  # of the last add_device call
    f1, f2 = _finish(ix, *whole), _finish(ix, *whole)
    assert f1[0].tobytes() == f2[0].tobytes() and f1[1].tobytes() == f2[1].tobytes()


# ---- the host forms ----------------------------------------------------------------------------------------------------------
def _cover_host_reference(orc, text, seqs, offs, min_length, ep, lengths, strands, into=None, count=None):
    _, (maps, m_offs, m_ents) = _host_reference(orc, text, seqs, offs, min_length, ep, piece_starts(lengths, strands), strands)
    return maps, cover_reference(maps, m_offs, m_ents, lengths, into=into, count=count)


def _host_state(ix, lengths):
    """(depth, mism, summary, runs at min_depth 0) of the handle's arrays."""
    G = int(np.sum(lengths))
    depth, mism = ix.cover_depth(0, G)
    return depth, mism, ix.cover_summary(len(lengths)), ix.cover_runs(0)


def _assert_host(ix, lengths, want):
    depth, mism, summary, runs = _host_state(ix, lengths)
    w_depth = depth_of(want[0])
    assert np.array_equal(depth, w_depth) and np.array_equal(mism, want[1])
    assert np.array_equal(summary, summary_reference(*want, lengths)) and np.array_equal(runs, runs_reference(w_depth, want[1], lengths, 0))
    assert np.array_equal(ix.cover_runs(1), runs_reference(w_depth, want[1], lengths, 1))
    part = ix.cover_depth(3, 17)
    assert np.array_equal(part[0], w_depth[3:20]) and np.array_equal(part[1], want[1][3:20])


@pytest.mark.parametrize("strands", [1, 2])
def test_cover_host_on_an_index_from_the_oracles_side(gpu, oracle_mod, strands):
    rng = np.random.default_rng(180 + strands)
    text = cases.repetitive_text(rng, 40_000, DNA)
    raw = synth.index_from_text(torch.from_numpy(text), doc_lengths=[text.size // 2, text.size - text.size // 2])
    orc = oracle_mod.OracleIndex.from_raw(raw)
    ix = capi.Index.from_raw(raw, 0)
    ix.set_text(torch.from_numpy(text.copy()))
    seqs, offs = cases.reads_mixed(rng, text, DNA, 300, 500, [ord("N")])
    offs = offs.astype(np.uint64)
    half = int(offs[150])
    A, B = (seqs[:half].copy(), offs[:151].copy()), (seqs[half:].copy(), offs[150:] - offs[150])
    lengths = table(rng, 150, strands, text.size)
    ix.set_sequences(lengths, strands)
    ix.cover_reset()
    count = {}
    maps_a, state = _cover_host_reference(orc, text, *A, 6, None, lengths, strands, count=count)
    got = ix.cover_add_host(*A, 6, want_docs=True)
    assert got.dtype == MAPPING_DTYPE and np.array_equal(got, maps_a)
    _assert_host(ix, lengths, state)
    # a second batch with other parameters adds to the first; the stats count since the reset
    ep = ExtendParams(40, 3, 1, 2)
    maps_b, state = _cover_host_reference(orc, text, *B, 12, ep, lengths, strands, into=state, count=count)
    assert np.array_equal(ix.cover_add_host(*B, 12, extend_params=ep, want_docs=True), maps_b)
    _assert_host(ix, lengths, state)
    st = ix.cover_stats()
    assert (st["reads"], st["mapped"], st["added"], st["skipped"], st["intervals"], st["atomics"], st["error"], st["overflow"]) == \
        (offs.size - 1, count["mapped"], count["added"], 0, count["intervals"], count["atomics"], 0, 0), (st, count)
    assert count["added"] > 100 and state[1].any() and state[2][:, 1].any() and len(st["step_ms"]) == 3
    # the entries never come back, and an empty batch adds nothing
    with pytest.raises(capi.SpxError, match="spn_map_fetch without a successful spn_map_begin"):
        capi._check(capi._spn().spn_map_fetch(ix._h, None, None))
    assert ix.cover_add_host(np.zeros(0, dtype=np.uint8), [0], 4).size == 0
    _assert_host(ix, lengths, state)
    # a reset zeroes
    ix.cover_reset()
    zero = cover_reference(*mbatch([]), lengths)
    _assert_host(ix, lengths, zero)
    assert ix.cover_stats()["reads"] == 0
    ix.close()


def test_a_clone_has_its_own_arrays_and_the_refusals(gpu):
    rng = np.random.default_rng(11)
    genome = cases.repetitive_text(rng, 20_000, DNA)
    raw = capi.build_raw(genome)
    seqs, offs = cases.reads_mixed(rng, genome, DNA, 120, 300, [ord("N")])
    offs = offs.astype(np.uint64)
    lengths = table(rng, 20, 2, genome.size)
    ix = capi.Index.from_raw(raw, 0)
    with pytest.raises(capi.SpxError, match="spx error -1: spd_cover_reset needs the sequence table: the index has none"):
        ix.cover_reset()
    with pytest.raises(capi.SpxError, match="spx error -1: spd_cover_add_batch needs the sequence table"):
        ix.cover_add_host(seqs, offs, 6)
    with pytest.raises(capi.SpxError, match="no coverage has been computed"):
        ix.cover_stats()
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    with pytest.raises(capi.SpxError, match="spx error -1: spd_cover_add_device needs the sequence table"):
        ix.cover_add_device(t, t[:2], t, t, t, t)
    with pytest.raises(capi.SpxError, match="spx error -1: spd_cover_finish_device needs the sequence table"):
        ix.cover_finish_device(t, t, t, d_depth=t, d_out=t)
    with pytest.raises(capi.SpxError, match="spx error -1: spd_cover_runs_device needs the sequence table"):
        ix.cover_runs_device(t, t, 1, 4, d_runs=t, d_count=t)
    ix.set_sequences(lengths, 2)
    for call in (lambda: ix.cover_add_host(seqs, offs, 6), lambda: ix.cover_summary(20), lambda: ix.cover_runs(1), lambda: ix.cover_depth(0, 5)):
        with pytest.raises(capi.SpxError, match="spx error -1: spd_cover_[a-z_]+ without a successful spd_cover_reset"):
            call()
    with pytest.raises(capi.SpxError, match="spd_cover_runs_fetch without a successful spd_cover_runs_begin"):
        capi._check(capi._spd().spd_cover_runs_fetch(ix._h, None))
    S = capi._spd()
    p = t.data_ptr()
    assert S.spd_cover_add_device(ix._h, p, p, p, 4, 1, None, p, p, None) == -1 and b"must be non-null" in capi.lib().spx_last_error()
    assert S.spd_cover_add_device(ix._h, p + 8, p, p, 4, 1, p, p, p, None) == -1 and b"16-byte aligned" in capi.lib().spx_last_error()
    assert S.spd_cover_finish_device(ix._h, p, p, p, None, p, None) == -1 and b"must be non-null" in capi.lib().spx_last_error()
    assert S.spd_cover_finish_device(ix._h, p, p, p + 4, p, p, None) == -1 and b"8-byte aligned" in capi.lib().spx_last_error()
    assert S.spd_cover_runs_device(ix._h, p, p, 1, 4, None, p, None) == -1 and b"must be non-null" in capi.lib().spx_last_error()
    assert S.spd_cover_runs_device(ix._h, p, p + 2, 1, 4, p, p, None) == -1 and b"8-byte aligned" in capi.lib().spx_last_error()
    ix.cover_reset()
    ix.cover_add_host(seqs, offs, 6)
    mine = _host_state(ix, lengths)
    assert mine[0].any()
    with pytest.raises(capi.SpxError, match="n_seqs is 19, the sequence table has 20"):
        ix.cover_summary(19)
    with pytest.raises(capi.SpxError, match="does not lie in the forward genome"):
        ix.cover_depth(genome.size // 2 - 3, 4)
    # a clone starts with arrays of its own, empty, and what it adds stays its own
    other = ix.clone(0)
    theirs = _host_state(other, lengths)
    assert not theirs[0].any() and not theirs[1].any() and not theirs[2]["reads"].any()
    half = int(offs[60])
    other.cover_add_host(seqs[:half].copy(), offs[:61].copy(), 6)
    assert all(np.array_equal(a, b) for a, b in zip(_host_state(ix, lengths), mine))
    fresh = capi.Index.from_raw(raw, 0)
    fresh.set_sequences(lengths, 2)
    fresh.cover_reset()
    fresh.cover_add_host(seqs[:half].copy(), offs[:61].copy(), 6)
    assert all(np.array_equal(a, b) for a, b in zip(_host_state(other, lengths), _host_state(fresh, lengths)))
    fresh.close()
    other.close()
    # a new table drops the arrays, and the next call says so
    ix.set_sequences(table(rng, 5, 2, genome.size), 2)
    for call in (lambda: ix.cover_add_host(seqs, offs, 6), lambda: ix.cover_summary(5)):
        with pytest.raises(capi.SpxError, match="spn_set_sequences replaced the sequence table after spd_cover_reset and dropped the coverage"):
            call()
    ix.cover_reset()
    assert not ix.cover_summary(5)["reads"].any()
    # a reset with no add behind it and then a new table: nothing was enqueued, and the handle goes on working
    ix.set_sequences(lengths, 2)
    assert ix.map_host(seqs, offs, 6)[0].size == offs.size - 1
    ix.cover_reset()
    ix.cover_add_host(seqs, offs, 6)
    assert all(np.array_equal(a, b) for a, b in zip(_host_state(ix, lengths), mine))
    ix.close()


def test_the_nine_products_interleaved_on_one_handle(gpu):
    """Every product's answers on a handle that the others have used are those of a fresh handle; the coverage's arrays
    live through the other products' calls, and every later add lands on what the earlier ones left."""
    rng = np.random.default_rng(190)
    genome = cases.repetitive_text(rng, 40_000, DNA)
    raw = capi.build_raw(genome, doc_lengths=[genome.size // 3, genome.size - genome.size // 3])
    seqs, offs = cases.reads_mixed(rng, genome, DNA, 300, 500, [ord("N")])
    A = (seqs, offs.astype(np.uint64))
    B = (seqs[:int(offs[120])].copy(), offs[:121].astype(np.uint64))
    lengths = table(rng, 120, 2, genome.size)
    cover = lambda ix, reads, **kw: ([ix.cover_add_host(*reads, 6, **kw)] + list(_host_state(ix, lengths)), None)
    steps = [("cover A", lambda ix: cover(ix, A)),
             ("map A", lambda ix: (list(ix.map_host(*A, 6)), ix.map_stats())),
             ("cover B docs", lambda ix: cover(ix, B, want_docs=True)),
             ("extend A", lambda ix: (list(ix.extend_host(*A, 6)), ix.extend_stats())),
             ("cigar A", lambda ix: (list(ix.cigar_host(*A, 6)), ix.cigar_stats())),
             ("cover A narrow", lambda ix: cover(ix, A, extend_params=ExtendParams(20, 2, 1, 1))),
             ("align B", lambda ix: (list(ix.align_host(*B, 6)), ix.align_stats())),
             ("chain A", lambda ix: (list(ix.chain_host(*A, 6)), ix.chain_stats())),
             ("mems B", lambda ix: (list(ix.mems_host(*B, 6)), ix.mems_stats())),
             ("place A", lambda ix: (list(ix.place_host(*A, 6)), ix.place_stats())),
             ("assign B", lambda ix: (list(ix.assign_host(capi.SPX_MODE_MS, *B, 6)), ix.votes_stats())),
             ("cover B", lambda ix: cover(ix, B)),
             ("map A", lambda ix: (list(ix.map_host(*A, 6)), ix.map_stats()))]
    ix = capi.Index.from_raw(raw, 0)
    ix.set_sequences(lengths, 2)
    ix.cover_reset()
    done = []  # the cover steps so far: a fresh handle replays them, so that its arrays hold what this one's hold
    for name, step in steps:
        got, got_stats = step(ix)
        fresh = capi.Index.from_raw(raw, 0)
        fresh.set_sequences(lengths, 2)
        fresh.cover_reset()
        for earlier in done:
            earlier(fresh)
        want, want_stats = step(fresh)
        fresh.close()
        if name.startswith("cover"):
            done.append(step)
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (name, i)
        for s in (got_stats, want_stats):
            for key in ("kernel_ms", "step_ms", "wave_fill_ticks", "wave_back_ticks"):
                (s or {}).pop(key, None)
        assert got_stats == want_stats, (name, got_stats, want_stats)
    st = ix.cover_stats()
    assert st["reads"] == 2 * 300 + 2 * 120 and st["added"] > 300 and st["error"] == 0
    ix.close()


# ---- the command: ground truth that does not rest on the rule ---------------------------------------------------------------
def _cover_cli(planted, reads, name, extra=(), env=None, write=True):
    d = planted["dir"]
    path = d / name
    if write:
        path.write_bytes(b"".join(b">r%d\n%s\n" % (q, r) for q, r in enumerate(reads)))
    for suffix in (".cover", ".bedgraph"):
        if os.path.exists(str(path) + suffix):
            os.remove(str(path) + suffix)
    r = _cli(["cover", "-r", str(d / "ref"), "-p", str(path), "-n", "-L", "12"] + list(extra),
             dict(os.environ, SPUMONI_TEXT=str(d / "ref.fa.rawtext"), **(env or {})))
    assert r.returncode == 0, r.stderr.decode()
    bed = (path.parent / (name + ".bedgraph")).read_bytes() if "-b" in extra else None
    assert ("-b" in extra) == os.path.exists(str(path) + ".bedgraph")
    return (path.parent / (name + ".cover")).read_bytes(), bed, r.stderr.decode()


def _six(num, den):
    scaled = (num * 2_000_000 + den) // (2 * den)
    return b"%d.%06d" % (scaled // 1_000_000, scaled % 1_000_000)


def _expected_files(planted, depth, reads_per_seq, min_depth):
    """The two files from per-sequence depth arrays counted by the test: exact reads have no mismatches and no indels."""
    cover, bed = [], []
    for name in planted["names"]:
        d = depth[name]
        L = d.size
        cover.append(b"%s\t%d\t%d\t%d\t%s\t%d\t%s\t%d\t0\t0\n" % (name, L, reads_per_seq[name], int((d > 0).sum()), _six(int((d > 0).sum()), L),
                                                               int(d.sum()), _six(int(d.sum()), L), int(d.max())))
        start = 0
        for p in range(1, L + 1):
            if p == L or d[p] != d[start]:
                if d[start] >= min_depth:
                    bed.append(b"%s\t%d\t%d\t%d\n" % (name, start, p, int(d[start])))
                start = p
    return b"".join(cover), b"".join(bed)


def _plant(planted, rng, per_seq, m=60):
    truth, reads = [], []
    for name in planted["names"]:
        s = planted["seqs"][name]
        for off in [0, len(s) - m] + [int(v) for v in rng.integers(0, len(s) - m, per_seq)]:
            for strand in (b"+", b"-") if planted["rc"] else (b"+",):
                truth.append((name, off))
                reads.append(s[off:off + m] if strand == b"+" else revcomp(s[off:off + m]))
    depth = {name: np.zeros(len(planted["seqs"][name]), dtype=np.int64) for name in planted["names"]}
    per = {name: 0 for name in planted["names"]}
    for name, off in truth:
        depth[name][off:off + m] += 1  # the depth of a base is the number of plants that cover it
        per[name] += 1
    return reads, depth, per


def test_planted_reads_give_the_depth_the_test_counts(planted):
    rng = np.random.default_rng(31)
    reads, depth, per = _plant(planted, rng, 12)
    reads.append(b"ACGT" * 5)  # (an unmapped read adds nothing)
    d = planted["dir"]
    # `spumoni map` on the same file, before and after: the coverage changes nothing of it
    env = dict(os.environ, SPUMONI_TEXT=str(d / "ref.fa.rawtext"))
    (d / "cov.fa").write_bytes(b"".join(b">r%d\n%s\n" % (q, r) for q, r in enumerate(reads)))
    assert _cli(["map", "-r", str(d / "ref"), "-p", str(d / "cov.fa"), "-n", "-L", "12"], env).returncode == 0
    paf = (d / "cov.fa.paf").read_bytes()
    for min_depth in (1, 0, 3):
        w_cover, w_bed = _expected_files(planted, depth, per, min_depth)
        cover, bed, err = _cover_cli(planted, reads, "cov.fa", extra=("-b",) + (("-D", str(min_depth)) if min_depth != 1 else ()), write=False)
        assert cover.split(b"\n") == w_cover.split(b"\n") and bed.split(b"\n") == w_bed.split(b"\n"), min_depth
        assert f"{len(reads)} reads, {len(reads) - 1} mapped, {len(reads) - 1} added to the coverage, 1 without a mapping" in err
    cover, bed, _ = _cover_cli(planted, reads, "cov.fa", write=False)
    assert cover == w_cover and bed is None
    # small super-batches accumulate to the same files
    again = _cover_cli(planted, reads, "cov.fa", extra=("-b", "-D", "3"), env=dict(SPUMONI_SUPER_BATCH="1000"), write=False)
    assert again[0] == w_cover and again[1] == w_bed
    assert _cli(["map", "-r", str(d / "ref"), "-p", str(d / "cov.fa"), "-n", "-L", "12"], env).returncode == 0
    assert (d / "cov.fa.paf").read_bytes() == paf


def test_a_full_super_batch_cut_into_two_calls_gives_the_same_files(planted):
    """33.75 M characters in one super-batch of 64 Mi are two calls of spd_cover_add_batch that add up; in super-batches of
    16 Mi they are three calls.  The depth is counted from where the reads were taken."""
    rng = np.random.default_rng(34)
    nreads, m = 225_000, 150
    names = planted["names"]
    which = rng.integers(0, 3, nreads)
    room = np.array([len(planted["seqs"][name]) - m for name in names])[which]
    at = (rng.random(nreads) * room).astype(np.int64)
    depth, per = {}, {}
    d = planted["dir"]
    with open(d / "bigcov.fa", "wb") as f:
        for w, name in enumerate(names):
            s = np.frombuffer(planted["seqs"][name], dtype=np.uint8)
            mine = np.flatnonzero(which == w)
            rs = s[at[mine].astype(np.int32)[:, None] + np.arange(m, dtype=np.int32)[None, :]]
            f.write(b"".join(b">r%d\n%s\n" % (q, rs[q].tobytes()) for q in range(mine.size)))
            dd = np.zeros(s.size + 1, dtype=np.int64)
            np.add.at(dd, at[mine], 1)
            np.add.at(dd, at[mine] + m, -1)
            depth[name], per[name] = np.cumsum(dd)[:-1], mine.size
    w_cover, w_bed = _expected_files(planted, depth, per, 1)
    for batch in (64 << 20, 16 << 20):
        cover, bed, err = _cover_cli(planted, None, "bigcov.fa", extra=("-b", "-L", "20"), env=dict(SPUMONI_SUPER_BATCH=str(batch)), write=False)
        assert f"{nreads} reads, {nreads} mapped, {nreads} added".encode() in err.encode()
        assert cover == w_cover and bed == w_bed, batch
    for suffix in ("", ".cover", ".bedgraph"):
        os.remove(str(d / "bigcov.fa") + suffix)
