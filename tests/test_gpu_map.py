"""-m gpu: the mappings (spumoni_amd/csrc/spx_map.hip, include/spumoni_map.h) against the definition
(spumoni_amd/map.py: map_reference), bit for bit: the records, the op offsets and every entry.

map_device gets crafted records, entries and read offsets (tests/test_map_cpu.py's alignment and batch) on an index whose
text only has to have the table's length: the kernels read neither the text nor the reads.  map_host is held to the
oracle's MS arrays -> mems_reference -> chain_reference -> extend_reference -> map_reference, and `spumoni map` to reads
planted in a FASTA the test writes itself, replayed against that FASTA.  A read is one lane's: the crafted reads have 0 to
1 300 entries, the tables 1 to 5 000 sequences."""
import os

import numpy as np
import pytest
import torch

from spumoni_amd import capi, synth
from spumoni_amd.align import ALIGN_DTYPE, UNALIGNED
from spumoni_amd.chain import chain_reference
from spumoni_amd.cigar import MAX_LENGTH, OP_D, OP_EQ, OP_I, OP_N, OP_X
from spumoni_amd.extend import OP_S, ExtendParams, cigar_text, extend_reference
from spumoni_amd.map import CUT_LEFT, CUT_RIGHT, MAPPING_DTYPE, UNMAPPED, map_reference, piece_starts, read_seq_table
from spumoni_amd.mems import mems_reference
from tests import cases
from tests.test_gpu_align import DNA, FENCE, _cli
from tests.test_map_cpu import READ_OPS, TEXT_OPS, alignment, batch, check_invariants, entries_of, random_alignment

pytestmark = pytest.mark.gpu
N = 10_000  # the crafted text: 5 000 sequences of one character on both strands
UNMAPPED_REC = (0, 0, UNMAPPED, 0, 0, 0, 0, 0, 0, 0)


@pytest.fixture(scope="module")
def gpu(built_all):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    capi.lib()
    return 0


def _index_of(n_text):
    ix = capi.Index.from_raw(synth.statistical_rlbwt(5000, 60, 4.0, seed=3, with_samples=True, n_docs=8), 0)
    ix.set_text(torch.from_numpy(np.full(n_text, ord("A"), dtype=np.uint8)), unchecked=True)
    return ix


@pytest.fixture(scope="module")
def ix(gpu):
    """Any index with a text of N characters: the kernels read the table and nothing else of the index."""
    index = _index_of(N)
    yield index
    index.close()


def table(rng, n_seqs, strands, n_text=N):
    """n_seqs random lengths that fill n_text on `strands` strands."""
    total = n_text // strands
    cuts = np.sort(rng.choice(np.arange(1, total), n_seqs - 1, replace=False)) if n_seqs > 1 else np.zeros(0, dtype=np.int64)
    return np.diff(np.r_[0, cuts, total]).astype(np.uint64)


def _run(ix, args, op_cap=None):
    """map_device with every output fenced on both sides; returns (records, op_offsets, entries up to what fits)."""
    recs, ooffs, ents, roffs = args
    nreads = recs.size
    d_rec = torch.from_numpy(np.concatenate([recs, np.zeros(1, dtype=ALIGN_DTYPE)]).view(np.int32).reshape(-1, 12).copy()).cuda()[:nreads]
    d_ooffs = torch.from_numpy(np.asarray(ooffs, dtype=np.uint64).view(np.int64).copy()).cuda()
    d_ents = torch.from_numpy(np.r_[ents, np.zeros(1, dtype=np.uint32)].view(np.int32).copy()).cuda()[:ents.size]
    d_roffs = torch.from_numpy(np.asarray(roffs, dtype=np.uint64).view(np.int64).copy()).cuda()
    if op_cap is None:
        op_cap = ents.size + 2 * nreads
    fenced = torch.full((nreads + 6, 12), FENCE, dtype=torch.int32, device="cuda")
    f_ooffs = torch.full((nreads + 1 + 4,), FENCE, dtype=torch.int64, device="cuda")
    f_ops = torch.full((op_cap + 8,), FENCE, dtype=torch.int32, device="cuda")
    ix.map_device(d_rec, d_ooffs, d_ents, d_roffs, op_capacity=op_cap, in_entries=ents.size, d_out=fenced[3:3 + nreads],
                  d_out_op_offsets=f_ooffs[2:3 + nreads], d_out_ops=f_ops[4:4 + op_cap] if op_cap else f_ops[4:5])
    torch.cuda.synchronize()
    assert (fenced[:3] == FENCE).all().item() and (fenced[3 + nreads:] == FENCE).all().item()
    got_offs = f_ooffs.cpu().numpy()
    assert (got_offs[:2] == FENCE).all() and (got_offs[3 + nreads:] == FENCE).all()
    got_offs = got_offs[2:3 + nreads].copy().view(np.uint64)
    written = int(got_offs[1:][got_offs[1:] <= op_cap].max(initial=0))
    ops = f_ops.cpu().numpy()
    assert (ops[:4] == FENCE).all() and (ops[4 + written:] == FENCE).all()  # nothing past the reads that fit, or the capacity
    return fenced[3:3 + nreads].cpu().numpy().view(MAPPING_DTYPE).reshape(-1), got_offs, ops[4:4 + written].copy().view(np.uint32)


def _check(ix, args, lengths, strands, error=0):
    ix.set_sequences(lengths, strands)
    P = piece_starts(lengths, strands)
    count = {}
    want, w_offs, w_ents = map_reference(*args, P, strands, count=count)
    got, offs, ents = _run(ix, args)
    assert np.array_equal(offs, w_offs), np.flatnonzero(offs != w_offs)[:5]
    bad = np.flatnonzero(ents != w_ents)
    assert bad.size == 0, (bad[:5], ents[bad[:5]], w_ents[bad[:5]])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    assert count["error"] == error
    if error:
        with pytest.raises(capi.SpxError, match="spx error -5: a read's extended alignment failed the mapping's checks"):
            ix.map_stats()
    else:
        st = ix.map_stats()
        assert (st["reads"], st["mapped"], st["cut_reads"], st["reverse_reads"], st["entries_in"], st["entries_out"], st["cut_chars"]) == \
            (args[0].size, count["mapped"], count["cut"], count["reverse"], count["entries_in"], count["entries_out"], count["cut_chars"]), \
            (st, count)
        assert st["error"] == 0 and st["overflow"] == 0 and len(st["step_ms"]) == 2, st
    return want, w_offs, w_ents, count


HAND = [("6=", 4), ("7=", 4), ("7=", 9), ("2S8=1S", 10), ("3=4D4=", 5), ("4=4D3=", 4), ("3=2I4N4=", 5), ("4=4N1X3=", 4),
        ("2=2D1=1N2=1X1=", 0), ("4=2I3=", 6), ("2=2I3=", 8), ("3=4D3=", 5), ("6=", 7), ("1X3=1X2=1X", 10), ("2=3=1X1X4=", 0)]


def test_the_hand_cases(gpu):
    """tests/test_map_cpu.py's hand cases: the borders, 'D', 'N' and 'I' at them, three pieces, the tie, the split clips."""
    two, three, four = _index_of(18), _index_of(14), _index_of(28)
    args = batch([alignment(c, s) for c, s in HAND] + [None])
    want, offs, ents, count = _check(two, args, [10, 8], 1)
    texts = [cigar_text(ents[int(offs[q]):int(offs[q + 1])]) for q in range(len(HAND))]
    assert texts[:4] == ["6=", "6=1S", "1S6=", "2S8=1S"] and texts[9:13] == ["4=5S", "4S3=", "3=3S", "3=3S"]
    assert want["cut"].tolist()[:4] == [0, CUT_RIGHT, CUT_LEFT, 0] and count["cut"] >= 10
    lead = [(MAX_LENGTH - 2) << 4 | OP_S]
    split = batch([alignment(lead + entries_of("5=8="), 5), alignment(entries_of("8=5=") + [MAX_LENGTH << 4 | OP_S, 7 << 4 | OP_S], 2)])
    _, offs, ents, _ = _check(two, split, [10, 8], 1)
    assert cigar_text(ents) == f"{MAX_LENGTH}S3S8=8={MAX_LENGTH}S12S"
    _, _, ents, _ = _check(four, batch([alignment(lead + entries_of("5=8="), 5)]), [10, 4], 2)
    assert cigar_text(ents) == f"8=3S{MAX_LENGTH}S"
    want, _, ents, _ = _check(three, batch([alignment("9=", 3), alignment("1S8=", 2)]), [5, 3, 6], 1)
    assert cigar_text(ents) == "5S4=1S3=5S" and want["seq"].tolist() == [2, 0]
    rev = _index_of(36)
    want, offs, ents, _ = _check(rev, batch([alignment(c, s) for c, s in (("1S2=1X1=2S", 12), ("8=", 6), ("9=", 6), ("3=1I5=", 17), ("5=1I3=", 23),
                                                                       ("3=1D5=", 25))]), [10, 8], 2)
    assert [cigar_text(ents[int(offs[q]):int(offs[q + 1])]) for q in range(6)] == ["2S1=1X2=1S", "4=4S", "5=4S", "4S5=", "5=4S", "5=3S"]
    assert want["strand"].tolist() == [1, 0, 1, 0, 0, 1]
    for index in (two, three, four, rev):
        index.close()


@pytest.mark.parametrize("n_seqs,strands", [(1, 1), (1, 2), (2, 2), (3, 1), (64, 2), (65, 1), (65, 2), (5000, 1), (5000, 2)])
def test_tables_of_one_to_many_sequences(gpu, ix, n_seqs, strands):
    """The binary search over one piece, a few, just over a wavefront's worth and 10 000; at 5 000 x 2 every piece has
    length 1 and every text-consuming column stands in a piece of its own."""
    rng = np.random.default_rng(n_seqs * 2 + strands)
    lengths = table(rng, n_seqs, strands)
    if n_seqs * strands == N:
        assert (lengths == 1).all()
    alignments = [random_alignment(rng, N, max_runs=10, max_len=1 + 2000 // n_seqs) if rng.random() < 0.95 else None for _ in range(400)]
    # alignments that begin at a piece's first and end at its last character, and at the text's two ends
    P = piece_starts(lengths, strands)
    for p in (0, (len(P) - 1) // 2, len(P) - 2):
        alignments.append(alignment(f"{P[p + 1] - P[p]}=", P[p]))
    alignments += [alignment("1=", 0), alignment("1=", N - 1), alignment(f"3S{min(N, MAX_LENGTH)}=", 0)]
    want, offs, ents, count = _check(ix, batch(alignments), lengths, strands)
    check_invariants(want, offs, ents, batch(alignments)[0], batch(alignments)[3], P, strands)
    assert count["mapped"] > 350 and (count["cut"] > 50 or n_seqs == 1 and strands == 1)
    assert (count["reverse"] > 20) == (strands == 2)


def with_entries(rng, k, n_text):
    """An alignment of exactly k entries (k >= 1) of one to three columns each."""
    while True:
        ops = rng.choice((OP_EQ, OP_EQ, OP_EQ, OP_X, OP_I, OP_D, OP_N), k)
        ents = [int(rng.integers(1, 4)) << 4 | int(op) for op in ops]
        text = sum(e >> 4 for e in ents if e & 15 in TEXT_OPS)
        if OP_EQ in ops and text <= n_text:
            return alignment(ents, int(rng.integers(0, n_text - text + 1)))


@pytest.mark.parametrize("strands", [1, 2])
def test_reads_of_0_to_1300_entries(gpu, ix, strands):
    rng = np.random.default_rng(20 + strands)
    alignments = []
    for k in (0, 1, 2, 16, 17, 64, 65, 1300) * 3:
        alignments.append(with_entries(rng, k, N) if k else None)
        if k >= 3:  # the same with both clips among the k entries
            a = with_entries(rng, k - 2, N)
            alignments.append(alignment([5 << 4 | OP_S] + a[1] + [1 << 4 | OP_S], int(a[0]["ref_start"])))
    args = batch(alignments)
    assert sorted(set(np.diff(args[1].astype(np.int64)).tolist())) == [0, 1, 2, 16, 17, 64, 65, 1300]
    for n_seqs in (7, 300):
        want, offs, ents, count = _check(ix, args, table(rng, n_seqs, strands), strands)
        assert count["cut"] >= 10 or n_seqs == 7
    _check(ix, args, table(rng, N // strands, strands), strands)


@pytest.mark.parametrize("nreads", [0, 1, 63, 64, 65, 3000])
def test_read_counts_around_the_wavefront(gpu, ix, nreads):
    rng = np.random.default_rng(nreads)
    lengths = table(rng, 40, 2)
    alignments = [random_alignment(rng, N, max_runs=6, max_len=80) if rng.random() < 0.9 else None for _ in range(nreads)]
    want, offs, ents, count = _check(ix, batch(alignments), lengths, 2)
    assert count["mapped"] >= nreads * 3 // 4 and offs.size == nreads + 1


def test_clips_beyond_the_longest_entry_by_offsets_alone(gpu, ix):
    """A read of nearly 2^32 characters exists in the offsets only: the kernels read no read bytes."""
    full = MAX_LENGTH << 4 | OP_S
    alignments = [alignment([full] * 15 + entries_of("40=60="), 960),                   # the cut takes the 16th entry's worth in
                  alignment(entries_of("60=40=") + [full] * 15 + [100 << 4 | OP_S], 940),
                  alignment([full, 5 << 4 | OP_S] + entries_of("10=") + [full, full], 3000),
                  alignment([(MAX_LENGTH - 39) << 4 | OP_S] + entries_of("40=60="), 960),   # exactly MAX_LENGTH + 1 after the cut
                  alignment([(MAX_LENGTH - 40) << 4 | OP_S] + entries_of("40=60="), 960)]   # exactly MAX_LENGTH
    args = batch(alignments)
    assert int(args[3][-1]) > 2**33
    for strands in (1, 2):
        lengths = np.array([1000] * (N // 1000 // strands), dtype=np.uint64)
        want, offs, ents, _ = _check(ix, args, lengths, strands)
        assert np.diff(offs.astype(np.int64)).tolist() == [17, 17, 5, 3, 2]
        assert int(want["read_start"][0]) == 15 * MAX_LENGTH + 40 and want["cut"].tolist() == [CUT_LEFT, CUT_RIGHT, 0, CUT_LEFT, CUT_LEFT]
    # a read of 2^32 characters or more has no place in the record's 32-bit spans: refused like a bad record
    rec, ents, _ = alignment("40=", 100)
    long = (rec, [full] * 16 + ents + [15 << 4 | OP_S], 16 * MAX_LENGTH + 40 + 15)
    assert long[2] == 2**32 + 39
    args = batch([long, alignment("5=", 0)])
    want, _, _, _ = _check(ix, args, lengths, 2, error=1)
    assert want["seq"].tolist() == [UNMAPPED, 0]


def _spoil(kind):
    """[good, spoiled, good] with the middle read's record, entries or length made wrong; the reference refuses it too."""
    alignments = [alignment("2S30=1X20=3S", 100), alignment("4S25=2I1X30=2D10=6S", 2000), alignment("60=", 5000)]
    rec, ents, length = alignments[1]
    change = {"read_end_beyond_the_read": lambda: rec.__setitem__("read_end", length + 1),
              "read_start_behind_read_end": lambda: rec.__setitem__("read_start", int(rec["read_end"]) + 1),
              "ref_end_beyond_the_text": lambda: rec.__setitem__("ref_end", N + 1),
              "ref_start_behind_ref_end": lambda: rec.__setitem__("ref_start", int(rec["ref_end"]) + 1),
              "read_start_is_not_the_clip": lambda: rec.__setitem__("read_start", 3),
              "read_sum_is_not_the_span": lambda: rec.__setitem__("read_end", int(rec["read_end"]) - 1),
              "text_sum_is_not_the_span": lambda: rec.__setitem__("ref_end", int(rec["ref_end"]) + 1),
              "text_sum_is_below_the_span": lambda: ents.__setitem__(6, 9 << 4 | OP_EQ),
              "right_clip_is_not_the_rest": lambda: ents.__setitem__(7, 7 << 4 | OP_S),
              "an_operation_of_code_0": lambda: ents.__setitem__(3, 1 << 4 | 0),
              "an_operation_of_code_5": lambda: ents.__setitem__(3, 1 << 4 | 5),
              "an_operation_of_code_15": lambda: ents.__setitem__(1, 25 << 4 | 15),
              "a_clip_between_two_operations": lambda: ents.__setitem__(3, 1 << 4 | OP_S),
              "no_equal_column": lambda: [ents.__setitem__(k, ents[k] >> 4 << 4 | OP_X) for k in (1, 4, 6)],
              "an_equal_run_of_length_0_alone": lambda: [ents.__setitem__(k, v) for k, v in ((1, 26 << 4 | OP_X), (4, 30 << 4 | OP_X),
                                                                                         (6, 10 << 4 | OP_X), (3, 0 << 4 | OP_EQ))]}
    change[kind]()
    alignments[1] = (rec, ents, length)
    return alignments


@pytest.mark.parametrize("kind", ["read_end_beyond_the_read", "read_start_behind_read_end", "ref_end_beyond_the_text", "ref_start_behind_ref_end",
                                  "read_start_is_not_the_clip", "read_sum_is_not_the_span", "text_sum_is_not_the_span",
                                  "text_sum_is_below_the_span", "right_clip_is_not_the_rest", "an_operation_of_code_0", "an_operation_of_code_5",
                                  "an_operation_of_code_15", "a_clip_between_two_operations", "no_equal_column",
                                  "an_equal_run_of_length_0_alone"])
def test_bad_inputs_are_refused(gpu, ix, kind):
    """The spoiled read comes back unmapped without entries, the error is reported, the others are as the reference has them
    and the fences (_run's, on both sides of every output) stand."""
    args = batch(_spoil(kind))
    lengths = table(np.random.default_rng(3), 30, 2)
    want, offs, ents, count = _check(ix, args, lengths, 2, error=1)
    assert want[1].tolist() == UNMAPPED_REC and want["seq"][0] != UNMAPPED and want["seq"][2] != UNMAPPED
    assert int(offs[1]) == int(offs[2]) and count["mapped"] == 2


def test_input_offsets_outside_the_entries_are_refused(gpu, ix):
    """Offsets that decrease, or end beyond in_entries: no entry outside the buffer is read, the read is unmapped."""
    ix.set_sequences(table(np.random.default_rng(4), 30, 2), 2)
    good = batch(_spoil_free())
    for q, value in ((2, 10**9), (1, 0)):
        recs, ooffs, ents, roffs = (a.copy() for a in good)
        ooffs[q] = value
        got, offs, out = _run(ix, (recs, ooffs, ents, roffs))
        with pytest.raises(capi.SpxError, match="spx error -5"):
            ix.map_stats()
        assert (got["seq"] == UNMAPPED).sum() >= 1 and got["seq"][0 if q == 2 else 2] != UNMAPPED


def _spoil_free():
    return [alignment("2S30=1X20=3S", 100), alignment("4S25=2I1X30=2D10=6S", 2000), alignment("60=", 5000)]


def test_op_capacity_zero_short_exact_and_above(gpu, ix):
    rng = np.random.default_rng(6)
    lengths = table(rng, 50, 2)
    ix.set_sequences(lengths, 2)
    args = batch([random_alignment(rng, N, max_runs=6, max_len=60) for _ in range(5)])
    want, w_offs, w_ents = map_reference(*args, piece_starts(lengths, 2), 2)
    total = int(w_offs[-1])
    assert (np.diff(w_offs.astype(np.int64)) >= 1).all() and total > 8
    for op_cap in (0, total - 1, int(w_offs[2]) + 1, int(w_offs[1]), total, total + 9):
        got, offs, ents = _run(ix, args, op_cap=op_cap)
        assert np.array_equal(offs, w_offs), op_cap  # the count of a read that does not fit stays in the offsets
        fits = w_offs[1:] <= op_cap
        assert np.array_equal(got[fits], want[fits]) and all(r.tolist() == UNMAPPED_REC for r in got[~fits]), op_cap
        whole = int(w_offs[1:][fits].max(initial=0))
        assert ents.size == whole and np.array_equal(ents, w_ents[:whole]), op_cap
        st = ix.map_stats()
        assert st["overflow"] == int(not fits.all()) and st["error"] == 0 and st["mapped"] == int(fits.sum()), (op_cap, st)
        assert st["entries_out"] == whole, (op_cap, st)
    with pytest.raises(capi.SpxError, match="op_capacity must be at most"):
        _run(ix, args, op_cap=2**32)


def test_repeated_calls_a_batch_in_two_calls_and_a_clone(gpu, ix):
    rng = np.random.default_rng(7)
    lengths = table(rng, 90, 2)
    ix.set_sequences(lengths, 2)
    alignments = [random_alignment(rng, N, max_runs=8, max_len=50) if rng.random() < 0.9 else None for _ in range(300)]
    args = batch(alignments)
    a = _run(ix, args)
    b = _run(ix, args)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a, b))
    other = ix.clone(0)  # (a clone has its own copy of the table)
    ix.set_sequences(table(rng, 3, 2), 2)  # ... and keeps it when the first handle takes another
    c = _run(other, args)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a, c))
    d = _run(ix, args)
    assert d[0].tobytes() != a[0].tobytes()
    ix.set_sequences(lengths, 2)
    first, second = _run(ix, batch(alignments[:150])), _run(other, batch(alignments[150:]))
    assert np.array_equal(np.concatenate([first[0], second[0]]), a[0]) and np.array_equal(np.concatenate([first[2], second[2]]), a[2])
    want = map_reference(*args, piece_starts(lengths, 2), 2)
    assert all(np.array_equal(p, q) for p, q in zip(a, want))
    assert other.map_stats()["reads"] == 150 and ix.map_stats()["entries_out"] == first[2].size
    other.close()


def test_calls_without_a_table_and_the_tables_refusals(gpu):
    bare = _index_of(100)
    args = batch([alignment("5=", 3)])
    seqs, one = np.frombuffer(b"ACGT", dtype=np.uint8), [0, 4]
    with pytest.raises(capi.SpxError, match="spx error -1: spn_map_device needs the sequence table: the index has none"):
        _run(bare, args)
    with pytest.raises(capi.SpxError, match="spx error -1: spn_map_begin needs the sequence table: the index has none"):
        bare.map_host(seqs, one, 1)
    with pytest.raises(capi.SpxError, match="no mappings have been computed"):
        bare.map_stats()
    with pytest.raises(capi.SpxError, match="spn_map_fetch without a successful spn_map_begin"):
        capi._check(capi._spn().spn_map_fetch(bare._h, None, None))
    for lengths, strands, message in (([50], 0, "strands must be 1 or 2"), ([50], 3, "strands must be 1 or 2"),
                                      ([50, 0, 50], 1, "sequence 1 of the table has length 0"),
                                      ([50, 49], 1, "the sequences add up to 99 characters, the text has 100"),
                                      ([50, 50], 2, "the sequences add up to more than the text's 100 characters"),
                                      ([2**63, 2**63], 1, "the sequences add up to more than the text's")):
        with pytest.raises(capi.SpxError, match="spx error -1: " + message):
            bare.set_sequences(np.array(lengths, dtype=np.uint64), strands)
    with pytest.raises(capi.SpxError, match="spx error -1: spn_map_device needs the sequence table"):  # (a refused table leaves none)
        _run(bare, args)
    bare.set_sequences([25, 25], 2)
    got, offs, ents = _run(bare, args)
    assert got[0].tolist() == (3, 8, 0, 0, 0, 5, 5, 0, 5, 0) and cigar_text(ents) == "5="
    S = capi._spn()
    t = [torch.zeros(64, dtype=torch.int64, device="cuda") for _ in range(7)]
    ptr = [x.data_ptr() for x in t]
    call = lambda **kw: S.spn_map_device(kw.get("ix", bare._h), kw.get("rec", ptr[0]), kw.get("oo", ptr[1]), kw.get("ops", ptr[2]), 4,
                                         kw.get("ro", ptr[3]), 1, 4, kw.get("out", ptr[4]), kw.get("ooo", ptr[5]), kw.get("oops", ptr[6]), None)
    for kw in (dict(rec=None), dict(oo=None), dict(ops=None), dict(ro=None), dict(out=None), dict(ooo=None), dict(oops=None)):
        assert call(**kw) == -1, kw
        assert b"must be non-null" in capi.lib().spx_last_error()
    for kw in (dict(rec=ptr[0] + 8), dict(out=ptr[4] + 8), dict(oo=ptr[1] + 4), dict(ro=ptr[3] + 4), dict(ooo=ptr[5] + 4), dict(ops=ptr[2] + 2),
               dict(oops=ptr[6] + 2)):
        assert call(**kw) == -1, kw
        assert b"16-byte aligned" in capi.lib().spx_last_error()
    bare.close()
    no_text = capi.Index.from_raw(synth.statistical_rlbwt(2000, 20, 3.0, seed=1, with_samples=True, n_docs=4), 0)
    with pytest.raises(capi.SpxError, match="the sequence table needs the text"):
        no_text.set_sequences([10], 1)
    no_text.close()


# ---- map_host against the oracle -> mems_reference -> chain_reference -> extend_reference -> map_reference ----------------
def _host_reference(orc, text, seqs, offs, min_length, ep, P, strands, count=None):
    ms = orc.ms(seqs, offs, want_docs=True, text=text)
    m = mems_reference(ms["lengths"], ms["pointers"], offs, min_length, ms["docs"])
    chains, _, pred = chain_reference(m[0], m[1], None, m[2])
    ext = extend_reference(seqs, offs, text, m[0], m[1], chains, pred, None, ep)
    return ext, map_reference(ext[0], ext[1], ext[2], offs, P, strands, count=count)


@pytest.mark.parametrize("strands", [1, 2])
def test_map_host_on_an_index_from_the_oracles_side(gpu, oracle_mod, strands):
    """The kernels do not read the text: any table that fills it cuts the same alignments, whatever the pieces hold."""
    rng = np.random.default_rng(80 + strands)
    text = cases.repetitive_text(rng, 40_000, DNA)
    cuts = [text.size // 5, text.size // 2, text.size - text.size // 5 - text.size // 2]
    raw = synth.index_from_text(torch.from_numpy(text), doc_lengths=cuts)
    orc = oracle_mod.OracleIndex.from_raw(raw)
    ix = capi.Index.from_raw(raw, 0)
    ix.set_text(torch.from_numpy(text.copy()))
    seqs, offs = cases.reads_mixed(rng, text, DNA, 300, 500, [ord("N")])
    offs = offs.astype(np.uint64)
    cut = 0
    for n_seqs, min_length, ep in ((1, 6, None), (150, 6, None), (150, 12, ExtendParams(40, 3, 1, 2)), (150, 10**6, None)):
        lengths = table(rng, n_seqs, strands, text.size)
        P = piece_starts(lengths, strands)
        ix.set_sequences(lengths, strands)
        count = {}
        ext, (want, w_offs, w_ents) = _host_reference(orc, text, seqs, offs, min_length, ep, P, strands, count)
        got, g_offs, g_ents, recs = ix.map_host(seqs, offs, min_length, extend_params=ep, want_docs=True)
        st = ix.map_stats()
        bad = np.flatnonzero(got != want)
        assert got.dtype == MAPPING_DTYPE and bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
        assert g_offs.dtype == np.uint64 and np.array_equal(g_offs, w_offs) and g_ents.dtype == np.uint32 and np.array_equal(g_ents, w_ents)
        assert (st["reads"], st["mapped"], st["cut_reads"], st["reverse_reads"], st["entries_in"], st["entries_out"], st["cut_chars"],
                st["error"], st["overflow"]) == (offs.size - 1, count["mapped"], count["cut"], count["reverse"], count["entries_in"],
                                                 count["entries_out"], count["cut_chars"], 0, 0), (st, count)
        check_invariants(want, w_offs, w_ents, ext[0], offs, P, strands)
        # its middle is extend_host's on the same reads
        e_got, e_offs, e_ents, _, _, _ = ix.extend_host(seqs, offs, min_length, extend_params=ep, want_docs=True)
        assert np.array_equal(recs, e_got) and np.array_equal(recs, ext[0]) and np.array_equal(e_ents, ext[2])
        assert ix.extend_stats()["entries"] == ext[2].size == count["entries_in"]
        if n_seqs == 1 and strands == 1:
            assert count["cut"] == 0 and np.array_equal(g_ents, ext[2])  # one piece: nothing to cut, the entries are extend's
        if min_length == 10**6:
            assert (want["seq"] == UNMAPPED).all() and g_ents.size == 0 and not g_offs.any()
        cut += count["cut"]
    assert cut > 10
    got = ix.map_host(np.zeros(0, dtype=np.uint8), [0], 4)
    assert got[0].size == 0 and got[1].tolist() == [0] and got[2].size == 0 and got[3].size == 0 and ix.map_stats()["reads"] == 0
    ix.close()


def test_the_eight_products_interleaved_on_one_handle(gpu):
    rng = np.random.default_rng(90)
    genome = cases.repetitive_text(rng, 40_000, DNA)
    raw = capi.build_raw(genome, doc_lengths=[genome.size // 3, genome.size - genome.size // 3])
    seqs, offs = cases.reads_mixed(rng, genome, DNA, 300, 500, [ord("N")])
    A = (seqs, offs.astype(np.uint64))
    B = (seqs[:int(offs[120])].copy(), offs[:121].astype(np.uint64))
    lengths = table(rng, 120, 2, genome.size)

    steps = [("map A", lambda ix: (list(ix.map_host(*A, 6)), ix.map_stats())),
             ("extend A", lambda ix: (list(ix.extend_host(*A, 6)), ix.extend_stats())),
             ("map B docs", lambda ix: (list(ix.map_host(*B, 6, want_docs=True)), ix.map_stats())),
             ("cigar A", lambda ix: (list(ix.cigar_host(*A, 6)), ix.cigar_stats())),
             ("map A", lambda ix: (list(ix.map_host(*A, 6)), ix.map_stats())),
             ("align B", lambda ix: (list(ix.align_host(*B, 6)), ix.align_stats())),
             ("chain A", lambda ix: (list(ix.chain_host(*A, 6)), ix.chain_stats())),
             ("mems B", lambda ix: (list(ix.mems_host(*B, 6)), ix.mems_stats())),
             ("map A narrow", lambda ix: (list(ix.map_host(*A, 6, extend_params=ExtendParams(20, 2, 1, 1))), ix.map_stats())),
             ("place A", lambda ix: (list(ix.place_host(*A, 6)), ix.place_stats())),
             ("assign B", lambda ix: (list(ix.assign_host(capi.SPX_MODE_MS, *B, 6)), ix.votes_stats())),
             ("extend A", lambda ix: (list(ix.extend_host(*A, 6)), ix.extend_stats())),
             ("map A", lambda ix: (list(ix.map_host(*A, 6)), ix.map_stats()))]
    ix = capi.Index.from_raw(raw, 0)
    ix.set_sequences(lengths, 2)
    seen = {}
    for name, step in steps:
        got, got_stats = step(ix)
        fresh = capi.Index.from_raw(raw, 0)
        fresh.set_sequences(lengths, 2)
        want, want_stats = step(fresh)
        fresh.close()
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (name, i)
        for s in (got_stats, want_stats):
            for key in ("kernel_ms", "step_ms", "wave_fill_ticks", "wave_back_ticks"):
                s.pop(key, None)
        assert got_stats == want_stats, (name, got_stats, want_stats)
        if name in seen:
            assert all(g.tobytes() == w.tobytes() for g, w in zip(got, seen[name])), name
        seen[name] = got
    # the entries of a map call wait for ITS fetch alone, and it has used up extend's
    ix.map_host(*A, 6)
    with pytest.raises(capi.SpxError, match="spe_extend_fetch without a successful spe_extend_begin"):
        capi._check(capi._spe().spe_extend_fetch(ix._h, None, None))
    with pytest.raises(capi.SpxError, match="spn_map_fetch without a successful spn_map_begin"):
        capi._check(capi._spn().spn_map_fetch(ix._h, None, None))
    ix.close()


# ---- the commands: ground truth that does not rest on the rule -----------------------------------------------------------
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return bytes(s).translate(COMP)[::-1]


def _wrap(s, width):
    return b"".join(s[i:i + width] + b"\n" for i in range(0, len(s), width))


@pytest.fixture(scope="module", params=[True, False], ids=["both_strands", "forward_only"])
def planted(request, gpu, tmp_path_factory):
    """An index `spumoni build -n -M -s` makes of two files with three random sequences, once with the reverse complement
    and once with -c."""
    rc = request.param
    d = tmp_path_factory.mktemp("planted")
    rng = np.random.default_rng(7 + rc)
    seqs = [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(n))].tobytes() for n in rng.integers(300, 501, 3)]
    names = [b"one", b"two", b"three"]
    (d / "a.fa").write_bytes(b">one the first sequence\n" + _wrap(seqs[0], 70) + b">two\n" + _wrap(seqs[1], 61))
    (d / "b.fa").write_bytes(b">three\tof the second file\n" + _wrap(seqs[2], 500))
    (d / "list.txt").write_text(f"{d / 'a.fa'}\n{d / 'b.fa'}\n")
    r = _cli(["build", "-i", str(d / "list.txt"), "-o", str(d / "ref"), "-n", "-M", "-s"] + ([] if rc else ["-c"]), dict(os.environ))
    assert r.returncode == 0, r.stderr.decode()
    tnames, lengths, strands = read_seq_table(str(d / "ref.fa.seqs"), n_text=os.path.getsize(d / "ref.fa.rawtext"))
    assert (tnames, lengths, strands) == (names, [len(s) for s in seqs], 2 if rc else 1)
    return dict(dir=d, seqs=dict(zip(names, seqs)), names=names, rc=rc, text=(d / "ref.fa.rawtext").read_bytes(),
                P=piece_starts(lengths, strands), strands=strands)


def _map_cli(planted, reads, name, extra=(), env=None):
    d = planted["dir"]
    path = d / name
    path.write_bytes(b"".join(b">r%d\n%s\n" % (q, r) for q, r in enumerate(reads)))
    if os.path.exists(str(path) + ".paf"):
        os.remove(str(path) + ".paf")
    r = _cli(["map", "-r", str(d / "ref"), "-p", str(path), "-n", "-L", "12"] + list(extra),
             dict(os.environ, SPUMONI_TEXT=str(d / "ref.fa.rawtext"), **(env or {})))
    assert r.returncode == 0, r.stderr.decode()
    rows = {}
    with open(str(path) + ".paf", "rb") as f:
        for line in f:
            fields = line.rstrip(b"\n").split(b"\t")
            assert len(fields) >= 16 and fields[11] == b"255"
            tags = dict((t[:2], t[5:]) for t in fields[12:])
            assert [t[:5] for t in fields[12:]] == [b"NM:i:", b"an:i:", b"ct:i:", b"cg:Z:"]
            rows[int(fields[0][1:])] = (fields, tags)
    return rows, r.stderr.decode()


def replay_paf(fields, tags, read, seqs):
    """One PAF line against the FASTA the test wrote: '=' columns equal, 'X' columns unequal, the columns add up, NM is
    right.  Returns (read characters clipped, cigar)."""
    length, rs, re_ = int(fields[1]), int(fields[2]), int(fields[3])
    target = seqs[fields[5]]
    Lp, ts, te = int(fields[6]), int(fields[7]), int(fields[8])
    assert length == len(read) and Lp == len(target) and 0 <= rs < re_ <= length and 0 <= ts < te <= Lp
    q = read[rs:re_] if fields[4] == b"+" else revcomp(read[rs:re_])
    x, y, nm, matches, block = 0, ts, 0, 0, 0
    import re as _re
    ops = _re.findall(rb"(\d+)([=XIDN])", tags[b"cg"])
    assert b"".join(n + c for n, c in ops) == tags[b"cg"] and ops[0][1] == b"=" and ops[-1][1] == b"="
    for n, c in ops:
        n = int(n)
        if c in b"=X":
            a, b = np.frombuffer(q[x:x + n], dtype=np.uint8), np.frombuffer(target[y:y + n], dtype=np.uint8)
            assert a.size == n and b.size == n and ((a == b) if c == b"=" else (a != b)).all(), (fields, c, x, y)
            x, y = x + n, y + n
            matches += n if c == b"=" else 0
        elif c == b"I":
            x += n
        else:
            y += n
        nm += n if c in b"XID" else 0
        block += n if c != b"N" else 0
    assert x == len(q) and y == te and nm == int(tags[b"NM"]) and matches == int(fields[9]) and block == int(fields[10])
    return length - (re_ - rs), tags[b"cg"]


def test_planted_exact_reads_are_named_by_sequence_strand_and_position(planted):
    rng = np.random.default_rng(11)
    truth, reads = [], []
    for name in planted["names"]:
        s = planted["seqs"][name]
        for off in [0, len(s) - 60] + [int(v) for v in rng.integers(0, len(s) - 60, 10)]:
            for strand in (b"+", b"-") if planted["rc"] else (b"+",):
                truth.append((name, strand, off))
                reads.append(s[off:off + 60] if strand == b"+" else revcomp(s[off:off + 60]))
    rows, err = _map_cli(planted, reads, "exact.fa")
    assert sorted(rows) == list(range(len(reads)))  # every planted read has a line: none is skipped
    for q, (name, strand, off) in enumerate(truth):
        f, tags = rows[q]
        assert (f[5], f[4], int(f[7]), int(f[8])) == (name, strand, off, off + 60), (q, f)
        assert tags[b"cg"] == b"60=" and (f[1], f[2], f[3], f[9], f[10]) == (b"60", b"0", b"60", b"60", b"60")
        assert (tags[b"NM"], tags[b"ct"], tags[b"an"]) == (b"0", b"0", b"1")
        assert int(f[6]) == len(planted["seqs"][name])
    assert f"{len(reads)} reads, {len(reads)} mapped, 0 without a mapping, 0 cut" in err
    assert f"{sum(t[1] == b'-' for t in truth)} on the reverse strand" in err


def test_reads_with_substitutions_and_an_indel_replay_against_the_fasta(planted):
    rng = np.random.default_rng(12)
    reads, truth = [], []
    other = bytes.maketrans(b"ACGT", b"CGTA")
    for q in range(60):
        name = planted["names"][q % 3]
        s = planted["seqs"][name]
        off = int(rng.integers(0, len(s) - 120))
        r = bytearray(s[off:off + 120])
        for at in (25 + int(rng.integers(0, 5)), 95 + int(rng.integers(0, 5))):
            r[at:at + 1] = bytes(r[at:at + 1]).translate(other)
        at = 58 + int(rng.integers(0, 6))
        if q % 2:
            del r[at]
        else:
            r[at:at] = bytes(r[at:at + 1]).translate(other)
        r = bytes(r)
        strand = b"-" if planted["rc"] and q % 4 >= 2 else b"+"
        reads.append(r if strand == b"+" else revcomp(r))
        truth.append((name, strand, off))
    rows, _ = _map_cli(planted, reads, "noisy.fa")
    assert len(rows) >= 55
    whole = 0
    for q, (f, tags) in rows.items():
        clipped, cigar = replay_paf(f, tags, reads[q], planted["seqs"])
        name, strand, off = truth[q]
        assert (f[5], f[4]) == (name, strand) and off <= int(f[7]) and int(f[8]) <= off + 121
        whole += clipped == 0 and int(tags[b"NM"]) == 3
    assert whole >= 40  # most reads are aligned end to end with exactly the planted edits


def test_reads_across_a_border_are_cut_and_land_on_one_sequence(planted):
    text, P, strands = planted["text"], planted["P"], planted["strands"]
    reads, want = [], []
    for p in range(1, len(P) - 1):
        for left, right in ((30, 30), (40, 20), (20, 40)):
            reads.append(text[P[p] - left:P[p] + right])
            want.append(p - 1 if left >= right else p)  # 30 + 30 is a tie: the lower piece
    rows, err = _map_cli(planted, reads, "border.fa")
    assert sorted(rows) == list(range(len(reads)))
    for q, (f, tags) in rows.items():
        clipped, cigar = replay_paf(f, tags, reads[q], planted["seqs"])
        p = want[q]
        kept = max(60 - clipped, 0)
        assert (f[5], f[4]) == (planted["names"][p // strands], b"-" if p % strands else b"+"), (q, f)
        assert int(tags[b"ct"]) == (2 if p == want[q] and kept and q % 3 != 2 else 1) and cigar == b"%d=" % kept
        assert kept == (30 if q % 3 == 0 else 40)
        Lp = int(f[6])
        # the kept part touches the border: the sequence's end on a piece read towards the border, its start behind it
        at_end = (q % 3 != 2) != (f[4] == b"-")
        assert (int(f[8]) == Lp) if at_end else (int(f[7]) == 0)
    assert f"{len(reads)} mapped, 0 without a mapping, {len(reads)} cut" in err


def test_an_unmapped_read_has_no_line_and_small_super_batches_give_the_same_file(planted):
    rng = np.random.default_rng(13)
    s = planted["seqs"][b"two"]
    reads = [s[o:o + 80] for o in map(int, rng.integers(0, len(s) - 80, 300))] + [b"ACGT" * 5]
    one, err = _map_cli(planted, reads, "many.fa")
    assert "301 reads, 300 mapped, 1 without a mapping" in err and 300 not in one
    whole = (planted["dir"] / "many.fa.paf").read_bytes()
    _map_cli(planted, reads, "many.fa", env=dict(SPUMONI_SUPER_BATCH="1000"))
    assert (planted["dir"] / "many.fa.paf").read_bytes() == whole


def test_a_full_super_batch_cut_into_two_calls_gives_the_same_file(planted):
    """33.75 M characters in one super-batch of 64 Mi are two calls of spn_map_begin, the second with offsets that do not
    start at 0 and entries behind the first call's; in super-batches of 16 Mi they are three calls of one piece each."""
    rng = np.random.default_rng(14)
    text = np.frombuffer(planted["text"], dtype=np.uint8)
    nreads, m = 225_000, 150
    at = rng.integers(0, text.size - m, nreads)
    rs = text[at.astype(np.int32)[:, None] + np.arange(m, dtype=np.int32)[None, :]]
    d = planted["dir"]
    with open(d / "big.fa", "wb") as f:
        for i in range(0, nreads, 25_000):
            f.write(b"".join(b">r%d\n%s\n" % (q, rs[q].tobytes()) for q in range(i, i + 25_000)))
    files = []
    for batch in (64 << 20, 16 << 20):
        r = _cli(["map", "-r", str(d / "ref"), "-p", str(d / "big.fa"), "-n", "-L", "20"],
                 dict(os.environ, SPUMONI_TEXT=str(d / "ref.fa.rawtext"), SPUMONI_SUPER_BATCH=str(batch)))
        assert r.returncode == 0, r.stderr.decode()
        assert f"{nreads} reads, {nreads} mapped".encode() in r.stderr
        files.append((d / "big.fa.paf").read_bytes())
        os.remove(d / "big.fa.paf")
    assert files[0] == files[1] and files[0].count(b"\n") == nreads
    os.remove(d / "big.fa")


def test_map_refuses_a_table_that_does_not_add_up(planted):
    d = planted["dir"]
    good = (d / "ref.fa.seqs").read_bytes()
    (d / "r.fa").write_bytes(b">r\n" + planted["text"][:50] + b"\n")
    try:
        lines = good.split(b"\n")
        (d / "ref.fa.seqs").write_bytes(b"\n".join(lines[:-2]) + b"\n")  # the last sequence is missing
        r = _cli(["map", "-r", str(d / "ref"), "-p", str(d / "r.fa"), "-n", "-L", "12"], dict(os.environ, SPUMONI_TEXT=str(d / "ref.fa.rawtext")))
        assert r.returncode == 1 and b"ref.fa.seqs: the sequences add up to" in r.stderr and not os.path.exists(d / "r.fa.paf"), r.stderr.decode()
        os.remove(d / "ref.fa.seqs")
        r = _cli(["map", "-r", str(d / "ref"), "-p", str(d / "r.fa"), "-n", "-L", "12"], dict(os.environ, SPUMONI_TEXT=str(d / "ref.fa.rawtext")))
        assert r.returncode == 1 and b"has no sequence table" in r.stderr and b"build it with -s" in r.stderr
        assert not os.path.exists(d / "r.fa.paf")
    finally:
        (d / "ref.fa.seqs").write_bytes(good)


# ---- the table of `spumoni build -s` -------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", [True, False])
def test_build_writes_the_table_build_index_writes_and_nothing_else_without_the_option(gpu, tmp_path, rc, capfd):
    import filecmp

    from spumoni_amd import build_index

    rng = np.random.default_rng(15)
    L = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)

    def s(n):
        return L[rng.integers(0, L.size, n)].tobytes()

    (tmp_path / "a.fa").write_bytes(_wrap(s(230), 60) + b">chr1 first\n" + _wrap(s(700), 80) + b">empty\n\n>\n" + _wrap(s(90), 90) +
                                    b">chr1\tagain\r\n" + _wrap(s(333), 50) + b">   \n" + s(40) + b"\n")
    (tmp_path / "b.fa").write_bytes(b">only|one description here\n" + _wrap(s(1000), 70) + b">last")
    (tmp_path / "list.txt").write_text(f"{tmp_path / 'a.fa'}\n{tmp_path / 'b.fa'}\n")
    flags_c, flags_p = ([] if rc else ["-c"]), ([] if rc else ["--no-rev-comp"])
    listings = {}
    for kind, extra_c, extra_p in (("with", ["-s"], ["--seq-table"]), ("without", [], [])):
        for who in ("cli", "py"):
            (tmp_path / kind / who).mkdir(parents=True)
        r = _cli(["build", "-i", str(tmp_path / "list.txt"), "-o", str(tmp_path / kind / "cli" / "x"), "-P", "-M", "-n"] + flags_c + extra_c,
                 dict(os.environ))
        assert r.returncode == 0, r.stderr.decode()
        capfd.readouterr()
        build_index.main(["-l", str(tmp_path / "list.txt"), "-o", str(tmp_path / kind / "py" / "x")] + flags_p + extra_p)
        py_err = capfd.readouterr().err
        listings[kind] = sorted(os.listdir(tmp_path / kind / "cli"))
        assert listings[kind] == sorted(os.listdir(tmp_path / kind / "py"))
        for f in listings[kind]:
            assert filecmp.cmp(tmp_path / kind / "cli" / f, tmp_path / kind / "py" / f, shallow=False), (kind, f)
        if kind == "with":
            assert r.stderr.count(b"more than once in the sequence table") == 1 and py_err.count("more than once in the sequence table") == 1
    assert listings["with"] == sorted(listings["without"] + ["x.fa.seqs"])
    for f in listings["without"]:
        assert filecmp.cmp(tmp_path / "with" / "cli" / f, tmp_path / "without" / "cli" / f, shallow=False), f
    strands = 2 if rc else 1
    table = (tmp_path / "with" / "cli" / "x.fa.seqs").read_bytes().split(b"\n")
    assert [ln.split(b"\t")[0] for ln in table[:-1]] == [b"seq1", b"chr1", b"seq3", b"chr1", b"seq5", b"only|one"]
    assert [int(ln.split(b"\t")[1]) for ln in table[:-1]] == [230, 700, 90, 333, 40, 1000] and table[-1] == b""
    assert all(ln.endswith(b"\t%d" % strands) for ln in table[:-1])
    names = capi.prepare_fasta([(tmp_path / "a.fa").read_bytes(), (tmp_path / "b.fa").read_bytes()], rev_comp=rc)["names"]
    assert names == [b"seq1", b"chr1", b"seq3", b"chr1", b"seq5", b"only|one"]
