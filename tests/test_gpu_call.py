"""The pileup and the calls on the GPU (include/spumoni_call.h): crafted mappings, entries and reads through the device
forms against spumoni_amd/call.py in every word of alt, other, ins, ddiff and del and in every call record, with every buffer
fenced on both sides; the host forms against the oracle's MS arrays -> mems -> chain -> extend -> map -> cover + pileup ->
calls references, alone and interleaved with the nine products before it on one handle; and `spumoni call` against a file
computed from planted reads."""
import os

import numpy as np
import pytest
import torch

from spumoni_amd import capi, synth
from spumoni_amd.call import CALL_DTYPE, calls_reference, check_read, del_of, pileup_reference
from spumoni_amd.cigar import OP_D, OP_EQ, OP_I, OP_N, OP_X
from spumoni_amd.cover import cover_reference, depth_of, seq_starts, summary_reference
from spumoni_amd.extend import OP_S, ExtendParams
from spumoni_amd.map import MAPPING_DTYPE, piece_starts
from tests import cases
from tests.test_call_cpu import ALPHABET, CALL_BAD, GOOD_READS, TEXT_OPS, rbatch, read_length, spoiled_call
from tests.test_cover_cpu import BAD_LENGTHS, mapping
from tests.test_gpu_align import DNA, FENCE, _cli
from tests.test_gpu_cover import _fenced, _unfence
from tests.test_gpu_map import _host_reference, _index_of, gpu, planted, revcomp, table  # noqa: F401 (gpu, planted: fixtures)

pytestmark = pytest.mark.gpu
N = 10_000
TILE, PER_THREAD = 4096, 16  # positions of a calls tile and of one of its threads (spx_call.hip)
TEXT_LETTERS = np.frombuffer(b"ACGTACGTACGTACGTacgtN", dtype=np.uint8)
PARAMS = [(1, 1, 0), (2, 2, 500), (1, 2, 1000), (3, 1, 250)]


def _index_with_text(n_text, seed=0):
    """(index, text): any index with a text of n_text letters, a few of them lower case or N -- the kernels read the table,
    the text and nothing else of the index."""
    text = TEXT_LETTERS[np.random.default_rng(1000 + seed).integers(0, TEXT_LETTERS.size, n_text)]
    index = _index_of(n_text)
    index.set_text(torch.from_numpy(text.copy()), unchecked=True)
    return index, text


@pytest.fixture(scope="module")
def ixt(gpu):
    index, text = _index_with_text(N)
    yield index, text
    index.close()


def _device_inputs(args):
    recs, ooffs, ents, reads, roffs = args
    nreads = recs.size
    d_map = torch.from_numpy(np.concatenate([recs, np.zeros(1, dtype=MAPPING_DTYPE)]).view(np.int32).reshape(-1, 12).copy()).cuda()[:nreads]
    d_ooffs = torch.from_numpy(np.asarray(ooffs, dtype=np.uint64).view(np.int64).copy()).cuda()
    d_ents = torch.from_numpy(np.r_[ents, np.zeros(1, dtype=np.uint32)].view(np.int32).copy()).cuda()[:ents.size]
    d_reads = torch.from_numpy(np.r_[reads, np.zeros(1, dtype=np.uint8)].copy()).cuda()[:reads.size]
    d_roffs = torch.from_numpy(np.asarray(roffs, dtype=np.uint64).view(np.int64).copy()).cuda()
    return d_map, d_ooffs, d_ents, d_reads, d_roffs


def _add(ix, args, G, into=None, in_entries=None, in_chars=None):
    """pileup_add_device with the four arrays fenced on both sides; returns (alt, other, ins, ddiff)."""
    d_map, d_ooffs, d_ents, d_reads, d_roffs = _device_inputs(args)
    zero = (4 * G, G, G, G + 1) if into is None else into
    bufs = [_fenced(z, np.uint32) for z in zero]
    ix.pileup_add_device(d_map, d_ooffs, d_ents, d_reads, d_roffs, *(view for _, view in bufs),
                         in_entries=args[2].size if in_entries is None else in_entries, in_chars=args[3].size if in_chars is None else in_chars)
    torch.cuda.synchronize()
    return tuple(_unfence(whole, n, np.uint32) for (whole, _), n in zip(bufs, (4 * G, G, G, G + 1)))


def _finish(ix, ddiff):
    """pileup_finish_device with del fenced; ddiff must come back unchanged."""
    G = ddiff.size - 1
    (w_ddiff, d_ddiff), (w_del, d_del) = _fenced(ddiff, np.uint32), _fenced(G, np.uint32)
    ix.pileup_finish_device(d_ddiff, d_del=d_del)
    torch.cuda.synchronize()
    assert np.array_equal(_unfence(w_ddiff, G + 1, np.uint32), ddiff)
    return _unfence(w_del, G, np.uint32)


def _calls(ix, depth, mism, alt, other, ins, dele, params, cap):
    """calls_device with the records and the count fenced, the inputs too; returns (the records that fit, the count)."""
    ins_ = [_fenced(a, np.uint32) for a in (depth, mism, alt, other, ins, dele)]
    w_calls = torch.full((cap + 4, 6), FENCE, dtype=torch.int64, device="cuda")
    w_count, d_count = _fenced(1, np.uint64)
    ix.calls_device(*(view for _, view in ins_), *params, call_capacity=cap, d_calls=w_calls[2:2 + max(cap, 1)] if cap else None, d_count=d_count)
    torch.cuda.synchronize()
    for (whole, _), a in zip(ins_, (depth, mism, alt, other, ins, dele)):
        assert np.array_equal(_unfence(whole, a.size, np.uint32), a)
    total = int(_unfence(w_count, 1, np.uint64)[0])
    calls = w_calls.cpu().numpy()
    fit = min(total, cap)
    assert (calls[:2] == FENCE).all() and (calls[2 + fit:] == FENCE).all(), "a record outside the calls that fit"
    return calls[2:2 + fit].copy().view(CALL_DTYPE).reshape(-1), total


def _same(name, got, want):
    bad = np.flatnonzero((got != want).reshape(-1))
    assert got.dtype == want.dtype and got.shape == want.shape and bad.size == 0, (name, bad[:5], got.reshape(-1)[bad[:5]], want.reshape(-1)[bad[:5]])


def _check_calls(ix, text, lengths, strands, depth, mism, alt, other, ins, dele, params_list=PARAMS):
    n = 0
    for params in params_list:
        want = calls_reference(depth, mism, alt, other, ins, dele, text, lengths, strands, *params)
        got, total = _calls(ix, depth, mism, alt, other, ins, dele, params, want.size + 3)
        assert total == want.size == ix.call_stats()["calls"], (params, total, want.size)
        bad = [i for i in range(want.size) if got[i].tobytes() != want[i].tobytes()]
        assert got.size == want.size and not bad, (params, bad[:5], got[bad[:5]], want[bad[:5]])
        n += want.size
    return n


def _check(ixt, args, lengths, strands=1, error=0, in_entries=None, in_chars=None, clean=None, params_list=PARAMS):
    """Everything of one batch against the references: the add, its stats, the finish, and the calls the arrays and the
    batch's own depth give."""
    ix, text = ixt
    ix.set_sequences(lengths, strands)
    G = seq_starts(lengths)[-1]
    count = {}
    want = pileup_reference(*args, lengths, count=count, in_entries=in_entries, in_chars=in_chars)
    if clean is not None:  # the reference that never saw the bad read
        assert all(a.tobytes() == b.tobytes() for a, b in zip(want, pileup_reference(*clean, lengths)))
    got = _add(ix, args, G, in_entries=in_entries, in_chars=in_chars)
    for name, g, w in zip(("alt", "other", "ins", "ddiff"), got, want):
        _same(name, g, w)
    assert count["error"] == error
    if error:
        with pytest.raises(capi.SpxError, match="spx error -5: a read failed the pileup's checks"):
            ix.call_stats()
    else:
        st = ix.call_stats()
        keys = ("mapped", "added", "skipped", "x_columns", "other_columns", "insertions", "deletions", "atomics", "error")
        assert st["reads"] == args[0].size and [st[k] for k in keys] == [count[k] for k in keys], (st, count)
    dele = _finish(ix, want[3])
    _same("del", dele, del_of(want[3]))
    # the depth of the same reads: the coverage's own rule skips what it skips, which is all the calls need
    cov = cover_reference(args[0], args[1], args[2], lengths, in_entries=in_entries)
    n_calls = _check_calls(ix, text, lengths, strands, depth_of(cov[0]), cov[1], want[0], want[1], want[2], dele, params_list)
    return want, dele, count, n_calls


def random_read(rng, lengths, max_runs=8, max_len=9, strand=None):
    """(mapping, read bytes): a few random runs that fit a random sequence and pass the pileup's checks, on a random strand."""
    F = seq_starts(lengths)
    s = int(rng.integers(0, len(lengths)))
    L = int(lengths[s])
    while True:
        k = int(rng.integers(1, max_runs + 1))
        ents = [int(rng.integers(1, max_len + 1)) << 4 | int(op) for op in rng.choice((OP_EQ, OP_EQ, OP_X, OP_X, OP_I, OP_D, OP_N), k)]
        if L < 4:
            ents = [int(rng.integers(1, L + 1)) << 4 | int(rng.choice((OP_EQ, OP_X)))]
        text = sum(e >> 4 for e in ents if e & 15 in TEXT_OPS)
        if text > L:
            continue
        if rng.random() < 0.3:
            ents = [3 << 4 | OP_S] + ents + [2 << 4 | OP_S]
        m = mapping(ents, s, int(rng.integers(0, L - text + 1)), strand=int(rng.integers(0, 2)) if strand is None else strand)
        if check_read(m[0], m[1], read_length(ents), F) is not None:
            return m, ALPHABET[rng.integers(0, ALPHABET.size, read_length(ents))].tobytes()


def batch_of(pairs):
    """rbatch of [(mapping, read) or None]."""
    return rbatch([p[0] if p else None for p in pairs], [p[1] if p else b"ACGTN" for p in pairs])


def with_entries(rng, k, L):
    """(mapping, read) of exactly k entries of zero to three columns each on a sequence of L bases."""
    while True:
        ops = rng.choice((OP_EQ, OP_EQ, OP_X, OP_X, OP_I, OP_D, OP_N), k)
        ents = [int(rng.integers(0 if k > 4 else 1, 4)) << 4 | int(op) for op in ops]
        text = sum(e >> 4 for e in ents if e & 15 in TEXT_OPS)
        m = mapping(ents, 0, int(rng.integers(0, max(L - text, 0) + 1)), strand=int(rng.integers(0, 2)))
        if text <= L and check_read(m[0], m[1], read_length(ents), [0, L]) is not None:
            return m, ALPHABET[rng.integers(0, ALPHABET.size, read_length(ents))].tobytes()


@pytest.mark.parametrize("n_seqs,strands", [(1, 1), (1, 2), (3, 1), (65, 2), (5000, 2)])
def test_tables_of_one_to_many_sequences(gpu, ixt, n_seqs, strands):
    """One sequence, a few, just over a wavefront's worth, and 5 000 of one base each: there every position is a border and
    a tile of the calls spans 4 096 sequences."""
    rng = np.random.default_rng(n_seqs * 2 + strands)
    lengths = table(rng, n_seqs, strands)
    if n_seqs == 5000:
        assert (lengths == 1).all()
    pairs = [random_read(rng, lengths, max_len=1 + 400 // n_seqs) if rng.random() < 0.95 else None for _ in range(900)]
    # 'X' reads on the first and the last base of the genome, and a deletion that ends at G
    pairs += [(mapping("1X", 0, 0), b"c"), (mapping("1X", n_seqs - 1, int(lengths[-1]) - 1, strand=1), b"g")] * 2
    if lengths[-1] >= 3:
        pairs.append((mapping("1=2D", n_seqs - 1, int(lengths[-1]) - 3), b"A"))
    want, dele, count, n_calls = _check(ixt, batch_of(pairs), lengths, strands)
    assert count["added"] > 700 and want[0].any() and n_calls > 0 and (n_seqs > 100 or (want[2].any() and dele.any()))


@pytest.mark.parametrize("lengths", [[TILE - 1, 9], [TILE, 9], [TILE + 1, 9], [1, 2 * TILE - 2, 7]])
def test_sequences_around_the_calls_tile(gpu, lengths):
    """Sequences one below, at and one above the tile, so that borders fall on the last position of a tile, on its first
    and one behind it; 'X' runs and 'D' runs across a thread's border (position 16), across the tile's border and across
    the sequence's end region, several reads deep so that they are calls."""
    ixt = _index_with_text(sum(lengths), seed=sum(lengths))
    rng = np.random.default_rng(4)
    pairs = [random_read(rng, lengths, max_runs=12, max_len=40) for _ in range(400)]
    big = int(np.argmax(lengths))
    L = lengths[big]
    for at in (PER_THREAD - 3, TILE - 5 - seq_starts(lengths)[big], L - 8):
        at = max(0, min(at, L - 8))
        for r in range(3):  # (the same letters three times: alt counts of 3 on every column of the run)
            pairs.append((mapping("1=6X1=", big, at, strand=r % 2), b"AACCGGTA" if r % 2 == 0 else revcomp(b"AACCGGTA")))
            pairs.append((mapping("1=6D1=", big, at), b"AC"))
    for s, n in enumerate(lengths):
        pairs += [(mapping(f"{min(n, 5)}X", s, n - min(n, 5)), b"ACGTN"[:min(n, 5)]), (mapping(f"{n}=", s, 0), b"A" * n)]
    want, dele, count, n_calls = _check(ixt, batch_of(pairs), lengths)
    assert count["added"] == len(pairs) and n_calls > 10 and dele.max() >= 3
    ixt[0].close()


def test_reads_of_0_to_1300_entries_on_both_sides_of_the_switch(gpu, ixt):
    """Long and short reads mixed in one batch: up to 64 entries a lane walks the read, above a wavefront does.  The same
    batch with every read given a wavefront, and with every read given a lane, adds the same bytes."""
    ix, _ = ixt
    rng = np.random.default_rng(21)
    lengths = np.array([N], dtype=np.uint64)
    pairs = []
    for k in (0, 1, 2, 16, 63, 64, 65, 127, 128, 129, 1300) * 3:
        pairs.append(with_entries(rng, k, N))
        if k >= 3:  # the same with both clips among the k entries
            (rec, ents), _ = with_entries(rng, k - 2, N)
            ents = [5 << 4 | OP_S] + ents + [1 << 4 | OP_S]
            pairs.append(((rec, ents), ALPHABET[rng.integers(0, ALPHABET.size, read_length(ents))].tobytes()))
    pairs.append(None)
    args = batch_of(pairs)
    assert sorted(set(np.diff(args[1].astype(np.int64)).tolist())) == [0, 1, 2, 16, 63, 64, 65, 127, 128, 129, 1300]
    want, _, count, _ = _check(ixt, args, lengths)
    assert count["added"] == len(pairs) - 1 and count["insertions"] > 100 and count["deletions"] > 100
    try:
        for switch in (0, 1 << 20):
            ix.set_option("call_switch", switch)
            got = _add(ix, args, N)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), switch
            st = ix.call_stats()
            assert (st["added"], st["x_columns"], st["other_columns"], st["atomics"]) == \
                (count["added"], count["x_columns"], count["other_columns"], count["atomics"]), (switch, st)
    finally:
        ix.set_option("call_switch", 64)


@pytest.mark.parametrize("columns", [1, 16, 17, 64, 65, 200])
def test_one_x_entry_of_1_to_200_columns(gpu, ixt, columns):
    """One 'X' entry by a lane and by a wavefront: up to 16 columns the entry's own lane adds them, above they are dealt to
    the wavefront; both strands, clips in front, and two long entries in one step of 64."""
    ix, _ = ixt
    rng = np.random.default_rng(columns)
    lengths = np.array([3000, 7000], dtype=np.uint64)
    pairs = []
    for strand in (0, 1):
        for cigar in (f"{columns}X", f"3S2={columns}X1=", f"1={columns}X2I1={columns}X3D1="):
            m = mapping(cigar, 1, int(rng.integers(0, 5000)), strand=strand)
            pairs.append((m, ALPHABET[rng.integers(0, ALPHABET.size, read_length(m[1]))].tobytes()))
    args = batch_of(pairs)
    want, _, count, _ = _check(ixt, args, lengths)
    assert count["x_columns"] == 8 * columns and count["added"] == 6
    try:
        ix.set_option("call_switch", 0)
        got = _add(ix, args, N)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
        assert ix.call_stats()["x_columns"] == 8 * columns
    finally:
        ix.set_option("call_switch", 64)


@pytest.mark.parametrize("nreads", [0, 1, 63, 64, 65, 3000])
def test_read_counts_around_the_wavefront(gpu, ixt, nreads):
    rng = np.random.default_rng(nreads)
    lengths = table(rng, 40, 2)
    pairs = [random_read(rng, lengths, max_runs=6, max_len=30) if rng.random() < 0.9 else None for _ in range(nreads)]
    _, _, count, _ = _check(ixt, batch_of(pairs), lengths, 2)
    assert count["mapped"] >= nreads * 3 // 4 and count["reads"] == nreads


def test_all_reads_with_an_x_on_one_base(gpu, ixt):
    """3 000 reads whose 'X' column is one position: four words of alt and one of other take every add."""
    rng = np.random.default_rng(5)
    lengths = table(rng, 16, 1)
    F = seq_starts(lengths)
    letters = b"ACGTn"
    pairs = [(mapping("1X", 9, 2, strand=q % 2), letters[q % 5:q % 5 + 1]) for q in range(3000)]
    want, _, count, n_calls = _check(ixt, batch_of(pairs), lengths)
    g = F[9] + 2
    assert want[0].reshape(-1, 4)[g].sum() == 2400 and want[1][g] == 600 and want[0].sum() == 2400 and count["atomics"] == 3000
    assert sorted(want[0].reshape(-1, 4)[g].tolist()) == [600, 600, 600, 600] and n_calls >= 1
    # ... and 3 000 insertions in front of one base, 3 000 deletions of it
    pairs = [(mapping("1=2I1=", 9, 1), b"ACGT") if q % 2 else (mapping("1=1D1=", 9, 1), b"AC") for q in range(3000)]
    want, dele, _, _ = _check(ixt, batch_of(pairs), lengths)
    assert want[2][g] == 1500 and dele[g] == 1500 and dele.sum() == 1500


def test_both_strands_of_the_same_read_give_the_same_arrays(gpu, ixt):
    ix, _ = ixt
    rng = np.random.default_rng(6)
    lengths = table(rng, 30, 2)
    G = int(lengths.sum())
    pairs = [random_read(rng, lengths, strand=0) for _ in range(300)]
    ix.set_sequences(lengths, 2)
    a = _add(ix, batch_of(pairs), G)
    turned = []
    for (rec, ents), read in pairs:
        rec = rec.copy()
        rec["strand"] = 1
        turned.append(((rec, ents), bytes(read).translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1]))
    b = _add(ix, batch_of(turned), G)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and a[0].any()
    want = pileup_reference(*batch_of(turned), lengths)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(b, want))


def test_every_byte_class(gpu, ixt):
    """All 256 bytes in 'X' columns on both strands: eight of them are letters, the rest go to `other`."""
    lengths = np.array([N], dtype=np.uint64)
    every = bytes(range(256))
    pairs = [(mapping("256X", 0, 100, strand=0), every), (mapping("256X", 0, 100, strand=1), every),
             (mapping("2S9X", 0, 7, strand=1), b"\x00\xffAcGtNn-@\x80")]
    want, _, count, _ = _check(ixt, batch_of(pairs), lengths)
    assert count["other_columns"] == 2 * 248 + 5 and want[0].sum() == 16 + 4


@pytest.mark.parametrize("switch", [64, 0], ids=["lane", "wavefront"])
@pytest.mark.parametrize("kind", CALL_BAD)
def test_bad_inputs_are_skipped_whole_and_reported(gpu, kind, switch):
    """tests/test_call_cpu.py's bad reads one by one, by a lane and by a wavefront: the error is reported and the arrays are
    those of the batch without the read."""
    ixt = _index_with_text(sum(BAD_LENGTHS))
    ixt[0].set_option("call_switch", switch)
    args, clean, in_entries, in_chars = spoiled_call(kind)
    ix, text = ixt
    ix.set_sequences(BAD_LENGTHS, 1)
    count = {}
    want = pileup_reference(*args, BAD_LENGTHS, count=count, in_entries=in_entries, in_chars=in_chars)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(want, pileup_reference(*clean, BAD_LENGTHS))) and count["error"] == 1
    got = _add(ix, args, sum(BAD_LENGTHS), in_entries=in_entries, in_chars=in_chars)
    for name, g, w in zip(("alt", "other", "ins", "ddiff"), got, want):
        _same(name, g, w)
    with pytest.raises(capi.SpxError, match="spx error -5: a read failed the pileup's checks"):
        ix.call_stats()
    _check(ixt, clean, BAD_LENGTHS)  # (and the next call on the handle reports no error)
    ix.close()


def test_call_capacity_from_zero_to_above(gpu, ixt):
    ix, text = ixt
    rng = np.random.default_rng(8)
    lengths = table(rng, 50, 1)
    ix.set_sequences(lengths, 1)
    G = int(lengths.sum())
    depth = rng.integers(0, 7, G).astype(np.uint32)
    alt = (rng.integers(0, 4, 4 * G) * (rng.random(4 * G) < 0.2)).astype(np.uint32)
    other, ins, dele, mism = (rng.integers(0, 3, G).astype(np.uint32) for _ in range(4))
    params = (2, 2, 400)
    want = calls_reference(depth, mism, alt, other, ins, dele, text, lengths, 1, *params)
    assert want.size > 100
    for cap in (0, 1, want.size - 1, want.size, want.size + 1):
        got, total = _calls(ix, depth, mism, alt, other, ins, dele, params, cap)
        st = ix.call_stats()
        assert total == want.size == st["calls"] and got.tobytes() == want[:cap].tobytes(), cap  # the count is kept
        assert st["overflow"] == int(cap < want.size), (cap, st)
    for bad in ((0, 1, 0), (1, 0, 0), (1, 1, 1001)):
        with pytest.raises(capi.SpxError, match="spx error -1: min_depth and min_alt must be at least 1 and min_permille between 0 and 1000"):
            _calls(ix, depth, mism, alt, other, ins, dele, bad, 4)


def test_random_arrays_on_many_tables(gpu, ixt):
    """The calls kernels alone on arrays no add made: dense counts, so that most positions are judged in full."""
    ix, text = ixt
    rng = np.random.default_rng(18)
    for n_seqs, strands in ((1, 1), (7, 2), (300, 1), (5000, 2)):
        lengths = table(rng, n_seqs, strands)
        ix.set_sequences(lengths, strands)
        G = int(lengths.sum())
        depth = rng.integers(0, 9, G).astype(np.uint32)
        alt = rng.integers(0, 5, 4 * G).astype(np.uint32)
        other, ins, dele, mism = (rng.integers(0, 3, G).astype(np.uint32) for _ in range(4))
        assert _check_calls(ix, text, lengths, strands, depth, mism, alt, other, ins, dele) > G // 2


def test_two_adds_equal_one_and_repeated_calls_give_the_same_bytes(gpu, ixt):
    ix, text = ixt
    rng = np.random.default_rng(9)
    lengths = table(rng, 90, 2)
    ix.set_sequences(lengths, 2)
    G = int(lengths.sum())
    pairs = [random_read(rng, lengths, max_len=40) if rng.random() < 0.9 else None for _ in range(500)]
    whole = _add(ix, batch_of(pairs), G)
    again = _add(ix, batch_of(pairs), G)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, again))
    first = _add(ix, batch_of(pairs[:200]), G)
    both = _add(ix, batch_of(pairs[200:]), G, into=first)
    other = _add(ix, batch_of(pairs[:200][::-1]), G, into=_add(ix, batch_of(pairs[200:]), G))
    want = pileup_reference(*batch_of(pairs), lengths)
    for a, b, c, w in zip(whole, both, other, want):
        assert a.tobytes() == b.tobytes() == c.tobytes() == w.tobytes()
    assert ix.call_stats()["reads"] == 200  # of the last add_device call
    d1, d2 = _finish(ix, whole[3]), _finish(ix, whole[3])
    assert d1.tobytes() == d2.tobytes()
    depth = depth_of(cover_reference(*batch_of(pairs)[:3], lengths)[0])
    c1 = _calls(ix, depth, whole[1], whole[0], whole[1], whole[2], d1, (1, 1, 0), G)
    c2 = _calls(ix, depth, whole[1], whole[0], whole[1], whole[2], d1, (1, 1, 0), G)
    assert c1[1] == c2[1] > 0 and c1[0].tobytes() == c2[0].tobytes()


# ---- the host forms ----------------------------------------------------------------------------------------------------------
def _call_host_reference(orc, text, seqs, offs, min_length, ep, lengths, strands, into=(None, None), count=None):
    _, (maps, m_offs, m_ents) = _host_reference(orc, text, seqs, offs, min_length, ep, piece_starts(lengths, strands), strands)
    return maps, (cover_reference(maps, m_offs, m_ents, lengths, into=into[0]),
                  pileup_reference(maps, m_offs, m_ents, seqs, offs, lengths, into=into[1], count=count))


def _host_state(ix, lengths):
    """Everything the handle's arrays give: depth, mism, the summary, alt, other, ins, del, the calls at two parameter sets."""
    G = int(np.sum(lengths))
    return list(ix.cover_depth(0, G)) + [ix.cover_summary(len(lengths))] + list(ix.pileup_counts(0, G)) + [ix.calls(1, 1, 0), ix.calls()]


def _assert_host(ix, text, lengths, strands, state):
    cov, pile = state
    depth, dele = depth_of(cov[0]), del_of(pile[3])
    got = _host_state(ix, lengths)
    want = [depth, cov[1], summary_reference(*cov, lengths), pile[0].reshape(-1, 4), pile[1], pile[2], dele,
            calls_reference(depth, cov[1], pile[0], pile[1], pile[2], dele, text, lengths, strands, 1, 1, 0),
            calls_reference(depth, cov[1], pile[0], pile[1], pile[2], dele, text, lengths, strands)]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), i
    part = ix.pileup_counts(3, 17)
    assert np.array_equal(part[0], want[3][3:20]) and np.array_equal(part[3], dele[3:20])
    return want[7].size


@pytest.mark.parametrize("strands", [1, 2])
def test_call_host_on_an_index_from_the_oracles_side(gpu, oracle_mod, strands):
    rng = np.random.default_rng(280 + strands)
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
    ix.call_reset()
    count = {}
    maps_a, state = _call_host_reference(orc, text, *A, 6, None, lengths, strands, count=count)
    got = ix.call_add_host(*A, 6, want_docs=True)
    assert got.dtype == MAPPING_DTYPE and np.array_equal(got, maps_a)
    _assert_host(ix, text, lengths, strands, state)
    # a second batch with other parameters adds to the first; the stats count since the reset.  The batch's offsets do
    # not start at 0 in the caller's array: seqs[offsets[0] ..] is what is copied
    ep = ExtendParams(40, 3, 1, 2)
    maps_b, state = _call_host_reference(orc, text, *B, 12, ep, lengths, strands, into=state, count=count)
    assert np.array_equal(ix.call_add_host(seqs, offs[150:].copy(), 12, extend_params=ep, want_docs=True), maps_b)
    n_calls = _assert_host(ix, text, lengths, strands, state)
    st = ix.call_stats()
    keys = ("mapped", "added", "skipped", "x_columns", "other_columns", "insertions", "deletions", "atomics", "error")
    assert st["reads"] == offs.size - 1 and [st[k] for k in keys] == [count[k] for k in keys] and st["overflow"] == 0, (st, count)
    assert count["added"] > 100 and count["x_columns"] > 0 and n_calls > 0 and len(st["step_ms"]) == 3
    # the coverage of spl_call_add_batch is the coverage spd_cover_add_batch gives on a second handle
    second = capi.Index.from_raw(raw, 0)
    second.set_text(torch.from_numpy(text.copy()))
    second.set_sequences(lengths, strands)
    second.cover_reset()
    second.cover_add_host(*A, 6, want_docs=True)
    second.cover_add_host(*B, 12, extend_params=ep, want_docs=True)
    assert second.cover_summary(150).tobytes() == ix.cover_summary(150).tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(second.cover_depth(0, int(lengths.sum())), ix.cover_depth(0, int(lengths.sum()))))
    cs, ms = second.cover_stats(), ix.cover_stats()
    assert all(cs[k] == ms[k] for k in ("reads", "mapped", "added", "skipped", "intervals", "atomics", "error"))
    second.close()
    # the entries never come back, and an empty batch adds nothing
    with pytest.raises(capi.SpxError, match="spn_map_fetch without a successful spn_map_begin"):
        capi._check(capi._spn().spn_map_fetch(ix._h, None, None))
    assert ix.call_add_host(np.zeros(0, dtype=np.uint8), [0], 4).size == 0
    _assert_host(ix, text, lengths, strands, state)
    # a reset zeroes the pileup and the coverage
    ix.call_reset()
    zero = (cover_reference(*rbatch([], [])[:3], lengths), pileup_reference(*rbatch([], []), lengths))
    assert _assert_host(ix, text, lengths, strands, zero) == 0
    assert ix.call_stats()["reads"] == 0 and ix.cover_stats()["reads"] == 0
    ix.close()


def test_a_clone_has_its_own_arrays_and_the_refusals(gpu):
    rng = np.random.default_rng(12)
    genome = cases.repetitive_text(rng, 20_000, DNA)
    raw = capi.build_raw(genome)
    seqs, offs = cases.reads_mixed(rng, genome, DNA, 120, 300, [ord("N")])
    offs = offs.astype(np.uint64)
    lengths = table(rng, 20, 2, genome.size)
    ix = capi.Index.from_raw(raw, 0)
    with pytest.raises(capi.SpxError, match="spx error -1: spl_call_reset needs the sequence table: the index has none"):
        ix.call_reset()
    with pytest.raises(capi.SpxError, match="spx error -1: spl_call_add_batch needs the sequence table"):
        ix.call_add_host(seqs, offs, 6)
    with pytest.raises(capi.SpxError, match="no pileup has been computed"):
        ix.call_stats()
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    with pytest.raises(capi.SpxError, match="spx error -1: spl_pileup_add_device needs the sequence table"):
        ix.pileup_add_device(t, t[:2], t, t, t[:2], t, t, t, t)
    with pytest.raises(capi.SpxError, match="spx error -1: spl_pileup_finish_device needs the sequence table"):
        ix.pileup_finish_device(t, d_del=t)
    with pytest.raises(capi.SpxError, match="spx error -1: spl_calls_device needs the sequence table"):
        ix.calls_device(t, t, t, t, t, t, call_capacity=1, d_calls=t, d_count=t)
    ix.set_sequences(lengths, 2)
    for call in (lambda: ix.call_add_host(seqs, offs, 6), lambda: ix.calls(), lambda: ix.pileup_counts(0, 5)):
        with pytest.raises(capi.SpxError, match="spx error -1: spl_[a-z_]+ without a successful spl_call_reset"):
            call()
    with pytest.raises(capi.SpxError, match="spl_calls_fetch without a successful spl_calls_begin"):
        capi._check(capi._spl().spl_calls_fetch(ix._h, None))
    S = capi._spl()
    p = t.data_ptr()
    err = capi.lib().spx_last_error
    assert S.spl_pileup_add_device(ix._h, p, p, p, 4, p, p, 4, 1, None, p, p, p, None) == -1 and b"must be non-null" in err()
    assert S.spl_pileup_add_device(ix._h, p, p, p, 4, p, p, 4, 1, p + 8, p, p, p, None) == -1 and b"16-byte aligned" in err()
    assert S.spl_pileup_add_device(ix._h, p, p, p, 4, p, p + 4, 4, 1, p, p, p, p, None) == -1 and b"8-byte" in err()
    assert S.spl_pileup_finish_device(ix._h, p, None, None) == -1 and b"must be non-null" in err()
    assert S.spl_pileup_finish_device(ix._h, p, p + 2, None) == -1 and b"4-byte aligned" in err()
    assert S.spl_calls_device(ix._h, p, p, p, p, p, p, 1, 1, 0, 4, None, p, None) == -1 and b"must be non-null" in err()
    assert S.spl_calls_device(ix._h, p, p, p, p, p, p, 1, 1, 0, 4, p + 8, p, None) == -1 and b"16-byte aligned" in err()
    ix.call_reset()
    ix.call_add_host(seqs, offs, 6)
    mine = _host_state(ix, lengths)
    assert mine[0].any() and mine[3].any()
    with pytest.raises(capi.SpxError, match="does not lie in the forward genome"):
        ix.pileup_counts(genome.size // 2 - 3, 4)
    with pytest.raises(capi.SpxError, match="min_depth and min_alt must be at least 1"):
        ix.calls(0, 1, 0)
    # a clone starts with arrays of its own, empty, and what it adds stays its own
    other = ix.clone(0)
    theirs = _host_state(other, lengths)
    assert not any(theirs[i].any() for i in (0, 1, 3, 4, 5, 6)) and theirs[7].size == 0
    half = int(offs[60])
    other.call_add_host(seqs[:half].copy(), offs[:61].copy(), 6)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(_host_state(ix, lengths), mine))
    fresh = capi.Index.from_raw(raw, 0)
    fresh.set_sequences(lengths, 2)
    fresh.call_reset()
    fresh.call_add_host(seqs[:half].copy(), offs[:61].copy(), 6)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(_host_state(other, lengths), _host_state(fresh, lengths)))
    fresh.close()
    other.close()
    # a new table drops the arrays, and the next call says so
    ix.set_sequences(table(rng, 5, 2, genome.size), 2)
    for call in (lambda: ix.call_add_host(seqs, offs, 6), lambda: ix.calls(), lambda: ix.pileup_counts(0, 5)):
        with pytest.raises(capi.SpxError, match="spn_set_sequences replaced the sequence table after spl_call_reset and dropped the pileup"):
            call()
    ix.call_reset()
    assert ix.calls(1, 1, 0).size == 0 and not ix.cover_summary(5)["reads"].any()
    # a cover_reset alone does not bring the pileup back after another new table; a call_reset does
    ix.set_sequences(lengths, 2)
    ix.cover_reset()
    with pytest.raises(capi.SpxError, match="dropped the pileup"):
        ix.call_add_host(seqs, offs, 6)
    ix.call_reset()
    ix.call_add_host(seqs, offs, 6)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(_host_state(ix, lengths), mine))
    ix.close()


def test_the_ten_products_interleaved_on_one_handle(gpu):
    """Every product's answers on a handle that the others have used are those of a fresh handle; the pileup's and the
    coverage's arrays live through the other products' calls, and every later add lands on what the earlier ones left."""
    rng = np.random.default_rng(290)
    genome = cases.repetitive_text(rng, 40_000, DNA)
    raw = capi.build_raw(genome, doc_lengths=[genome.size // 3, genome.size - genome.size // 3])
    seqs, offs = cases.reads_mixed(rng, genome, DNA, 300, 500, [ord("N")])
    A = (seqs, offs.astype(np.uint64))
    B = (seqs[:int(offs[120])].copy(), offs[:121].astype(np.uint64))
    lengths = table(rng, 120, 2, genome.size)
    call = lambda ix, reads, **kw: ([ix.call_add_host(*reads, 6, **kw)] + _host_state(ix, lengths), None)
    cover = lambda ix, reads, **kw: ([ix.cover_add_host(*reads, 6, **kw)] + _host_state(ix, lengths), None)
    steps = [("call A", lambda ix: call(ix, A)),
             ("map A", lambda ix: (list(ix.map_host(*A, 6)), ix.map_stats())),
             ("cover B docs", lambda ix: cover(ix, B, want_docs=True)),
             ("extend A", lambda ix: (list(ix.extend_host(*A, 6)), ix.extend_stats())),
             ("call B docs", lambda ix: call(ix, B, want_docs=True)),
             ("cigar A", lambda ix: (list(ix.cigar_host(*A, 6)), ix.cigar_stats())),
             ("call A narrow", lambda ix: call(ix, A, extend_params=ExtendParams(20, 2, 1, 1))),
             ("align B", lambda ix: (list(ix.align_host(*B, 6)), ix.align_stats())),
             ("chain A", lambda ix: (list(ix.chain_host(*A, 6)), ix.chain_stats())),
             ("mems B", lambda ix: (list(ix.mems_host(*B, 6)), ix.mems_stats())),
             ("place A", lambda ix: (list(ix.place_host(*A, 6)), ix.place_stats())),
             ("assign B", lambda ix: (list(ix.assign_host(capi.SPX_MODE_MS, *B, 6)), ix.votes_stats())),
             ("call B", lambda ix: call(ix, B)),
             ("map A", lambda ix: (list(ix.map_host(*A, 6)), ix.map_stats()))]
    ix = capi.Index.from_raw(raw, 0)
    ix.set_sequences(lengths, 2)
    ix.call_reset()
    done = []  # the adds so far: a fresh handle replays them, so that its arrays hold what this one's hold
    for name, step in steps:
        got, got_stats = step(ix)
        fresh = capi.Index.from_raw(raw, 0)
        fresh.set_sequences(lengths, 2)
        fresh.call_reset()
        for earlier in done:
            earlier(fresh)
        want, want_stats = step(fresh)
        fresh.close()
        if name.startswith(("call", "cover")):
            done.append(step)
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (name, i)
        for s in (got_stats, want_stats):
            for key in ("kernel_ms", "step_ms", "wave_fill_ticks", "wave_back_ticks"):
                (s or {}).pop(key, None)
        assert got_stats == want_stats, (name, got_stats, want_stats)
    st = ix.call_stats()
    assert st["reads"] == 2 * 300 + 2 * 120 and st["added"] > 300 and st["error"] == 0 and ix.cover_stats()["reads"] == 2 * 300 + 3 * 120
    ix.close()


# ---- the command: ground truth that does not rest on the rule ---------------------------------------------------------------
VCF_INFO = [b'##INFO=<ID=DP,Number=1,Type=Integer,Description="Reads that cover the base with an = or X column">',
            b'##INFO=<ID=AD,Number=2,Type=Integer,Description="Reads that match the reference, reads that carry the called allele">',
            b'##INFO=<ID=BC,Number=4,Type=Integer,Description="Mismatching reads by letter: A, C, G, T">',
            b'##INFO=<ID=OT,Number=1,Type=Integer,Description="Mismatching reads with a byte outside ACGT">',
            b'##INFO=<ID=DL,Number=1,Type=Integer,Description="Reads that delete the base">',
            b'##INFO=<ID=IN,Number=1,Type=Integer,Description="Insertions in front of the base">',
            b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]


def _call_cli(planted, name, extra=(), env=None):
    d = planted["dir"]
    path = d / name
    if os.path.exists(str(path) + ".vcf"):
        os.remove(str(path) + ".vcf")
    r = _cli(["call", "-r", str(d / "ref"), "-p", str(path), "-n", "-L", "12"] + list(extra),
             dict(os.environ, SPUMONI_TEXT=str(d / "ref.fa.rawtext"), **(env or {})))
    assert r.returncode == 0, r.stderr.decode()
    return (path.parent / (name + ".vcf")).read_bytes(), r.stderr.decode()


def _expected_vcf(planted, depth, alt, min_depth, min_alt, min_permille):
    """The file from per-sequence depth and letter counts the test kept while it planted: substitutions only, so the reads
    that match the reference at a base are the depth less the substituted ones."""
    lines = [b"##fileformat=VCFv4.2"]
    lines += [b"##contig=<ID=%s,length=%d>" % (name, len(planted["seqs"][name])) for name in planted["names"]]
    lines += VCF_INFO
    for name in planted["names"]:
        s = planted["seqs"][name]
        for i in np.flatnonzero(alt[name].sum(axis=1)):
            counts = [int(v) for v in alt[name][i]]
            d = int(depth[name][i])
            best = max((c for c in range(4) if b"ACGT"[c] != s[i]), key=lambda c: (counts[c], -c))
            if d >= min_depth and counts[best] >= min_alt and counts[best] * 1000 >= min_permille * d:
                lines.append(b"%s\t%d\t.\t%c\t%c\t.\t.\tDP=%d;AD=%d,%d;BC=%d,%d,%d,%d;OT=0;DL=0;IN=0" %
                             (name, i + 1, s[i], b"ACGT"[best], d, d - sum(counts), counts[best], *counts))
    return b"".join(line + b"\n" for line in lines)


def test_planted_substitutions_give_the_file_the_test_computes(planted):
    """Exact 60-mers with one substitution at least 20 characters from either end, on both strands where the index has
    both: three reads with the same substitution (a call), one alone (below min_alt), two among six reads of depth (below
    the share), two letters at one base, and two exact reads."""
    m = 60
    names = planted["names"]
    depth = {name: np.zeros(len(planted["seqs"][name]), dtype=np.int64) for name in names}
    alt = {name: np.zeros((len(planted["seqs"][name]), 4), dtype=np.int64) for name in names}
    reads = []

    def plant(name, off, sub=None, letter=None, reverse=False):
        seg = bytearray(planted["seqs"][name][off:off + m])
        depth[name][off:off + m] += 1
        if sub is not None:
            assert 20 <= sub - off < m - 20 and b"ACGT"[letter] != seg[sub - off]
            seg[sub - off] = b"ACGT"[letter]
            alt[name][sub, letter] += 1
        reads.append(revcomp(bytes(seg)) if reverse and planted["rc"] else bytes(seg))

    for name in names:
        s = planted["seqs"][name]
        other = lambda at, k=1: (b"ACGT".index(s[at:at + 1]) + k) % 4
        a, b, c, e = 40, 110, 180, 250
        for r in range(3):  # three reads, different offsets, both strands: a call at the defaults
            plant(name, a - 22 - 5 * r, a, other(a), reverse=r == 1)
        plant(name, b - 30, b, other(b))  # alone: below min_alt
        for r in range(6):  # two of six: 333 thousandths
            plant(name, c - 21 - 3 * r, c if r < 2 else None, other(c) if r < 2 else None, reverse=r % 2 == 1)
        for r in range(5):  # two letters at one base: three against two, and the largest is called
            plant(name, e - 25 - r, e, other(e, 1 if r < 3 else 2), reverse=r == 4)
        for off in (len(s) - m, 55):  # exact reads: one over the lone substitution, one at the end (it may reach `e`)
            plant(name, off, reverse=off % 2 == 1)
    reads.append(b"ACGT" * 5)  # (an unmapped read adds nothing)
    d = planted["dir"]
    (d / "snv.fa").write_bytes(b"".join(b">r%d\n%s\n" % (q, r) for q, r in enumerate(reads)))
    env = dict(os.environ, SPUMONI_TEXT=str(d / "ref.fa.rawtext"))
    # `spumoni cover` on the same file, before and after: the calls change nothing of it
    assert _cli(["cover", "-r", str(d / "ref"), "-p", str(d / "snv.fa"), "-n", "-L", "12", "-b"], env).returncode == 0
    before = ((d / "snv.fa.cover").read_bytes(), (d / "snv.fa.bedgraph").read_bytes())
    want = _expected_vcf(planted, depth, alt, 2, 2, 500)
    got, err = _call_cli(planted, "snv.fa")
    assert got.split(b"\n") == want.split(b"\n")
    assert want.count(b"\n") == 4 + len(VCF_INFO) + 2 * 3  # (the three-read site and the two-letter site of each sequence)
    assert f"{len(reads)} reads, {len(reads) - 1} mapped, 1 without a mapping, 6 calls" in err
    for params in ((1, 1, 0), (2, 2, 300), (7, 1, 0), (1, 3, 1000)):
        want = _expected_vcf(planted, depth, alt, *params)
        got, _ = _call_cli(planted, "snv.fa", extra=("-D", str(params[0]), "-A", str(params[1]), "-Q", str(params[2])))
        assert got.split(b"\n") == want.split(b"\n"), params
    assert _expected_vcf(planted, depth, alt, 1, 1, 0).count(b"\n") == 4 + len(VCF_INFO) + 4 * 3
    # small super-batches accumulate to the same file
    want = _expected_vcf(planted, depth, alt, 2, 2, 500)
    assert _call_cli(planted, "snv.fa", env=dict(SPUMONI_SUPER_BATCH="1000"))[0] == want
    assert _cli(["cover", "-r", str(d / "ref"), "-p", str(d / "snv.fa"), "-n", "-L", "12", "-b"], env).returncode == 0
    assert ((d / "snv.fa.cover").read_bytes(), (d / "snv.fa.bedgraph").read_bytes()) == before


def test_a_full_super_batch_cut_into_two_calls_gives_the_same_file(planted):
    """33.75 M characters in one super-batch of 64 Mi are two calls of spl_call_add_batch that add up.  Every 40th read
    carries a substitution at its column 75; depth and letters are counted from where the reads were taken."""
    rng = np.random.default_rng(44)
    nreads, m = 225_000, 150
    names = planted["names"]
    which = rng.integers(0, 3, nreads)
    room = np.array([len(planted["seqs"][name]) - m for name in names])[which]
    at = (rng.random(nreads) * room).astype(np.int64)
    depth, alt = {}, {}
    d = planted["dir"]
    code = np.full(256, 4, dtype=np.int64)
    code[list(b"ACGT")] = np.arange(4)
    with open(d / "bigsnv.fa", "wb") as f:
        for w, name in enumerate(names):
            s = np.frombuffer(planted["seqs"][name], dtype=np.uint8)
            mine = np.flatnonzero(which == w)
            rs = s[at[mine].astype(np.int32)[:, None] + np.arange(m, dtype=np.int32)[None, :]].copy()
            sub = np.arange(0, mine.size, 40)
            letters = (code[rs[sub, 75]] + 1 + (sub // 40) % 3) % 4  # (never the reference's own)
            rs[sub, 75] = np.frombuffer(b"ACGT", dtype=np.uint8)[letters]
            f.write(b"".join(b">r%d\n%s\n" % (q, rs[q].tobytes()) for q in range(mine.size)))
            dd = np.zeros(s.size + 1, dtype=np.int64)
            np.add.at(dd, at[mine], 1)
            np.add.at(dd, at[mine] + m, -1)
            depth[name] = np.cumsum(dd)[:-1]
            alt[name] = np.zeros((s.size, 4), dtype=np.int64)
            np.add.at(alt[name], (at[mine][sub] + 75, letters), 1)
    for params in ((2, 3, 0), (2, 4, 0)):  # (a few substituted reads among thousands: the share is left out)
        want = _expected_vcf(planted, depth, alt, *params)
        got, err = _call_cli(planted, "bigsnv.fa", extra=("-L", "20", "-A", str(params[1]), "-Q", "0"), env=dict(SPUMONI_SUPER_BATCH=str(64 << 20)))
        assert f"{nreads} reads, {nreads} mapped".encode() in err.encode()
        assert got == want, params
    assert 4 + len(VCF_INFO) < _expected_vcf(planted, depth, alt, 2, 4, 0).count(b"\n") < _expected_vcf(planted, depth, alt, 2, 3, 0).count(b"\n")
    for suffix in ("", ".vcf"):
        os.remove(str(d / "bigsnv.fa") + suffix)
