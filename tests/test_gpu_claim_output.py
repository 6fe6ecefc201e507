"""-m gpu: the claim-staged output of the plain walk (spx_walk_fast.inc, STAGE) against the oracle, bit for bit.

The dynamic deal's PML walk without document ids holds the results of a claim of 64 consecutive reads in LDS -- per read
the word of reset bits and the class record -- until the claim's last read has ended, then writes the claim's lengths in
whole aligned lines and its class records as one stretch.  Reads longer than a word, empty reads and claims that find none
of the wavefront's CSLOTS slots free keep the one-store-per-word path.  What must not show: which path a read took.  So the
batches here mix the three kinds inside every claim, end claims early, leave claims empty, run the slots out, start the
output at an odd position of a fenced buffer, repeat a call on one handle, and come from the digestion (in_starts).

As in test_gpu_dynamic_deal.py the launch is shrunk with "waves_per_cu" = 4 (one 256-thread block per CU) so that "more
reads than lanes" is some 10^5 short reads, and every batch goes through tests.test_gpu_parity._compare_all: PML with
16- and 32-bit values, with and without out_lengths, the classes -- and the instances that do not stage (PML + doc, MS)."""
import numpy as np
import pytest
import torch

from spumoni_amd import capi, shard, synth
from tests import cases
from tests.test_gpu_parity import _compare_all

pytestmark = pytest.mark.gpu

CLAIM = 64   # spx_walk_fast.inc: CHUNK_CLAIM
CSLOTS = 3   # spx_walk_fast.inc: claims a wavefront can hold in LDS
STEP_REPS = 2  # spx_walk_fast.inc: characters a lane can take per iteration, at most
POOL_READS, POOL_LEN = 2048, 3000
AROUND_THE_WORD = [0, 1, 2, 43, 44, 45, 63, 64, 65, 66, 127, 128, 129, 300]


def _nlanes():
    """lanes of a plain launch at waves_per_cu = 4: one block of 256 threads per CU"""
    return torch.cuda.get_device_properties(0).multi_processor_count * 256


@pytest.fixture(scope="module")
def stat_case():
    """the small statistical index (r = 2^14, sigma = 253, SA samples, documents), its oracle and a pool of reads"""
    raw = synth.statistical_rlbwt(1 << 14, 253, 6.0, seed=11, device="cuda", zipf=1.0, with_samples=True, n_docs=8)
    pool, _ = synth.simulate_reads(raw, POOL_READS, POOL_LEN, seed=12, f_mis=0.05, warmup=2)
    return raw, pool.cpu().numpy().reshape(POOL_READS, POOL_LEN)


def _index(raw):
    ix = capi.Index.from_raw(raw, 0)
    ix.set_option("waves_per_cu", 4)
    ix.set_option("chunk_mode", 1)  # never chunked: these batches are for the plain walk
    return ix


def _batch(pool, lens):
    """read q: the last lens[q] characters of pool read q (mod the pool)"""
    lens = np.asarray(lens, dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n, plen = pool.shape
    parts = [pool[q % n, plen - l:] for q, l in enumerate(lens) if l]
    seqs = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    return np.ascontiguousarray(seqs, dtype=np.uint8), offs


def _check(oracle_mod, raw, pool, lens):
    seqs, offs = _batch(pool, lens)
    _compare_all(oracle_mod, raw, None, seqs, offs, ix=_index(raw))


@pytest.mark.parametrize("kind", ["mixed", "all_64", "all_1"])
def test_lengths_around_the_word(oracle_mod, stat_case, kind):
    """2 * lanes + 65 reads.  mixed: lengths drawn from 0, 1, 2, 43 .. 45, 63 .. 66, 127 .. 129, 300 -- every claim of 64 holds
    staged reads (up to 64 characters), direct ones (65 and more: one store per word, as before) and empty ones; all_64: every
    read fills its word exactly; all_1: 64 reads to a line of the output."""
    raw, pool = stat_case
    n = 2 * _nlanes() + 65
    if kind == "mixed":
        lens = np.random.default_rng(21).choice(AROUND_THE_WORD, size=n)
        lens[5::CLAIM], lens[9::CLAIM], lens[11::CLAIM] = 0, 300, 44  # (no claim is left to chance)
        per_claim = lens[: n // CLAIM * CLAIM].reshape(-1, CLAIM)
        assert ((per_claim == 0).any(1) & (per_claim > 64).any(1) & ((per_claim > 0) & (per_claim <= 64)).any(1)).all()
    else:
        lens = np.full(n, 64 if kind == "all_64" else 1)
    _check(oracle_mod, raw, pool, lens)


@pytest.mark.parametrize("count", ["lanes+1", "lanes+64", "lanes+64+5", "3*lanes+7"])
def test_claims_that_end_early(oracle_mod, stat_case, count):
    """read counts that leave the last claim with 1, 64, 5 and 7 reads (a claim past the batch's end is clipped)"""
    raw, pool = stat_case
    nl = _nlanes()
    n = {"lanes+1": nl + 1, "lanes+64": nl + 64, "lanes+64+5": nl + 64 + 5, "3*lanes+7": 3 * nl + 7}[count]
    lens = np.random.default_rng(22 + n % 1000).integers(0, 70, size=n)
    lens[-1] = 17  # (the batch's last read is a real one)
    _check(oracle_mod, raw, pool, lens)


def test_claims_that_hold_nothing(oracle_mod, stat_case):
    """70 and 300 empty reads in a row inside the claimed part (whole claims of empty reads: they are counted as ended when
    they are looked at, and the claim writes nothing), a run of them across the boundary between the strided round and the
    claimed part; and a batch whose last claim is all empty."""
    raw, pool = stat_case
    nl = _nlanes()
    rng = np.random.default_rng(23)
    n = nl + 5000
    lens = rng.integers(1, 70, size=n)
    lens[nl - 10: nl + 200] = 0
    lens[nl + 1000: nl + 1070] = 0
    lens[nl + 2000: nl + 2300] = 0
    lens[::97] = 0
    _check(oracle_mod, raw, pool, lens)
    n = nl + 3 * CLAIM
    lens = rng.integers(1, 70, size=n)
    lens[n - CLAIM:] = 0  # reads [lanes + 128, lanes + 192): one claim
    _check(oracle_mod, raw, pool, lens)


def test_slots_run_out(oracle_mod, stat_case):
    """Most reads 3 .. 10 characters, one of 3000 in every fourth claim: a claim with such a read stays open while the claims
    after it come and go, a wavefront soon holds CSLOTS of them, and every further claim it takes finds no slot -- its reads
    leave by the one-store-per-word path.  Same answers.

    That slots do run out, from the lengths alone: a lane takes at most STEP_REPS characters an iteration, so a 3000-character
    read keeps its claim open for 1500 iterations and more.  A wavefront's 64 lanes end a short claim's 64 reads of at most
    10 characters in 10 * 64 / 64 = 10 iterations at one character a lane and iteration; at a tenth of that pace it is 100.
    With the claims taken in turn by the lanes / 64 wavefronts, a wavefront that took a claim with a long read is handed
    every (lanes / 64)-th claim after it: more than CSLOTS of them within those 1500 iterations."""
    raw, pool = stat_case
    nl = _nlanes()
    waves = nl // CLAIM
    rng = np.random.default_rng(24)
    per_wave = 12  # claims a wavefront takes after its first round
    n = nl + waves * per_wave * CLAIM + 9
    lens = rng.integers(3, 11, size=n)
    long_at = np.arange(0, n // CLAIM, 4) * CLAIM + 17  # a read in the middle of every fourth claim
    lens[long_at] = 3000
    # the count: for every claim with a long read, the later claims of the same wavefront (every waves-th) that are over
    # within the long read's 1500 iterations at 100 iterations a claim
    open_for = 3000 // STEP_REPS
    later = np.minimum((n // CLAIM - 1 - long_at // CLAIM) // waves, open_for // 100)
    assert later.max() > CSLOTS and (later > CSLOTS).sum() > waves
    _check(oracle_mod, raw, pool, lens)


def _device_pml(ix, d_seqs, d_offs, total, n, vt, fence_front, want_len=True, want_class=True):
    """the device entry point on sentinel-filled buffers: lengths buffer of fence_front + total + 8 values addressed from its
    start (offs[0] = fence_front), class buffer of n + 8 records"""
    d_len = torch.full((fence_front + total + 8,), -1, dtype=vt, device="cuda") if want_len else None
    d_cls = torch.full((n + 8, 2), -1, dtype=torch.int64, device="cuda") if want_class else None
    ix.query_device(capi.SPX_MODE_PML, d_seqs, d_offs, total, d_lengths=d_len, d_class=d_cls, bin_width=7, max_value_thr=3,
                    narrow=vt == torch.int16)
    torch.cuda.synchronize()
    st = ix.last_stats()
    st.pop("kernel_ms")
    return (d_len.cpu().numpy() if want_len else None), (d_cls.cpu().numpy() if want_class else None), st


@pytest.mark.parametrize("shape", ["around_the_word", "short"])
@pytest.mark.parametrize("vt", [torch.int16, torch.int32])
def test_nothing_outside_the_stretch(oracle_mod, stat_case, vt, shape):
    """A batch cut out of a larger one (shard.shard, as bench.py cuts a rank's share) whose first offset is no multiple of
    64: the claims' first and last lines are masked, only values [offs[0], offs[n]) and n class records differ from the
    sentinel the buffers were filled with -- the 8 values and 8 records of slack behind them too -- and they are the
    oracle's.  around_the_word: most claims' stretches are longer than 64 lines (the writer that searches); short: lengths
    0 .. 66, every stretch within 64 lines (the writer that maps positions through the bit map), unstaged reads among them."""
    raw, pool = stat_case
    nl = _nlanes()
    rng = np.random.default_rng(25)
    n_all = nl + 7 * CLAIM + 300
    lens = rng.choice(AROUND_THE_WORD, size=n_all) if shape == "around_the_word" else rng.integers(0, 67, size=n_all)
    seqs_all, offs_all = _batch(pool, lens)
    lo = 150
    while offs_all[lo] % 64 == 0:
        lo += 1
    hi = lo + nl + 5 * CLAIM + 11
    seqs, offs0 = shard.shard(seqs_all, offs_all, lo, hi)
    org, n, total = int(offs_all[lo]), hi - lo, int(offs0[-1])
    assert org % 64 != 0 and n > nl + CLAIM
    orc = oracle_mod.OracleIndex.from_raw(raw.cpu())
    want = orc.pml(seqs, offs0)
    _, a, b, s = oracle_mod.classify(want, offs0, 7, 3)
    # the cut stays where it was in the larger batch: offs[0] = org
    d_seqs = capi.pad_seqs(torch.from_numpy(seqs_all[: org + total].copy()).cuda())
    d_offs = torch.from_numpy(offs0 + org).cuda()
    ix = _index(raw)
    mask = 0xffff if vt == torch.int16 else 0xffffffff
    got, cls, _ = _device_pml(ix, d_seqs, d_offs, total, n, vt, org)
    assert (got[:org] == -1).all() and (got[org + total:] == -1).all() and got.size == org + total + 8
    assert np.array_equal(got[org: org + total].astype(np.int64) & mask, want.astype(np.int64))
    assert (cls[n:] == -1).all() and cls.shape[0] == n + 8
    rec = np.ascontiguousarray(cls[:n]).view(capi.CLASS_DTYPE).reshape(-1)
    assert np.array_equal(rec["above"], a) and np.array_equal(rec["below"], b) and np.array_equal(rec["sum_max"], s)
    # classes alone: the same records, nothing else
    _, cls2, _ = _device_pml(ix, d_seqs, d_offs, total, n, vt, org, want_len=False)
    assert np.array_equal(cls2, cls)
    # lengths alone
    got2, _, _ = _device_pml(ix, d_seqs, d_offs, total, n, vt, org, want_class=False)
    assert np.array_equal(got2, got)


def test_same_handle_three_calls(oracle_mod, stat_case):
    """three calls on one handle: the same outputs and the same walk statistics (the slots' state is the launch's own)"""
    raw, pool = stat_case
    n = 2 * _nlanes() + 7
    seqs, offs = _batch(pool, np.random.default_rng(26).choice(AROUND_THE_WORD[:-1], size=n))
    want = oracle_mod.OracleIndex.from_raw(raw.cpu()).pml(seqs, offs)
    d_seqs = capi.pad_seqs(torch.from_numpy(seqs).cuda())
    d_offs = torch.from_numpy(offs).cuda()
    ix = _index(raw)
    for vt in (torch.int16, torch.int32):
        runs = [_device_pml(ix, d_seqs, d_offs, int(offs[-1]), n, vt, 0) for _ in range(3)]
        for got, cls, st in runs[1:]:
            assert st == runs[0][2] and np.array_equal(got, runs[0][0]) and np.array_equal(cls, runs[0][1])
        mask = 0xffff if vt == torch.int16 else 0xffffffff
        assert runs[0][2]["steps"] == int(offs[-1])
        assert np.array_equal(runs[0][0][: int(offs[-1])].astype(np.int64) & mask, want.astype(np.int64))


def test_parked_reads(oracle_mod):
    """Digest + walk in one call with the digested reads left where the digestion parked them ("digest_parked" = 2): a read's
    characters are at in_starts[q], its results go to offs[q] -- the staged claim is addressed by the latter."""
    kind = capi.SPX_DIGEST_DNA
    rng = np.random.default_rng(27)
    genome = cases.repetitive_text(rng, 30000, list(b"ACGT"))
    k, w = 4, 11
    dtext = oracle_mod.digest(kind, k, w, genome)
    raw = synth.index_from_text(torch.from_numpy(dtext.copy()), doc_lengths=[dtext.size // 2, dtext.size - dtext.size // 2])
    orc = oracle_mod.OracleIndex.from_raw(raw)
    ix = _index(raw)
    n = _nlanes() + 2 * CLAIM + 5
    lens = rng.integers(0, 160, size=n)  # (digested reads of 0 .. some 130 characters)
    lens[::13] = 0
    lens[5000:5100] = 0
    starts = rng.integers(0, genome.size - 160, size=n)
    seqs = np.concatenate([genome[s: s + l] for s, l in zip(starts, lens)]).astype(np.uint8)
    seqs[rng.random(seqs.size) < 0.01] = ord("N")
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    dseqs, doffs = oracle_mod.digest_batch(kind, k, w, seqs, offs)
    dl = np.diff(doffs.astype(np.int64))
    assert (dl > 64).any() and (dl == 0).any() and ((dl > 0) & (dl <= 64)).sum() > n // 4
    want_l = orc.pml(dseqs, doffs.astype(np.int64))
    _, a, b, sm = oracle_mod.classify(want_l, doffs.astype(np.int64), 5, 2)
    total_in, tot = int(offs[-1]), int(doffs[-1])
    d_seqs = torch.zeros(total_in + 64, dtype=torch.uint8, device="cuda")
    d_seqs[:total_in] = torch.from_numpy(seqs).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    ix.set_option("digest_parked", 2)
    for vt in (torch.int16, torch.int32):
        d_len = torch.full((total_in + 8,), -1, dtype=vt, device="cuda")
        d_cls = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
        d_oo, _ = ix.digest_query_device(capi.SPX_MODE_PML, kind, k, w, d_seqs, d_offs, total_in, d_lengths=d_len, d_class=d_cls,
                                         bin_width=5, max_value_thr=2)
        torch.cuda.synchronize()
        assert np.array_equal(d_oo.cpu().numpy().astype(np.uint64), doffs)
        mask = 0xffff if vt == torch.int16 else 0xffffffff
        assert np.array_equal(d_len[:tot].cpu().numpy().astype(np.int64) & mask, want_l.astype(np.int64))
        cls = d_cls.cpu().numpy().view(capi.CLASS_DTYPE).reshape(-1)
        assert np.array_equal(cls["above"], a) and np.array_equal(cls["below"], b) and np.array_equal(cls["sum_max"], sm)
