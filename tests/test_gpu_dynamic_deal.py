"""-m gpu: the dynamic deal of the plain walk (spx_walk_fast.inc, DYN) against the oracle, bit for bit.

A plain k_walk_fast launch with more reads than lanes deals only its first round by lane index; after it the wavefronts
claim read indices from one device word (WalkCounters::claim, zeroed per call) and hand them to the lanes that end a read.
Which lane walks which read must not show: PML, PML + doc, MS, MS + doc, 16- and 32-bit entry points, with and without
out_lengths (tests.test_gpu_parity._compare_all asks for all of them) on batches shaped to stress the hand-out -- read
lengths from a heavy tail, runs of empty reads (a lane that is handed an empty read wants the next one in the same
iteration), read counts around the lane count and a claim's size, the same batch several times on one index (the word is
zeroed per call), the state-machine walk (SPX_OLD_WALK=1, a child process) on the same batch, reads parked by the digestion
(BatchArgs::in_starts), and a chunked batch with fallback reads between two dynamic ones.

The launch is shrunk with the "waves_per_cu" option (4: one 256-thread block per CU), so that "more reads than lanes" is
some 10^5 short reads."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from spumoni_amd import capi, synth
from tests import cases
from tests.test_gpu_parity import _compare_all

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLAIM = 64  # spx_walk_fast.inc: CHUNK_CLAIM
POOL_READS, POOL_LEN = 2048, 3000


def _nlanes():
    """lanes of a plain launch at waves_per_cu = 4: one block of 256 threads per CU"""
    return torch.cuda.get_device_properties(0).multi_processor_count * 256


@pytest.fixture(scope="module")
def stat_case():
    """a promoted-alphabet index (bytes >= 128 take the quirk paths) with SA samples and documents, and a pool of reads"""
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


def _check_all(oracle_mod, raw, seqs, offs, ix):
    """PML, PML + doc, MS + doc, 16 / 32 bits, with and without out_lengths (_compare_all); and MS without documents"""
    _, st = _compare_all(oracle_mod, raw, None, seqs, offs, ix=ix)
    w = oracle_mod.OracleIndex.from_raw(raw.cpu()).ms(seqs, offs, want_docs=False)
    got = ix.query_host(capi.SPX_MODE_MS, seqs, offs, want_lengths=False, want_docs=False)
    assert np.array_equal(got["pointers"], w["pointers"])
    return st


def test_heavy_tailed_read_lengths(oracle_mod, stat_case):
    """Lengths 1 .. 3000 from a Pareto tail in one batch of 2 * lanes + 65 reads: most reads take a few iterations, a few
    take thousands -- a lane's share of the batch is whatever it has time for."""
    raw, pool = stat_case
    rng = np.random.default_rng(1)
    n = 2 * _nlanes() + 65
    lens = np.minimum(POOL_LEN, 1 + np.floor(6.0 * rng.pareto(1.1, size=n))).astype(np.int64)
    lens[rng.integers(0, n, size=40)] = rng.integers(1500, POOL_LEN + 1, size=40)
    assert lens.min() == 1 and lens.max() > 2000
    seqs, offs = _batch(pool, lens)
    _check_all(oracle_mod, raw, seqs, offs, _index(raw))


def test_runs_of_empty_reads(oracle_mod, stat_case):
    """Empty reads in runs: at the very start (lanes of the first, strided round that want a read in their first iteration,
    before any claim was made), 70 and 300 in a row inside the claimed part (more than a wavefront's lanes, more than a
    claim), across the boundary between the strided and the claimed part, and at the very end."""
    raw, pool = stat_case
    rng = np.random.default_rng(2)
    nl = _nlanes()
    n = nl + 5000
    lens = rng.integers(1, 40, size=n)
    lens[:130] = 0
    lens[nl - 10: nl + 200] = 0
    lens[nl + 1000: nl + 1070] = 0
    lens[nl + 2000: nl + 2300] = 0
    lens[::97] = 0
    lens[n - 131:] = 0
    seqs, offs = _batch(pool, lens)
    _check_all(oracle_mod, raw, seqs, offs, _index(raw))
    # ... and nothing but empty reads
    seqs, offs = _batch(pool, np.zeros(nl + 3 * CLAIM + 1, dtype=np.int64))
    ix = _index(raw)
    got = ix.query_host(capi.SPX_MODE_PML, seqs, offs, classify=(7, 3))
    assert not got["class"]["above"].any() and not got["class"]["below"].any() and ix.last_stats()["steps"] == 0


@pytest.mark.parametrize("extra", [-1, 0, 1, 63, CLAIM + 1, None])
def test_read_counts_around_the_lane_count(oracle_mod, stat_case, extra):
    """lanes - 1, lanes, lanes + 1, lanes + 63, one read past the first claim, 2 * lanes + 65 (None) reads"""
    raw, pool = stat_case
    nl = _nlanes()
    n = 2 * nl + 65 if extra is None else nl + extra
    rng = np.random.default_rng(3 + n % 1000)
    lens = rng.integers(0, 30, size=n)
    lens[-1] = 17  # (the batch's last read is a real one)
    seqs, offs = _batch(pool, lens)
    _check_all(oracle_mod, raw, seqs, offs, _index(raw))


def _device_run(ix, mode, seqs, offs, vt, want_len=True):
    d_seqs = capi.pad_seqs(torch.from_numpy(seqs).cuda())
    d_offs = torch.from_numpy(offs).cuda()
    tot, n = int(offs[-1]), offs.size - 1
    pml = mode == capi.SPX_MODE_PML
    d_len = torch.full((tot + 8,), -1, dtype=vt, device="cuda") if pml and want_len else None
    d_ptr = None if pml else torch.full((tot + 8,), -1, dtype=torch.int64, device="cuda")
    d_doc = torch.full((tot + 8,), -1, dtype=vt, device="cuda")
    d_cls = torch.zeros((n, 2), dtype=torch.int64, device="cuda") if pml else None
    ix.query_device(mode, d_seqs, d_offs, tot, d_lengths=d_len, d_pointers=d_ptr, d_docs=d_doc, d_class=d_cls, bin_width=7,
                    max_value_thr=3)
    torch.cuda.synchronize()
    st = ix.last_stats()
    st.pop("kernel_ms")
    out = [t[:tot].cpu().numpy() for t in (d_len, d_ptr, d_doc) if t is not None]
    if d_cls is not None:
        out.append(d_cls.cpu().numpy())
    return out, st


def test_same_batch_three_times_on_one_index(oracle_mod, stat_case):
    """The claim word is zeroed per call: three calls in a row give the same outputs and the same walk statistics (a word
    left standing would send every wavefront home after the strided round)."""
    raw, pool = stat_case
    rng = np.random.default_rng(5)
    n = 2 * _nlanes() + 7
    seqs, offs = _batch(pool, rng.integers(0, 50, size=n))
    ix = _index(raw)
    orc = oracle_mod.OracleIndex.from_raw(raw.cpu())
    wl, wd = orc.pml(seqs, offs, want_docs=True)
    wm = orc.ms(seqs, offs, want_docs=True)
    for mode, vt in ((capi.SPX_MODE_PML, torch.int16), (capi.SPX_MODE_PML, torch.int32), (capi.SPX_MODE_MS, torch.int32)):
        runs = [_device_run(ix, mode, seqs, offs, vt) for _ in range(3)]
        for out, st in runs[1:]:
            assert st == runs[0][1]
            assert all(np.array_equal(x, y) for x, y in zip(out, runs[0][0]))
        assert runs[0][1]["steps"] == int(offs[-1])
        out = runs[0][0]
        mask = 0xffff if vt == torch.int16 else 0xffffffff
        if mode == capi.SPX_MODE_PML:
            assert np.array_equal(out[0].astype(np.int64) & mask, wl.astype(np.int64))
            assert np.array_equal(out[1].astype(np.int64) & mask, wd.astype(np.int64))
        else:
            assert np.array_equal(out[0].view(np.uint64), wm["pointers"])
            assert np.array_equal(out[1].view(np.uint32), wm["docs"])
    # without out_lengths (document ids and classes only)
    a, _ = _device_run(ix, capi.SPX_MODE_PML, seqs, offs, torch.int32, want_len=False)
    assert np.array_equal(a[0].view(np.uint32), wd)


_CHILD = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from spumoni_amd import capi, synth
d = np.load(sys.argv[2])
raw = synth.statistical_rlbwt(1 << 14, 253, 6.0, seed=11, device="cuda", zipf=1.0, with_samples=True, n_docs=8)
ix = capi.Index.from_raw(raw, 0)
ix.set_option("waves_per_cu", 4)
ix.set_option("chunk_mode", 1)
p = ix.query_host(capi.SPX_MODE_PML, d["seqs"], d["offs"], want_docs=True, classify=(7, 3))
m = ix.query_host(capi.SPX_MODE_MS, d["seqs"], d["offs"], want_lengths=False, want_docs=True)
np.savez(sys.argv[3], lengths=p["lengths"], docs=p["docs"], cls=p["class"], pointers=m["pointers"], mdocs=m["docs"])
'''


def test_state_machine_walk_gives_the_same(stat_case, tmp_path):
    """SPX_OLD_WALK=1 (read once per process: a child) routes the batch through k_walk_lanes and its strided deal."""
    raw, pool = stat_case
    rng = np.random.default_rng(6)
    n = _nlanes() + 3 * CLAIM + 9
    lens = rng.integers(0, 60, size=n)
    lens[100:180] = 0
    seqs, offs = _batch(pool, lens)
    np.savez(tmp_path / "in.npz", seqs=seqs, offs=offs)
    env = dict(os.environ)
    env["SPX_OLD_WALK"] = "1"
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    old = np.load(tmp_path / "out.npz")
    ix = _index(raw)
    pm = ix.query_host(capi.SPX_MODE_PML, seqs, offs, want_docs=True, classify=(7, 3))
    ms = ix.query_host(capi.SPX_MODE_MS, seqs, offs, want_lengths=False, want_docs=True)
    tot = int(offs[-1])
    assert np.array_equal(pm["lengths"][:tot], old["lengths"][:tot]) and np.array_equal(pm["docs"][:tot], old["docs"][:tot])
    assert np.array_equal(pm["class"], old["cls"])
    assert np.array_equal(ms["pointers"][:tot], old["pointers"][:tot]) and np.array_equal(ms["docs"][:tot], old["mdocs"][:tot])


@pytest.mark.parametrize("kind", [capi.SPX_DIGEST_PROMOTED, capi.SPX_DIGEST_DNA])
def test_parked_reads(oracle_mod, kind):
    """Digest + walk in one call with the digested reads left where the digestion parked them ("digest_parked" = 2): the walk
    takes read q's characters at in_starts[q], which a lane loads for whichever read it was handed."""
    rng = np.random.default_rng(70 + kind)
    genome = cases.repetitive_text(rng, 30000, list(b"ACGT"))
    k, w = 4, 11
    dtext = oracle_mod.digest(kind, k, w, genome)
    raw = synth.index_from_text(torch.from_numpy(dtext.copy()), doc_lengths=[dtext.size // 2, dtext.size - dtext.size // 2])
    orc = oracle_mod.OracleIndex.from_raw(raw)
    ix = _index(raw)
    n = _nlanes() + 2 * CLAIM + 5
    lens = rng.integers(0, 160, size=n)
    lens[::13] = 0
    lens[5000:5100] = 0
    starts = rng.integers(0, genome.size - 160, size=n)
    seqs = np.concatenate([genome[s: s + l] for s, l in zip(starts, lens)]).astype(np.uint8)
    seqs[rng.random(seqs.size) < 0.01] = ord("N")
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    dseqs, doffs = oracle_mod.digest_batch(kind, k, w, seqs, offs)
    want_l, want_d = orc.pml(dseqs, doffs.astype(np.int64), want_docs=True)
    want_ms = orc.ms(dseqs, doffs.astype(np.int64), want_docs=True)
    f, a, b, sm = oracle_mod.classify(want_l, doffs.astype(np.int64), 5, 2)
    total_in, tot = int(offs[-1]), int(doffs[-1])
    d_seqs = torch.zeros(total_in + 64, dtype=torch.uint8, device="cuda")
    d_seqs[:total_in] = torch.from_numpy(seqs).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    ix.set_option("digest_parked", 2)
    for vt in (torch.int16, torch.int32):
        d_len = torch.full((total_in + 8,), -1, dtype=vt, device="cuda")
        d_doc = torch.full((total_in + 8,), -1, dtype=vt, device="cuda")
        d_cls = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
        d_oo, _ = ix.digest_query_device(capi.SPX_MODE_PML, kind, k, w, d_seqs, d_offs, total_in, d_lengths=d_len, d_docs=d_doc,
                                         d_class=d_cls, bin_width=5, max_value_thr=2)
        torch.cuda.synchronize()
        assert np.array_equal(d_oo.cpu().numpy().astype(np.uint64), doffs)
        mask = 0xffff if vt == torch.int16 else 0xffffffff
        assert np.array_equal(d_len[:tot].cpu().numpy().astype(np.int64) & mask, want_l.astype(np.int64))
        assert np.array_equal(d_doc[:tot].cpu().numpy().astype(np.int64) & mask, want_d.astype(np.int64))
        cls = d_cls.cpu().numpy().view(capi.CLASS_DTYPE).reshape(-1)
        assert np.array_equal(cls["above"], a) and np.array_equal(cls["sum_max"], sm)
    d_ptr = torch.zeros(total_in + 8, dtype=torch.int64, device="cuda")
    d_doc = torch.zeros(total_in + 8, dtype=torch.int32, device="cuda")
    ix.digest_query_device(capi.SPX_MODE_MS, kind, k, w, d_seqs, d_offs, total_in, d_pointers=d_ptr, d_docs=d_doc)
    torch.cuda.synchronize()
    assert np.array_equal(d_ptr[:tot].cpu().numpy().view(np.uint64), want_ms["pointers"])
    assert np.array_equal(d_doc[:tot].cpu().numpy().view(np.uint32), want_ms["docs"])


def test_chunked_batch_with_fallback_reads_between_dynamic_batches(oracle_mod, stat_case):
    """One index, three calls: a batch dealt on demand, a long-read batch that takes the chunked walk and leaves reads to the
    plain walk (chunks of 32 characters: a third of the reads keep a seam open through every round), the first batch again.
    The chunked call's passes and its fallback share the call's counters with the claim word: the fallback count and the
    statistics are what they were, and the batch after it is dealt from a zeroed word."""
    raw, pool = stat_case
    orc = oracle_mod.OracleIndex.from_raw(raw.cpu())
    rng = np.random.default_rng(8)
    s_seqs, s_offs = _batch(pool, rng.integers(0, 40, size=_nlanes() + CLAIM + 30))
    l_seqs, l_offs = synth.simulate_reads(raw, 300, 2200, seed=16)
    l_seqs, l_offs = l_seqs.cpu().numpy(), l_offs.cpu().numpy()
    want_s = orc.pml(s_seqs, s_offs, want_docs=True)
    want_l = orc.pml(l_seqs, l_offs, want_docs=True)
    ix = capi.Index.from_raw(raw, 0)
    ix.set_option("waves_per_cu", 4)
    stats = []
    for seqs, offs, want, chunked in ((s_seqs, s_offs, want_s, False), (l_seqs, l_offs, want_l, True), (s_seqs, s_offs, want_s, False)):
        ix.set_option("chunk_mode", 2 if chunked else 1)
        ix.set_option("chunk_shift", 5)
        for bits in (32, 16):
            got = ix.query_host(capi.SPX_MODE_PML, seqs, offs, want_docs=True, classify=(7, 3), bits=bits)
            assert np.array_equal(got["lengths"], want[0]) and np.array_equal(got["docs"], want[1])
            f, a, b, s = oracle_mod.classify(want[0], offs, 7, 3)
            assert np.array_equal(got["class"]["above"], a) and np.array_equal(got["class"]["sum_max"], s)
        st = ix.last_stats()
        st.pop("kernel_ms")
        cs = ix.last_chunk_stats()
        if chunked:
            assert cs["chunk_len"] == 32 and 0 < cs["fallback_reads"] < 300
            assert int(offs[-1]) <= st["steps"] <= int(offs[-1]) + cs["fallback_reads"] * 2200
        else:
            assert cs["chunk_len"] == 0 and cs["fallback_reads"] == 0 and st["steps"] == int(offs[-1])
        stats.append(st)
    assert stats[0] == stats[2]
