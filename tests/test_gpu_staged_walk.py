"""-m gpu: the three products over one staged walk (spumoni_amd/csrc/spx_stage.hip) interleaved on ONE handle.

assign_host, mems_host and place_host share the handle's staging buffers, which grow under one another: a batch of 16-bit
values, then one with a read of 70 000 characters (32-bit values, every buffer grows), PML and MS, with and without ids,
with and without digestion.  Every call must return the bytes the same call returns on a fresh handle, and count what it
counts there.  Equality with the oracle is held by the tests of each product; this one is about state carried between
calls."""
import numpy as np
import pytest
import torch

from spumoni_amd import capi
from tests import cases

pytestmark = pytest.mark.gpu

DNA = list(b"ACGT")
K, W = 4, 11


@pytest.fixture(scope="module")
def gpu(built_all):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    capi.lib()
    return 0


def _assign(mode, batch, digest=None):
    def step(ix):
        rec = ix.assign_host(mode, batch[0], batch[1], 4, digest=digest)
        return [rec], ix.votes_stats()
    return step


def _mems(batch, digest=None, want_docs=False):
    def step(ix):
        out = ix.mems_host(batch[0], batch[1], 4, digest=digest, want_docs=want_docs)
        return list(out), ix.mems_stats()
    return step


def _place(batch, digest=None):
    def step(ix):
        out = ix.place_host(batch[0], batch[1], 4, digest=digest)
        return list(out), ix.place_stats()
    return step


@pytest.mark.parametrize("index_kind", [0, capi.SPX_DIGEST_DNA])
def test_three_products_interleaved_on_one_handle(gpu, oracle_mod, index_kind):
    rng = np.random.default_rng(70 + index_kind)
    genome = cases.repetitive_text(rng, 40_000, DNA)
    text = oracle_mod.digest(index_kind, K, W, genome) if index_kind else genome
    cuts = [text.size // 5, text.size // 2, text.size - text.size // 5 - text.size // 2]
    raw = capi.build_raw(text, doc_lengths=cuts)
    seqs, offs = cases.reads_mixed(rng, genome, DNA, 600, 500, [ord("N")])
    A = (seqs, offs.astype(np.uint64))
    # 50 reads, one of them of 70 000 characters: the values go to 32 bits and every buffer grows
    seqs, offs = cases.reads_mixed(rng, genome, DNA, 49, 500, [ord("N")])
    long_read = np.tile(genome, 2)[:70_000].copy()
    long_read[rng.integers(0, long_read.size, 200)] = ord("N")
    lens = np.r_[np.diff(offs)[:20], long_read.size, np.diff(offs)[20:]]
    B = (np.r_[seqs[: int(offs[20])], long_read, seqs[int(offs[20]):]], np.r_[0, np.cumsum(lens)].astype(np.uint64))
    assert B[1].size - 1 == 50 and int(np.diff(B[1].astype(np.int64)).max()) == 70_000
    dig = (capi.SPX_DIGEST_DNA, K, W)
    steps = [("assign MS A", _assign(capi.SPX_MODE_MS, A)), ("mems A docs", _mems(A, want_docs=True)), ("place A", _place(A)),
             ("place B", _place(B)), ("mems B", _mems(B)), ("assign PML B", _assign(capi.SPX_MODE_PML, B)),
             ("assign MS A digested", _assign(capi.SPX_MODE_MS, A, dig)), ("mems A digested docs", _mems(A, dig, want_docs=True)),
             ("place A digested", _place(A, dig)), ("mems A", _mems(A))]
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
    ix.close()
