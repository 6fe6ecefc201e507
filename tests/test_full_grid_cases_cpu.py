"""CPU tier of tests/test_gpu_full_grids.py: every case of tests/grid_cases.py is built, is in the regime it exists for
(`reaches`, on the references' answers alone), stays within the cells a case may spend, and its references within their
time.  No device and no library: what fails here is the batch, not a kernel."""
import numpy as np
import pytest
import torch

from spumoni_amd import synth
from tests import grid_cases as gc


@pytest.mark.parametrize("name", gc.NAMES)
def test_the_case_reaches_its_regime_within_the_budget(name):
    c = gc.case(name)
    c.reaches()
    print(f"{name}: {c.cells} cells, references {c.seconds:.2f} s")
    assert c.cells <= gc.MAX_CELLS and c.seconds <= gc.MAX_SECONDS, (name, c.cells, c.seconds)
    if "align" in c.product or c.product == "cigar":
        gaps = c.align[2]  # the count from the gap table: a * b of every filled gap with a table
        a, b = gaps["a"].astype(np.int64), gaps["b"].astype(np.int64)
        tabled = (gaps["edits"] != gc.UNFILLED) & (a >= 1) & (b >= 1) & ~((a == 1) & (b == 1))
        assert int((a * b)[tabled].sum()) == c.cells


def test_the_host_batch_reaches_its_regime_within_the_budget(oracle_mod):
    """The GPU module indexes the text with capi.build_raw; here synth.index_from_text stands in (the same index)."""
    T, seqs, offs = gc.host_batch()
    raw = synth.index_from_text(torch.from_numpy(T.copy()))
    c = gc.host_expectation(oracle_mod, raw, T, seqs, offs)
    c.reaches()
    print(f"host forms: {c.cells} cells, oracle and references {c.seconds:.2f} s")
    assert c.cells <= gc.MAX_CELLS and c.seconds <= gc.MAX_SECONDS, (c.cells, c.seconds)


def test_the_vectorised_chain_batch_is_the_kind_that_the_chain_module_crafts():
    """chain_batch restates tests/test_gpu_chain.py's _batch without the loop: x sorted inside a read, records in front of
    and behind the batch, reads of every count, and chains that follow the diagonal through most of a read's anchors."""
    rng = np.random.default_rng(0)
    counts = np.array([0, 1, 6, 0, 17, 200, 3])
    offs, rec, D = gc.chain_batch(rng, counts, front=2, n_docs=3)
    assert offs.tolist() == [2, 2, 3, 9, 9, 26, 226, 229] and rec.size == 232 and D.size == 232
    for o, e in zip(offs[:-1].astype(int), offs[1:].astype(int)):
        assert (np.diff(rec["read_pos"][o:e].astype(np.int64)) >= 0).all()
    chains, _, _ = gc.chain_reference(offs, rec)
    assert int(chains["anchors"][5]) > 64 and int(chains["anchors"][4]) > 8
