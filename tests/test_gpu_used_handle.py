"""-m gpu: every query entry point on a handle that has been used, against the oracle.

A worker keeps one spx_index for hours and feeds it batches whose size, read lengths, walk and mode change from call to call,
while the handle's sixty grow-only scratch buffers keep whatever the last call left in them: a kernel that reads a flag, a
seam record, a tile table or a bitmap that no kernel of the SAME call wrote gets a plausible value of the call before.  A
fresh handle hides that (fresh device memory is very often zero), and so does repeating one batch.  tests/handle_steps.py
holds the catalogue: some fifty steps -- every host and device form of the query, the chunked walk, digestion, digest +
query, the text path, the votes, the matches -- each with the oracle's expectation and with a dirtier, the call chosen from
the code to leave more bytes and other content in exactly the scratch the step uses.  Here the steps run in four orders:

(a) alone on a fresh handle (the catalogue is right);
(b) dirtier, step and step, dirtier on one handle;
(c) the step on all, an eighth and a half of its reads, in that order, on one handle (scratch larger, then smaller than needed);
(d) seeded permutations of the whole catalogue, each step with its dirtier, on one set of handles from start to end -- odd
    seeds on same-device clones whose sources run the catalogue between the clones' calls, in this thread
    (SPX_HANDLE_FIRST / SPX_HANDLE_SEEDS for longer sweeps).

THE PROMISE UNDER TEST in (b) and (d) is the header's "queries on one index are serialised internally": the calls of a group
are enqueued back to back, the device forms rotating over torch's current stream and two others, the host forms on the
handle's own stream, and the test does not wait between one call and the next -- their inputs and outputs are separate
tensors, only the handle's state is shared, so the library's own event waits decide the results.  The test synchronises only
for its own data: once after the uploads, and per step before it reads the results back.

Every value of every output is compared.  Device outputs sit between 64-byte fences that must come back untouched; each test
asserts the path the library reports (chunk size and fallbacks, row encoding, reads per vote path, matches)."""
import os

import pytest
import torch

from spumoni_amd import capi
from tests import handle_steps as hs

pytestmark = pytest.mark.gpu

_FIRST = int(os.environ.get("SPX_HANDLE_FIRST", "0"))
_COUNT = int(os.environ.get("SPX_HANDLE_SEEDS", "4"))
STEPS = range(hs.N_STEPS)


@pytest.fixture(scope="module")
def cat(oracle_mod):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    capi.lib()
    return hs.build(oracle_mod)


def test_the_catalogue_and_its_pairs(cat):
    """as many steps as the parametrised tests run, no batch above 40 000 characters, every dirtier 4 to 10 times its step and
    different from it in the way the pair was chosen for"""
    assert len(cat.steps) == hs.N_STEPS
    assert cat.check_claims() == hs.N_STEPS
    assert {s.form for s in cat.every()} == {"host", "device"}


@pytest.mark.parametrize("i", STEPS)
def test_fresh_handle(cat, i):
    hs.run_fresh(cat, cat.every()[i])


@pytest.mark.parametrize("i", STEPS)
def test_dirtier_then_step_and_step_then_dirtier(cat, i):
    hs.run_pair(cat, cat.every()[i])


@pytest.mark.parametrize("i", STEPS)
def test_large_small_medium(cat, i):
    hs.run_sizes(cat, cat.every()[i])


@pytest.mark.parametrize("seed", range(_FIRST, _FIRST + _COUNT))
def test_random_sequence_on_one_set_of_handles(cat, seed):
    assert hs.run_sequence(cat, seed) >= 2 * hs.N_STEPS
