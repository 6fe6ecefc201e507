"""CPU tier: the catalogue of tests/handle_steps.py without a GPU.

What runs here validates the catalogue, the pair assertions and the comparison code -- the test's own machinery -- so that
they are right before anyone has a GPU: the pair assertions need the oracle alone; the host-form steps run in all four
orders of tests/test_gpu_used_handle.py in a subprocess that loads tests/fake_device (the C-ABI answered by the CPU oracle)
through SPUMONI_GPU_LIB; and the comparator and the fences are shown to report what they are there for.  It says nothing
about the HIP path: the stand-in library keeps no scratch between calls."""
import os
import subprocess
import sys

import pytest

from tests import handle_steps as hs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cat(oracle_mod):
    return hs.build(oracle_mod)


def test_every_pair_differs_the_way_it_was_chosen_for(cat):
    """no library: from the expected arrays -- resets per character 1.0 against < 0.05, matches per value 1.0 against reads /
    values, ...; the dirtier on the step's index, 4 to 10 times its characters, 400 000 at most; steps of 40 000 at most"""
    assert len(cat.steps) == hs.N_STEPS and cat.check_claims() == hs.N_STEPS
    for step in cat.every():
        big, small, medium = (step.resize(k).chars for k in step.sizes())
        assert big > medium > small, step.name  # the characters go down, then up


def test_the_comparator_and_the_fences_report_failures(cat):
    steps = cat.every()
    a = next(s for s in steps if s.name == "query_host PML 32 + docs + class")
    b = next(s for s in steps if s.name == "query_host PML 16 + class")
    hs.compare(a.name, a.want, a.want)
    with pytest.raises(hs.Mismatch, match="keys"):
        hs.compare(a.name, b.want, a.want)  # two steps' expectations swapped
    swapped = dict(a.want, **{"class": b.want["class"]})
    with pytest.raises(hs.Mismatch, match="class"):
        hs.compare(a.name, swapped, a.want)
    one_off = dict(a.want, lengths=a.want["lengths"].copy())
    one_off["lengths"][-1] ^= 1
    with pytest.raises(hs.Mismatch, match="lengths: 1 of"):
        hs.compare(a.name, one_off, a.want)
    for at in (0, hs.FENCE - 1, hs.FENCE + 3 * 16, hs.FENCE + 3 * 16 + hs.FENCE - 1):
        f = hs.HostFence("records", 3)
        f.out["above"] = 1
        f.values()
        f.buf[at] ^= 0x01  # one byte of the fence flipped
        with pytest.raises(hs.Mismatch, match="1 fence bytes written"):
            f.values()


SCRIPT = r'''
import oracle
from spumoni_amd import capi
from tests import handle_steps as hs

assert "fake-device" in capi.version()
cat = hs.build(oracle, device_forms=False, native_only=False)
steps = cat.every()
assert len(steps) >= 25 and all(s.form == "host" for s in steps)
cat.check_claims()
calls = 0
for s in steps:
    hs.run_fresh(cat, s, fake=True)
    hs.run_pair(cat, s, fake=True)
    hs.run_sizes(cat, s, fake=True)
for seed in range(4):
    calls += hs.run_sequence(cat, seed, fake=True)
# the self-check on what the library returned: another step's expectation, and a fence with one byte flipped
job = steps[0].prepare()
job.launch(cat.handle(steps[0].index), None)
got = job.collect()
hs.compare(steps[0].name, got, steps[0].want)
other = cat.steps["query_host PML 16 + class"]  # (the same reads, another call)
for wrong in (other.want, dict(got, docs=got["docs"][::-1].copy())):
    try:
        hs.compare(steps[0].name, got, wrong)
        raise SystemExit("the comparator let a wrong expectation pass")
    except hs.Mismatch:
        pass
f = hs.HostFence("records", 5)
f.buf[hs.FENCE + 5 * 16] ^= 0x80
try:
    f.values()
    raise SystemExit("the fence let a flipped byte pass")
except hs.Mismatch:
    pass
print("USED HANDLE OK", len(steps), "steps", calls, "calls in sequences")
'''


def test_host_steps_in_every_order_on_the_fake_device(fake_device, oracle_mod):
    env = dict(os.environ, SPUMONI_GPU_LIB=os.path.join(fake_device, "libspumoni_gpu.so"), PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", SCRIPT], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and "USED HANDLE OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
