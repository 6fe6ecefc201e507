"""The bin-max classifier's rule as a second opinion on the oracle (no GPU).

tests/test_gpu_classify.py holds every classifier path of the library to oracle.classify over bin widths up to 2^63 and
thresholds up to 2^64 - 1.  That expectation is only as good as orc_classify, whose `start_pos + bin_width` is size_t
arithmetic; here the rule of compute_ms_pml.cpp:969-995 is restated in plain Python integers (tests/cases.py:
classify_bins, classify_rule -- bins [k w, (k + 1) w), the last one takes the rest, one bin at least, above iff
max >= thr, sum of the maxima) and the oracle is held to it over the same grid, on random arrays and on the batch the
GPU tests use.  The conditions that batch has to meet are checked here as well, where no GPU is needed to see them fail."""
import numpy as np
import pytest

from tests import cases

W = cases.CLASSIFY_WIDTHS


@pytest.fixture(scope="module")
def batch(oracle_mod):
    raw, text, seqs, offs = cases.classify_case()
    orc = oracle_mod.OracleIndex.from_raw(raw)
    pml = orc.pml(seqs, offs)
    ms = orc.ms(seqs, offs, text=text)["lengths"]
    return offs, pml, ms


def _hold_oracle_to_the_rule(oracle_mod, lengths, offs, widths, thresholds):
    for w in widths:
        for thr in thresholds:
            f, a, b, s = oracle_mod.classify(lengths, offs, w, thr)
            want = cases.classify_rule(lengths, offs, w, thr)
            got = list(zip(a.tolist(), b.tolist(), s.tolist()))
            assert got == want, (w, thr)
            # FOUND iff more than half of the bins are above (:993); a read without bins is not found
            assert f.tolist() == [1 if x + y > 0 and 2 * x > x + y else 0 for x, y, _ in want], (w, thr)


def test_widths_and_thresholds_of_the_grid():
    """the grid is the issue's: the widths around 8, 64, 256, 512, a read's length, 2^16, 2^32; thresholds of 64 bits"""
    for w in (8, 64, 256, 512):
        assert {w - 1, w, w + 1} <= set(W)
        assert {2 * w - 1, 2 * w, 2 * w + 1} <= set(cases.CLASSIFY_LENGTHS) | set(W)
    assert {999, 1000, 1001, 65535, 65536, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63} <= set(W)
    thr, med, mx = cases.classify_thresholds(np.array([3, 9, 4, 100, 5], dtype=np.uint32))
    assert (med, mx) == (5, 100) and thr == [0, 1, 5, 100, 101, 65535, 65536, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 64) - 1]


@pytest.mark.parametrize("seed", range(4))
def test_oracle_classify_is_the_rule_on_random_arrays(oracle_mod, seed):
    """Random lengths arrays: small values, values around 2^16 and up to 2^32 - 1 (what a uint32 length can hold), reads
    of 0 .. 1300 values."""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 1300, size=24)
    m[:6] = [0, 1, 1000, 999, 1001, 513]
    offs = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
    lengths = rng.integers(0, 30, size=int(offs[-1])).astype(np.uint32)
    hit = rng.random(lengths.size) < 0.02
    lengths[hit] = rng.choice(np.array([65535, 65536, (1 << 32) - 1, 1 << 31, 70000], dtype=np.uint32), size=int(hit.sum()))
    thr, _, _ = cases.classify_thresholds(lengths)
    _hold_oracle_to_the_rule(oracle_mod, lengths, offs, W, thr + [7, 20])


@pytest.mark.parametrize("kind", ["pml", "ms"])
def test_oracle_classify_is_the_rule_on_the_gpu_tests_batch(oracle_mod, batch, kind):
    offs, pml, ms = batch
    lengths = pml if kind == "pml" else ms
    thr, _, _ = cases.classify_thresholds(lengths)
    _hold_oracle_to_the_rule(oracle_mod, lengths, offs, W, thr)


@pytest.mark.parametrize("kind", ["pml", "ms"])
def test_the_gpu_tests_batch_meets_its_conditions(oracle_mod, batch, kind):
    offs, pml, ms = batch
    lengths = pml if kind == "pml" else ms
    med, mx = cases.classify_conditions(oracle_mod, lengths, offs)
    assert 1 < med < mx < 65535  # (the thresholds of the grid are distinct, and the 16-bit entry points hold every value)
    m = np.diff(offs)
    assert all((m == x).sum() >= 2 for x in cases.CLASSIFY_LENGTHS)
    run3 = (m[:-2] == 0) & (m[1:-1] == 0) & (m[2:] == 0)  # three empty reads in a row start here
    assert run3[0] and run3[-1] and run3[10:-10].any()


def test_a_width_of_2_32_or_more_is_one_bin_like_2_32_minus_1(oracle_mod):
    """A read has fewer than 2^32 values, so the library may take any bin_width >= 2^32 as 2^32 - 1: the same bins for
    every m < 2^32 -- by the rule at the lengths where it could differ, and by the oracle on arrays."""
    top = (1 << 32) - 1
    for w in (1 << 32, (1 << 32) + 1, (1 << 32) + 7, 1 << 40, 1 << 63, (1 << 64) - 1):
        for m in (0, 1, 2, 1000, 1 << 31, top - 1, top):
            assert cases.classify_bins(m, w) == cases.classify_bins(m, top) == ([(0, m)] if m else [])
    assert len(cases.classify_bins(2 * top, top)) == 2 and len(cases.classify_bins(2 * top, 1 << 32)) == 1  # (not for longer ones)
    rng = np.random.default_rng(9)
    offs = np.array([0, 0, 1, 900, 2100], dtype=np.int64)
    lengths = rng.integers(0, 50, size=2100).astype(np.uint32)
    want = oracle_mod.classify(lengths, offs, top, 9)
    for w in (1 << 32, (1 << 32) + 1, (1 << 32) + 7, (1 << 32) + 64, 1 << 40, 1 << 63):
        got = oracle_mod.classify(lengths, offs, w, 9)
        assert all(np.array_equal(x, y) for x, y in zip(got, want)), w
    assert want[1].tolist() == [0, 1, 1, 1] and want[2].tolist() == [0, 0, 0, 0]
