"""Matching statistics from first principles, without a GPU: tests/brute_ms.c is held to the definition itself
(brute.true_ms) on small inputs and run under ASan / UBSan as a program; every case of tests/ms_cases.py reaches what it
is for; the oracle (tiers T2 and T1) owes the catalogue what tests/test_gpu_ms_math.py asks of
the HIP path -- lengths equal to the true MS, pointers that name an occurrence, PML <= MS; and three deliberately wrong
copies of the oracle, built into a temporary directory, show that these assertions bite.

The wrong copies (each in a child process: a wrong walk may read out of range), what fails them here and whether the
old known-answer test (test_oracle_kat.py::test_ms_lengths_equal_bruteforce_matching_statistics, six texts of 33 .. 257
characters) fails them too -- asserted below, so the note stays true:
  unchanged      the control: fails nothing
  pos_le_thr     `pos < thr` as `pos <= thr` in the four query loops
  no_carry       the `l - 1` carried from one position to the next dropped (l = 0)
  start_sample   samples_start of every run one too large
When written, each of the three failed every case of the catalogue (lengths that differ from the matching statistics;
asserted for the one case named in WRONG_FAILS, the count is printed), and the old
test fails each of them as well, on five of its six texts (all but the one-letter text of 33 characters): none of these
three mistakes needed the larger cases to be seen.
"""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import brute, ms_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C reference against the definition ---------------------------------------------------------------------------
def _ms_of(text, reads):
    text = np.asarray(text, dtype=np.uint8)
    ref = brute.BruteIndex(text)
    seqs, offs = ms_cases.batch([np.asarray(r, dtype=np.uint8) for r in reads])
    got = brute.brute_ms(text, ref.sa, seqs, offs)
    return [got[offs[q]: offs[q + 1]].tolist() for q in range(len(reads))]


def test_c_reference_is_the_definition_on_every_small_binary_input():
    reads = [[2 + ((code >> i) & 1) for i in range(m)] for m in range(0, 7) for code in range(1 << m)]
    for length in range(1, 10):
        for code in range(1 << length):
            text = [2 + ((code >> i) & 1) for i in range(length)]
            for rd, g in zip(reads, _ms_of(text, reads)):
                assert g == brute.true_ms(text, rd), (text, rd)


def test_c_reference_is_the_definition_on_random_inputs():
    rng = np.random.default_rng(2025)
    for trial in range(200):
        sigma = 1 + trial % 5
        length = int(rng.integers(1, 201))
        text = (2 + rng.integers(0, sigma, size=length)).astype(np.uint8)
        reads = []
        for _ in range(4):
            m = int(rng.integers(0, 60))
            if rng.random() < 0.5 and length > 1:
                s = int(rng.integers(0, length))
                rd = text[s: s + m].copy()
                if rd.size and rng.random() < 0.7:
                    rd[rng.integers(0, rd.size)] = 2 + rng.integers(0, sigma + 1)  # sometimes a letter the text lacks
            else:
                rd = (2 + rng.integers(0, sigma + 1, size=m)).astype(np.uint8)
            reads.append(rd)
        reads.append(text.copy())
        for rd, g in zip(reads, _ms_of(text, reads)):
            assert g == brute.true_ms(text.tolist(), rd.tolist()), (text.tolist(), rd.tolist())


def test_c_reference_refuses_what_it_cannot_answer():
    text = np.frombuffer(b"GATTACA", dtype=np.uint8)
    sa = brute.BruteIndex(text).sa
    seqs, offs = ms_cases.batch([text[:3]])
    with pytest.raises(ValueError):
        brute.brute_ms(text, sa[:-1], seqs, offs)
    twice = sa.copy()
    twice[3] = twice[2]
    with pytest.raises(ValueError):
        brute.brute_ms(text, twice, seqs, offs)
    with pytest.raises(ValueError):
        brute.brute_ms(text, sa, seqs, np.array([0, 3, 2]))


def test_c_reference_under_sanitizers(tmp_path):
    """The stand-alone program (-DBRUTE_MS_MAIN) under ASan and UBSan; it checks every value against a scan of all text
    positions itself.  The checksum is the unsanitised build's."""
    out = {}
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / f"brute_ms_{name}")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-DBRUTE_MS_MAIN"] + flags + ["-o", exe, brute.BRUTE_MS_C], check=True)
        p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        assert "brute ms ok" in p.stdout and not p.stderr, p.stdout + p.stderr
        out[name] = p.stdout
    assert out["plain"] == out["san"]


# ---- the catalogue ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ms_cases.CASES, ids=lambda c: c.name)
def test_case_reaches_what_it_is_for(case):
    text, _, ref, _, _, ms = ms_cases.reference(case)
    assert case.unmet(text, ref.sa, ref.lcp, ms) == []


def test_catalogue_holds_what_it_lists():
    sizes = {c.name: ms_cases.reference(c)[0].size for c in ms_cases.CASES}
    assert {sizes[f"repetitive_{n}"] for n in (4096, 65535, 65536, 65537)} == {4096, 65535, 65536, 65537}
    assert sorted({sizes[f"tail_{j}_suffix_1"] % 8 for j in range(8)}) == list(range(8))
    assert all(f"tail_{j}_suffix_{k}" in sizes for j in range(8) for k in ms_cases.SUFFIXES)
    assert max(sizes.values()) <= 100_000
    longest = {c.name: int(np.diff(c.reads()[1]).max()) for c in ms_cases.CASES}
    assert set(ms_cases.LONG_READS) == {name for name, m in longest.items() if m >= 1000}
    assert {"whole_text_65535", "whole_text_65534_and_a_letter", "whole_text_and_a_letter", "match_of_66000"} <= set(ms_cases.LONG_READS)
    assert longest["whole_text_65535"] == longest["whole_text_65534_and_a_letter"] == 65535 and longest["whole_text_and_a_letter"] == 65536


@pytest.mark.parametrize("case", ms_cases.CASES, ids=lambda c: c.name)
def test_oracle_owes_the_mathematics(oracle_mod, case):
    text, _, ref, seqs, offs, ms = ms_cases.reference(case)
    assert case.reaches(text, ref.sa, ref.lcp, ms), "the case does not reach what it is for"
    raw = ms_cases.raw_index(ref)
    orc = oracle_mod.OracleIndex.from_raw(raw)
    res = orc.ms(seqs, offs, text=text)
    compared = ms_cases.check_answers(case, res["lengths"], res["pointers"], pml=orc.pml(seqs, offs))
    assert compared >= 0.8 * ms.size
    if case.name in ms_cases.UNIQUE_SUFFIX:
        assert ms_cases.last_suffix_ends_the_text(case, res["lengths"], res["pointers"])
    # tier T1 returns pointers only, and the lengths follow from them and the text: its pointers are T2's, checked above,
    # so what T1 adds is its own PML against the mathematics
    t1 = oracle_mod.OracleT1Index.from_raw(raw)
    assert np.array_equal(t1.ms(seqs, offs)["pointers"], res["pointers"])
    assert (t1.pml(seqs, offs).astype(np.int64) <= ms).all()


# ---- the assertions bite --------------------------------------------------------------------------------------------------
WRONG = {
    "unchanged": ("spumoni_oracle.c", "l = (l == 0 ? 0 : (l - 1));", "l = (l == 0 ? 0 : (l - 1));", 1),  # the control
    "pos_le_thr": ("orc_queries.inc", "if (pos < thr) {", "if (pos <= thr) {", 4),
    "no_carry": ("spumoni_oracle.c", "l = (l == 0 ? 0 : (l - 1));", "l = 0;", 1),
    "start_sample": ("spumoni_oracle.c", "#define Q_SAMPLE_START(ix, k) ((ix)->samples_start[(k)])",
                     "#define Q_SAMPLE_START(ix, k) ((ix)->samples_start[(k)] + 1)", 1),
}
# (the case that must fail, whether the old known-answer test fails the copy too)
WRONG_FAILS = {"unchanged": (None, False), "pos_le_thr": ("binary_tied_minima", True), "no_carry": ("match_of_66000", True),
               "start_sample": ("repetitive_65536", True)}

_CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])   # the wrong copy of oracle/ comes first
sys.path.insert(1, sys.argv[2])
import numpy as np
import oracle
assert oracle.__file__.startswith(sys.argv[1])
oracle.build()
from tests import ms_cases, test_oracle_kat
out = {"cases": {}, "kat": []}
for case in ms_cases.CASES:
    text, _, ref, seqs, offs, ms = ms_cases.reference(case)
    orc = oracle.OracleIndex.from_raw(ms_cases.raw_index(ref))
    res = orc.ms(seqs, offs, text=text)
    try:
        ms_cases.check_answers(case, res["lengths"], res["pointers"], pml=orc.pml(seqs, offs))
    except AssertionError as e:
        out["cases"][case.name] = str(e.args[0][1]) if e.args and isinstance(e.args[0], tuple) else "failed"
for seed, n, letters in test_oracle_kat.CASES:
    try:
        test_oracle_kat.test_ms_lengths_equal_bruteforce_matching_statistics(oracle, seed, n, letters)
    except AssertionError:
        out["kat"].append(n)
print("RESULT " + json.dumps(out))
'''


def run_wrong_copy(name, tmp_path):
    """Builds the copy `name` of oracle/ with its one change and runs the catalogue and the old known-answer test on it in a
    child process.  Returns {"cases": {failed case: what}, "kat": [text sizes the old test failed]}."""
    fname, old, new, count = WRONG[name]
    d = tmp_path / name / "oracle"
    os.makedirs(d)
    for f in os.listdir(os.path.join(ROOT, "oracle")):
        if f.endswith((".c", ".h", ".inc", ".py")) or f == "Makefile":
            shutil.copy(os.path.join(ROOT, "oracle", f), d / f)
    src = (d / fname).read_text()
    assert src.count(old) == count, (name, "the line to change is not where it was")
    (d / fname).write_text(src.replace(old, new))
    p = subprocess.run([sys.executable, "-c", _CHILD, str(tmp_path / name), ROOT], capture_output=True, text=True, timeout=600, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert p.returncode == 0 and lines, (name, p.returncode, p.stdout[-1500:], p.stderr[-1500:])
    return json.loads(lines[-1][7:])


@pytest.mark.parametrize("name", sorted(WRONG))
def test_wrong_oracle_copy_fails(name, tmp_path):
    got = run_wrong_copy(name, tmp_path)
    must_fail, kat = WRONG_FAILS[name]
    print(name, "fails", len(got["cases"]), "cases; old known-answer test fails on texts of", got["kat"])
    if must_fail is None:
        assert got["cases"] == {}, got
    else:
        assert must_fail in got["cases"], got  # (how many more fail is printed above, not part of the contract)
    assert bool(got["kat"]) == kat, got
