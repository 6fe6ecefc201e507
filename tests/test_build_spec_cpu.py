"""The specification of the index, synth.index_from_text (which builds the indexes of nearly every other test, of the
oracle's known-answer tests and of bench.py), held on the CPU to first principles: tests/brute_index.c -- qsort over
the suffixes, LCP by characters, every field by a loop -- over the catalogue of tests/build_cases.py, after the C
reference itself is held to the Python restatement on small texts and run under ASan / UBSan as a program."""
import os
import subprocess

import numpy as np
import pytest
import torch

from spumoni_amd import synth
from tests import brute, build_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_as_python(text, docs):
    want = brute._brute_spec(text, docs)
    got = brute.BruteIndex(np.asarray(text, dtype=np.uint8), docs)
    t = list(text) + [0]
    sa = brute.naive_sa(t)
    assert got.n == len(t) and got.sa.tolist() == sa and got.lcp.tolist() == brute.naive_lcp(t, sa), (text, docs)
    for f, v in want.items():
        assert getattr(got, f).tolist() == v, (text, docs, f)


def test_c_reference_is_the_python_restatement_on_every_small_binary_text():
    for length in range(1, 10):
        for code in range(1 << length):
            text = [2 + ((code >> i) & 1) for i in range(length)]
            _same_as_python(text, [length] if length < 3 else [1, length - 2, 1])


def test_c_reference_is_the_python_restatement_on_random_texts():
    rng = np.random.default_rng(2024)
    for trial in range(100):
        sigma = (1, 2, 4, 16, 254)[trial % 5]
        length = int(rng.integers(1, 201))
        text = (2 + rng.integers(0, sigma, size=length)).tolist()
        cuts = sorted(rng.integers(0, length + 1, size=int(rng.integers(0, 5))).tolist())  # empty documents too
        _same_as_python(text, np.diff([0] + cuts + [length]).tolist())


def test_c_reference_refuses_what_it_cannot_answer():
    ok = np.frombuffer(b"ACGT", dtype=np.uint8)
    for text, docs in ((np.zeros(0, dtype=np.uint8), None), (np.array([65, 1, 66], dtype=np.uint8), None), (ok, [1, 2])):
        with pytest.raises(ValueError):
            brute.BruteIndex(text, docs)


def test_c_reference_under_sanitizers(tmp_path):
    """The stand-alone program (-DBRUTE_INDEX_MAIN) under ASan and UBSan: texts with empty documents, one character,
    one letter, a refused byte.  The checksum is the unsanitised build's: the sanitizers change nothing it computes."""
    src = os.path.join(ROOT, "tests", "brute_index.c")
    out = {}
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / f"brute_index_{name}")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-DBRUTE_INDEX_MAIN"] + flags + ["-o", exe, src], check=True)
        p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        assert "brute index ok" in p.stdout and not p.stderr, p.stdout + p.stderr
        out[name] = p.stdout
    assert out["plain"] == out["san"]


@pytest.mark.parametrize("case", build_cases.CASES, ids=lambda c: c.name)
def test_specification_is_the_c_reference(case):
    text, docs, samples, ref = build_cases.reference(case)
    assert not case.unmet(ref), "the case does not reach what it is for"
    got = synth.index_from_text(torch.from_numpy(text), doc_lengths=docs, with_samples=samples)
    assert ref.mismatches(got) == []


@pytest.mark.parametrize("name", build_cases.TOLD_FROM_DNA)
def test_reaches_tells_its_text_from_random_dna(name):
    case = build_cases.BY_NAME[name]
    text, docs, samples, ref = build_cases.reference(case)
    assert case.reaches(ref)
    dna = brute.BruteIndex(build_cases.random_dna(text.size, 1), docs, samples)
    assert not case.reaches(dna), "random DNA of the same length reaches it too: the condition asserts nothing"


def test_catalogue_holds_what_it_lists():
    names = set(build_cases.BY_NAME)
    for p in build_cases.SIZE_POINTS:
        for n in (p - 1, p, p + 1):
            assert {f"size_dna_{n}", f"size_binary_{n}"} <= names
    assert {f"size_dna_{(1 << 20) + d}" for d in (-1, 0, 1)} <= names
    assert sorted(build_cases.reference(build_cases.BY_NAME[f"tail_{j}"])[3].n % 8 for j in range(8)) == list(range(8))
    for ell in build_cases.REPEAT_LENGTHS:
        assert f"repeat_{ell}" in names and (ell < 4095 or f"repeat_{ell}_at_border" in names)
    sizes = [build_cases.reference(c)[0].size for c in build_cases.CASES]
    assert max(sizes) <= 1_050_000 and min(sizes) == build_cases.reference(build_cases.SMALLEST)[0].size
    assert max(sizes) == build_cases.reference(build_cases.LARGEST)[0].size
