"""The HIP index builder (include/spumoni_build.h) on the device: every field bit-identical to the
specification synth.index_from_text, brute force on small texts, the catalogue of tests/build_cases.py against the
first-principles reference tests/brute_index.c, a build past 2^31 characters, build_index through it, and its refusals."""
import os

import numpy as np
import pytest
import torch

from spumoni_amd import build_index, capi, synth
from tests import brute, build_cases, cases

pytestmark = pytest.mark.gpu

FIELDS = ("heads", "lens", "thr", "ssa", "esa", "doc_start", "doc_end")


def _same(got, want, what=""):
    assert got.n == want.n, what
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert (a is None) == (b is None), (what, f)
        if a is not None:
            assert torch.equal(a.cpu().to(torch.int64), b.cpu().to(torch.int64)), (what, f)


def _check(text, doc_lengths=None, with_samples=True, spec_device="cuda"):
    text = np.ascontiguousarray(text, dtype=np.uint8)
    got = capi.build_raw(text, doc_lengths=doc_lengths, with_samples=with_samples)
    want = synth.index_from_text(torch.from_numpy(text).to(spec_device), doc_lengths=doc_lengths,
                                 with_samples=with_samples).cpu()
    _same(got, want, (text.size, None if doc_lengths is None else len(doc_lengths), with_samples))
    assert np.array_equal(got.text.numpy(), text)
    return got


def _check_brute(text, doc_lengths):
    got = capi.build_raw(np.asarray(text, dtype=np.uint8), doc_lengths=doc_lengths)
    want = brute._brute_spec(text, doc_lengths)
    assert got.n == len(text) + 1
    for f, v in want.items():
        assert getattr(got, f).tolist() == v, (bytes(text), doc_lengths, f)


def test_brute_force_every_small_binary_text():
    for length in range(1, 11):
        for code in range(1 << length):
            text = [2 + ((code >> i) & 1) for i in range(length)]
            docs = [length] if length < 3 else [1, length - 2, 1]
            _check_brute(text, docs)


@pytest.mark.parametrize("sigma", [1, 2, 4, 16, 253])
def test_brute_force_random_texts(sigma):
    rng = np.random.default_rng(sigma)
    for trial in range(25):
        length = int(rng.integers(1, 201))
        text = (2 + rng.integers(0, sigma, size=length)).tolist()
        cuts = sorted(set(rng.integers(1, length, size=min(3, length - 1)).tolist())) if length > 1 else []
        docs = np.diff([0] + cuts + [length]).tolist()
        _check_brute(text, docs)


def _check_case(case):
    """capi.build_raw against the C reference alone, after the reference shows that the case reaches its path."""
    text, docs, samples, ref = build_cases.reference(case)
    assert not case.unmet(ref), "the case does not reach what it is for"
    got = capi.build_raw(text, doc_lengths=docs, with_samples=samples)
    assert ref.mismatches(got) == []
    assert np.array_equal(got.text.numpy(), text)


@pytest.mark.parametrize("case", build_cases.CASES, ids=lambda c: c.name)
def test_catalogue_against_first_principles(case):
    _check_case(case)


def test_largest_case_directly_after_the_smallest():
    """One process, no other build in between: nothing of a build of 62 characters may be left for one of 2^20."""
    for case in (build_cases.SMALLEST, build_cases.LARGEST, build_cases.SMALLEST):
        _check_case(case)


@pytest.mark.parametrize("kind", ["one_letter", "alternating", "byte_255", "single"])
def test_edge_texts(kind):
    text = {
        "one_letter": np.full(100_000, 65, dtype=np.uint8),  # the LCP's worst case: every PLCP chunk starts long
        "alternating": np.tile(np.array([67, 71], dtype=np.uint8), 30_000),
        "byte_255": np.full(5_000, 255, dtype=np.uint8),
        "single": np.array([84], dtype=np.uint8),
    }[kind]
    for with_samples in (True, False):
        _check(text, doc_lengths=[text.size] if with_samples else None, with_samples=with_samples)


def _docs(n, k, rng):
    if k == 1:
        return [n]
    cuts = sorted(rng.choice(np.arange(1, n), size=k - 1, replace=False).tolist())
    return np.diff([0] + cuts + [n]).tolist()


@pytest.mark.parametrize("what", ["repetitive", "real_case", "random_dna"])
def test_bit_identical_to_the_specification(what):
    rng = np.random.default_rng(7)
    if what == "repetitive":
        text = cases.repetitive_text(rng, 300_000, list(range(2, 256)))
    elif what == "real_case":
        _, text = cases.real_case(5, 200_000, list(b"ACGT"))
    else:
        text = synth.random_genome(1_000_000, seed=3)
    for k in (1, 3, 200):
        _check(text, doc_lengths=_docs(text.size, k, rng))
    _check(text, doc_lengths=None, with_samples=True)
    _check(text, doc_lengths=None, with_samples=False)


def _haplotypes(genome_bp, count, seed=1):
    base = synth.random_genome(genome_bp, seed=seed)
    return [base] + [synth.mutate(base, seed=sd) for sd in range(seed + 1, seed + count)]


def test_bit_identical_digested_pangenome():
    """The text of bench.py's real_bwt_digest_walk leg: 10 haplotypes of a 20 Mbp genome (+ reverse complements),
    promoted-minimizer digested (k = 4, w = 11)."""
    dig = capi.digester(0)
    parts = []
    for g in _haplotypes(20_000_000, 10):
        for seq in (g, synth.revcomp(g)):
            d, _ = dig.digest_host(capi.SPX_DIGEST_PROMOTED, 4, 11, seq, np.array([0, seq.size], dtype=np.uint64))
            parts.append(d.copy())
    dig.close()
    text = np.concatenate(parts)
    rng = np.random.default_rng(11)
    for k, samples in ((1, False), (3, True), (200, True)):
        _check(text, doc_lengths=_docs(text.size, k, rng) if samples else None, with_samples=samples)
        torch.cuda.empty_cache()


def test_bit_identical_undigested_pangenome():
    """About 3 * 10^8 characters: 8 haplotypes of a 19 Mbp genome and their reverse complements, one document each."""
    text, doc_lengths = synth.pangenome_text(_haplotypes(19_000_000, 8))
    _check(text, doc_lengths=doc_lengths)
    torch.cuda.empty_cache()


def _need_big_device():
    free, total = torch.cuda.mem_get_info(0)
    if total < 250e9:
        pytest.skip(f"the device has {total / 1e9:.0f} GB in all; a build of 2.2 * 10^9 characters is tested on >= 250 GB")
    if free < 120e9:
        pytest.fail(f"the device is busy: {free / 1e9:.0f} of {total / 1e9:.0f} GB free; this process holds "
                    f"{torch.cuda.memory_reserved(0) / 1e9:.1f} GB through torch, other processes the rest")


def test_build_past_2_to_the_31(oracle_mod):
    """n ~ 2.2 * 10^9 (where the torch builder does not fit): the structure of the arrays, the text rebuilt from the MS
    index built over them, and MS / PML of 10^4 reads against the oracle."""
    _need_big_device()
    genome_bp = 110_000_000
    text, doc_lengths = synth.pangenome_text(_haplotypes(genome_bp, 10, seed=31))
    assert text.size > 2**31
    raw = capi.build_raw(text, doc_lengths=doc_lengths)
    n, r = raw.n, raw.r
    assert n == text.size + 1
    lens = raw.lens.numpy()
    heads = raw.heads.numpy()
    assert int(lens.sum()) == n and (lens > 0).all()
    assert (heads[1:] != heads[:-1]).all() and int((heads == 0).sum()) == 1
    starts = np.cumsum(lens) - lens
    order = np.argsort(heads, kind="stable")
    hs = heads[order]
    first = np.ones(r, dtype=bool)
    first[1:] = hs[1:] != hs[:-1]
    thr = raw.thr.numpy()[order]
    assert (thr[first] == 0).all()
    lo = (starts + lens)[order[:-1]][~first[1:]]
    hi = starts[order[1:]][~first[1:]]
    t = thr[1:][~first[1:]]
    assert ((lo <= t) & (t <= hi)).all()
    for samp, doc in ((raw.ssa.numpy(), raw.doc_start.numpy()), (raw.esa.numpy(), raw.doc_end.numpy())):
        assert (samp < n).all()
        assert (np.diff(doc[np.argsort(samp, kind="stable")]) >= 0).all()
    del order, hs, first, thr, lo, hi, t, starts
    ix = capi.Index.from_raw(synth.RawIndex(heads=raw.heads, lens=raw.lens, thr=raw.thr, n=n, ssa=raw.ssa, esa=raw.esa,
                                            doc_start=raw.doc_start, doc_end=raw.doc_end), 0)
    ix.rebuild_text()
    assert np.array_equal(ix.text(), text)
    seqs, offs = synth.sample_reads(text, 10_000, 120, seed=5)
    orc = oracle_mod.OracleIndex.from_raw(raw)
    got = ix.query_host(capi.SPX_MODE_PML, seqs, offs)
    assert np.array_equal(got["lengths"], orc.pml(seqs, offs))
    w = orc.ms(seqs, offs, want_docs=True, text=text)
    g = ix.query_host(capi.SPX_MODE_MS, seqs, offs, want_docs=True)
    assert np.array_equal(g["pointers"], w["pointers"]) and np.array_equal(g["lengths"], w["lengths"])
    assert np.array_equal(g["docs"], w["docs"])
    ix.close()


def _fasta(path, name, seq):
    with open(path, "w") as f:
        f.write(f">{name}\n")
        s = seq.tobytes().decode()
        for i in range(0, len(s), 70):
            f.write(s[i: i + 70] + "\n")


def test_build_index_files_identical_to_the_torch_path(tmp_path, monkeypatch):
    g1 = synth.random_genome(40_000, seed=41)
    g2 = synth.mutate(g1, seed=42)
    g3 = synth.mutate(g1, seed=43)
    for name, g in (("a.fa", g1), ("b.fa", g2), ("c.fa", g3)):
        _fasta(tmp_path / name, name, g)
    (tmp_path / "list.txt").write_text(f"{tmp_path / 'a.fa'} 1\n{tmp_path / 'b.fa'} 2\n{tmp_path / 'c.fa'} 2\n")
    assert build_index.hip_builder_available()
    for flags in (["--doc"], ["--doc", "-m"]):
        out = {}
        for way in ("hip", "torch"):
            if way == "torch":
                monkeypatch.setattr(build_index, "hip_builder_available", lambda: False)
            d = tmp_path / (way + "".join(flags))
            build_index.main(["-l", str(tmp_path / "list.txt"), "-o", str(d / "idx")] + flags)
            monkeypatch.undo()
            out[way] = d
        names = sorted(os.listdir(out["hip"]))
        assert names == sorted(os.listdir(out["torch"])) and any(x.endswith(".thr_pos") for x in names)
        for x in names:
            assert open(out["hip"] / x, "rb").read() == open(out["torch"] / x, "rb").read(), (flags, x)


def _still_works():
    _check(np.frombuffer(b"GATTACAGATTACACATTAG", dtype=np.uint8), doc_lengths=[7, 13])


def test_one_document_past_the_limit_is_refused_by_name():
    """65 535 documents are built (build_cases.py: documents_65535); 65 536 are not."""
    text = np.full(70_000, 65, dtype=np.uint8)
    with pytest.raises(capi.SpxError, match="65536 documents: the builder takes 1 to 65535"):
        capi.build_raw(text, doc_lengths=[1] * 65_535 + [70_000 - 65_535])
    _check_case(build_cases.SMALLEST)


def test_refusals_leave_the_device_usable():
    ok = np.frombuffer(b"ACGTTGCAACGT", dtype=np.uint8)
    for text, docs, msg in ((np.frombuffer(b"ACG\x00T", dtype=np.uint8), None, "bytes must be >= 2"),
                            (np.frombuffer(b"AC\x01GT", dtype=np.uint8), None, "bytes must be >= 2"),
                            (ok, [5, 5], "sum to 10"),
                            (np.full(70_000, 65, dtype=np.uint8), [1] * 70_000, "1 to 65535")):
        with pytest.raises(capi.SpxError, match=msg):
            capi.build_raw(text, doc_lengths=docs)
        _still_works()
    # a build that does not fit in free memory is refused before it allocates anything
    free, _ = torch.cuda.mem_get_info(0)
    hold = torch.empty(max(0, free - (2 << 30)), dtype=torch.uint8, device="cuda:0")
    try:
        big = np.full(200_000_000, 67, dtype=np.uint8)
        with pytest.raises(capi.SpxError, match=r"does not fit on the device: it needs \d+ bytes .* \d+ bytes are free"):
            capi.build_raw(big)
    finally:
        del hold
        torch.cuda.empty_cache()
    _still_works()
