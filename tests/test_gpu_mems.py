"""-m gpu: the matches (spumoni_amd/csrc/spx_mems.hip, include/spumoni_mems.h) against the definition
(spumoni_amd/mems.py: mems_reference), bit for bit.

mems_device gets crafted arrays (the expectation is mems_reference over the same arrays); mems_host and `spumoni mems`
are held to mems_reference over the ORACLE's MS lengths, pointers and document ids, or over the committed golden files
-- never over the library's own arrays.  The kernels work on 64-value words, a wavefront on 512 (16-bit) or 256 (32-bit)
values and a workgroup on four times that: the crafted reads end and start around each of those."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from spumoni_amd import capi, synth
from spumoni_amd.mems import MATCH_DTYPE, mems_reference
from tests import cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
FILES = os.path.join(ROOT, "tests", "golden", "files")
DNA = list(b"ACGT")
FENCE = -7


@pytest.fixture(scope="module")
def gpu(built_all):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    capi.lib()
    return 0


@pytest.fixture(scope="module")
def any_index(gpu):
    raw = synth.statistical_rlbwt(5000, 60, 4.0, seed=3, with_samples=True, n_docs=8)
    ix = capi.Index.from_raw(raw, 0)
    yield ix
    ix.close()


def _to_device(a, bits):
    dt, st = {16: (np.uint16, np.int16), 32: (np.uint32, np.int32), 64: (np.uint64, np.int64)}[bits]
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt).view(st).copy()).cuda()


def _records(t):
    return t.cpu().numpy().view(MATCH_DTYPE).reshape(-1)


def _run(ix, L, P, offs, min_length, bits, D=None, **kw):
    assert int(np.max(L, initial=0)) < (1 << bits) and (D is None or int(np.max(D, initial=0)) < (1 << bits))
    out = ix.mems_device(_to_device(L, bits), _to_device(P, 64), _to_device(offs, 64), min_length,
                         d_docs=None if D is None else _to_device(D, bits), **kw)
    torch.cuda.synchronize()
    return out


def _check(ix, L, P, offs, min_length, bits, D=None):
    got = _run(ix, L, P, offs, min_length, bits, D)
    want = mems_reference(L, P, offs, min_length, D)
    assert np.array_equal(got[0].cpu().numpy().view(np.uint64), want[0]), (bits, min_length)
    rec = _records(got[1])
    assert rec.size == want[1].size, (bits, min_length, rec.size, want[1].size)
    bad = np.flatnonzero(rec != want[1])
    assert bad.size == 0, (bits, min_length, bad[:5], rec[bad[:5]], want[1][bad[:5]])
    if D is not None:
        assert np.array_equal(got[2].cpu().numpy().view(np.uint32), want[2])
    st = ix.mems_stats()
    lo, hi = (int(offs[0]), int(offs[-1])) if len(offs) > 1 else (0, 0)
    assert st["values"] == hi - lo and st["matches"] == want[1].size and st["written"] == want[1].size, st
    assert st["longest"] == int(want[1]["length"].max(initial=0)), st
    return want


EDGES = [0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049]


def _pointers(rng, L):
    P = rng.integers(0, 1 << 40, L.size).astype(np.uint64)
    P[::7] += np.uint64(1 << 63)  # (all 64 bits travel)
    P[np.asarray(L) == 0] = np.uint64(2**64 - 1)
    return P


def _crafted(bits, kind, seed):
    """Reads of every length of the list (and, 32-bit, of 70 000 and 10^6 values) in a random order, twice, with runs of
    empty reads at the front, in the middle and at the end; offs[0] != 0; the values by `kind`."""
    rng = np.random.default_rng(seed)
    lens = EDGES * 2 + ([70_000, 1_000_000] if bits == 32 else [])
    lens = np.array(lens)[rng.permutation(len(lens))]
    lens = np.r_[[0, 0, 0], lens[:20], [0] * 5, lens[20:], [5, 0, 0, 61, 0, 0, 0, 0]]
    offs = (77 + np.r_[0, np.cumsum(lens)]).astype(np.uint64)
    tot = int(offs[-1]) + 9  # (values behind the batch, too)
    if kind == "random":
        L = rng.integers(0, 40, tot)
    elif kind == "ms":  # what an extension leaves: down by one, or a new match
        jump = rng.integers(0, 60, tot) * (rng.random(tot) < 0.08)
        L = np.zeros(tot, dtype=np.int64)
        for i in range(1, min(tot, 200_000)):
            L[i] = max(L[i - 1] - 1, jump[i])
        L[200_000:] = np.resize(L[:200_000], max(tot - 200_000, 0))
    elif kind == "constant":  # every position starts
        L = np.full(tot, 21)
    else:  # "falling": strictly falling inside every read, so only its first position starts
        L = np.zeros(tot, dtype=np.int64)
        for o, e in zip(offs[:-1].astype(np.int64), offs[1:].astype(np.int64)):
            L[o:e] = np.arange(e - o, 0, -1) + 16
    D = rng.choice([0, 1, 255, 256, 65535], size=tot)
    return L, _pointers(rng, L), D, offs


@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("kind", ["random", "ms", "constant", "falling"])
def test_crafted_reads_of_every_length(gpu, any_index, bits, kind):
    L, P, D, offs = _crafted(bits, kind, seed=bits + len(kind))
    nonempty = int((np.diff(offs.astype(np.int64)) > 0).sum())
    for min_length, docs in ((1, D), (17, None), (22, D), (1 << 33, None)):
        want = _check(any_index, L, P, offs, min_length, bits, docs)
        if kind == "constant":  # all start / none is long enough
            assert want[1].size == (int(offs[-1] - offs[0]) if min_length <= 21 else 0)
        if kind == "falling" and min_length <= 17:
            assert want[1].size == nonempty and (want[1]["read_pos"] == 0).all()
        if min_length == 1 << 33:
            assert want[1].size == 0


@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("nreads", [0, 1, 63, 64, 65, 3000])
def test_read_counts_around_the_lane_count(gpu, any_index, bits, nreads):
    rng = np.random.default_rng(nreads)
    lens = rng.integers(0, 66, nreads)
    offs = np.r_[0, np.cumsum(lens)].astype(np.uint64)
    L = rng.integers(0, 20, int(offs[-1]) + 1)
    P, D = _pointers(rng, L), rng.integers(0, 5, L.size)
    for min_length in (1, 10, 20):
        _check(any_index, L, P, offs, min_length, bits, D)
    _check(any_index, L, P, offs, 3, bits)


@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("front", [0, 77])
def test_a_read_that_starts_on_a_boundary_behind_a_large_value(gpu, any_index, bits, front):
    """Positions 64, 256, 512, 1024, 2048, 4096 each start a read whose first value is small, right behind a read that
    ends on a large one: only the read's start can report them."""
    bounds = [64, 256, 512, 1024, 2048, 4096]
    cuts = sorted(c for c in set([front] + bounds + [b + 5 for b in bounds] + [4200]) if c >= front)
    bounds = [b for b in bounds if b > front]
    offs = np.array(cuts, dtype=np.uint64)
    L = np.full(4300, 9)
    for b in bounds:
        L[b - 1], L[b], L[b + 1] = 60_000, 3, 2
    rng = np.random.default_rng(front)
    want = _check(any_index, L, _pointers(rng, L), offs, 3, bits, rng.integers(0, 9, L.size))
    starts = {int(offs[q]) + int(r) for q in range(offs.size - 1) for r in want[1]["read_pos"][int(want[0][q]):int(want[0][q + 1])]}
    assert set(bounds) <= starts and not {b + 1 for b in bounds} & starts


def _mix(seed, nreads, longest):
    rng = np.random.default_rng(seed)
    lens = np.minimum((rng.pareto(1.1, nreads) * 30).astype(np.int64), 20_000)
    lens[rng.integers(0, nreads)] = longest
    offs = np.r_[0, np.cumsum(lens)].astype(np.uint64)
    L = rng.integers(0, 50, int(offs[-1]))
    return L, _pointers(rng, L), rng.integers(0, 300, L.size), offs


@pytest.mark.parametrize("bits", [16, 32])
def test_capacity_bounds_what_is_written(gpu, any_index, bits):
    L, P, D, offs = _mix(14, 2000, 30_000)
    want = mems_reference(L, P, offs, 25, D)
    n = want[1].size
    assert n > 1000
    for cap in (0, n - 1, n, n + 5):
        d_out = torch.full((n + 8, 4), FENCE, dtype=torch.int32, device="cuda")
        d_docs = torch.full((n + 8,), FENCE, dtype=torch.int32, device="cuda")
        mo, _, _ = _run(any_index, L, P, offs, 25, bits, D, capacity=cap, d_out=d_out, d_out_docs=d_docs)
        assert np.array_equal(mo.cpu().numpy().view(np.uint64), want[0]), cap
        k = min(cap, n)
        assert np.array_equal(_records(d_out[:k]), want[1][:k]) and np.array_equal(d_docs[:k].cpu().numpy().view(np.uint32), want[2][:k])
        assert (d_out[k:] == FENCE).all().item() and (d_docs[k:] == FENCE).all().item(), cap
        st = any_index.mems_stats()
        assert st["matches"] == n and st["written"] == k and st["values"] == L.size, (cap, st)
        assert st["longest"] == int(want[1]["length"].max()) and st["kernel_ms"] > 0, (cap, st)


def test_repeated_call_and_split_batch_give_the_same_bytes(gpu, any_index):
    L, P, D, offs = _mix(15, 3000, 100_000)
    nreads = offs.size - 1
    for bits in (16, 32):
        d_L, d_P, d_D, d_offs = _to_device(L, bits), _to_device(P, 64), _to_device(D, bits), _to_device(offs, 64)
        whole = any_index.mems_device(d_L, d_P, d_offs, 25, d_docs=d_D)
        again = any_index.mems_device(d_L, d_P, d_offs, 25, d_docs=d_D)
        torch.cuda.synchronize()
        for x, y in zip(whole, again):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
        want = mems_reference(L, P, offs, 25, D)
        assert np.array_equal(_records(whole[1]), want[1])
        for cut in (1, 1234, nreads - 1):
            a = any_index.mems_device(d_L, d_P, d_offs[: cut + 1], 25, d_docs=d_D)
            b = any_index.mems_device(d_L, d_P, d_offs[cut:], 25, d_docs=d_D)
            torch.cuda.synchronize()
            assert torch.cat([a[1], b[1]]).cpu().numpy().tobytes() == whole[1].cpu().numpy().tobytes(), (bits, cut)
            assert torch.cat([a[2], b[2]]).cpu().numpy().tobytes() == whole[2].cpu().numpy().tobytes(), (bits, cut)
            assert torch.cat([a[0][:-1], b[0] + a[0][-1]]).cpu().numpy().tobytes() == whole[0].cpu().numpy().tobytes(), (bits, cut)


def test_a_second_query_context_has_its_own_scratch(gpu, any_index):
    L, P, D, offs = _mix(16, 500, 5000)
    other = any_index.clone(0)
    want = mems_reference(L, P, offs, 30)
    a = _run(any_index, L, P, offs, 30, 16)
    b = _run(other, L, P, offs, 30, 16)
    assert np.array_equal(_records(a[1]), want[1]) and np.array_equal(_records(b[1]), want[1])
    assert other.mems_stats()["matches"] == any_index.mems_stats()["matches"] == want[1].size
    other.close()


def test_argument_errors(gpu, any_index):
    L, P, offs = np.arange(40) % 7, np.arange(40), np.array([0, 10, 40], dtype=np.uint64)
    d_L, d_P, d_offs = _to_device(L, 16), _to_device(P, 64), _to_device(offs, 64)
    with pytest.raises(capi.SpxError, match="min_length must be at least 1"):
        any_index.mems_device(d_L, d_P, d_offs, 0)
    with pytest.raises(capi.SpxError, match="16-byte aligned"):
        any_index.mems_device(d_L[1:], d_P, d_offs, 1)
    with pytest.raises(capi.SpxError, match="same width"):
        any_index.mems_device(d_L, d_P, d_offs, 1, d_docs=_to_device(L, 32))
    mo = torch.empty(3, dtype=torch.int64, device="cuda")
    S = capi._spm()
    rc = S.spm_mems_device(any_index._h, d_L.data_ptr(), 8, d_P.data_ptr(), None, d_offs.data_ptr(), 2, 40, 1, mo.data_ptr(), None, 0, None, None)
    assert rc == -1 and b"value_bits" in capi.lib().spx_last_error()
    # more values than total_values said: nothing is touched beyond what the scratch was sized for, and the stats say so
    big = np.arange(5000) % 9
    offs2 = np.array([0, 100, 5000], dtype=np.uint64)
    d_big, d_bigp, d_offs2 = _to_device(big, 16), _to_device(big, 64), _to_device(offs2, 64)
    rc = S.spm_mems_device(any_index._h, d_big.data_ptr(), 16, d_bigp.data_ptr(), None, d_offs2.data_ptr(), 2, 1000, 1, mo.data_ptr(),
                           None, 0, None, None)
    assert rc == 0
    with pytest.raises(capi.SpxError, match="more values than total_values"):
        any_index.mems_stats()
    torch.cuda.synchronize()
    without_text = capi.Index.from_raw(synth.statistical_rlbwt(2000, 20, 3.0, seed=1, with_samples=True, n_docs=4), 0)
    with pytest.raises(capi.SpxError, match="text"):
        without_text.mems_host(np.frombuffer(b"ACGT", dtype=np.uint8), [0, 4], 1)
    without_text.close()


# ---- mems_host against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, capi.SPX_DIGEST_PROMOTED, capi.SPX_DIGEST_DNA])
def test_mems_host_on_a_real_text_built_on_the_device(gpu, oracle_mod, kind):
    """Several documents, indexed by capi.build_raw (digested first for -m / -a); DNA reads through digestion, walk, MS
    extension and the match kernels in one call, 16-bit arrays and -- with a read of 70 000 characters -- 32-bit ones."""
    rng = np.random.default_rng(60 + kind)
    genome = cases.repetitive_text(rng, 40_000, DNA)
    k, w = 4, 11
    text = oracle_mod.digest(kind, k, w, genome) if kind else genome
    cuts = [text.size // 5, text.size // 2, text.size - text.size // 5 - text.size // 2]
    raw = capi.build_raw(text, doc_lengths=cuts)
    orc = oracle_mod.OracleIndex.from_raw(raw)
    ix = capi.Index.from_raw(raw, 0)
    seqs, offs = cases.reads_mixed(rng, genome, DNA, 600, 500, [ord("N")])
    long_read = np.concatenate([genome[s:s + 7000] for s in rng.integers(0, 30_000, 10)])
    wide = (np.r_[seqs[: int(offs[100])], long_read], np.r_[offs[:101], offs[100] + long_read.size])
    for s, o in ((seqs, offs), wide):
        o = o.astype(np.uint64)
        dseqs, doffs = oracle_mod.digest_batch(kind, k, w, s, o) if kind else (s, o)
        values = np.diff(doffs.astype(np.int64))
        ms = orc.ms(dseqs, doffs, want_docs=True, text=text)
        top = int(ms["lengths"].max())
        for min_length, want_docs in ((1, True), (4, False), (top + 1, True)):
            want = mems_reference(ms["lengths"], ms["pointers"], doffs, min_length, ms["docs"] if want_docs else None)
            got = ix.mems_host(s, o, min_length, digest=(kind, k, w) if kind else None, want_docs=want_docs)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (min_length, want_docs)
            if want_docs:
                assert np.array_equal(got[2], want[2]) and len(set(want[2].tolist())) >= (3 if min_length == 1 else 0)
            assert np.array_equal(got[-1], values)
            assert want[1].size == 0 if min_length > top else want[1].size > 50
            st = ix.mems_stats()
            assert st["matches"] == st["written"] == want[1].size and st["values"] == int(values.sum()), st
    with pytest.raises(capi.SpxError, match="spx error -1: min_length must be at least 1"):
        ix.mems_host(seqs, offs, 0)
    ix.close()


# ---- the command -------------------------------------------------------------------------------------------------------
def _parse_values(path):
    ids, vals = [], []
    with open(path, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                ids.append(line[1:-1])
            else:
                vals.append(np.array(line.split(), dtype=np.uint64))
    return ids, vals


def _cli(args, env):
    return subprocess.run([HOST_BIN] + args, capture_output=True, env=env, timeout=300)  # (every child has its time limit)


@pytest.mark.parametrize("case", ["dna_multiline_fasta", "dna_fastq", "promoted_alphabet_fasta"])
def test_cli_mems_equals_the_reference_over_the_golden_files(gpu, tmp_path, case):
    work = tmp_path / case
    shutil.copytree(os.path.join(FILES, case), work)
    ref, reads = str(work / "ref"), str(work / "reads.fa")
    env = dict(os.environ, SPUMONI_TEXT=ref + ".fa.rawtext", SPUMONI_SUPER_BATCH="3000")
    gold = os.path.join(FILES, case, "expected_M", "reads.fa")
    ids, L = _parse_values(gold + ".lengths")
    _, P = _parse_values(gold + ".pointers")
    _, D = _parse_values(gold + ".doc_numbers")
    offs = np.r_[0, np.cumsum([v.size for v in L])].astype(np.uint64)
    L, P, D = np.concatenate(L), np.concatenate(P), np.concatenate(D)
    for extra, min_length, docs in ((["-L", "4", "-d"], 4, True), (["-L", "8", "-d"], 8, True), (["-L", "8"], 8, False), (["-M"], None, False)):
        if os.path.exists(reads + ".mems"):
            os.remove(reads + ".mems")
        r = _cli(["mems", "-r", ref, "-p", reads, "-n"] + extra, env)
        assert r.returncode == 0, r.stderr.decode()
        if min_length is None:  # the default: what `run -M -c` classifies with, named on stderr
            min_length = int(r.stderr.decode().split("a match is reported from length ")[1].split()[0])
            assert min_length >= 1
        mo, rec, dd = mems_reference(L, P, offs, min_length, D)
        lines = []
        for q in range(len(ids)):
            for j in range(int(mo[q]), int(mo[q + 1])):
                f = [ids[q]] + [str(int(x)).encode() for x in (rec["read_pos"][j], rec["length"][j], rec["ref_pos"][j])]
                lines.append(b"\t".join(f + ([str(int(dd[j])).encode()] if docs else [])) + b"\n")
        assert open(reads + ".mems", "rb").read() == b"".join(lines), (extra, r.stderr.decode())
        without = int((np.diff(mo.astype(np.int64)) == 0).sum())
        assert f"{len(ids)} reads, {rec.size} matches, {without} reads without a match".encode() in r.stderr
        if min_length == 8:  # both outcomes are exercised
            assert rec.size > 0 and without > 0
    assert sorted(f for f in os.listdir(work) if f.startswith("reads.fa")) == ["reads.fa", "reads.fa.mems"]


def test_cli_mems_writes_no_file_when_it_fails(gpu, tmp_path):
    work = tmp_path / "c"
    shutil.copytree(os.path.join(FILES, "dna_multiline_fasta"), work)
    text = open(work / "ref.fa.rawtext", "rb").read()
    with open(work / "reads.fa", "wb") as f:  # a read without characters ends the run, as it ends `run`: behind 40 good ones
        for q in range(40):
            f.write(b">r%d\n" % q + text[17 * q: 17 * q + 60] + b"\n")
        f.write(b">bad_one\n>after\n" + text[:40] + b"\n")
    env = dict(os.environ, SPUMONI_TEXT=str(work / "ref.fa.rawtext"), SPUMONI_SUPER_BATCH="1000")
    before = sorted(os.listdir(work))
    r = _cli(["mems", "-r", str(work / "ref"), "-p", str(work / "reads.fa"), "-n", "-L", "4"], env)
    assert r.returncode == 1 and b"bad_one was empty after digestion" in r.stderr, r.stderr.decode()
    assert sorted(os.listdir(work)) == before
