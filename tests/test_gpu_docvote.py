"""-m gpu: the document votes (spumoni_amd/csrc/spx_docvote.hip, include/spumoni_docvote.h) against the definition
(spumoni_amd/docvote.py: votes_reference), bit for bit.

votes_device gets crafted arrays (the expectation is votes_reference over the same arrays); assign_host and `spumoni
assign` are held to votes_reference over the ORACLE's per-position lengths and document ids, or over the numbers
`spumoni run -d` wrote -- never over the library's own arrays.  votes_stats() must show that every kernel path took reads:
several reads per wavefront (short), a workgroup per read (medium), several workgroups per read (long), and the reads
without a value."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from spumoni_amd import capi, synth
from spumoni_amd.docvote import NO_DOC, VOTE_DTYPE, votes_reference
from tests import cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
FILES = os.path.join(ROOT, "tests", "golden", "files")
FIELDS = list(VOTE_DTYPE.names)
DNA = list(b"ACGT")


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


def _table(rec):
    return np.stack([rec[f] for f in FIELDS], axis=1).astype(np.uint32)


def _to_device(a, bits):
    dt, st = (np.uint16, np.int16) if bits == 16 else (np.uint32, np.int32)
    a = np.ascontiguousarray(a, dtype=dt)
    return torch.from_numpy(a.view(st).copy()).cuda()


def _votes(ix, L, D, offs, min_length, bits, d_out=None):
    assert int(np.max(L, initial=0)) < (1 << bits) and int(np.max(D, initial=0)) < (1 << bits)
    d_L, d_D = _to_device(L, bits), _to_device(D, bits)
    d_offs = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.uint64).view(np.int64).copy()).cuda()
    out = ix.votes_device(d_L, d_D, d_offs, min_length, d_out=d_out)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def _check(ix, L, D, offs, min_length, bits):
    got = _votes(ix, L, D, offs, min_length, bits)
    want = _table(votes_reference(L, D, offs, min_length))
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (bits, min_length, bad[:5], got[bad[:5]], want[bad[:5]], np.diff(offs)[bad[:5]])
    st = ix.votes_stats()
    lens = np.diff(np.asarray(offs, dtype=np.int64))
    assert st["reads_short"] + st["reads_medium"] + st["reads_long"] + st["reads_empty"] == lens.size
    assert st["reads_empty"] == int((lens == 0).sum())
    assert st["voting_positions"] == int(want[:, 0].sum())
    return st


LENGTHS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 65535]


def _crafted(bits, kind, seed):
    """Reads of every length of the list (and, 32-bit, 70 000 and 10^6), runs of empty reads between them, in a random
    order, twice; the document ids by `kind`."""
    rng = np.random.default_rng(seed)
    lens = LENGTHS * 2 + [0] * 40 + ([70_000, 1_000_000] if bits == 32 else [])
    lens = np.array(lens)[rng.permutation(len(lens))]
    lens = np.r_[lens, [0, 0, 0, 5, 0, 0, 61, 62, 63, 64, 0]]
    offs = np.r_[0, np.cumsum(lens)].astype(np.uint64)
    tot = int(offs[-1])
    L = rng.integers(0, 40, tot)
    if kind == "one":
        D = np.full(tot, 65535)
    elif kind == "distinct":  # inside every read no id twice (reads of up to 65536 values), 0 and 65535 among them
        # (the reads of 70 000 / 10^6 values: their first 65536 ids are distinct, the rest random)
        fix = []
        for m in lens:
            ids = (np.arange(min(m, 65536)) * 40503 + int(rng.integers(0, 65536))) % 65536
            fix.append(np.r_[ids, rng.integers(0, 65536, m - ids.size)])
        D = np.concatenate(fix)
    elif kind == "few":
        D = rng.choice([0, 1, 255, 256, 32768, 65535], size=tot)
    else:  # "ties": every id of a read has the same number of votes, whatever the rank
        parts = []
        for m in lens:
            ids = np.array([65535, 4000, 17, 900, 5])[: max(1, min(5, m))]
            reps = np.repeat(ids, m // ids.size) if m else np.zeros(0, dtype=np.int64)
            pad = 70 + np.arange(m - reps.size) if m >= 5 else np.full(m - reps.size, ids[0])  # (the remainder: one vote each)
            parts.append(rng.permutation(np.r_[reps, pad]))
        D = np.concatenate(parts)
        L[:] = 30
    return L, D.astype(np.int64), offs


@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("kind", ["one", "distinct", "few", "ties"])
def test_crafted_reads_of_every_length(gpu, any_index, bits, kind):
    L, D, offs = _crafted(bits, kind, seed=bits + len(kind))
    for min_length in (0, 17, 1000):
        st = _check(any_index, L, D, offs, min_length, bits)
        assert st["reads_short"] > 0 and st["reads_medium"] > 0 and st["reads_long"] > 0 and st["reads_empty"] > 0, st
        assert st["long_tiles"] >= 2 * st["reads_long"]
    if kind == "ties":
        want = votes_reference(L, D, offs, 0)
        big = np.diff(offs.astype(np.int64)) >= 10
        assert (want["top_votes"][big] == want["second_votes"][big]).all() and (want["top_doc"][big] == 5).all()
    if kind == "distinct":
        want = votes_reference(L, D, offs, 0)
        assert int(want["top_votes"].max()) <= (1 if bits == 16 else 40) and (want["voters"] == np.diff(offs.astype(np.int64))).all()


def test_all_ids_of_one_read_distinct(gpu, any_index):
    """65 536 distinct ids in one read: every count is 1, the smallest id wins, the runner-up has as many."""
    rng = np.random.default_rng(9)
    D = rng.permutation(65536)
    L = np.full(65536, 7)
    got = _votes(any_index, L, D, [0, 65536], 0, 32)
    assert got.tolist() == [[65536, 0, 1, 1]]
    got = _votes(any_index, L[:65535], D[D != 0], [0, 65535], 7, 16)
    assert got.tolist() == [[65535, 1, 1, 1]]
    assert _votes(any_index, L, D, [0, 65536], 8, 32).tolist() == [[0, NO_DOC, 0, 0]]


@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("nreads", [0, 1, 3, 15, 16, 17, 63, 64, 65, 255, 257])
def test_read_counts_around_the_lane_count(gpu, any_index, bits, nreads):
    rng = np.random.default_rng(nreads)
    lens = rng.integers(0, 66, nreads)
    offs = np.r_[0, np.cumsum(lens)].astype(np.uint64)
    L = rng.integers(0, 20, int(offs[-1]))
    D = rng.integers(0, 5, int(offs[-1]))
    for min_length in (0, 10, 20):
        _check(any_index, L, D, offs, min_length, bits)


def test_a_million_short_reads(gpu, any_index):
    rng = np.random.default_rng(11)
    n = 1_000_000
    lens = np.full(n, 44)
    lens[rng.integers(0, n, 1000)] = rng.integers(0, 65, 1000)
    offs = np.r_[0, np.cumsum(lens)].astype(np.uint64)
    L = rng.integers(0, 30, int(offs[-1]))
    D = rng.integers(0, 6, int(offs[-1]))
    st = _check(any_index, L, D, offs, 12, 16)
    assert st["reads_short"] >= n - 1000 and st["reads_medium"] == 0 and st["reads_long"] == 0 and st["kernel_ms"] > 0


def _heavy_tail(rng, nreads, longest):
    lens = np.minimum((rng.pareto(1.1, nreads) * 30).astype(np.int64), 200_000)
    lens[rng.integers(0, nreads)] = longest
    offs = np.r_[0, np.cumsum(lens)].astype(np.uint64)
    tot = int(offs[-1])
    return rng.integers(0, 50, tot), rng.integers(0, 300, tot), offs


def test_heavy_tailed_mix(gpu, any_index):
    L, D, offs = _heavy_tail(np.random.default_rng(12), 200_000, 1_000_000)
    st = _check(any_index, L, D, offs, 20, 32)
    assert st["reads_short"] > 1000 and st["reads_medium"] > 100 and st["reads_long"] > 10 and st["reads_empty"] > 0, st


def test_split_batch_and_repeated_call_give_the_same_bytes(gpu, any_index):
    L, D, offs = _heavy_tail(np.random.default_rng(13), 30_000, 300_000)
    want = _table(votes_reference(L, D, offs, 25))
    for bits in (16, 32):
        d_L, d_D = _to_device(L, bits), _to_device(D, bits)
        d_offs = torch.from_numpy(offs.view(np.int64).copy()).cuda()
        nreads = offs.size - 1
        whole = any_index.votes_device(d_L, d_D, d_offs, 25)
        again = any_index.votes_device(d_L, d_D, d_offs, 25)
        torch.cuda.synchronize()
        assert whole.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
        assert np.array_equal(whole.cpu().numpy().view(np.uint32), want)
        for cut in (1, 12_345, nreads - 1):
            parts = torch.full((nreads, 4), -7, dtype=torch.int32, device="cuda")
            any_index.votes_device(d_L, d_D, d_offs[: cut + 1], 25, d_out=parts[:cut])
            any_index.votes_device(d_L, d_D, d_offs[cut:], 25, d_out=parts[cut:])
            torch.cuda.synchronize()
            assert parts.cpu().numpy().tobytes() == whole.cpu().numpy().tobytes(), (bits, cut)


def test_argument_errors(gpu, any_index):
    L, D, offs = np.arange(40) % 7, np.arange(40) % 3, np.array([0, 10, 40], dtype=np.uint64)
    d_L, d_D = _to_device(L, 16), _to_device(D, 16)
    d_offs = torch.from_numpy(offs.view(np.int64).copy()).cuda()
    with pytest.raises(capi.SpxError, match="16-byte aligned"):
        any_index.votes_device(d_L[1:], d_D, d_offs, 0)
    with pytest.raises(capi.SpxError, match="same width"):
        any_index.votes_device(d_L, _to_device(D, 32), d_offs, 0)
    out = torch.empty((2, 4), dtype=torch.int32, device="cuda")
    rc = capi._spv().spv_votes_device(any_index._h, d_L.data_ptr(), d_D.data_ptr(), 8, d_offs.data_ptr(), 2, 40, 0, out.data_ptr(), None)
    assert rc == -1 and b"value_bits" in capi.lib().spx_last_error()
    nodoc = capi.Index.from_raw(synth.statistical_rlbwt(2000, 20, 3.0, seed=1, with_samples=True), 0)
    with pytest.raises(capi.SpxError, match="no document array"):
        nodoc.votes_device(d_L, d_D, d_offs, 0)
    with pytest.raises(capi.SpxError, match="no document array"):
        nodoc.assign_host(capi.SPX_MODE_PML, np.frombuffer(b"ACGT", dtype=np.uint8), [0, 4], 0)
    ms_without_text = capi.Index.from_raw(synth.statistical_rlbwt(2000, 20, 3.0, seed=1, with_samples=True, n_docs=4), 0)
    with pytest.raises(capi.SpxError, match="text"):
        ms_without_text.assign_host(capi.SPX_MODE_MS, np.frombuffer(b"ACGT", dtype=np.uint8), [0, 4], 0)


# ---- assign_host against the oracle ---------------------------------------------------------------------------------
def _expect(oracle_mod, orc, mode, seqs, offs, min_length, text=None):
    if mode == capi.SPX_MODE_PML:
        L, D = orc.pml(seqs, offs, want_docs=True)
    else:
        w = orc.ms(seqs, offs, want_docs=True, text=text)
        L, D = w["lengths"], w["docs"]
    return votes_reference(L, D, offs, min_length)


def _assert_assign(got, want, values):
    for f in FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, (f, bad[:5], got[bad[:5]], want[bad[:5]])
    assert np.array_equal(got["values"], values)


@pytest.mark.parametrize("n_docs", [8, 65536])
def test_assign_host_on_a_statistical_index(gpu, oracle_mod, n_docs):
    raw = synth.statistical_rlbwt(150_000, 120, 5.0, seed=n_docs, zipf=1.0, with_samples=True, n_docs=n_docs)
    orc = oracle_mod.OracleIndex.from_raw(raw)
    ix = capi.Index.from_raw(raw, 0)
    rng = np.random.default_rng(n_docs)
    text = np.asarray(raw.heads.numpy()[1:])[rng.integers(0, raw.r - 1, raw.n - 1)]  # (no text has this BWT: any will do)
    ix.set_text(torch.from_numpy(text.copy()), unchecked=True)
    parts = [synth.simulate_reads(raw, nr, ln, seed=7 + i) for i, (nr, ln) in enumerate([(3000, 44), (300, 700), (6, 9000)])]
    seqs = np.concatenate([p[0].numpy() for p in parts])
    lens = np.concatenate([np.diff(p[1].numpy()) for p in parts])
    offs = np.r_[0, np.cumsum(lens)].astype(np.uint64)
    for mode in (capi.SPX_MODE_PML, capi.SPX_MODE_MS):
        for min_length in (0, 3, 6):
            want = _expect(oracle_mod, orc, mode, seqs, offs, min_length, text)
            got = ix.assign_host(mode, seqs, offs, min_length)
            _assert_assign(got, want, lens)
        st = ix.votes_stats()
        assert st["reads_short"] == 3000 and st["reads_medium"] == 300 and st["reads_long"] == 6, st
    if n_docs == 65536:  # (ids beyond 8 bits win reads)
        all_vote = _expect(oracle_mod, orc, capi.SPX_MODE_PML, seqs, offs, 0)
        assert int(all_vote["top_doc"][all_vote["top_votes"] > 0].max()) > 255
    # a read of 65536 characters or more: the 32-bit arrays
    long_seqs, long_offs = synth.simulate_reads(raw, 3, 70_000, seed=99)
    seqs2 = np.r_[seqs[: int(offs[100])], long_seqs.numpy()]
    offs2 = np.r_[offs[:100], offs[100] + long_offs.numpy().astype(np.uint64)]
    want = _expect(oracle_mod, orc, capi.SPX_MODE_PML, seqs2, offs2, 3)
    _assert_assign(ix.assign_host(capi.SPX_MODE_PML, seqs2, offs2, 3), want, np.diff(offs2.astype(np.int64)))
    ix.close()


def test_assign_host_in_several_pieces(gpu, oracle_mod):
    """More characters than one piece of the pipeline holds: the records of every piece land where they belong."""
    raw = synth.statistical_rlbwt(150_000, 120, 5.0, seed=21, zipf=1.0, with_samples=True, n_docs=8)
    orc = oracle_mod.OracleIndex.from_raw(raw)
    ix = capi.Index.from_raw(raw, 0)
    seqs, offs = synth.simulate_reads(raw, 340_000, 100, seed=22)
    seqs, offs = seqs.numpy(), offs.numpy().astype(np.uint64)
    assert int(offs[-1]) > (32 << 20)
    want = _expect(oracle_mod, orc, capi.SPX_MODE_PML, seqs, offs, 4)
    _assert_assign(ix.assign_host(capi.SPX_MODE_PML, seqs, offs, 4), want, np.diff(offs.astype(np.int64)))
    assert ix.votes_stats()["reads_medium"] == 340_000
    ix.close()


@pytest.mark.parametrize("kind", [0, capi.SPX_DIGEST_PROMOTED, capi.SPX_DIGEST_DNA])
def test_assign_host_on_a_real_text_built_on_the_device(gpu, oracle_mod, kind):
    """Several documents, indexed by capi.build_raw (digested first for -m / -a); DNA reads through digestion, walk, MS
    extension and votes in one call."""
    rng = np.random.default_rng(50 + kind)
    genome = cases.repetitive_text(rng, 40_000, DNA)
    k, w = 4, 11
    text = oracle_mod.digest(kind, k, w, genome) if kind else genome
    cuts = [text.size // 5, text.size // 2, text.size - text.size // 5 - text.size // 2]
    raw = capi.build_raw(text, doc_lengths=cuts)
    orc = oracle_mod.OracleIndex.from_raw(raw)
    ix = capi.Index.from_raw(raw, 0)
    seqs, offs = cases.reads_mixed(rng, genome, DNA, 600, 500, [ord("N")])
    offs = offs.astype(np.uint64)
    dseqs, doffs = oracle_mod.digest_batch(kind, k, w, seqs, offs) if kind else (seqs, offs)
    values = np.diff(doffs.astype(np.int64))
    assert (values == 0).any() and (values > 64).any()
    for mode in (capi.SPX_MODE_PML, capi.SPX_MODE_MS):
        for min_length in (0, 4):
            want = _expect(oracle_mod, orc, mode, dseqs, doffs, min_length, text)
            got = ix.assign_host(mode, seqs, offs, min_length, digest=(kind, k, w) if kind else None)
            _assert_assign(got, want, values)
            assert len(set(want["top_doc"].tolist())) >= 3
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
    r = subprocess.run([HOST_BIN] + args, capture_output=True, env=env, timeout=300)  # (every child has its time limit)
    return r


@pytest.mark.parametrize("case", ["dna_multiline_fasta", "dna_fastq", "promoted_alphabet_fasta"])
@pytest.mark.parametrize("mode", ["-P", "-M"])
def test_cli_assign_equals_votes_over_what_run_wrote(gpu, tmp_path, case, mode):
    work = tmp_path / case
    shutil.copytree(os.path.join(FILES, case), work)
    ref, reads = str(work / "ref"), str(work / "reads.fa")
    env = dict(os.environ, SPUMONI_TEXT=ref + ".fa.rawtext", SPUMONI_SUPER_BATCH="3000")
    r = _cli(["run", "-r", ref, "-p", reads, "-n", "-d", mode], env)
    assert r.returncode == 0, r.stderr.decode()
    ids, L = _parse_values(reads + (".pseudo_lengths" if mode == "-P" else ".lengths"))
    ids_d, D = _parse_values(reads + ".doc_numbers")
    assert ids == ids_d and len(ids) > 20
    offs = np.r_[0, np.cumsum([v.size for v in L])].astype(np.uint64)
    for extra, min_length in ((["-T", "2"], 2), (["-T", "0"], 0), (["-T", "9"], 9), ([], None)):
        for f in (reads + ".assignments", reads + ".assignments.by_doc"):
            if os.path.exists(f):
                os.remove(f)
        a = _cli(["assign", "-r", ref, "-p", reads, "-n", mode] + extra, env)
        assert a.returncode == 0, a.stderr.decode()
        if min_length is None:  # the default: what `run -c` classifies with, named on stderr
            min_length = int(a.stderr.decode().split("a position votes from ")[1].split()[0])
            assert min_length >= 3
        want = votes_reference(np.concatenate(L), np.concatenate(D), offs, min_length)
        lines = open(reads + ".assignments", "rb").read().split(b"\n")
        assert lines[-1] == b"" and len(lines) - 1 == len(ids)
        tally = {}
        for q, line in enumerate(lines[:-1]):
            top = -1 if want["top_votes"][q] == 0 else int(want["top_doc"][q])
            exp = b"\t".join([ids[q]] + [str(x).encode() for x in (top, int(want["top_votes"][q]), int(want["second_votes"][q]),
                                                                   int(want["voters"][q]), L[q].size)])
            assert line == exp, (q, line, exp)
            tally[top] = tally.get(top, 0) + 1
        order = sorted(k for k in tally if k >= 0) + ([-1] if -1 in tally else [])
        assert open(reads + ".assignments.by_doc").read() == "".join(f"{k}\t{tally[k]}\n" for k in order)
        assert min_length != 0 or len([k for k in tally if k >= 0]) >= 2  # (every position votes: several documents win reads)


def test_cli_assign_refuses_an_index_without_doc(gpu, tmp_path):
    work = tmp_path / "c"
    shutil.copytree(os.path.join(FILES, "dna_fastq"), work)
    os.remove(work / "ref.fa.doc")
    a = _cli(["assign", "-r", str(work / "ref"), "-p", str(work / "reads.fa"), "-n", "-P"], dict(os.environ))
    assert a.returncode == 1 and b"ref.fa.doc) is not present, so it cannot be used." in a.stderr
    assert not os.path.exists(work / "reads.fa.assignments")


def test_cli_assign_keeps_what_is_in_front_of_a_failing_read(gpu, tmp_path):
    """A read without characters ends the run as it ends `run`: what is in front of it is assigned and written first,
    and the summary by document is not."""
    work = tmp_path / "c"
    shutil.copytree(os.path.join(FILES, "dna_multiline_fasta"), work)
    text = open(work / "ref.fa.rawtext", "rb").read()
    good = b"".join(b">r%d\n" % q + text[17 * q: 17 * q + 60] + b"\n" for q in range(40))
    env = dict(os.environ, SPUMONI_TEXT=str(work / "ref.fa.rawtext"), SPUMONI_SUPER_BATCH="1000")
    args = ["assign", "-r", str(work / "ref"), "-p", str(work / "reads.fa"), "-n", "-P", "-T", "2"]
    with open(work / "reads.fa", "wb") as f:
        f.write(good)
    a = _cli(args, env)
    assert a.returncode == 0, a.stderr.decode()
    want = open(work / "reads.fa.assignments", "rb").read()
    assert want.count(b"\n") == 40 and os.path.exists(work / "reads.fa.assignments.by_doc")
    os.remove(work / "reads.fa.assignments")
    os.remove(work / "reads.fa.assignments.by_doc")
    with open(work / "reads.fa", "wb") as f:
        f.write(good + b">bad_one\n>after\n" + text[:40] + b"\n")
    a = _cli(args, env)
    assert a.returncode == 1 and b"bad_one was empty after digestion" in a.stderr, a.stderr.decode()
    assert open(work / "reads.fa.assignments", "rb").read() == want
    assert not os.path.exists(work / "reads.fa.assignments.by_doc")
