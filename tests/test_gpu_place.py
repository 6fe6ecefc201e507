"""-m gpu: the placements (spumoni_amd/csrc/spx_place.hip, include/spumoni_place.h) against the definition
(spumoni_amd/place.py: place_reference), bit for bit.

place_device gets crafted arrays on a small index whose text is handed in unchecked (the expectation is place_reference
over the same arrays and the same text); place_host and `spumoni place` are held to place_reference over the ORACLE's MS
lengths, pointers and document ids, or over the committed golden files -- never over the library's own arrays.  The kernel
gives a read 16 lanes, 8 (16-bit) or 4 (32-bit) values and 16 characters per lane and round, and a read of more than 2048
values a whole wavefront: the crafted reads, ties and stops lie around each of those."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from spumoni_amd import capi, synth
from spumoni_amd.place import NO_DOC, PLACEMENT_DTYPE, UNPLACED, place_reference
from tests import cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
FILES = os.path.join(ROOT, "tests", "golden", "files")
DNA = list(b"ACGT")
FENCE = -7
N_TEXT = 1_200_000


@pytest.fixture(scope="module")
def gpu(built_all):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    capi.lib()
    return 0


@pytest.fixture(scope="module")
def text():
    return np.asarray(DNA, dtype=np.uint8)[np.random.default_rng(77).integers(0, 4, N_TEXT)]


@pytest.fixture(scope="module")
def any_index(gpu, text):
    raw = synth.statistical_rlbwt(5000, 60, 4.0, seed=3, with_samples=True, n_docs=8)
    ix = capi.Index.from_raw(raw, 0)
    ix.set_text(torch.from_numpy(text.copy()), unchecked=True)  # (no text has this BWT: the kernels see the text alone)
    yield ix
    ix.close()


def _to_device(a, bits):
    """The array on the device, behind it zeros up to a multiple of 16 bytes (the lengths are read as whole vectors)."""
    dt, st = {8: (np.uint8, np.uint8), 16: (np.uint16, np.int16), 32: (np.uint32, np.int32), 64: (np.uint64, np.int64)}[bits]
    a = np.ascontiguousarray(a, dtype=dt)
    pad = np.zeros(-a.size % (128 // bits) + (36 if bits == 8 else 0), dtype=dt)  # (the reads: the walk's 32 bytes of slack)
    return torch.from_numpy(np.r_[a, pad].view(st).copy()).cuda()[: a.size]


def _records(t):
    return t.cpu().numpy().view(PLACEMENT_DTYPE).reshape(-1)


def _run(ix, R, L, P, offs, params, bits, D=None, **kw):
    assert int(np.max(L, initial=0)) < (1 << bits) and (D is None or int(np.max(D, initial=0)) < (1 << bits))
    nreads = len(offs) - 1
    fenced = torch.full((nreads + 3, 8), FENCE, dtype=torch.int32, device="cuda")
    out = ix.place_device(_to_device(R, 8), _to_device(L, bits), _to_device(P, 64), _to_device(offs, 64), *params,
                          d_docs=None if D is None else _to_device(D, bits), d_out=fenced[:nreads], **kw)
    torch.cuda.synchronize()
    assert (fenced[nreads:] == FENCE).all().item()
    return _records(out)


def _check(ix, text, R, L, P, offs, params, bits, D=None):
    got = _run(ix, R, L, P, offs, params, bits, D)
    want = place_reference(R, L, P, offs, text, *params, docs=D)
    bad = np.flatnonzero(got != want)
    lens = np.diff(np.asarray(offs).astype(np.int64))
    assert bad.size == 0, (bits, params, bad[:5], lens[bad[:5]], got[bad[:5]], want[bad[:5]])
    st = ix.place_stats()
    ok = want["ref_start"] != np.uint64(UNPLACED)
    span = want["read_end"][ok].astype(np.int64) - want["read_start"][ok] - want["seed_len"][ok]
    assert st["values"] == (int(offs[-1]) - int(offs[0]) if len(offs) > 1 else 0), st
    assert st["placed"] == int(ok.sum()) and st["seed_values"] == int(want["seed_len"][ok].sum()), st
    assert st["extended_values"] == int(span.sum()), st
    return want


def _on_diagonals(rng, text, lens, front, bits, err=0.03, top=30):
    """Reads that lie on a diagonal of the text with substitutions -- cut by the text's start or by its end for some --
    lengths that are random but for one seed per read (the rule is one on the arrays), pointers on the diagonal."""
    offs = (front + np.r_[0, np.cumsum(lens)]).astype(np.uint64)
    tot = int(offs[-1]) + 9  # (values behind the batch, too)
    R = np.asarray(DNA, dtype=np.uint8)[rng.integers(0, 4, tot)]
    L = rng.integers(0, top, tot)
    P = rng.integers(0, text.size, tot).astype(np.uint64)
    for q, (o, e) in enumerate(zip(offs[:-1].astype(np.int64), offs[1:].astype(np.int64))):
        m = int(e - o)
        if m == 0:
            continue
        where = q % 7
        d = -(m // 3) - 1 if where == 0 else (text.size - m + m // 3 + 1 if where == 1 else int(rng.integers(0, text.size - m)))
        if m < 3:
            d = int(rng.integers(0, text.size - m))
        j0, j1 = max(0, -d), min(m, text.size - d)  # the positions that face the text
        keep = rng.random(j1 - j0) >= err
        R[o + j0:o + j1] = np.where(keep, text[d + j0:d + j1], R[o + j0:o + j1])
        P[o + j0:o + j1] = d + np.arange(j0, j1)
        s = int(rng.integers(j0, j1))  # the seed: on the diagonal
        if q % 5 == 0 and m < (1 << bits):
            s, L[o] = 0, m  # a seed that is the whole read
        else:
            L[o + s] = min(top + 1 + int(rng.integers(0, 30)), (1 << bits) - 1)
        if q % 11 == 3 and s + 1 < m:
            L[o + s + 1:e][rng.integers(0, m - s - 1)] = L[o + s]  # the maximum, once more behind it
    D = rng.choice([0, 1, 255, 256, 65535], size=tot)
    return R, L, P, D, offs


PARAMS = [(1, 4, 16), (35, 0, 0), (1, 65535, 2**31 - 1), (20, 1, 0), (31, 0, 2**31 - 1), (1 << 33, 4, 16)]
EDGES = [0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2047, 2048, 2049]


@pytest.mark.parametrize("bits", [16, 32])
def test_crafted_reads_of_every_length(gpu, any_index, text, bits):
    rng = np.random.default_rng(bits)
    lens = np.array(EDGES * 3 + list(range(3, 15)) + [70_000, 1_000_000])
    lens = lens[rng.permutation(lens.size)]
    lens = np.r_[[0, 0, 0], lens[:25], [0] * 5, lens[25:], [17] * 16, [5, 0, 0, 61, 0, 0, 0, 0]]  # (16 x 17: every alignment)
    R, L, P, D, offs = _on_diagonals(rng, text, lens, 77, bits)
    assert set((offs[:-1] % 16).tolist()) == set(range(16))  # reads start at every alignment
    longest = whole = at_start = at_end = 0
    for i, params in enumerate(PARAMS):
        want = _check(any_index, text, R, L, P, offs, params, bits, D if i % 2 == 0 else None)
        ok = want["ref_start"] != np.uint64(UNPLACED)
        if params[0] == 1 << 33:
            assert not ok.any()  # every read unplaced
            continue
        assert ok.sum() >= 30 and set(want["doc"][ok].tolist()) >= ({0, 65535} if i % 2 == 0 else {NO_DOC})
        span = want["read_end"][ok].astype(np.int64) - want["read_start"][ok]
        longest = max(longest, int(span.max()))
        at_start += int((want["ref_start"][ok] == 0).sum())
        at_end += int((want["ref_start"][ok].astype(np.int64) + span == text.size).sum())
        whole += int((ok & (want["seed_pos"] == 0) & (want["seed_len"] == np.diff(offs.astype(np.int64)))).sum())
    assert longest > 500_000 and at_start and at_end and whole >= 5  # (what the batch was made for)


@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("nreads", [0, 1, 3, 4, 5, 63, 64, 65, 3000])
def test_read_counts_around_the_group_count(gpu, any_index, text, bits, nreads):
    rng = np.random.default_rng(nreads)
    R, L, P, D, offs = _on_diagonals(rng, text, rng.integers(0, 260, nreads), 0, bits)
    _check(any_index, text, R, L, P, offs, (1, 4, 16), bits, D)
    _check(any_index, text, R, L, P, offs, (35, 2, 5), bits)


@pytest.mark.parametrize("bits", [16, 32])
def test_ties_of_the_maximum_go_to_the_smaller_position(gpu, any_index, text, bits):
    """Two positions with the largest length: in neighbouring lanes, in different vectors, and in different rounds of the
    group's (128 or 64 values) and of the wavefront's (512 or 256 values) loop over the read."""
    shapes = [(100, 5, 6), (100, 5, 20), (100, 7, 9), (300, 7, 200), (300, 130, 299), (2000, 3, 1999), (5000, 10, 11),
              (5000, 10, 300), (5000, 10, 4000), (5000, 700, 4999)]
    rng = np.random.default_rng(5)
    R, L, P, D, offs = _on_diagonals(rng, text, [m for m, _, _ in shapes], 3, bits)
    for (m, a, b), o in zip(shapes, offs[:-1].astype(np.int64)):
        L[o:o + m] = np.minimum(L[o:o + m], 30)
        L[o + a] = L[o + b] = 44
    want = _check(any_index, text, R, L, P, offs, (1, 4, 16), bits, D)
    assert want["seed_pos"].tolist() == [a for _, a, _ in shapes] and (want["seed_len"] == 44).all()


DISTANCES = [15, 16, 17, 63, 64, 65, 1023, 1024, 1025]


@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("wide", [False, True], ids=["group", "wavefront"])
def test_an_extension_stops_one_above_the_drop_and_not_at_it(gpu, any_index, text, bits, wide):
    """Reads that equal the text but for two neighbouring characters, the second at distance d from the seed's edge: with
    penalty 4 the drop there is 8.  x_drop 7 stops the side at step d with its best d - 2 steps out, in the lane before
    for d = 16, 17, 64, ...; x_drop 8 does not stop it and the side runs to the read's end."""
    seed_len, tail = 8, 40
    reads = []
    for side in ("left", "right"):
        for d in DISTANCES:
            near, far = d + tail, (2100 if wide else 5)  # characters on the side under test, and on the other one
            reads.append((side, d, far if side == "right" else near, near if side == "right" else far))
    lens = [a + seed_len + b for _, _, a, b in reads]
    offs = (9 + np.r_[0, np.cumsum(lens)]).astype(np.uint64)
    tot = int(offs[-1])
    R, L, P = np.zeros(tot, dtype=np.uint8), np.zeros(tot, dtype=np.int64), np.zeros(tot, dtype=np.uint64)
    rng = np.random.default_rng(6)
    for (side, d, before, behind), o, m in zip(reads, offs[:-1].astype(np.int64), lens):
        at = int(rng.integers(10, text.size - m - 10))
        R[o:o + m] = text[at:at + m]
        P[o:o + m] = at + np.arange(m)
        L[o + before] = seed_len
        for step in (d - 1, d):
            j = before + seed_len + step - 1 if side == "right" else before - step
            R[o + j] = DNA[(DNA.index(int(R[o + j])) + 1) % 4]
    for x_drop in (7, 8):
        want = _check(any_index, text, R, L, P, offs, (8, 4, x_drop), bits)
        for (side, d, before, behind), r, m in zip(reads, want, lens):
            left, right = before - int(r["read_start"]), int(r["read_end"]) - before - seed_len
            near, other = (left, right) if side == "left" else (right, left)
            assert other == (behind if side == "left" else before), (side, d, x_drop)
            assert near == (d - 2 if x_drop == 7 else d + tail), (side, d, x_drop, near)
            assert int(r["matches"]) == (m - 2 if x_drop == 8 else m - tail - 2)


def _mix(seed, nreads, longest, text, bits):
    rng = np.random.default_rng(seed)
    lens = np.minimum((rng.pareto(1.1, nreads) * 30).astype(np.int64), 20_000)
    lens[rng.integers(0, nreads)] = longest
    return _on_diagonals(rng, text, lens, 0, bits)


def test_repeated_call_and_split_batch_give_the_same_bytes(gpu, any_index, text):
    for bits in (16, 32):
        R, L, P, D, offs = _mix(15, 3000, 100_000, text, bits)
        nreads = offs.size - 1
        d = [_to_device(R, 8), _to_device(L, bits), _to_device(P, 64)]
        d_D, d_offs = _to_device(D, bits), _to_device(offs, 64)
        whole = any_index.place_device(*d, d_offs, 20, d_docs=d_D)
        again = any_index.place_device(*d, d_offs, 20, d_docs=d_D)
        torch.cuda.synchronize()
        assert whole.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
        assert np.array_equal(_records(whole), place_reference(R, L, P, offs, text, 20, docs=D))
        for cut in (1, 1234, nreads - 1):
            a = any_index.place_device(*d, d_offs[: cut + 1], 20, d_docs=d_D)
            b = any_index.place_device(*d, d_offs[cut:], 20, d_docs=d_D)
            torch.cuda.synchronize()
            assert torch.cat([a, b]).cpu().numpy().tobytes() == whole.cpu().numpy().tobytes(), (bits, cut)


def test_a_second_query_context_has_its_own_scratch(gpu, any_index, text):
    R, L, P, D, offs = _mix(16, 500, 5000, text, 16)
    other = any_index.clone(0)
    want = place_reference(R, L, P, offs, text, 25)
    a = _run(any_index, R, L, P, offs, (25, 4, 16), 16)
    b = _run(other, R, L, P, offs, (25, 4, 16), 16)
    assert np.array_equal(a, want) and np.array_equal(b, want)
    assert other.place_stats()["placed"] == any_index.place_stats()["placed"] == int((want["ref_start"] != np.uint64(UNPLACED)).sum())
    other.close()


def test_argument_errors(gpu, any_index, text):
    R, L, P, D, offs = _on_diagonals(np.random.default_rng(1), text, [10, 30], 0, 16)
    d_R, d_L, d_P, d_offs = _to_device(R, 8), _to_device(L, 16), _to_device(P, 64), _to_device(offs, 64)
    with pytest.raises(capi.SpxError, match="min_seed must be at least 1"):
        any_index.place_device(d_R, d_L, d_P, d_offs, 0)
    with pytest.raises(capi.SpxError, match="mismatch_penalty must be 0 .. 65535"):
        any_index.place_device(d_R, d_L, d_P, d_offs, 1, mismatch_penalty=65536)
    with pytest.raises(capi.SpxError, match="x_drop must be 0 .. 2\\^31 - 1"):
        any_index.place_device(d_R, d_L, d_P, d_offs, 1, x_drop=2**31)
    with pytest.raises(capi.SpxError, match="16-byte aligned"):
        any_index.place_device(d_R, d_L[1:], d_P, d_offs, 1)
    with pytest.raises(capi.SpxError, match="16-byte aligned"):
        any_index.place_device(d_R, d_L, d_P, d_offs, 1, d_out=torch.empty(20, dtype=torch.int32, device="cuda")[1:17].view(2, 8))
    with pytest.raises(capi.SpxError, match="same width"):
        any_index.place_device(d_R, d_L, d_P, d_offs, 1, d_docs=_to_device(L, 32))
    out = torch.full((3, 8), FENCE, dtype=torch.int32, device="cuda")
    S = capi._spp()
    rc = S.spp_place_device(any_index._h, d_R.data_ptr(), d_L.data_ptr(), 8, d_P.data_ptr(), None, d_offs.data_ptr(), 2, 40, 1, 4, 16,
                            out.data_ptr(), None)
    assert rc == -1 and b"value_bits" in capi.lib().spx_last_error()
    # more values than total_values said: the reads behind it are not looked at, and the stats say so
    R, L, P, D, offs = _on_diagonals(np.random.default_rng(2), text, [100, 4900], 0, 16)
    got = _run(any_index, R, L, P, offs, (1, 4, 16), 16, total_values=1000)
    with pytest.raises(capi.SpxError, match="spx error -5: the batch holds more values than total_values"):
        any_index.place_stats()
    want = place_reference(R, L, P, offs, text, 1)
    assert got[0] == want[0] and got[1].tolist() == (UNPLACED, 0, 0, 0, 0, 0, NO_DOC)
    without_text = capi.Index.from_raw(synth.statistical_rlbwt(2000, 20, 3.0, seed=1, with_samples=True, n_docs=4), 0)
    with pytest.raises(capi.SpxError, match="spx_index_set_text / spx_index_rebuild_text"):
        without_text.place_device(d_R, d_L, d_P, d_offs, 1)
    with pytest.raises(capi.SpxError, match="spx_index_set_text / spx_index_rebuild_text"):
        without_text.place_host(np.frombuffer(b"ACGT", dtype=np.uint8), [0, 4], 1)
    without_text.close()


# ---- place_host against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, capi.SPX_DIGEST_PROMOTED, capi.SPX_DIGEST_DNA])
def test_place_host_on_a_real_text_built_on_the_device(gpu, oracle_mod, kind):
    """Several documents, indexed by capi.build_raw (digested first for -m / -a); DNA reads through digestion, walk, MS
    extension and the placement in one call, 16-bit arrays and -- with a read of 70 000 characters -- 32-bit ones."""
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
    placed = 0
    for s, o in ((seqs, offs), wide):
        o = o.astype(np.uint64)
        dseqs, doffs = oracle_mod.digest_batch(kind, k, w, s, o) if kind else (s, o)
        values = np.diff(doffs.astype(np.int64))
        ms = orc.ms(dseqs, doffs, want_docs=True, text=text)
        top = int(ms["lengths"].max())
        for params, want_docs in (((1, 4, 16), True), ((6, 0, 0), False), ((6, 2, 30), True), ((top + 1, 4, 16), True)):
            want = place_reference(dseqs, ms["lengths"], ms["pointers"], doffs, text, *params, docs=ms["docs"] if want_docs else None)
            got, vals = ix.place_host(s, o, *params, digest=(kind, k, w) if kind else None, want_docs=want_docs)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (params, want_docs, bad[:5], got[bad[:5]], want[bad[:5]])
            assert np.array_equal(vals, values)
            ok = want["ref_start"] != np.uint64(UNPLACED)
            assert not ok.any() if params[0] > top else ok.any()
            placed += int(ok.sum())
            if want_docs and params[0] == 1:
                assert len(set(want["doc"][ok].tolist())) >= 2  # (seeds in more than one document)
            st = ix.place_stats()
            assert st["placed"] == int(ok.sum()) and st["values"] == int(values.sum()) and st["seed_values"] == int(want["seed_len"].sum()), st
    assert placed > 500  # (the batches place enough reads for the comparison to mean something)
    with pytest.raises(capi.SpxError, match="spx error -1: min_seed must be at least 1"):
        ix.place_host(seqs, offs, 0)
    ix.close()


def test_place_host_in_several_pieces(gpu, oracle_mod):
    """More reads than one piece of the pipeline holds (4 Mi): the records of every piece land where they belong."""
    rng = np.random.default_rng(31)
    text = np.asarray(DNA, dtype=np.uint8)[rng.integers(0, 4, 100_000)]
    raw = capi.build_raw(text)
    ix = capi.Index.from_raw(raw, 0)
    nreads = (4 << 20) + 50_000
    lens = np.ones(nreads, dtype=np.int64)
    real = np.arange(0, nreads, 997)
    lens[real] = 150
    offs = np.r_[0, np.cumsum(lens)].astype(np.uint64)
    seqs = np.full(int(offs[-1]), ord("A"), dtype=np.uint8)
    for q, at in zip(real, rng.integers(0, text.size - 150, real.size)):
        seqs[int(offs[q]):int(offs[q]) + 150] = text[at:at + 150]
        seqs[int(offs[q]) + 60] = ord("N")
    ms = oracle_mod.OracleIndex.from_raw(raw).ms(seqs, offs, text=text)
    want = place_reference(seqs, ms["lengths"], ms["pointers"], offs, text, 20)
    got, vals = ix.place_host(seqs, offs, 20)
    assert np.array_equal(got, want) and np.array_equal(vals, lens)
    placed = np.flatnonzero(want["ref_start"] != np.uint64(UNPLACED))
    assert np.array_equal(placed, real) and placed[-1] > (4 << 20) and (want["read_end"][real] == 150).all()
    assert ix.place_stats()["placed"] == real.size and ix.place_stats()["values"] == int(offs[-1])
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


def _parse_reads(path):
    """The reads of a FASTA or FASTQ file as the walk sees them: the sequence lines joined, upper-cased."""
    lines = open(path, "rb").read().split(b"\n")
    reads = []
    if lines[0].startswith(b"@"):
        return [lines[i + 1].upper() for i in range(0, len(lines) - 3, 4)]
    for line in lines:
        if line.startswith(b">"):
            reads.append(b"")
        elif reads:
            reads[-1] += line.upper()
    return reads


def _cli(args, env):
    return subprocess.run([HOST_BIN] + args, capture_output=True, env=env, timeout=300)  # (every child has its time limit)


@pytest.mark.parametrize("case", ["dna_multiline_fasta", "dna_fastq", "promoted_alphabet_fasta"])
def test_cli_place_equals_the_reference_over_the_golden_files(gpu, tmp_path, case):
    work = tmp_path / case
    shutil.copytree(os.path.join(FILES, case), work)
    ref, reads = str(work / "ref"), str(work / "reads.fa")
    env = dict(os.environ, SPUMONI_TEXT=ref + ".fa.rawtext", SPUMONI_SUPER_BATCH="3000")
    gold = os.path.join(FILES, case, "expected_M", "reads.fa")
    ids, L = _parse_values(gold + ".lengths")
    _, P = _parse_values(gold + ".pointers")
    _, D = _parse_values(gold + ".doc_numbers")
    R = _parse_reads(reads)[: len(ids)]  # (FASTQ: the reference drops the file's last batch, and so does the command)
    assert [len(r) for r in R] == [v.size for v in L]
    offs = np.r_[0, np.cumsum([v.size for v in L])].astype(np.uint64)
    L, P, D, R = np.concatenate(L), np.concatenate(P), np.concatenate(D), np.frombuffer(b"".join(R), dtype=np.uint8)
    text = np.fromfile(ref + ".fa.rawtext", dtype=np.uint8)
    both = 0
    for extra, params, docs in ((["-L", "4", "-d"], (4, 4, 16), True), (["-B", "0", "-X", "0", "-L", "8"], (8, 0, 0), False),
                                (["-L", "4", "-M"], (4, 4, 16), False)):
        if os.path.exists(reads + ".placements"):
            os.remove(reads + ".placements")
        r = _cli(["place", "-r", ref, "-p", reads, "-n"] + extra, env)
        assert r.returncode == 0, r.stderr.decode()
        want = place_reference(R, L, P, offs, text, *params, docs=D if docs else None)
        lines = []
        for q in range(len(ids)):
            w = want[q]
            ok = w["ref_start"] != np.uint64(UNPLACED)
            f = [ids[q]] + [str(int(x)).encode() for x in (offs[q + 1] - offs[q], w["read_start"], w["read_end"])]
            f += [str(int(w["ref_start"])).encode() if ok else b"-1"] + [str(int(w[x])).encode() for x in ("matches", "seed_pos", "seed_len")]
            lines.append(b"\t".join(f + ([str(int(w["doc"])).encode() if ok else b"-1"] if docs else [])) + b"\n")
        assert open(reads + ".placements", "rb").read() == b"".join(lines), (extra, r.stderr.decode())
        placed = int((want["ref_start"] != np.uint64(UNPLACED)).sum())
        assert f"{len(ids)} reads, {placed} placed, {len(ids) - placed} unplaced".encode() in r.stderr
        both += 0 < placed < len(ids)
    assert both  # both outcomes are exercised
    assert sorted(f for f in os.listdir(work) if f.startswith("reads.fa")) == ["reads.fa", "reads.fa.placements"]


def test_cli_place_writes_no_file_when_it_fails(gpu, tmp_path):
    work = tmp_path / "c"
    shutil.copytree(os.path.join(FILES, "dna_multiline_fasta"), work)
    text = open(work / "ref.fa.rawtext", "rb").read()
    with open(work / "reads.fa", "wb") as f:  # a read without characters ends the run, as it ends `run`: behind 40 good ones
        for q in range(40):
            f.write(b">r%d\n" % q + text[17 * q: 17 * q + 60] + b"\n")
        f.write(b">bad_one\n>after\n" + text[:40] + b"\n")
    env = dict(os.environ, SPUMONI_TEXT=str(work / "ref.fa.rawtext"), SPUMONI_SUPER_BATCH="1000")
    before = sorted(os.listdir(work))
    r = _cli(["place", "-r", str(work / "ref"), "-p", str(work / "reads.fa"), "-n", "-L", "4"], env)
    assert r.returncode == 1 and b"bad_one was empty after digestion" in r.stderr, r.stderr.decode()
    assert sorted(os.listdir(work)) == before
