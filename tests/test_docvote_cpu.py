"""CPU tier of the document votes: the definition (spumoni_amd/docvote.py: votes_reference) against a brute-force loop,
the plain-C header include/spumoni_docvote.h and the library's exports, the loud failure without a device, and `spumoni
assign`'s usage, validation messages and its failure against a library without the votes.  What the kernels and the
command compute is tests/test_gpu_docvote.py's business."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from spumoni_amd import capi
from spumoni_amd.docvote import NO_DOC, VOTE_DTYPE, votes_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
HEADER = os.path.join(ROOT, "include", "spumoni_docvote.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "files", "dna_fastq")


@pytest.fixture(scope="module")
def built(built_all):
    return capi.lib()


def _brute(L, D, offs, min_length):
    out = np.zeros(len(offs) - 1, dtype=VOTE_DTYPE)
    for q in range(len(offs) - 1):
        votes = {}
        for i in range(int(offs[q]), int(offs[q + 1])):
            if int(L[i]) >= min_length:
                votes[int(D[i])] = votes.get(int(D[i]), 0) + 1
        ranked = sorted(votes.items(), key=lambda kv: (-kv[1], kv[0]))
        out[q] = (sum(votes.values()), ranked[0][0] if ranked else NO_DOC, ranked[0][1] if ranked else 0,
                  ranked[1][1] if len(ranked) > 1 else 0)
    return out


@pytest.mark.parametrize("seed,ndocs,dtype", [(0, 3, np.uint16), (1, 8, np.uint32), (2, 65536, np.uint16), (3, 2, np.uint32)])
def test_reference_against_brute_force(seed, ndocs, dtype):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 40, 300)
    lens[rng.integers(0, 300, 30)] = 0  # empty reads, runs of them
    lens[100:110] = 0
    offs = np.r_[0, np.cumsum(lens)].astype(np.uint64)
    L = rng.integers(0, 12, int(offs[-1])).astype(dtype)
    D = rng.integers(0, ndocs, int(offs[-1])).astype(dtype)
    D[D == 1] = ndocs - 1  # the largest id takes part
    for min_length in (0, 1, 6, 11, 12, 1 << 40):
        got = votes_reference(L, D, offs, min_length)
        assert got.dtype == VOTE_DTYPE and np.array_equal(got, _brute(L, D, offs, min_length)), min_length
    assert (votes_reference(L, D, offs, 12)["top_doc"] == NO_DOC).all()  # above every value: nobody votes
    assert (votes_reference(L, D, offs, 0)["voters"] == lens).all()      # 0: every position votes


def test_reference_ties_and_offsets_that_do_not_start_at_zero():
    L = np.array([9, 9, 5, 5, 5, 5, 5, 5, 1, 5], dtype=np.uint16)
    D = np.array([7, 7, 4, 2, 4, 2, 9, 9, 3, 3], dtype=np.uint16)
    got = votes_reference(L, D, [2, 8, 8, 10], 5)
    assert got.tolist() == [(6, 2, 2, 2), (0, NO_DOC, 0, 0), (1, 3, 1, 0)]  # three documents with two votes: the smallest id
    assert votes_reference(L, D, [0], 0).size == 0


def test_reference_handles_a_million_reads():
    rng = np.random.default_rng(5)
    n = 1_000_000
    offs = np.arange(n + 1, dtype=np.uint64) * 20
    L = rng.integers(0, 30, n * 20).astype(np.uint16)
    D = rng.integers(0, 8, n * 20).astype(np.uint16)
    got = votes_reference(L, D, offs, 10)
    pick = rng.integers(0, n, 200)
    sub = np.r_[0, np.cumsum(np.full(200, 20))].astype(np.uint64)
    idx = (pick[:, None] * 20 + np.arange(20)[None, :]).ravel()
    assert np.array_equal(got[pick], _brute(L[idx], D[idx], sub, 10))


def _declared():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return code, sorted(set(re.findall(r"\b(spv_[a-z_0-9]+)\s*\(", code)))


def test_docvote_header_is_plain_c(tmp_path):
    src = tmp_path / "v.c"
    src.write_text('#include "spumoni_docvote.h"\nint main(void) { spv_vote v; spv_votes_stats s; (void)v; (void)s; '
                   'return sizeof(spv_vote) == 16 ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "v"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "v")]).returncode == 0
    code, _ = _declared()
    assert "hipStream_t" not in code and "std::" not in code and "#include <hip" not in code


def test_docvote_header_symbols_exported(built):
    _, names = _declared()
    assert names == sorted(capi.DOCVOTE_EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(spv_[a-z_0-9]+)\b", out))) == names
    assert not set(capi.DOCVOTE_EXPORTS) & set(capi.EXPORTS)  # spumoni_gpu.h stays as it is
    assert np.dtype(VOTE_DTYPE).itemsize == 16


def test_assign_batch_without_device_fails_loudly(built):
    if built.spx_device_count() > 0:
        pytest.skip("a device is visible: the no-device path is this machine's CPU tier")
    L = capi._spv()
    seqs, offs = np.frombuffer(b"ACGT", dtype=np.uint8), np.array([0, 4], dtype=np.uint64)
    out = np.zeros(1, dtype=VOTE_DTYPE)
    rc = L.spv_assign_batch(None, 0, 0, 0, 0, seqs.ctypes.data, offs.ctypes.data, 1, 0, out.ctypes.data, None)
    assert rc == -3 and b"no CPU fallback" in L.spx_last_error()


def _assign(args, cwd, env=None):
    return subprocess.run([BIN, "assign"] + args, cwd=cwd, capture_output=True, text=True, env=env, timeout=120)


def test_usage_without_arguments(built, tmp_path):
    r = _assign([], str(tmp_path))
    assert r.returncode == 1
    assert "spumoni assign - " in r.stderr
    for opt in ("-h, --help", "-r, --ref", "-p, --pattern", "-M, --MS", "-P, --PML", "-n, --no-digest", "-m, --minimizer-alphabet",
                "-a, --dna-minimizer", "-K, --small-window", "-W, --large-window", "-T, --min-length"):
        assert opt in r.stderr, opt
    top = subprocess.run([BIN], capture_output=True, text=True)
    assert top.returncode == 1 and "\tassign\t" in top.stderr and "\trun\t" in top.stderr and "\tbuild\t" in top.stderr


def _index(tmp_path, doc=True):
    for f in os.listdir(GOLDEN):
        if os.path.isfile(os.path.join(GOLDEN, f)) and (doc or not f.endswith(".doc")):
            shutil.copy(os.path.join(GOLDEN, f), tmp_path / f)
            if f.startswith("ref.fa"):  # the same files under the name -m looks for
                shutil.copy(os.path.join(GOLDEN, f), tmp_path / ("ref.bin" + f[len("ref.fa"):]))


@pytest.mark.parametrize("args,message", [
    (["-p", "reads.fa", "-P", "-n"], "Both a reference file (-r) and pattern file (-p) must be provided."),
    (["-r", "ref", "-p", "reads.fa", "-n"], "An output type with -M or -P must be specified, only one can be used at a time."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-M", "-P"], "An output type with -M or -P must be specified, only one can be used at a time."),
    (["-r", "nosuch", "-p", "reads.fa", "-P", "-n"], "The following path is not valid: nosuch.fa"),
    (["-r", "ref", "-p", "missing.fa", "-P", "-n"], "The following path is not valid: missing.fa"),
    (["-r", "ref", "-p", "reads.txt", "-P", "-n"], "The pattern file provided does not appear to be a FASTA"),
    (["-r", "ref", "-p", "reads.fa", "-P", "-m", "-a"], "Only one type of minimizer can be specified from either -m or -a."),
    (["-r", "ref", "-p", "reads.fa", "-P"], "A minimizer type must be specified using -m or -a."),
    (["-r", "ref", "-p", "reads.fa", "-P", "-n", "-a"],
     "A minimizer type should not be specified if intending not to use minimizer digestion."),
    (["-r", "ref", "-p", "reads.fa", "-P", "-a", "-K", "5", "-W", "11"], "small window size (k) cannot be larger than 4 characters."),
    (["-r", "ref", "-p", "reads.fa", "-P", "-a", "-K", "4", "-W", "3"],
     "large window size (w) should be larger than the small window size (k)"),
])
def test_validation_messages(built, tmp_path, args, message):
    _index(tmp_path)
    shutil.copy(tmp_path / "reads.fa", tmp_path / "reads.txt")
    before = sorted(os.listdir(tmp_path))
    r = _assign(args, str(tmp_path))
    assert r.returncode == 1
    assert message in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_index_without_doc_is_refused(built, tmp_path):
    _index(tmp_path, doc=False)
    r = _assign(["-r", "ref", "-p", "reads.fa", "-P", "-n"], str(tmp_path))
    assert r.returncode == 1
    assert "document array file (ref.fa.doc) is not present, so it cannot be used." in r.stderr, r.stderr


def test_missing_entry_point_on_the_fake_device(built, fake_device, tmp_path):
    _index(tmp_path)
    before = sorted(os.listdir(tmp_path))
    env = dict(os.environ, LD_LIBRARY_PATH=fake_device + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = _assign(["-r", "ref", "-p", "reads.fa", "-P", "-n"], str(tmp_path), env=env)
    assert r.returncode == 1
    assert "has no spv_assign_batch" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_no_device_fails_loudly_and_writes_nothing(built, tmp_path):
    if built.spx_device_count() > 0:
        pytest.skip("a device is visible: the no-device path is this machine's CPU tier")
    _index(tmp_path)
    before = sorted(os.listdir(tmp_path))
    r = _assign(["-r", "ref", "-p", "reads.fa", "-P", "-n"], str(tmp_path))
    assert r.returncode == 1
    assert "no usable gfx950 device" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before
