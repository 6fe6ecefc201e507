"""CPU tier of the matches: the definition (spumoni_amd/mems.py: mems_reference) against a plain loop and against a
brute-force MEM finder over a small text, the plain-C header include/spumoni_mems.h and the library's exports, the loud
failure without a device, and `spumoni mems`' usage, validation messages and its failure against a library without the
match kernels.  What the kernels and the command compute is tests/test_gpu_mems.py's business."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from spumoni_amd import capi
from spumoni_amd.mems import MATCH_DTYPE, mems_reference
from tests import brute, cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
HEADER = os.path.join(ROOT, "include", "spumoni_mems.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "files", "dna_fastq")


@pytest.fixture(scope="module")
def built(built_all):
    return capi.lib()


def _loop(L, P, offs, min_length, D=None):
    moffs, rec, docs = [0], [], []
    for q in range(len(offs) - 1):
        o, e = int(offs[q]), int(offs[q + 1])
        for i in range(o, e):
            if (i == o or int(L[i]) >= int(L[i - 1])) and int(L[i]) >= min_length:
                rec.append((int(P[i]), i - o, int(L[i])))
                docs.append(0 if D is None else int(D[i]))
        moffs.append(len(rec))
    return np.array(moffs, dtype=np.uint64), np.array(rec, dtype=MATCH_DTYPE), np.array(docs, dtype=np.uint32)


def _same(got, want, with_docs):
    assert got[0].dtype == np.uint64 and np.array_equal(got[0], want[0])
    assert got[1].dtype == MATCH_DTYPE and np.array_equal(got[1], want[1])
    if with_docs:
        assert got[2].dtype == np.uint32 and np.array_equal(got[2], want[2])
    else:
        assert len(got) == 2


@pytest.mark.parametrize("seed,dtype", [(0, np.uint16), (1, np.uint32), (2, np.uint16), (3, np.uint32)])
def test_reference_against_a_plain_loop(seed, dtype):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 40, 300)
    lens[rng.integers(0, 300, 30)] = 0  # empty reads, runs of them: at the front, in the middle, at the end
    lens[:4] = 0
    lens[100:110] = 0
    lens[-3:] = 0
    front = 13 * (seed % 2)  # offs[0] != 0
    offs = (front + np.r_[0, np.cumsum(lens)]).astype(np.uint64)
    tot = int(offs[-1])
    top = 12 if seed < 2 else np.iinfo(dtype).max
    L = rng.integers(0, top, tot, endpoint=True).astype(dtype)
    P = rng.integers(0, 1 << 63, tot, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    P[L == 0] = np.uint64(2**64 - 1)
    D = rng.integers(0, 65536, tot).astype(dtype)
    for min_length in (1, 6, int(top), int(top) + 1, 1 << 40):
        for docs in (None, D):
            _same(mems_reference(L, P, offs, min_length, docs), _loop(L, P, offs, min_length, docs), docs is not None)
    above = mems_reference(L, P, offs, int(top) + 1)
    assert above[1].size == 0 and not above[0].any()
    ones = mems_reference(L, P, offs, 1)
    assert (ones[1]["length"] > 0).all() and (ones[1]["ref_pos"] != np.uint64(2**64 - 1)).all()  # a length of 0 never comes out


def test_reference_shapes_with_known_answers():
    P = np.arange(100, 112, dtype=np.uint64)
    const = np.full(12, 5, dtype=np.uint16)  # constant lengths: every position starts
    mo, rec = mems_reference(const, P, [0, 12], 5)
    assert mo.tolist() == [0, 12] and rec["read_pos"].tolist() == list(range(12)) and rec["ref_pos"].tolist() == P.tolist()
    falling = np.arange(12, 0, -1).astype(np.uint32)  # strictly falling: only position 0 starts
    mo, rec = mems_reference(falling, P, [0, 12], 1)
    assert mo.tolist() == [0, 1] and rec.tolist() == [(100, 0, 12)]
    # a read whose predecessor ends on a larger value: its first position starts all the same
    L = np.array([9, 9, 9, 2, 1, 7, 6], dtype=np.uint16)
    mo, rec, docs = mems_reference(L, P[:7], [0, 3, 3, 5, 7], 2, docs=np.arange(7))
    assert mo.tolist() == [0, 3, 3, 4, 5]
    assert rec.tolist() == [(100, 0, 9), (101, 1, 9), (102, 2, 9), (103, 0, 2), (105, 0, 7)] and docs.tolist() == [0, 1, 2, 3, 5]
    assert mems_reference(L, P[:7], [3, 5], 1)[1].tolist() == [(103, 0, 2)]  # offs[0] != 0
    mo, rec = mems_reference(L, P[:7], [0], 1)
    assert mo.tolist() == [0] and rec.size == 0
    with pytest.raises(ValueError):
        mems_reference(L, P[:7], [0, 7], 0)


def _brute_mems(text, read, min_length):
    """(read_pos, length) of the maximal exact matches: right-maximal by true_ms, left-maximal when the match of the
    position before does not reach as far."""
    ms = brute.true_ms(text, read)
    return [(i, ms[i]) for i in range(len(ms)) if ms[i] >= min_length and (i == 0 or ms[i - 1] < ms[i] + 1)]


def test_reference_finds_the_maximal_exact_matches_of_a_small_text(oracle_mod):
    letters = list(b"ACGT")
    raw, text = cases.real_case(7, 600, letters)
    orc = oracle_mod.OracleIndex.from_raw(raw)
    rng = np.random.default_rng(8)
    seqs, offs = cases.reads_mixed(rng, text, letters, 60, 50)  # (the text's own letters: no length is under-reported)
    w = orc.ms(seqs, offs, text=text)
    found = 0
    for min_length in (1, 4, 8):
        mo, rec = mems_reference(w["lengths"], w["pointers"], offs, min_length)
        for q in range(offs.size - 1):
            read = seqs[int(offs[q]):int(offs[q + 1])]
            mine = rec[int(mo[q]):int(mo[q + 1])]
            assert list(zip(mine["read_pos"].tolist(), mine["length"].tolist())) == _brute_mems(text, read, min_length), (q, min_length)
            for r in mine:
                p, i, n = int(r["ref_pos"]), int(r["read_pos"]), int(r["length"])
                assert bytes(text[p:p + n]) == bytes(read[i:i + n])
            found += mine.size
    assert found > 100


def _declared():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return code, sorted(set(re.findall(r"\b(spm_[a-z_0-9]+)\s*\(", code)))


def test_mems_header_is_plain_c(tmp_path):
    src = tmp_path / "m.c"
    src.write_text('#include "spumoni_mems.h"\nint main(void) { spm_match m; spm_mems_stats s; (void)m; (void)s; '
                   'return sizeof(spm_match) == 16 ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "m"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "m")]).returncode == 0
    code, _ = _declared()
    assert "hipStream_t" not in code and "std::" not in code and "#include <hip" not in code


def test_mems_header_symbols_exported(built):
    _, names = _declared()
    assert names == sorted(capi.MEMS_EXPORTS) and len(names) == 4
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(spm_[a-z_0-9]+)\b", out))) == names
    assert not set(capi.MEMS_EXPORTS) & set(capi.EXPORTS)  # spumoni_gpu.h stays as it is
    assert not set(capi.MEMS_EXPORTS) & set(capi.DOCVOTE_EXPORTS)
    assert np.dtype(MATCH_DTYPE).itemsize == 16


def test_mems_begin_without_device_fails_loudly(built):
    if built.spx_device_count() > 0:
        pytest.skip("a device is visible: the no-device path is this machine's CPU tier")
    L = capi._spm()
    seqs, offs = np.frombuffer(b"ACGT", dtype=np.uint8), np.array([0, 4], dtype=np.uint64)
    mo, n = np.zeros(2, dtype=np.uint64), capi.C.c_uint64()
    rc = L.spm_mems_begin(None, 0, 0, 0, seqs.ctypes.data, offs.ctypes.data, 1, 1, 0, mo.ctypes.data, None, capi.C.byref(n))
    assert rc == -3 and b"no CPU fallback" in L.spx_last_error()


def _mems(args, cwd, env=None):
    return subprocess.run([BIN, "mems"] + args, cwd=cwd, capture_output=True, text=True, env=env, timeout=120)


def test_usage_without_arguments(built, tmp_path):
    r = _mems([], str(tmp_path))
    assert r.returncode == 1
    assert "spumoni mems - " in r.stderr
    for opt in ("-h, --help", "-r, --ref", "-p, --pattern", "-n, --no-digest", "-m, --minimizer-alphabet", "-a, --dna-minimizer",
                "-K, --small-window", "-W, --large-window", "-d, --doc-array", "-L, --min-length"):
        assert opt in r.stderr, opt
    assert "-P, --PML" not in r.stderr
    top = subprocess.run([BIN], capture_output=True, text=True)
    assert top.returncode == 1 and "\tmems\t" in top.stderr and "\tassign\t" in top.stderr and "\trun\t" in top.stderr


def _index(tmp_path, doc=True):
    for f in os.listdir(GOLDEN):
        if os.path.isfile(os.path.join(GOLDEN, f)) and (doc or not f.endswith(".doc")):
            shutil.copy(os.path.join(GOLDEN, f), tmp_path / f)
            if f.startswith("ref.fa"):  # the same files under the name -m looks for
                shutil.copy(os.path.join(GOLDEN, f), tmp_path / ("ref.bin" + f[len("ref.fa"):]))


@pytest.mark.parametrize("args,message", [
    (["-p", "reads.fa", "-n"], "Both a reference file (-r) and pattern file (-p) must be provided."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-P"], "-P cannot be used with `spumoni mems`"),
    (["-r", "ref", "-p", "reads.fa", "-n", "-M", "-P"], "-P cannot be used with `spumoni mems`"),
    (["-r", "nosuch", "-p", "reads.fa", "-n"], "The following path is not valid: nosuch.fa"),
    (["-r", "ref", "-p", "missing.fa", "-n"], "The following path is not valid: missing.fa"),
    (["-r", "ref", "-p", "reads.txt", "-n"], "The pattern file provided does not appear to be a FASTA"),
    (["-r", "ref", "-p", "reads.fa", "-m", "-a"], "Only one type of minimizer can be specified from either -m or -a."),
    (["-r", "ref", "-p", "reads.fa"], "A minimizer type must be specified using -m or -a."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-a"],
     "A minimizer type should not be specified if intending not to use minimizer digestion."),
    (["-r", "ref", "-p", "reads.fa", "-a", "-K", "5", "-W", "11"], "small window size (k) cannot be larger than 4 characters."),
    (["-r", "ref", "-p", "reads.fa", "-a", "-K", "4", "-W", "3"],
     "large window size (w) should be larger than the small window size (k)"),
    (["-r", "ref", "-p", "reads.fa", "-n", "-L", "0"], "the minimum match length (-L) must be at least 1."),
])
def test_validation_messages(built, tmp_path, args, message):
    _index(tmp_path)
    shutil.copy(tmp_path / "reads.fa", tmp_path / "reads.txt")
    before = sorted(os.listdir(tmp_path))
    r = _mems(args, str(tmp_path))
    assert r.returncode == 1
    assert message in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_doc_ids_without_doc_file_are_refused(built, tmp_path):
    _index(tmp_path, doc=False)
    before = sorted(os.listdir(tmp_path))
    r = _mems(["-r", "ref", "-p", "reads.fa", "-n", "-d"], str(tmp_path))
    assert r.returncode == 1
    assert "document array file (ref.fa.doc) is not present, so it cannot be used." in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_missing_entry_point_on_the_fake_device(built, fake_device, tmp_path):
    _index(tmp_path)
    before = sorted(os.listdir(tmp_path))
    env = dict(os.environ, LD_LIBRARY_PATH=fake_device + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = _mems(["-r", "ref", "-p", "reads.fa", "-n", "-L", "4"], str(tmp_path), env=env)
    assert r.returncode == 1
    assert "has no spm_mems_begin" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_no_device_fails_loudly_and_writes_nothing(built, tmp_path):
    if built.spx_device_count() > 0:
        pytest.skip("a device is visible: the no-device path is this machine's CPU tier")
    _index(tmp_path)
    before = sorted(os.listdir(tmp_path))
    r = _mems(["-r", "ref", "-p", "reads.fa", "-n", "-d"], str(tmp_path))
    assert r.returncode == 1
    assert "no usable gfx950 device" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before
