"""CPU tier of the placements: the definition (spumoni_amd/place.py: place_reference) against a plain loop that takes one
character at a time, against a brute-force check over a small text and on a planted case with a known answer, the plain-C
header include/spumoni_place.h and the library's exports, the loud failure without a device, and `spumoni place`'s usage,
validation messages and its failure against a library without the placement kernels.  What the kernels and the command
compute is tests/test_gpu_place.py's business."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from spumoni_amd import capi, synth
from spumoni_amd.place import NO_DOC, PLACEMENT_DTYPE, UNPLACED, place_reference
from tests import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
HEADER = os.path.join(ROOT, "include", "spumoni_place.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "files", "dna_fastq")
M64, M32 = 2**64 - 1, 2**32 - 1


@pytest.fixture(scope="module")
def built(built_all):
    return capi.lib()


def _walk(K, same, penalty, x_drop):
    """(steps, equal characters inside) of one extension; same(k): step k compares equal."""
    s = top = best = best_k = equal = best_equal = 0
    for k in range(1, K + 1):
        eq = same(k)
        s += 1 if eq else -penalty
        equal += 1 if eq else 0
        top = max(top, s)
        if top - s > x_drop:
            break  # (s_k is below the maximum: it cannot be the best)
        if s > best:
            best, best_k, best_equal = s, k, equal
    return best_k, best_equal


def _loop(R, L, P, offs, T, min_seed, penalty, x_drop, D=None):
    out = []
    n_text = len(T)
    for q in range(len(offs) - 1):
        o, m = int(offs[q]), int(offs[q + 1]) - int(offs[q])
        seed, i = -1, 0
        for j in range(m):
            if int(L[o + j]) > seed:
                seed, i = int(L[o + j]), j
        if m == 0 or seed < min_seed:
            out.append((UNPLACED, 0, 0, 0, 0, 0, NO_DOC))
            continue
        p = int(P[o + i])
        e, te = i + seed, (p + seed) & M64
        right, eq_r = _walk(max(min(m - e, n_text - te), 0), lambda k: R[o + e + k - 1] == T[te + k - 1], penalty, x_drop)
        left, eq_l = _walk(min(i, p) if p <= n_text else 0, lambda k: R[o + i - k] == T[p - k], penalty, x_drop)
        out.append((p - left, i - left, (e + right) & M32, (seed + eq_l + eq_r) & M32, i, seed, NO_DOC if D is None else int(D[o + i])))
    return np.array(out, dtype=PLACEMENT_DTYPE) if out else np.zeros(0, dtype=PLACEMENT_DTYPE)


def _random_case(seed, dtype):
    """Reads that lie on a diagonal of a two-letter text with some errors; lengths are random (the rule is one on the
    arrays), pointers mostly on the diagonal, some before the text's start, behind its end, or with P + L behind it."""
    rng = np.random.default_rng(seed)
    T = rng.integers(65, 67, 400).astype(np.uint8)
    lens = rng.integers(0, 90, 120)
    lens[rng.integers(0, 120, 12)] = 0  # empty reads, runs of them: at the front, in the middle, at the end
    lens[:3] = 0
    lens[50:56] = 0
    lens[-2:] = 0
    front = 13 * (seed % 2)  # offs[0] != 0
    offs = (front + np.r_[0, np.cumsum(lens)]).astype(np.uint64)
    tot = int(offs[-1])
    R = rng.integers(65, 67, tot + 5).astype(np.uint8)
    P = rng.integers(0, T.size + 1, tot + 5).astype(np.uint64)
    for o, e in zip(offs[:-1].astype(int), offs[1:].astype(int)):
        d = int(rng.integers(-20, T.size - 10))  # the diagonal: may be cut by the text's start and by its end
        for j in range(e - o):
            if 0 <= d + j < T.size:
                if rng.random() > 0.15:
                    R[o + j] = T[d + j]
                if rng.random() > 0.1:
                    P[o + j] = d + j
    top = 12 if seed < 4 else 60
    L = rng.integers(0, top, tot + 5, endpoint=True).astype(dtype)
    P[rng.integers(0, tot + 5, 20)] = np.uint64(M64)  # behind the text: no left extension; P + L wraps
    P[rng.integers(0, tot + 5, 20)] = np.uint64(T.size + 7)
    D = rng.integers(0, 65536, tot + 5).astype(dtype)
    return R, L, P, offs, T, D, top


@pytest.mark.parametrize("seed,dtype", [(0, np.uint16), (1, np.uint32), (4, np.uint16), (5, np.uint32)])
def test_reference_against_a_plain_loop(seed, dtype):
    R, L, P, offs, T, D, top = _random_case(seed, dtype)
    placed = extended = cut = 0
    for min_seed in (1, top // 2, top + 1):
        for penalty, x_drop in ((4, 16), (0, 16), (4, 0), (0, 0), (65535, 2**31 - 1), (1, 3)):
            for docs in (None, D):
                got = place_reference(R, L, P, offs, T, min_seed, penalty, x_drop, docs)
                want = _loop(R, L, P, offs, T, min_seed, penalty, x_drop, docs)
                assert got.dtype == PLACEMENT_DTYPE and np.array_equal(got, want), (min_seed, penalty, x_drop)
                ok = got["ref_start"] != np.uint64(UNPLACED)
                placed += int(ok.sum())
                extended += int((got["read_end"][ok].astype(np.int64) - got["read_start"][ok] > got["seed_len"][ok]).sum())
                cut += int((got["ref_start"][ok] == 0).sum())
                if min_seed == top + 1:
                    assert not ok.any() and not got["matches"].any() and (got["doc"] == NO_DOC).all()
    assert placed > 500 and extended > 200 and cut > 0


def _one(R, L, P, T, min_seed=1, penalty=4, x_drop=16, D=None):
    R, T = np.frombuffer(R, dtype=np.uint8), np.frombuffer(T, dtype=np.uint8)
    offs = [0, R.size]
    got = place_reference(R, L, P, offs, T, min_seed, penalty, x_drop, D)
    assert np.array_equal(got, _loop(R, L, P, offs, T, min_seed, penalty, x_drop, D))
    return list(got[0].tolist())


def test_reference_shapes_with_known_answers():
    T = b"AAAACCCCGGGGTTTTACGTACGTAACCGGTT"  # 32 characters
    # ties of the maximum: the smaller position is the seed
    assert _one(b"CCGGXXCCGG", [4, 3, 2, 1, 0, 0, 4, 3, 2, 1], [6, 7, 8, 9, 0, 0, 6, 7, 8, 9], T, x_drop=0)[4:6] == [0, 4]
    # a seed at position 0 that covers the whole read: nothing to extend
    assert _one(b"CCGG", [4, 3, 2, 1], [6, 7, 8, 9], T) == [6, 0, 4, 4, 0, 4, NO_DOC]
    # a seed at the read's end: the left extension alone, over a mismatch (1 - 4 + 6 > 1) with x_drop 4, not with 3
    assert _one(b"AAAACCXCGGGG", [0] * 8 + [4, 3, 2, 1], [0] * 8 + [8] * 4, T, x_drop=4, D=np.arange(12)) == [0, 0, 12, 11, 8, 4, 8]
    assert _one(b"AAAACCXCGGGG", [0] * 8 + [4, 3, 2, 1], [0] * 8 + [8] * 4, T, x_drop=3) == [7, 7, 12, 5, 8, 4, NO_DOC]
    # a drop equal to x_drop does not stop; penalty 0 never drops and clips only the trailing mismatches
    assert _one(b"GGGGXTTTXX", [4, 3, 2, 1, 0, 0, 0, 0, 0, 0], [8] * 10, T, penalty=2, x_drop=2)[1:4] == [0, 8, 7]
    assert _one(b"GGGGXTTTXX", [4, 3, 2, 1, 0, 0, 0, 0, 0, 0], [8] * 10, T, penalty=2, x_drop=1)[1:4] == [0, 4, 4]
    assert _one(b"GGGGXTXTXX", [4, 3, 2, 1, 0, 0, 0, 0, 0, 0], [8] * 10, T, penalty=0, x_drop=0)[1:4] == [0, 8, 6]
    # the diagonal cut by the text's start (P[i*] < i*) and by its end; a pointer behind the text; P + L behind the text
    assert _one(b"TTAAAAC", [0, 0, 5, 4, 3, 2, 1], [0, 0, 0, 1, 2, 3, 4], T)[:4] == [0, 2, 7, 5]
    assert _one(b"GGTTAA", [4, 3, 2, 1, 0, 0], [28] * 6, T)[:4] == [28, 0, 4, 4]
    assert _one(b"AGGTT", [0, 4, 3, 2, 1], [40] * 5, T)[:4] == [40, 1, 5, 4]
    assert _one(b"GGGTTAA", [0, 9, 3, 2, 1, 0, 0], [30] * 7, T)[:4] == [29, 0, 10, 10]
    # below min_seed, and the empty read
    assert _one(b"CCGG", [4, 3, 2, 1], [6, 7, 8, 9], T, min_seed=5) == [UNPLACED, 0, 0, 0, 0, 0, NO_DOC]
    assert _one(b"", [], [], T) == [UNPLACED, 0, 0, 0, 0, 0, NO_DOC]
    assert place_reference(b"", [], [], [0], np.frombuffer(T, dtype=np.uint8), 1).size == 0
    for bad in ((0, 4, 16), (1, 65536, 16), (1, -1, 16), (1, 4, 2**31), (1, 4, -1)):
        with pytest.raises(ValueError):
            place_reference(np.frombuffer(b"CCGG", dtype=np.uint8), [4, 3, 2, 1], [6, 7, 8, 9], [0, 4], np.frombuffer(T, dtype=np.uint8), *bad)


def test_reference_places_reads_where_they_fit_on_a_small_text(oracle_mod):
    letters = list(b"ACGT")
    raw, text = cases.real_case(7, 600, letters)
    orc = oracle_mod.OracleIndex.from_raw(raw)
    rng = np.random.default_rng(8)
    seqs, offs = cases.reads_mixed(rng, text, letters, 60, 50)  # (the text's own letters: no length is under-reported)
    w = orc.ms(seqs, offs, text=text)
    placed = 0
    for min_seed, penalty, x_drop in ((1, 4, 16), (6, 4, 16), (6, 0, 0), (6, 1, 2)):
        rec = place_reference(seqs, w["lengths"], w["pointers"], offs, text, min_seed, penalty, x_drop)
        for q in range(offs.size - 1):
            read, r = seqs[int(offs[q]):int(offs[q + 1])], rec[q]
            top = int(w["lengths"][int(offs[q]):int(offs[q + 1])].max(initial=0))
            if top < min_seed:
                assert r["ref_start"] == np.uint64(UNPLACED) and r["matches"] == 0
                continue
            p, a, b, i, n = (int(r[f]) for f in ("ref_start", "read_start", "read_end", "seed_pos", "seed_len"))
            assert n == top and 0 <= a <= i and i + n <= b <= read.size and p + (b - a) <= text.size
            assert int((text[p:p + b - a] == read[a:b]).sum()) == int(r["matches"])
            sp = int(w["pointers"][int(offs[q]) + i])
            assert sp - i == p - a and bytes(text[sp:sp + n]) == bytes(read[i:i + n])  # on the diagonal; the seed is exact
            placed += 1
    assert placed > 100


def test_planted_reads_come_back_where_they_were_cut(oracle_mod):
    """150 characters cut from an i.i.d. text with substitutions at 20, 75 and 130: the seed is the 54-mer behind the first
    one (the one behind the second is as long: the smaller position wins), and the defaults extend it over all three."""
    rng = np.random.default_rng(2024)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    text = letters[rng.integers(0, 4, 20_000)]
    cuts = rng.integers(0, text.size - 150, 40)
    reads = []
    for c in cuts:
        rd = text[c:c + 150].copy()
        for at in (20, 75, 130):
            rd[at] = letters[(int(np.flatnonzero(letters == rd[at])[0]) + 1 + int(rng.integers(0, 3))) % 4]  # a different letter
            assert rd[at] != text[c + at]
        assert bytes(text).count(bytes(rd[21:75])) == 1  # the test's own precondition: the 54-mer occurs once
        reads.append(rd)
    seqs = np.concatenate(reads)
    offs = np.arange(0, 150 * len(reads) + 1, 150).astype(np.uint64)
    raw = synth.index_from_text(torch.from_numpy(text))
    w = oracle_mod.OracleIndex.from_raw(raw).ms(seqs, offs, text=text)
    rec = place_reference(seqs, w["lengths"], w["pointers"], offs, text, 20)  # penalty 4, x_drop 16: the defaults
    assert rec.size == len(cuts)
    for q, c in enumerate(cuts):
        assert list(rec[q].tolist()) == [int(c), 0, 150, 147, 21, 54, NO_DOC], (q, rec[q])


def _declared():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return code, sorted(set(re.findall(r"\b(spp_[a-z_0-9]+)\s*\(", code)))


def test_place_header_is_plain_c(tmp_path):
    src = tmp_path / "p.c"
    src.write_text('#include "spumoni_place.h"\nint main(void) { spp_placement p; spp_place_stats s; (void)p; (void)s; '
                   'return sizeof(spp_placement) == 32 && SPP_UNPLACED + 1 == 0 && SPP_NO_DOC == 4294967295u ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "p"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "p")]).returncode == 0
    code, _ = _declared()
    assert "hipStream_t" not in code and "std::" not in code and "#include <hip" not in code
    assert re.findall(r'#include\s+[<"]([^>"]+)', code) == ["stdint.h", "spumoni_gpu.h"]


def test_place_header_symbols_exported(built):
    _, names = _declared()
    assert names == sorted(capi.PLACE_EXPORTS) and len(names) in (3, 4)
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(spp_[a-z_0-9]+)\b", out))) == names
    for other in (capi.EXPORTS, capi.DOCVOTE_EXPORTS, capi.MEMS_EXPORTS, capi.REFTEXT_EXPORTS):
        assert not set(capi.PLACE_EXPORTS) & set(other)
    assert np.dtype(PLACEMENT_DTYPE).itemsize == 32
    assert PLACEMENT_DTYPE.names == ("ref_start", "read_start", "read_end", "matches", "seed_pos", "seed_len", "doc")


def test_place_batch_without_device_fails_loudly(built):
    if built.spx_device_count() > 0:
        pytest.skip("a device is visible: the no-device path is this machine's CPU tier")
    L = capi._spp()
    seqs, offs = np.frombuffer(b"ACGT", dtype=np.uint8), np.array([0, 4], dtype=np.uint64)
    out = np.zeros(1, dtype=PLACEMENT_DTYPE)
    rc = L.spp_place_batch(None, 0, 0, 0, seqs.ctypes.data, offs.ctypes.data, 1, 1, 4, 16, 0, out.ctypes.data, None)
    assert rc == -3 and b"no CPU fallback" in L.spx_last_error()


def _place(args, cwd, env=None):
    return subprocess.run([BIN, "place"] + args, cwd=cwd, capture_output=True, text=True, env=env, timeout=120)


def test_usage_without_arguments(built, tmp_path):
    r = _place([], str(tmp_path))
    assert r.returncode == 1
    assert "spumoni place - " in r.stderr
    for opt in ("-h, --help", "-r, --ref", "-p, --pattern", "-n, --no-digest", "-m, --minimizer-alphabet", "-a, --dna-minimizer",
                "-K, --small-window", "-W, --large-window", "-d, --doc-array", "-L, --min-seed", "-B, --mismatch-penalty",
                "-X, --x-drop"):
        assert opt in r.stderr, opt
    assert "-P, --PML" not in r.stderr
    top = subprocess.run([BIN], capture_output=True, text=True)
    assert top.returncode == 1
    for cmd in ("place", "mems", "assign", "run", "build"):
        assert f"\t{cmd}\t" in top.stderr, cmd


def _index(tmp_path, doc=True):
    for f in os.listdir(GOLDEN):
        if os.path.isfile(os.path.join(GOLDEN, f)) and (doc or not f.endswith(".doc")):
            shutil.copy(os.path.join(GOLDEN, f), tmp_path / f)
            if f.startswith("ref.fa"):  # the same files under the name -m looks for
                shutil.copy(os.path.join(GOLDEN, f), tmp_path / ("ref.bin" + f[len("ref.fa"):]))


@pytest.mark.parametrize("args,message", [
    (["-p", "reads.fa", "-n"], "Both a reference file (-r) and pattern file (-p) must be provided."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-P"], "-P cannot be used with `spumoni place`"),
    (["-r", "ref", "-p", "reads.fa", "-n", "-M", "-P"], "-P cannot be used with `spumoni place`"),
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
    (["-r", "ref", "-p", "reads.fa", "-n", "-L", "0"], "the minimum seed length (-L) must be at least 1."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-B", "65536"], "the mismatch penalty (-B) must be between 0 and 65535."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-X", "2147483648"], "the x-drop (-X) must be between 0 and 2147483647."),
])
def test_validation_messages(built, tmp_path, args, message):
    _index(tmp_path)
    shutil.copy(tmp_path / "reads.fa", tmp_path / "reads.txt")
    before = sorted(os.listdir(tmp_path))
    r = _place(args, str(tmp_path))
    assert r.returncode == 1
    assert message in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_doc_ids_without_doc_file_are_refused(built, tmp_path):
    _index(tmp_path, doc=False)
    before = sorted(os.listdir(tmp_path))
    r = _place(["-r", "ref", "-p", "reads.fa", "-n", "-d"], str(tmp_path))
    assert r.returncode == 1
    assert "document array file (ref.fa.doc) is not present, so it cannot be used." in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_missing_entry_point_on_the_fake_device(built, fake_device, tmp_path):
    _index(tmp_path)
    before = sorted(os.listdir(tmp_path))
    env = dict(os.environ, LD_LIBRARY_PATH=fake_device + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = _place(["-r", "ref", "-p", "reads.fa", "-n", "-L", "4"], str(tmp_path), env=env)
    assert r.returncode == 1
    assert "has no spp_place_batch" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_no_device_fails_loudly_and_writes_nothing(built, tmp_path):
    if built.spx_device_count() > 0:
        pytest.skip("a device is visible: the no-device path is this machine's CPU tier")
    _index(tmp_path)
    before = sorted(os.listdir(tmp_path))
    r = _place(["-r", "ref", "-p", "reads.fa", "-n", "-d"], str(tmp_path))
    assert r.returncode == 1
    assert "no usable gfx950 device" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before
