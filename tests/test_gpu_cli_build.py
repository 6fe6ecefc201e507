"""-m gpu: `spumoni build` (spumoni_amd/csrc/host/build_main.cpp) and the device text preparation
(include/spumoni_reftext.h, capi.prepare_fasta) against their specification, spumoni_amd/build_index.py: every file of
the CLI byte for byte that of `python -m spumoni_amd.build_index` with the mapped options, the device parser against
read_fasta on random FASTA shapes, the reference's complement table, gzip input, the refusals, and `spumoni run` on a
CLI-built index against the oracle harness."""
import filecmp
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from spumoni_amd import build_index, capi, synth
from tests.test_gpu_cli import _run_both

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
FILES = os.path.join(ROOT, "tests", "golden", "files", "dna_multiline_fasta")
EXTS = [".bwt.heads", ".bwt.len", ".thr_pos", ".ssa", ".esa", ".rawtext", ".fdi", ".pmlnulldb", ".msnulldb"]


@pytest.fixture(scope="module")
def built(built_all):
    assert torch.cuda.is_available()
    assert os.path.exists(BIN)


def _fasta(path, rng, nseq, lo, hi, lower=False, n_runs=False):
    """multi-record, multi-line FASTA of random DNA, some lowercase, some runs of N"""
    with open(path, "w") as f:
        for q in range(nseq):
            g = bytearray(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(rng.integers(lo, hi)))].tobytes())
            if n_runs and len(g) > 400:
                a, ln = int(rng.integers(0, len(g) - 200)), int(rng.integers(20, 200))
                g[a: a + ln] = b"N" * ln
            s = g.decode()
            if lower and q % 2:
                s = s.lower()
            f.write(f">seq{q} some description\n")
            width = int(rng.integers(50, 90))
            for i in range(0, len(s), width):
                f.write(s[i: i + width] + "\n")


def _cli(args, cwd=None):
    return subprocess.run([BIN, "build"] + args, capture_output=True, text=True, cwd=cwd, timeout=600)


def _py(args):
    return subprocess.run(["python", "-m", "spumoni_amd.build_index"] + args, capture_output=True, text=True, cwd=ROOT,
                          timeout=600)


def _same(a_prefix, b_prefix, exts, null_a, null_b):
    for e in exts:
        assert filecmp.cmp(a_prefix + e, b_prefix + e, shallow=False), e
    assert filecmp.cmp(a_prefix, b_prefix, shallow=False)
    assert filecmp.cmp(null_a, null_b, shallow=False)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("inputs")
    rng = np.random.default_rng(5)
    _fasta(d / "a.fa", rng, 5, 300, 3000, lower=True, n_runs=True)
    _fasta(d / "b.fa", rng, 3, 2000, 6000, n_runs=True)
    _fasta(d / "c.fa", rng, 40, 20, 400, lower=True)
    shutil.copy(os.path.join(FILES, "ref.fa"), d / "ref.fa")  # a header and no sequence
    shutil.copy(os.path.join(FILES, "reads.fa"), d / "reads.fa")
    return d


DIGESTS = [("-n", []), ("-m", ["-m"]), ("-t", ["-a"])]


@pytest.mark.parametrize("digest,pyflag", DIGESTS)
@pytest.mark.parametrize("rc", [True, False])
@pytest.mark.parametrize("source", ["single", "golden_reads", "list", "list_ids"])
def test_files_identical_to_build_index(built, inputs, tmp_path, digest, pyflag, rc, source):
    cli_args, py_args = [], []
    if source in ("single", "golden_reads"):
        name = {"single": "a.fa", "golden_reads": "reads.fa"}[source]
        cli_args, py_args = ["-r", str(inputs / name)], ["-r", str(inputs / name)]
    else:
        lst = tmp_path / "list.txt"
        if source == "list":
            lst.write_text(f"{inputs / 'a.fa'}\n{inputs / 'b.fa'}\n{inputs / 'c.fa'}\n")
        else:
            lst.write_text(f"{inputs / 'a.fa'} 1\n{inputs / 'b.fa'} 1\n{inputs / 'c.fa'} 2\n")
        cli_args, py_args = ["-i", str(lst), "-d"], ["-l", str(lst), "--doc"]
    extra_c = [] if rc else ["-c"]
    extra_p = [] if rc else ["--no-rev-comp"]
    (tmp_path / "cli").mkdir()
    (tmp_path / "py").mkdir()
    r = _cli(cli_args + ["-o", str(tmp_path / "cli" / "x"), "-P", "-M", digest] + extra_c)
    assert r.returncode == 0, r.stderr
    p = _py(py_args + ["-o", str(tmp_path / "py" / "x")] + pyflag + extra_p)
    assert p.returncode == 0, p.stderr
    ext = ".bin" if digest == "-m" else ".fa"
    exts = EXTS + ([".doc"] if "-d" in cli_args else [])
    _same(str(tmp_path / "cli" / "x") + ext, str(tmp_path / "py" / "x") + ext, exts,
          str(tmp_path / "cli" / "spumoni_null_reads.fa"), str(tmp_path / "py" / "spumoni_null_reads.fa"))


@pytest.mark.parametrize("window", [50, 400])
def test_window_sizes_identical(built, inputs, tmp_path, window):
    lst = tmp_path / "list.txt"
    lst.write_text(f"{inputs / 'a.fa'}\n{inputs / 'b.fa'}\n")
    (tmp_path / "cli").mkdir()
    (tmp_path / "py").mkdir()
    r = _cli(["-i", str(lst), "-o", str(tmp_path / "cli" / "x"), "-P", "-n", "-w", str(window)])
    assert r.returncode == 0, r.stderr
    p = _py(["-l", str(lst), "-o", str(tmp_path / "py" / "x"), "-w", str(window)])
    assert p.returncode == 0, p.stderr
    _same(str(tmp_path / "cli" / "x.fa"), str(tmp_path / "py" / "x.fa"), EXTS,
          str(tmp_path / "cli" / "spumoni_null_reads.fa"), str(tmp_path / "py" / "spumoni_null_reads.fa"))


def _spec(files, rc):
    """read_fasta + the order of build_index.main, on file contents"""
    text, fwd, ends, sfile, flen = [], [], [], [], []
    tmp = "/dev/shm" if os.path.isdir("/dev/shm") else None
    import tempfile

    for fi, data in enumerate(files):
        with tempfile.NamedTemporaryFile(dir=tmp) as f:
            f.write(data)
            f.flush()
            seqs = build_index.read_fasta(f.name, upper=False)
        total = 0
        for s in seqs:
            fwd.append(s.tobytes())
            ends.append(sum(len(x) for x in fwd))
            sfile.append(fi)
            u = s.tobytes().upper()
            text.append(u)
            total += len(u)
            if rc:
                text.append(_revcomp(u))
                total += len(u)
        flen.append(total)
    return b"".join(text), b"".join(fwd), ends, sfile, flen


_COMP = {ord(a): ord(b) for a, b in zip("ATUCGRYKMBVDH`", "TAAGCYRMKVBHD@")}


def _revcomp(u):
    return bytes(_COMP.get(c, c) for c in reversed(u))


def _random_file(rng):
    parts = []
    pieces = ["\n", "\r\n", "", " ", "\t", "  \t"]
    for _ in range(int(rng.integers(0, 12))):
        kind = rng.integers(0, 6)
        if kind == 0:
            parts.append(">" + "h" * int(rng.integers(0, 5)) + rng.choice(["\n", "\r\n"]))
        elif kind == 1:
            parts.append(rng.choice(pieces) + rng.choice(pieces))  # blank / whitespace-only line
        else:
            s = "".join(rng.choice(list("ACGTNacgtn>R ")) for _ in range(int(rng.integers(0, 40))))
            parts.append(rng.choice(["", " ", "\t"]) + s + rng.choice(["", " ", "\t", "\r"]) + rng.choice(["\n", "\r\n"]))
    data = "".join(parts)
    if data and rng.integers(0, 3) == 0:
        data = data.rstrip("\n")  # no final newline
    return data.encode()


def test_parser_fuzz_against_read_fasta(built):
    rng = np.random.default_rng(11)
    for case in range(220):
        files = [_random_file(rng) for _ in range(int(rng.integers(1, 4)))]
        rc = bool(case % 2)
        want_text, want_fwd, want_ends, want_file, want_len = _spec(files, rc)
        got = capi.prepare_fasta(files, rev_comp=rc)
        assert got["text"].tobytes() == want_text, (case, files)
        assert got["fwd"].tobytes() == want_fwd, (case, files)
        assert got["seq_ends"].tolist() == want_ends, (case, files)
        assert got["seq_file"].tolist() == want_file, (case, files)
        assert got["file_text_lengths"].tolist() == want_len, (case, files)


def _check_all(files, rc):
    want_text, want_fwd, want_ends, want_file, want_len = _spec(files, rc)
    got = capi.prepare_fasta(files, rev_comp=rc)
    assert got["text"].tobytes() == want_text
    assert got["fwd"].tobytes() == want_fwd
    assert got["seq_ends"].tolist() == want_ends
    assert got["seq_file"].tolist() == want_file
    assert got["file_text_lengths"].tolist() == want_len


def test_long_single_line_and_tile_boundaries(built):
    rng = np.random.default_rng(12)
    g = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, 3_000_001)].tobytes()
    files = [b">one\n" + g + b"\n>two\n" + g[:5000].lower() + b"\r\n", b"  " + g[:9000] + b"  \n>x", b""]
    _check_all(files, True)


TILE = 4096  # bytes per tile of the preparation kernels; 16 per thread


def test_parser_fuzz_across_tiles_and_threads(built):
    """random files of several tiles, with a header, a CR, a whitespace run, a line end or a file end placed on purpose at
    tile and thread boundaries (the states that cross them are the scans' business)"""
    rng = np.random.default_rng(21)
    for case in range(40):
        files = []
        for _ in range(int(rng.integers(1, 4))):
            data = bytearray()
            while len(data) < int(rng.integers(2, 5)) * TILE:
                data += _random_file(rng) + b"\n"
            for _ in range(6):  # something that straddles a tile or a thread boundary
                at = int(rng.integers(1, len(data) // TILE + 1)) * TILE - int(rng.integers(0, 3)) * 16 - int(rng.integers(0, 3))
                piece = [b">hdr line\n", b"\r\n", b" \t \t", b"\n\n", b"\n>", b"ACGT \tACGT"][int(rng.integers(0, 6))]
                at = max(0, min(at, len(data)))
                data[at:at] = piece
            files.append(bytes(data))
        if case % 5 == 0:  # a file ending exactly at a tile boundary
            files[0] = (files[0] + b"A" * TILE)[: (len(files[0]) // TILE + 1) * TILE]
        _check_all(files, bool(case % 2))


def test_many_tiles_per_scan_thread(built):
    """an input of over 1024 tiles (the tile-state scan gives each of its threads several tiles)"""
    rng = np.random.default_rng(22)
    lines = []
    size = 0
    while size < 9 * 1024 * 1024:
        r = int(rng.integers(0, 50))
        if r == 0:
            ln = b">h%d\n" % size
        elif r == 1:
            ln = b"  \t\r\n"
        else:
            ln = np.frombuffer(b"ACGTNacgt", dtype=np.uint8)[rng.integers(0, 9, int(rng.integers(1, 3000)))].tobytes()
            ln = b" " * int(rng.integers(0, 2)) + ln + b"\r" * int(rng.integers(0, 2)) + b"\n"
        lines.append(ln)
        size += len(ln)
    data = b"".join(lines)
    _check_all([data[: len(data) // 3], data[len(data) // 3:]], True)


@pytest.mark.parametrize("kind", [capi.SPX_DIGEST_PROMOTED, capi.SPX_DIGEST_DNA])
def test_digested_text_matches_per_piece_digestion(built, inputs, kind):
    files = [open(inputs / n, "rb").read() for n in ("a.fa", "b.fa", "c.fa")]
    got = capi.prepare_fasta(files, rev_comp=True, digest_kind=kind)
    dig = capi.digester(0)
    parts = []
    for data in files:
        import tempfile

        with tempfile.NamedTemporaryFile() as f:
            f.write(data)
            f.flush()
            for s in build_index.read_fasta(f.name):
                for p in (s, np.frombuffer(_revcomp(s.tobytes()), dtype=np.uint8)):
                    out, _ = dig.digest_host(kind, 4, 11, p, np.array([0, p.size], dtype=np.uint64))
                    parts.append(out.tobytes())
    assert got["text"].tobytes() == b"".join(parts)


def test_iupac_text_and_run_against_the_oracle(built, tmp_path):
    rng = np.random.default_rng(13)
    alpha = np.frombuffer(b"ACGTRYKMBVDHSWUN", dtype=np.uint8)
    seqs = [alpha[rng.integers(0, alpha.size, 4000)].tobytes() for _ in range(3)]
    data = b"".join(b">s%d\n" % i + s + b"\n" for i, s in enumerate(seqs))
    got = capi.prepare_fasta([data], rev_comp=True)
    want = b"".join(s + _revcomp(s) for s in seqs)
    assert got["text"].tobytes() == want
    assert bytes(_COMP.get(c, c) for c in b"RYKMBVDHSWUN") == b"YRMKVBHDSWAN"
    (tmp_path / "g.fa").write_bytes(data)
    p = _py(["-r", str(tmp_path / "g.fa"), "-o", str(tmp_path / "py" / "x")])
    assert p.returncode != 0  # build_index refuses the IUPAC codes
    (tmp_path / "idx").mkdir()
    ref = str(tmp_path / "idx" / "x")
    r = _cli(["-r", str(tmp_path / "g.fa"), "-o", ref, "-P", "-M", "-n"])
    assert r.returncode == 0, r.stderr
    prefix = ref + ".fa"
    text = np.fromfile(prefix + ".rawtext", dtype=np.uint8)
    assert text.tobytes() == want
    rs, ro = synth.sample_reads(text, 200, 150, seed=4)
    _run_both(tmp_path, ref, prefix, "reads.fa", rs, ro, rng, ["-c"], "-P")
    _run_both(tmp_path, ref, prefix, "reads.fa", rs, ro, rng, ["-c"], "-M")


def test_gzip_input_gives_the_same_files(built, inputs, tmp_path):
    with open(inputs / "a.fa", "rb") as f, gzip.open(tmp_path / "a.fa.gz", "wb") as g:
        g.write(f.read())
    (tmp_path / "plain").mkdir()
    (tmp_path / "gz").mkdir()
    r1 = _cli(["-r", str(inputs / "a.fa"), "-o", str(tmp_path / "plain" / "x"), "-P", "-M", "-m"])
    r2 = _cli(["-r", str(tmp_path / "a.fa.gz"), "-o", str(tmp_path / "gz" / "x"), "-P", "-M", "-m"])
    assert r1.returncode == 0 and r2.returncode == 0, r1.stderr + r2.stderr
    _same(str(tmp_path / "plain" / "x.bin"), str(tmp_path / "gz" / "x.bin"), EXTS,
          str(tmp_path / "plain" / "spumoni_null_reads.fa"), str(tmp_path / "gz" / "spumoni_null_reads.fa"))


@pytest.mark.parametrize("bad", [0, 1, 128, 255])
def test_refused_bytes(built, tmp_path, bad):
    data = b">first\nACGTACGT\n>second seq\nACGT" + bytes([bad]) + b"ACGT\n"
    with pytest.raises(capi.SpxError, match="file #0, sequence '>second seq'"):
        capi.prepare_fasta([data])
    (tmp_path / "g.fa").write_bytes(data)
    (tmp_path / "o").mkdir()
    r = _cli(["-r", str(tmp_path / "g.fa"), "-o", str(tmp_path / "o" / "x"), "-P", "-n"])
    assert r.returncode == 1 and "file #0 is " in r.stderr and "g.fa" in r.stderr, r.stderr
    assert os.listdir(tmp_path / "o") == []


def test_golden_reference_without_sequence(built, inputs, tmp_path):
    (tmp_path / "o").mkdir()
    r = _cli(["-r", str(inputs / "ref.fa"), "-o", str(tmp_path / "o" / "x"), "-P", "-n"])
    assert r.returncode == 1
    assert "After sequence digestion, there is no sequence left." in r.stderr, r.stderr
    assert os.listdir(tmp_path / "o") == []


def test_empty_after_digestion(built, tmp_path):
    (tmp_path / "g.fa").write_bytes(b">a\nACG\n>b\nNNNNNNNNNNNN\n")
    (tmp_path / "o").mkdir()
    r = _cli(["-r", str(tmp_path / "g.fa"), "-o", str(tmp_path / "o" / "x"), "-P", "-m"])
    assert r.returncode == 1
    assert "After sequence digestion, there is no sequence left." in r.stderr, r.stderr


def test_single_file_with_fdi(built, inputs, tmp_path):
    (tmp_path / "o").mkdir()
    pre = tmp_path / "o" / "x"
    text = _spec([open(inputs / "a.fa", "rb").read()], True)[0]
    (tmp_path / "o" / "x.fa.fdi").write_text(f"group_1\t{len(text) - 100}\ngroup_2\t99\n")
    r = _cli(["-r", str(inputs / "a.fa"), "-o", str(pre), "-P", "-n", "-d"])
    assert r.returncode == 1 and "sum to" in r.stderr, r.stderr
    (tmp_path / "o" / "x.fa.fdi").write_text(f"group_1\t{len(text) - 100}\ngroup_2\t100\n")
    r = _cli(["-r", str(inputs / "a.fa"), "-o", str(pre), "-P", "-n", "-d"])
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "o" / "x.fa.fdi").read_text() == f"group_1\t{len(text) - 100}\ngroup_2\t100\n"
    assert os.path.getsize(str(pre) + ".fa.doc") > 8


def test_end_to_end_build_then_run_against_the_oracle(built, tmp_path):
    g1 = synth.random_genome(30_000, seed=21)
    g2 = synth.mutate(g1, seed=22)
    for name, g in (("a.fa", g1), ("b.fa", g2)):
        with open(tmp_path / name, "w") as f:
            f.write(f">{name}\n")
            s = g.tobytes().decode()
            for i in range(0, len(s), 70):
                f.write(s[i: i + 70] + "\n")
    (tmp_path / "list.txt").write_text(f"{tmp_path / 'a.fa'} 1\n{tmp_path / 'b.fa'} 2\n")
    (tmp_path / "idx").mkdir()
    ref = str(tmp_path / "idx" / "pan")
    r = _cli(["-i", str(tmp_path / "list.txt"), "-o", ref, "-M", "-P", "-n", "-d"])
    assert r.returncode == 0, r.stderr
    prefix = ref + ".fa"
    text = np.fromfile(prefix + ".rawtext", dtype=np.uint8)
    seqs, offs = synth.sample_reads(text, 400, 180, seed=3)
    rng = np.random.default_rng(8)
    _run_both(tmp_path, ref, prefix, "reads.fa", seqs, offs, rng, ["-c", "-d"], "-M")
    _run_both(tmp_path, ref, prefix, "reads.fa", seqs, offs, rng, ["-c", "-d"], "-P")


@pytest.mark.parametrize("kind", [capi.SPX_DIGEST_PROMOTED, capi.SPX_DIGEST_DNA])
def test_long_pieces_with_n_runs_digested_by_chunks_match_the_oracle(built, oracle_mod, kind):
    """pieces of a chromosome's shape -- runs of N shorter than a k-mer, longer than a digestion item (4096 characters),
    at a piece's start and end, on item boundaries, other IUPAC letters -- digested by items of the chunked kernel with a
    halo counted in k-mers: bit for bit the oracle's sequential digestion"""
    rng = np.random.default_rng(40 + kind)
    reads = []
    for i in range(24):
        r = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(rng.integers(3000, 60000)))].copy()
        for _ in range(int(rng.integers(0, 12))):
            a, ln = int(rng.integers(0, r.size)), int(rng.choice([1, 2, 3, 5, 40, 4095, 4096, 9000]))
            r[a: a + ln] = ord("N")
        for at in (0, 4095, 4096, 8191, 8192, r.size - 1):
            if i % 3 == 0 and at < r.size:
                r[at] = ord("NRN"[i % 3])
        if i % 4 == 1:
            r[: 5000] = ord("N")
        reads.append(r)
    seqs = np.concatenate(reads)
    offs = np.concatenate([[0], np.cumsum([r.size for r in reads])]).astype(np.uint64)
    want, want_offs = oracle_mod.digest_batch(kind, 4, 11, seqs, offs)
    got, got_offs = capi.digester(0).digest_host(kind, 4, 11, seqs, offs)
    assert np.array_equal(got_offs, want_offs)
    assert np.array_equal(got, want)


def _genome_fasta(path, rng):
    """about 2.2e9 bp: one 3e8-character single-line sequence with runs of N, then 80-column sequences"""
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    sizes = [300_000_000]
    while sum(sizes) < 2_200_000_000:
        sizes.append(min(int(rng.integers(50_000_000, 150_000_000)), 2_200_000_000 - sum(sizes)))
    sizes[-1] = max(sizes[-1], 200_000)
    seqs = []
    with open(path, "wb") as f:
        for i, n in enumerate(sizes):
            s = acgt[rng.integers(0, 4, n, dtype=np.uint8)]
            s[:10_000] = ord("N")
            for _ in range(8):
                a = int(rng.integers(0, n - 100_000))
                s[a: a + int(rng.integers(1, 100_000))] = ord("N")
            seqs.append(s)
            f.write(b">chr%d\n" % i)
            if i == 0:
                f.write(s.tobytes() + b"\n")
            else:
                b = s.tobytes()
                for j in range(0, len(b), 1 << 24):
                    blk = b[j: j + (1 << 24)]
                    f.write(b"\n".join(blk[k: k + 80] for k in range(0, len(blk), 80)) + b"\n")
    return seqs


def test_scale_past_2_to_the_32(built, oracle_mod, tmp_path):
    """a genome whose undigested text with reverse complements is over 2^32 characters: -m builds, its text is the
    specification's (the first and last pieces digested by the oracle, the lengths of all), -n is refused with the
    limit message, and `spumoni run -P -c` finds reads sampled from the genome"""
    rng = np.random.default_rng(50)
    fa = tmp_path / "genome.fa"
    seqs = _genome_fasta(fa, rng)
    total = sum(s.size for s in seqs)
    assert 2 * total > 2**32 and total > 2_000_000_000
    (tmp_path / "n").mkdir()
    r = _cli(["-r", str(fa), "-o", str(tmp_path / "n" / "x"), "-P", "-n"])
    assert r.returncode == 1 and "fewer than 2^32 - 1" in r.stderr and "-m" in r.stderr, r.stderr
    assert os.listdir(tmp_path / "n") == []

    (tmp_path / "m").mkdir()
    ref = str(tmp_path / "m" / "x")
    r = _cli(["-r", str(fa), "-o", ref, "-P", "-M", "-m"])
    assert r.returncode == 0, r.stderr
    text = np.fromfile(ref + ".bin.rawtext", dtype=np.uint8)

    def dig(s):
        out, _ = oracle_mod.digest_batch(capi.SPX_DIGEST_PROMOTED, 4, 11, s, np.array([0, s.size], dtype=np.uint64))
        return out

    def rc(s):
        return np.frombuffer(_revcomp(s.tobytes()), dtype=np.uint8)

    head = [dig(seqs[0]), dig(rc(seqs[0]))]
    tail = [dig(seqs[-1]), dig(rc(seqs[-1]))]
    h = head[0].size + head[1].size
    t = tail[0].size + tail[1].size
    assert np.array_equal(text[: head[0].size], head[0])
    assert np.array_equal(text[head[0].size: h], head[1])
    assert np.array_equal(text[text.size - t: text.size - tail[1].size], tail[0])
    assert np.array_equal(text[text.size - tail[1].size:], tail[1])
    assert int(open(ref + ".bin.fdi").read().split()[1]) == text.size
    del head, tail, text

    reads = []
    for _ in range(300):
        s = seqs[int(rng.integers(0, len(seqs)))]
        while True:
            a = int(rng.integers(0, s.size - 300))
            if not (s[a: a + 300] == ord("N")).any():
                break
        reads.append(s[a: a + 300].tobytes())
    (tmp_path / "q").mkdir()
    reads_fa = tmp_path / "q" / "reads.fa"
    reads_fa.write_bytes(b"".join(b">r%d\n" % i + x + b"\n" for i, x in enumerate(reads)))
    out = subprocess.run([BIN, "run", "-r", ref, "-p", str(reads_fa), "-P", "-c", "-m"], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr
    rep = open(str(reads_fa) + ".report").read().splitlines()[1:]
    found = sum("FOUND" in ln and "NOT_PRESENT" not in ln for ln in rep)
    assert len(rep) == 300 and found >= 0.9 * len(rep), found
