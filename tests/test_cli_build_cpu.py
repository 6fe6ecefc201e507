"""CPU tier of `spumoni build` (spumoni_amd/csrc/host/build_main.cpp) and of the text preparation boundary
(include/spumoni_reftext.h): the usage and the reference's validation messages, the loud failure without a device, the
missing-builder failure against a library that lacks the spb_* / spr_* entry points, and the plain-C header.  What the
command computes is tests/test_gpu_cli_build.py's business."""
import os
import re
import subprocess

import pytest

from spumoni_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
HEADER = os.path.join(ROOT, "include", "spumoni_reftext.h")
FA = b">s1\nACGTACGTTTGACCA\n>s2\nGGGTTTAAACCC\n"


@pytest.fixture(scope="module")
def built():
    capi.build()
    return capi.lib()


def _build(args, cwd, env=None):
    return subprocess.run([BIN, "build"] + args, cwd=cwd, capture_output=True, text=True, env=env, timeout=120)


def test_usage_without_arguments(built, tmp_path):
    r = _build([], str(tmp_path))
    assert r.returncode == 1
    assert "spumoni build - builds the ms/pml index for a specified reference file." in r.stderr
    for opt in ("-r, --ref", "-i, --filelist", "-g, --general-text", "-c, --no-rev-comp", "-n, --no-digest",
                "-m, --minimizer-alphabet", "-t, --dna-minimizer", "-K, --small-window", "-W, --large-window",
                "-o, --prefix", "-M, --MS", "-P, --PML", "-k, --keep", "-d, --doc-array", "-w, --window",
                "-p, --hash-mod", "-h, --help", "-v, --verbose"):
        assert opt in r.stderr, opt


@pytest.mark.parametrize("args,message", [
    (["-r", "missing.fa", "-o", "out/x", "-P", "-n"], "The following path is not valid: missing.fa"),
    (["-i", "missing.txt", "-o", "out/x", "-P", "-n"], "The following path is not valid: missing.txt"),
    (["-r", "x.fa", "-b", "dir", "-o", "out/x", "-P", "-n"], "The -b option should not be set when using a single file."),
    (["-r", "x.txt", "-o", "out/x", "-P", "-n"], "The reference file provided does not appear to be a FASTA"),
    (["-r", "x.fa", "-o", "out/x", "-P", "-n", "-d"], "Cannot build a document array if you are indexing a single"),
    (["-r", "x.fa", "-o", "out/x", "-P", "-m", "-t"], "Only one type of minimizer can be specified."),
    (["-r", "x.fa", "-o", "out/x", "-P"], "A minimizer type must be specified."),
    (["-r", "x.fa", "-o", "out/x", "-P", "-n", "-m"],
     "A minimizer type should not be specified if intending not to use minimizer digestion."),
    (["-r", "x.fa", "-P", "-n"], "Need to specify an output prefix for the index files."),
    (["-r", "x.fa", "-o", "out/x", "-n"], "At least one index type (-M or -P) must be specified for build."),
    (["-r", "x.fa", "-o", "out/x", "-P", "-m", "-K", "5", "-W", "11"],
     "small window size (k) cannot be larger than 4 characters."),
    (["-r", "x.fa", "-o", "out/x", "-P", "-m", "-K", "4", "-W", "3"],
     "large window size (w) should be larger than the small window size (k)"),
    (["-r", "x.fa", "-o", "out/x", "-P", "-n", "-w", "20"],
     "the bin size provided is not optimal, re-run using a value between 50 and 400."),
    (["-r", "x.fa", "-o", "nodir/x", "-P", "-n"], "Output prefix path is not valid."),
    (["-r", "x.fa", "-o", "out/x", "-P", "-g"], "general-text input (-g) is not supported by this build"),
])
def test_validation_messages(built, tmp_path, args, message):
    (tmp_path / "x.fa").write_bytes(FA)
    (tmp_path / "x.txt").write_bytes(FA)
    (tmp_path / "out").mkdir()
    r = _build(args, str(tmp_path))
    assert r.returncode == 1
    assert message in r.stderr, r.stderr
    assert os.listdir(tmp_path / "out") == []


def test_no_device_fails_loudly_and_writes_nothing(built, tmp_path):
    if built.spx_device_count() > 0:
        pytest.skip("a device is visible: the no-device path is this machine's CPU tier")
    (tmp_path / "x.fa").write_bytes(FA)
    (tmp_path / "out").mkdir()
    r = _build(["-r", "x.fa", "-o", "out/x", "-P", "-M", "-n"], str(tmp_path))
    assert r.returncode == 1
    assert "no usable gfx950 device" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert os.listdir(tmp_path / "out") == []


def test_missing_builder_entry_point_on_the_fake_device(built, fake_device, tmp_path):
    (tmp_path / "x.fa").write_bytes(FA)
    (tmp_path / "out").mkdir()
    env = dict(os.environ, LD_LIBRARY_PATH=fake_device + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = _build(["-r", "x.fa", "-o", "out/x", "-P", "-M", "-n"], str(tmp_path), env=env)
    assert r.returncode == 1
    assert "has no spr_text_from_fasta" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert os.listdir(tmp_path / "out") == []


def _declared():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return code, sorted(set(re.findall(r"\b(spr_[a-z_0-9]+)\s*\(", code)))


def test_reftext_header_is_plain_c(tmp_path):
    src = tmp_path / "r.c"
    src.write_text('#include "spumoni_reftext.h"\nint main(void) { spr_text *t = 0; (void)t; return 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    code, _ = _declared()
    assert "hipStream_t" not in code and "std::" not in code and "#include <hip" not in code


def test_reftext_header_symbols_exported(built):
    _, names = _declared()
    assert names == sorted(capi.REFTEXT_EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r"\b(spr_[a-z_0-9]+)\b", out)))
    assert exported == names


def test_prepare_fasta_without_device_fails_loudly(built):
    if built.spx_device_count() > 0:
        pytest.skip("a device is visible")
    with pytest.raises(capi.SpxError, match="no CPU fallback"):
        capi.prepare_fasta([FA])
