"""CPU tier of the index builder (include/spumoni_build.h): the header is plain C, the real library exports what it
declares, and without a device the builder fails loudly (no CPU fallback).  What it computes is tests/test_gpu_build.py's
business."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from spumoni_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spumoni_build.h")


@pytest.fixture(scope="module")
def built():
    capi.build()
    return capi.lib()


def _declared():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return code, sorted(set(re.findall(r"\b(spb_[a-z_0-9]+)\s*\(", code)))


def test_build_header_is_plain_c(tmp_path):
    src = tmp_path / "b.c"
    src.write_text('#include "spumoni_build.h"\nint main(void) { spb_build *b = 0; (void)b; return 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    code, _ = _declared()
    assert "torch" not in code and "hipStream_t" not in code and "std::" not in code and "#include <hip" not in code


def test_build_header_symbols_exported(built):
    _, declared = _declared()
    assert declared == ["spb_build_copy", "spb_build_free", "spb_build_from_text", "spb_build_stats"]
    for name in declared:
        assert hasattr(built, name), name


def test_builder_without_gpu_fails_loudly(built):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = built
    L.spb_build_from_text.restype = ctypes.c_void_p
    L.spb_build_from_text.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int,
                                      ctypes.c_int]
    text = np.frombuffer(b"ACGTACGTTGCA", dtype=np.uint8).copy()
    h = L.spb_build_from_text(text.ctypes.data_as(ctypes.c_void_p), text.size, None, 0, 1, 0)
    assert not h
    assert "no CPU fallback" in L.spx_last_error().decode()
    with pytest.raises(capi.SpxError, match="no CPU fallback"):
        capi.build_raw(text)


SCRIPT = r'''
import numpy as np
from spumoni_amd import capi, build_index
assert "fake-device" in capi.version()
assert not build_index.hip_builder_available()  # the stand-in has no builder: build_index keeps the torch path
try:
    capi.build_raw(np.frombuffer(b"ACGTTGCA", dtype=np.uint8))
except capi.SpxError as e:
    assert "spb_build_from_text" in str(e), e
    print("SPXERROR OK")
'''


def test_build_raw_on_a_library_without_the_builder(fake_device):
    env = dict(os.environ, SPUMONI_GPU_LIB=os.path.join(fake_device, "libspumoni_gpu.so"), PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", SCRIPT], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and "SPXERROR OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
