"""ctypes binding of libspumoni_gpu.so (the C-ABI in include/spumoni_gpu.h).

This is plumbing for tests and bench: torch only provides device memory and
streams.  There is no CPU fallback -- if the library or a gfx950 device is
missing, loading / index construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SPUMONI_GPU_LIB: load another build of the same library (A/B experiments: tools/ab.sh)
LIB_PATH = os.environ.get("SPUMONI_GPU_LIB") or os.path.join(_HERE, "libspumoni_gpu.so")
CSRC = os.path.join(_HERE, "csrc")

SPX_MODE_PML = 0
SPX_MODE_MS = 1

EXPORTS = [
    "spx_last_error",
    "spx_device_count",
    "spx_index_from_runs",
    "spx_index_load_raw",
    "spx_index_free",
    "spx_index_stats",
    "spx_index_device_bytes",
    "spx_index_set_text",
    "spx_query_batch",
    "spx_query_batch_device",
    "spx_query_batch16",
    "spx_query_batch_device16",
    "spx_last_walk_stats",
    "spx_set_option",
    "spx_host_alloc",
    "spx_host_free",
    "spx_host_register",
    "spx_host_unregister",
    "spx_digest_capacity",
    "spx_digest_batch",
    "spx_digest_batch_device",
    "spx_digest_query_batch",
    "spx_digest_query_batch_device",
    "spx_digest_query_batch_device16",
    "spx_version",
    "spx_index_save",
    "spx_index_load_flat",
    "spx_index_clone",
    "spx_index_describe",
    "spx_last_chunk_stats",
    "spx_index_rebuild_text",
    "spx_index_copy_text",
    "spx_index_set_source_tag",
    "spx_index_source_tag",
    "spx_query_text_begin",
    "spx_query_text_fetch",
    "spx_query_text_reserve",
]
SPX_TEXT_LENGTHS, SPX_TEXT_POINTERS, SPX_TEXT_DOCS = 1, 2, 4
SPX_TEXT_UNCHECKED = 2

SPX_DIGEST_PROMOTED, SPX_DIGEST_DNA = 1, 2


class SpxClass(C.Structure):
    _fields_ = [("sum_max_bin_values", C.c_uint64), ("bins_above", C.c_uint32), ("bins_below", C.c_uint32)]


class SpxWalkStats(C.Structure):
    _fields_ = [
        ("steps", C.c_uint64),
        ("jumps", C.c_uint64),
        ("pred_jumps", C.c_uint64),
        ("row_loads", C.c_uint64),
        ("dir_loads", C.c_uint64),
        ("kernel_ms", C.c_float),
    ]


CLASS_DTYPE = np.dtype([("sum_max", "<u8"), ("above", "<u4"), ("below", "<u4")])


class SpxError(RuntimeError):
    pass


def build(force: bool = False) -> str:
    """Compile libspumoni_gpu.so for gfx950 (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC, "-j4"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


_LIB = None


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise SpxError(
                f"{LIB_PATH} is missing: build it with `make -C spumoni_amd/csrc` "
                "(there is no CPU fallback for the HIP path)"
            )
        L = C.CDLL(LIB_PATH)
        vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
        L.spx_last_error.restype = C.c_char_p
        L.spx_device_count.restype = i32
        L.spx_index_from_runs.restype = vp
        L.spx_index_from_runs.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, i32, i32]
        L.spx_index_load_raw.restype = vp
        L.spx_index_load_raw.argtypes = [C.c_char_p, i32, i32]
        L.spx_index_free.argtypes = [vp]
        L.spx_index_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        L.spx_index_device_bytes.argtypes = [vp, C.POINTER(u64)]
        L.spx_index_set_text.argtypes = [vp, vp, u64, i32]
        L.spx_index_set_source_tag.argtypes = [vp, C.c_char_p]
        L.spx_index_source_tag.restype = C.c_char_p
        L.spx_index_source_tag.argtypes = [vp]
        L.spx_query_text_begin.argtypes = [vp, i32, i32, C.c_uint32, C.c_uint32, vp, vp, u64, vp, C.c_uint32, vp, u64, u64, vp]
        L.spx_query_text_fetch.argtypes = [vp, vp, vp]
        L.spx_query_text_reserve.argtypes = [vp, i32, i32, C.c_uint32, u64, u64, C.c_uint32, i32, vp]
        L.spx_query_batch.argtypes = [vp, i32, vp, vp, u64, vp, vp, vp, vp, u64, u64]
        L.spx_query_batch_device.argtypes = [vp, i32, vp, vp, u64, u64, vp, vp, vp, vp, u64, u64, vp]
        L.spx_query_batch16.argtypes = [vp, i32, vp, vp, u64, vp, vp, vp, vp, u64, u64]
        L.spx_query_batch_device16.argtypes = [vp, i32, vp, vp, u64, u64, vp, vp, vp, vp, u64, u64, vp]
        L.spx_last_walk_stats.argtypes = [vp, C.POINTER(SpxWalkStats)]
        L.spx_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
        L.spx_host_alloc.restype = vp
        L.spx_host_alloc.argtypes = [C.c_size_t]
        L.spx_host_free.argtypes = [vp]
        L.spx_host_register.restype = i32
        L.spx_host_register.argtypes = [vp, C.c_size_t]
        L.spx_host_unregister.restype = i32
        L.spx_host_unregister.argtypes = [vp]
        u32 = C.c_uint32
        L.spx_digest_capacity.restype = u64
        L.spx_digest_capacity.argtypes = [i32, u32, u64]
        L.spx_digest_batch.argtypes = [vp, i32, u32, u32, vp, vp, u64, vp, u64, vp]
        L.spx_digest_batch_device.argtypes = [vp, i32, u32, u32, vp, vp, u64, u64, vp, u64, vp, vp]
        L.spx_digest_query_batch.argtypes = [vp, i32, i32, u32, u32, vp, vp, u64, vp, u64, vp, vp, vp, vp, u64, u64]
        for fn in (L.spx_digest_query_batch_device, L.spx_digest_query_batch_device16):
            fn.argtypes = [vp, i32, i32, u32, u32, vp, vp, u64, u64, vp, u64, vp, vp, vp, vp, vp, u64, u64, vp]
        L.spx_version.restype = C.c_char_p
        L.spx_index_save.argtypes = [vp, C.c_char_p]
        L.spx_index_load_flat.restype = vp
        L.spx_index_load_flat.argtypes = [C.c_char_p, i32]
        L.spx_index_clone.restype = vp
        L.spx_index_clone.argtypes = [vp, i32]
        L.spx_index_describe.argtypes = [vp, C.c_char_p, C.c_size_t]
        L.spx_last_chunk_stats.argtypes = [vp, C.POINTER(u64 * 4)]
        L.spx_index_rebuild_text.argtypes = [vp]
        L.spx_index_copy_text.argtypes = [vp, vp, u64, i32, C.POINTER(u64)]
        _LIB = L
    return _LIB


def version() -> str:
    """Layout + kernel version of the loaded library (keys the .spx cache and the measured traffic)."""
    return lib().spx_version().decode()


def _check(rc: int):
    if rc != 0:
        raise SpxError(f"spx error {rc}: {lib().spx_last_error().decode()}")


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _t_ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _class_buffer(classify, class_out, nreads):
    """Where a host query's class records go: nowhere, a fresh array, or the array the caller gave."""
    if not classify:
        return None
    if class_out is None:
        return np.zeros(max(nreads, 1), dtype=CLASS_DTYPE)
    if class_out.dtype != CLASS_DTYPE or class_out.ndim != 1 or class_out.size < nreads or not class_out.flags.c_contiguous:
        raise SpxError("class_out must be a contiguous CLASS_DTYPE array of nreads entries or more")
    return class_out


class Index:
    """An spx_index on one GPU."""

    def __init__(self, handle, device: int):
        self._h = handle
        self.device = device
        n, r = C.c_uint64(), C.c_uint64()
        _check(lib().spx_index_stats(self._h, C.byref(n), C.byref(r)))
        self.n, self.r = n.value, r.value
        self._n_seqs = 0  # of the sequence table set through this object (or the one it was cloned from)

    # -- construction -----------------------------------------------------
    @classmethod
    def from_raw(cls, raw, device: int = 0) -> "Index":
        """raw: spumoni_amd.synth.RawIndex (torch tensors on CPU or on `device`)."""
        import torch

        on_dev = raw.heads.is_cuda
        keep = []

        def prep(t, dt):
            if t is None:
                return None
            t = t.to(dt).contiguous()
            keep.append(t)
            return t

        heads = prep(raw.heads, torch.uint8)
        # int64 and uint64 share the bit pattern for the value range used here
        lens, thr = prep(raw.lens, torch.int64), prep(raw.thr, torch.int64)
        ssa, esa = prep(raw.ssa, torch.int64), prep(raw.esa, torch.int64)
        ds, de = prep(raw.doc_start, torch.int64), prep(raw.doc_end, torch.int64)
        if on_dev:
            torch.cuda.synchronize()
        h = lib().spx_index_from_runs(
            _t_ptr(heads), _t_ptr(lens), _t_ptr(thr), raw.r, _t_ptr(ssa), _t_ptr(esa), _t_ptr(ds), _t_ptr(de),
            1 if on_dev else 0, device,
        )
        if not h:
            raise SpxError(lib().spx_last_error().decode())
        ix = cls(h, device)
        if raw.text is not None:
            ix.set_text(raw.text)
        return ix

    @classmethod
    def load_raw(cls, prefix: str, mode: int = SPX_MODE_PML, device: int = 0) -> "Index":
        h = lib().spx_index_load_raw(prefix.encode(), mode, device)
        if not h:
            raise SpxError(lib().spx_last_error().decode())
        return cls(h, device)

    @classmethod
    def load_flat(cls, path: str, device: int = 0) -> "Index":
        """An index from a flat-layout cache written by save()."""
        h = lib().spx_index_load_flat(path.encode(), device)
        if not h:
            raise SpxError(lib().spx_last_error().decode())
        return cls(h, device)

    def save(self, path: str) -> None:
        _check(lib().spx_index_save(self._h, path.encode()))

    def set_source_tag(self, tag: str) -> None:
        """The caller's fingerprint of what the index was built from; travels with save() / load_flat() / clone()."""
        _check(lib().spx_index_set_source_tag(self._h, tag.encode()))

    def source_tag(self) -> str:
        return lib().spx_index_source_tag(self._h).decode()

    def clone(self, device: int) -> "Index":
        """A copy of this index on `device` (device-to-device, no re-flattening); onto the SAME device: a second query context --
        scratch, counters and stream of its own -- over the same arrays (nothing is copied)."""
        h = lib().spx_index_clone(self._h, device)
        if not h:
            raise SpxError(lib().spx_last_error().decode())
        out = Index(h, device)
        out._n_seqs = self._n_seqs  # (the table goes with the clone)
        return out

    def describe(self) -> dict:
        import json

        buf = C.create_string_buffer(1024)
        _check(lib().spx_index_describe(self._h, buf, 1024))
        return json.loads(buf.value.decode())

    def rebuild_text(self) -> None:
        """The indexed text from the MS index itself (LF chains from the SA samples): no text file needed."""
        _check(lib().spx_index_rebuild_text(self._h))

    def text(self) -> np.ndarray:
        """The text the index holds (set or rebuilt), as a host array."""
        n = C.c_uint64()
        _check(lib().spx_index_copy_text(self._h, None, 0, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint8)
        _check(lib().spx_index_copy_text(self._h, _np_ptr(out), n.value, 0, C.byref(n)))
        return out

    def set_text(self, text, unchecked: bool = False) -> None:
        """unchecked: skip the text-against-index validation (synthetic indexes that are no text's BWT)."""
        t = text.contiguous()
        where = (1 if t.is_cuda else 0) | (SPX_TEXT_UNCHECKED if unchecked else 0)
        _check(lib().spx_index_set_text(self._h, _t_ptr(t), t.numel(), where))

    def close(self):
        h, self._h = self._h, None
        if h:
            lib().spx_index_free(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device_bytes(self) -> int:
        b = C.c_uint64()
        _check(lib().spx_index_device_bytes(self._h, C.byref(b)))
        return b.value

    def set_option(self, key: str, value: int) -> None:
        _check(lib().spx_set_option(self._h, key.encode(), value))

    # -- queries, host buffers (numpy) --------------------------------------
    def query_host(self, mode, seqs, offs, want_lengths=True, want_docs=False, classify=None, bits=32, class_out=None):
        """bits=16: the 16-bit entry point (uint16 lengths / docs; reads shorter than 65536).  class_out: the caller's
        CLASS_DTYPE array for the class records (nreads entries at least; tests pass a slice of a larger, fenced one)."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        nreads = offs.size - 1
        tot = int(offs[-1]) if nreads > 0 else 0
        vt = np.uint16 if bits == 16 else np.uint32
        lens = np.zeros(max(tot, 1) + 8, dtype=vt) if want_lengths else None  # PML: None + classify = report only
        ptrs = np.zeros(max(tot, 1), dtype=np.uint64) if mode == SPX_MODE_MS else None
        docs = np.zeros(max(tot, 1) + 8, dtype=vt) if want_docs else None
        cls_ = _class_buffer(classify, class_out, nreads)
        bw, thr = classify if classify else (0, 0)
        fn = lib().spx_query_batch16 if bits == 16 else lib().spx_query_batch
        _check(fn(self._h, mode, _np_ptr(seqs), _np_ptr(offs), nreads, _np_ptr(lens),
                  _np_ptr(ptrs), _np_ptr(docs), _np_ptr(cls_), bw, thr))
        out = {}
        if lens is not None:
            out["lengths"] = lens[:tot]
        if ptrs is not None:
            out["pointers"] = ptrs[:tot]
        if docs is not None:
            out["docs"] = docs[:tot]
        if cls_ is not None:
            out["class"] = cls_[:nreads]
        return out

    def query_text(self, mode, seqs, offs, gap=None, streams=SPX_TEXT_LENGTHS, digest=(0, 0, 0), classify=None,
                   class_out=None):
        """The vectors as the text of the output files (spx_query_text_begin / _fetch).  Returns
        {"text": [bytes | None] * 3, "line_start": [uint64 array | None] * 3, "class": ...}; stream i = lengths,
        pointers, document ids."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        nreads = offs.size - 1
        g = None if gap is None else np.ascontiguousarray(gap, dtype=np.uint32)
        cls_ = _class_buffer(classify, class_out, nreads)
        bw, thr = classify if classify else (0, 0)
        nbytes = (C.c_uint64 * 3)()
        _check(lib().spx_query_text_begin(self._h, mode, digest[0], digest[1], digest[2], _np_ptr(seqs), _np_ptr(offs), nreads,
                                          _np_ptr(g), streams, _np_ptr(cls_), bw, thr, C.cast(nbytes, C.c_void_p)))
        bufs = [np.zeros(int(nbytes[i]) + 1, dtype=np.uint8) if nbytes[i] else None for i in range(3)]
        starts = [np.zeros(nreads + 1, dtype=np.uint64) if nbytes[i] else None for i in range(3)]
        tp = (C.c_void_p * 3)(*[_np_ptr(b) for b in bufs])
        lp = (C.c_void_p * 3)(*[_np_ptr(b) for b in starts])
        _check(lib().spx_query_text_fetch(self._h, C.cast(tp, C.c_void_p), C.cast(lp, C.c_void_p)))
        return {"text": [None if b is None else b[: int(nbytes[i])].tobytes() for i, b in enumerate(bufs)],
                "line_start": starts, "class": None if cls_ is None else cls_[:nreads]}

    def reserve_text(self, mode, max_chars, max_reads, streams=SPX_TEXT_LENGTHS, classify=False, digest=(0, 0), text_bytes=None):
        """spx_query_text_reserve: the device scratch of query_text calls up to this size, allocated now (a hint)."""
        tb = None
        if text_bytes is not None:
            tb = (C.c_uint64 * 3)(*[int(x) for x in text_bytes])
        _check(lib().spx_query_text_reserve(self._h, mode, digest[0], digest[1], int(max_chars), int(max_reads), streams,
                                            1 if classify else 0, None if tb is None else C.cast(tb, C.c_void_p)))

    # -- queries, device buffers (torch tensors on self.device) -------------
    def query_device(self, mode, d_seqs, d_offs, total_chars, d_lengths=None, d_pointers=None, d_docs=None,
                     d_class=None, bin_width=0, max_value_thr=0, stream=None, narrow=None):
        """Enqueue on `stream` (a torch.cuda.Stream or None = torch's current stream).  int16 / uint16
        tensors for d_lengths / d_docs select the 16-bit entry point; narrow=True / False says so where neither is given
        (PML classes alone)."""
        import torch

        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        nreads = d_offs.numel() - 1
        if narrow is None or d_lengths is not None or d_docs is not None:
            narrow = any(t is not None and t.element_size() == 2 for t in (d_lengths, d_docs))
        fn = lib().spx_query_batch_device16 if narrow else lib().spx_query_batch_device
        _check(fn(
            self._h, mode, _t_ptr(d_seqs), _t_ptr(d_offs), nreads, total_chars, _t_ptr(d_lengths),
            _t_ptr(d_pointers), _t_ptr(d_docs), _t_ptr(d_class), bin_width, max_value_thr,
            C.c_void_p(st.cuda_stream)))

    # -- minimizer digestion (run -m / -a) ------------------------------------
    def digest_host(self, kind, k, w, seqs, offs):
        """(digested seqs, offsets) of a batch of upper-cased reads; host buffers."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        nreads = offs.size - 1
        tot = int(offs[-1]) if nreads > 0 else 0
        cap = int(lib().spx_digest_capacity(kind, k, tot))
        out = np.zeros(cap, dtype=np.uint8)
        out_offs = np.zeros(nreads + 1, dtype=np.uint64)
        _check(lib().spx_digest_batch(self._h, kind, k, w, _np_ptr(seqs), _np_ptr(offs), nreads, _np_ptr(out), cap,
                                      _np_ptr(out_offs)))
        return out[: int(out_offs[-1])], out_offs

    def digest_device(self, kind, k, w, d_seqs, d_offs, total_chars, stream=None):
        """Digest on the device; returns (d_out_seqs, d_out_offs) torch tensors that can go
        straight into query_device (total = d_out_offs[-1])."""
        import torch

        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        nreads = d_offs.numel() - 1
        cap = int(lib().spx_digest_capacity(kind, k, total_chars))
        d_out = torch.empty(cap, dtype=torch.uint8, device=d_seqs.device)
        d_out_offs = torch.empty(nreads + 1, dtype=torch.int64, device=d_seqs.device)
        _check(lib().spx_digest_batch_device(self._h, kind, k, w, _t_ptr(d_seqs), _t_ptr(d_offs), nreads, total_chars,
                                             _t_ptr(d_out), cap, _t_ptr(d_out_offs), C.c_void_p(st.cuda_stream)))
        return d_out, d_out_offs

    def digest_query_device(self, mode, kind, k, w, d_seqs, d_offs, total_chars, d_lengths=None, d_pointers=None, d_docs=None,
                            d_class=None, bin_width=0, max_value_thr=0, stream=None, work=None):
        """Digest and query in one call, everything on the device (spx_digest_query_batch_device[16]): returns
        (d_out_offs, work).  The outputs (sized for total_chars entries) are laid out at d_out_offs; `work` = (digested
        bytes, offsets) buffers that a caller may hand back to avoid the allocations."""
        import torch

        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        nreads = d_offs.numel() - 1
        cap = int(lib().spx_digest_capacity(kind, k, total_chars))
        if work is None or work[0].numel() < cap or work[1].numel() < nreads + 1:
            work = (torch.empty(cap, dtype=torch.uint8, device=d_seqs.device),
                    torch.empty(nreads + 1, dtype=torch.int64, device=d_seqs.device))
        narrow = any(t is not None and t.element_size() == 2 for t in (d_lengths, d_docs))
        fn = lib().spx_digest_query_batch_device16 if narrow else lib().spx_digest_query_batch_device
        _check(fn(self._h, mode, kind, k, w, _t_ptr(d_seqs), _t_ptr(d_offs), nreads, total_chars, _t_ptr(work[0]), work[0].numel(),
                  _t_ptr(work[1]), _t_ptr(d_lengths), _t_ptr(d_pointers), _t_ptr(d_docs), _t_ptr(d_class), bin_width, max_value_thr,
                  C.c_void_p(st.cuda_stream)))
        return work[1], work

    def digest_query_host(self, mode, kind, k, w, seqs, offs, want_lengths=True, want_docs=False, classify=None,
                          class_out=None):
        """digest + query in one call (the reference's per-read loop body, for a batch)."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        nreads = offs.size - 1
        tot = int(offs[-1]) if nreads > 0 else 0
        cap = int(lib().spx_digest_capacity(kind, k, tot))
        out_offs = np.zeros(nreads + 1, dtype=np.uint64)
        lens = np.zeros(cap, dtype=np.uint32) if want_lengths else None
        ptrs = np.zeros(cap, dtype=np.uint64) if mode == SPX_MODE_MS else None
        docs = np.zeros(cap, dtype=np.uint32) if want_docs else None
        cls_ = _class_buffer(classify, class_out, nreads)
        bw, thr = classify if classify else (0, 0)
        _check(lib().spx_digest_query_batch(self._h, mode, kind, k, w, _np_ptr(seqs), _np_ptr(offs), nreads,
                                            _np_ptr(out_offs), cap, _np_ptr(lens), _np_ptr(ptrs), _np_ptr(docs),
                                            _np_ptr(cls_), bw, thr))
        dt = int(out_offs[-1])
        out = {"offsets": out_offs}
        if lens is not None:
            out["lengths"] = lens[:dt]
        if ptrs is not None:
            out["pointers"] = ptrs[:dt]
        if docs is not None:
            out["docs"] = docs[:dt]
        if cls_ is not None:
            out["class"] = cls_[:nreads]
        return out

    # -- document votes (include/spumoni_docvote.h) ---------------------------
    def votes_device(self, d_lengths, d_docs, d_offs, min_length, d_out=None, stream=None):
        """One record per read (spv_vote: voters, top_doc, top_votes, second_votes) from the per-position lengths and
        document ids of a query, on the device: returns d_out, an int32 tensor of shape (reads, 4).  int16 / uint16
        tensors select the 16-bit form; both arrays have the same width."""
        import torch

        L = _spv()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        nreads = d_offs.numel() - 1
        if d_lengths.element_size() != d_docs.element_size():
            raise SpxError("d_lengths and d_docs must have the same width")
        if d_out is None:
            d_out = torch.empty((max(nreads, 0), 4), dtype=torch.int32, device=d_offs.device)
        _check(L.spv_votes_device(self._h, _t_ptr(d_lengths), _t_ptr(d_docs), d_lengths.element_size() * 8, _t_ptr(d_offs),
                                  nreads, min(d_lengths.numel(), d_docs.numel()), int(min_length), _t_ptr(d_out),
                                  C.c_void_p(st.cuda_stream)))
        return d_out

    def assign_host(self, mode, seqs, offs, min_length, digest=None):
        """spv_assign_batch: reads in, one record per read out -- a structured array (docvote.VOTE_DTYPE plus "values",
        the read's positions after digestion).  digest: (kind, k, w) or None."""
        from .docvote import VOTE_DTYPE

        L = _spv()
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        nreads = offs.size - 1
        kind, k, w = digest if digest else (0, 0, 0)
        rec = np.zeros(max(nreads, 1), dtype=VOTE_DTYPE)
        vals = np.zeros(max(nreads, 1), dtype=np.uint64)
        _check(L.spv_assign_batch(self._h, mode, kind, k, w, _np_ptr(seqs), _np_ptr(offs), nreads, int(min_length),
                                  _np_ptr(rec), _np_ptr(vals)))
        out = np.zeros(nreads, dtype=np.dtype(VOTE_DTYPE.descr + [("values", "<u8")]))
        for f in VOTE_DTYPE.names:
            out[f] = rec[f][:nreads]
        out["values"] = vals[:nreads]
        return out

    def votes_stats(self) -> dict:
        """Of the most recent votes_device / assign_host call: reads per kernel path, voting positions, kernel time."""
        s = SpvVotesStats()
        _check(_spv().spv_last_votes_stats(self._h, C.byref(s)))
        return {f[0]: getattr(s, f[0]) for f in SpvVotesStats._fields_}

    # -- matches (include/spumoni_mems.h) --------------------------------------
    def mems_device(self, d_lengths, d_pointers, d_offs, min_length, d_docs=None, capacity=None, d_match_offsets=None,
                    d_out=None, d_out_docs=None, stream=None):
        """The reported match starts of every read (spm_match: ref_pos u64, read_pos u32, length u32) from the MS lengths
        and pointers of a query, on the device: returns (d_match_offsets int64[reads + 1], d_records int32 (capacity, 4)
        [, d_docs int32]).  int16 / uint16 lengths select the 16-bit form (d_docs has the same width).  capacity None: a
        first call counts, the host reads the count, a second call writes that many records; given: one call, records
        of rank >= capacity are left out (mems_stats() says so)."""
        import torch

        L = _spm()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        nreads = d_offs.numel() - 1
        if d_docs is not None and d_lengths.element_size() != d_docs.element_size():
            raise SpxError("d_lengths and d_docs must have the same width")
        if d_match_offsets is None:
            d_match_offsets = torch.empty(max(nreads, 0) + 1, dtype=torch.int64, device=d_offs.device)
        total = d_lengths.numel()

        def call(cap, out, out_docs):
            _check(L.spm_mems_device(self._h, _t_ptr(d_lengths), d_lengths.element_size() * 8, _t_ptr(d_pointers), _t_ptr(d_docs),
                                     _t_ptr(d_offs), nreads, total, int(min_length), _t_ptr(d_match_offsets), _t_ptr(out), cap,
                                     _t_ptr(out_docs), C.c_void_p(st.cuda_stream)))

        if capacity is None:
            call(0, None, None)
            st.synchronize()
            capacity = int(d_match_offsets[-1].item())
        if d_out is None:
            d_out = torch.empty((capacity, 4), dtype=torch.int32, device=d_offs.device)
        if d_docs is not None and d_out_docs is None:
            d_out_docs = torch.empty(capacity, dtype=torch.int32, device=d_offs.device)
        call(capacity, d_out, d_out_docs)
        return (d_match_offsets, d_out) if d_docs is None else (d_match_offsets, d_out, d_out_docs)

    def mems_host(self, seqs, offs, min_length, digest=None, want_docs=False):
        """spm_mems_begin / _fetch: reads in, (match_offsets uint64[reads + 1], records mems.MATCH_DTYPE[, docs uint32], values
        uint64[reads]) out; values = the read's positions after digestion.  digest: (kind, k, w) or None."""
        from .mems import MATCH_DTYPE

        L = _spm()
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        nreads = offs.size - 1
        kind, k, w = digest if digest else (0, 0, 0)
        moffs = np.zeros(max(nreads, 0) + 1, dtype=np.uint64)
        vals = np.zeros(max(nreads, 1), dtype=np.uint64)
        n = C.c_uint64()
        _check(L.spm_mems_begin(self._h, kind, k, w, _np_ptr(seqs), _np_ptr(offs), nreads, int(min_length), 1 if want_docs else 0,
                                _np_ptr(moffs), _np_ptr(vals), C.byref(n)))
        rec = np.zeros(max(n.value, 1), dtype=MATCH_DTYPE)
        docs = np.zeros(max(n.value, 1), dtype=np.uint32) if want_docs else None
        _check(L.spm_mems_fetch(self._h, _np_ptr(rec), _np_ptr(docs)))
        out = (moffs, rec[: n.value]) + ((docs[: n.value],) if want_docs else ())
        return out + (vals[:nreads],)

    def mems_stats(self) -> dict:
        """Of the most recent mems_device / mems_host call: values, matches, records written, longest length, kernel time."""
        s = SpmMemsStats()
        _check(_spm().spm_last_mems_stats(self._h, C.byref(s)))
        return {f[0]: getattr(s, f[0]) for f in SpmMemsStats._fields_}

    # -- placements (include/spumoni_place.h) ---------------------------------------
    def place_device(self, d_seqs, d_lengths, d_pointers, d_offs, min_seed, mismatch_penalty=4, x_drop=16, d_docs=None,
                     d_out=None, total_values=None, stream=None):
        """One record per read (spp_placement, place.PLACEMENT_DTYPE: where the read's longest match, extended without gaps,
        sits on the text) from the reads, the MS lengths and pointers of a query and the text the index holds, on the device:
        returns d_out, an int32 tensor of shape (reads, 8).  int16 / uint16 lengths select the 16-bit form (d_docs has the
        same width).  total_values: d_offs[-1] - d_offs[0] or an upper bound (default: what d_lengths holds)."""
        import torch

        L = _spp()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        nreads = d_offs.numel() - 1
        if d_docs is not None and d_lengths.element_size() != d_docs.element_size():
            raise SpxError("d_lengths and d_docs must have the same width")
        if d_out is None:
            d_out = torch.empty((max(nreads, 0), 8), dtype=torch.int32, device=d_offs.device)
        total = d_lengths.numel() if total_values is None else int(total_values)
        _check(L.spp_place_device(self._h, _t_ptr(d_seqs), _t_ptr(d_lengths), d_lengths.element_size() * 8, _t_ptr(d_pointers),
                                  _t_ptr(d_docs), _t_ptr(d_offs), nreads, total, int(min_seed), int(mismatch_penalty), int(x_drop),
                                  _t_ptr(d_out), C.c_void_p(st.cuda_stream)))
        return d_out

    def place_host(self, seqs, offs, min_seed, mismatch_penalty=4, x_drop=16, digest=None, want_docs=False):
        """spp_place_batch: reads in, (records place.PLACEMENT_DTYPE[reads], values uint64[reads]) out; values = the read's
        positions after digestion.  digest: (kind, k, w) or None."""
        from .place import PLACEMENT_DTYPE

        L = _spp()
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        nreads = offs.size - 1
        kind, k, w = digest if digest else (0, 0, 0)
        rec = np.zeros(max(nreads, 1), dtype=PLACEMENT_DTYPE)
        vals = np.zeros(max(nreads, 1), dtype=np.uint64)
        _check(L.spp_place_batch(self._h, kind, k, w, _np_ptr(seqs), _np_ptr(offs), nreads, int(min_seed), int(mismatch_penalty),
                                 int(x_drop), 1 if want_docs else 0, _np_ptr(rec), _np_ptr(vals)))
        return rec[:nreads], vals[:nreads]

    def place_stats(self) -> dict:
        """Of the most recent place_device / place_host call: values, placed reads, the sums of seed_len and of left + right,
        kernel time."""
        s = SppPlaceStats()
        _check(_spp().spp_last_place_stats(self._h, C.byref(s)))
        return {f[0]: getattr(s, f[0]) for f in SppPlaceStats._fields_}

    # -- chains (include/spumoni_chain.h) -------------------------------------------
    def chain_device(self, d_matches, d_match_offsets, params=None, d_match_docs=None, d_out=None, d_out_score=None,
                     d_out_pred=None, stream=None):
        """One record per read (spc_chain, chain.CHAIN_DTYPE: the best collinear chain of the read's matches) from the
        records mems_device left on the device: d_matches int32 (n, 4), d_match_offsets int64[reads + 1] (its first entry
        need not be 0), d_match_docs int32[n] or None.  Returns d_out, an int32 tensor of shape (reads, 12); d_out_score /
        d_out_pred (int32[n], optional) get f and pred of every anchor.  params: (lookback, max_dist, max_gap,
        gap_penalty) or None for the defaults."""
        import torch

        from .chain import ChainParams

        L = _spc()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        nreads = d_match_offsets.numel() - 1
        if d_out is None:
            d_out = torch.empty((max(nreads, 0), 12), dtype=torch.int32, device=d_match_offsets.device)
        if d_matches.numel() == 0:  # (no anchors at all: the library still wants an address)
            d_matches = torch.zeros((1, 4), dtype=torch.int32, device=d_match_offsets.device)
        p = SpcParams(*(int(v) for v in (ChainParams() if params is None else params)))
        _check(L.spc_chain_device(self._h, _t_ptr(d_matches), _t_ptr(d_match_docs), _t_ptr(d_match_offsets), nreads, C.byref(p),
                                  _t_ptr(d_out), _t_ptr(d_out_score), _t_ptr(d_out_pred), C.c_void_p(st.cuda_stream)))
        return d_out

    def chain_host(self, seqs, offs, min_length, params=None, digest=None, want_docs=False):
        """spc_chain_batch: reads in, (records chain.CHAIN_DTYPE[reads], values uint64[reads]) out; values = the read's
        positions after digestion.  digest: (kind, k, w) or None; params as in chain_device."""
        from .chain import CHAIN_DTYPE, ChainParams

        L = _spc()
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        nreads = offs.size - 1
        kind, k, w = digest if digest else (0, 0, 0)
        rec = np.zeros(max(nreads, 1), dtype=CHAIN_DTYPE)
        vals = np.zeros(max(nreads, 1), dtype=np.uint64)
        p = SpcParams(*(int(v) for v in (ChainParams() if params is None else params)))
        _check(L.spc_chain_batch(self._h, kind, k, w, _np_ptr(seqs), _np_ptr(offs), nreads, int(min_length), 1 if want_docs else 0,
                                 C.byref(p), _np_ptr(rec), _np_ptr(vals)))
        return rec[:nreads], vals[:nreads]

    def chain_stats(self) -> dict:
        """Of the most recent chain_device / chain_host call: reads, anchors, chained reads, the anchors in their chains,
        the eligible pairs evaluated, kernel time."""
        s = SpcChainStats()
        _check(_spc().spc_last_chain_stats(self._h, C.byref(s)))
        return {f[0]: getattr(s, f[0]) for f in SpcChainStats._fields_}

    # -- alignments (include/spumoni_align.h) ---------------------------------------
    def align_device(self, d_reads, d_read_offsets, d_matches, d_match_offsets, d_chains, d_pred, params=None, gap_capacity=None,
                     d_out=None, d_out_gap_offsets=None, d_out_gaps=None, stream=None):
        """One record per read (spa_alignment, align.ALIGN_DTYPE: the read aligned along its best chain, every gap between
        two anchors filled by an edit-distance table) from what mems_device and chain_device left on the device: d_reads
        uint8 with d_read_offsets int64[reads + 1], d_matches int32 (n, 4) with d_match_offsets int64[reads + 1], d_chains
        int32 (reads, 12) and d_pred int32[n] (chain_device's d_out and d_out_pred).  Returns (d_out int32 (reads, 12),
        d_out_gap_offsets int64[reads + 1], d_out_gaps int32 (gap_capacity, 4)); gap_capacity defaults to the number of
        matches, which always suffices.  params: (max_fill,) or None for the default."""
        import torch

        from .align import AlignParams

        L = _spa()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        dev = d_match_offsets.device
        nreads = d_match_offsets.numel() - 1
        if gap_capacity is None:
            gap_capacity = d_matches.numel() // 4
        if d_out is None:
            d_out = torch.empty((max(nreads, 0), 12), dtype=torch.int32, device=dev)
        if d_out_gap_offsets is None:
            d_out_gap_offsets = torch.empty(max(nreads, 0) + 1, dtype=torch.int64, device=dev)
        if d_out_gaps is None:
            d_out_gaps = torch.empty((max(int(gap_capacity), 1), 4), dtype=torch.int32, device=dev)
        p = SpaParams(*(int(v) for v in (AlignParams() if params is None else params)))
        _check(L.spa_align_device(self._h, _t_ptr(d_reads), _t_ptr(d_read_offsets), _t_ptr(d_matches), _t_ptr(d_match_offsets), nreads,
                                  _t_ptr(d_chains), _t_ptr(d_pred), C.byref(p), int(gap_capacity), _t_ptr(d_out),
                                  _t_ptr(d_out_gap_offsets), _t_ptr(d_out_gaps), C.c_void_p(st.cuda_stream)))
        return d_out, d_out_gap_offsets, d_out_gaps

    def align_host(self, seqs, offs, min_length, chain_params=None, params=None, digest=None, want_docs=False):
        """spa_align_batch: reads in, (records align.ALIGN_DTYPE[reads], chains chain.CHAIN_DTYPE[reads], values
        uint64[reads]) out; values = the read's positions after digestion.  digest: (kind, k, w) or None."""
        from .align import ALIGN_DTYPE, AlignParams
        from .chain import CHAIN_DTYPE, ChainParams

        L = _spa()
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        nreads = offs.size - 1
        kind, k, w = digest if digest else (0, 0, 0)
        rec = np.zeros(max(nreads, 1), dtype=ALIGN_DTYPE)
        chains = np.zeros(max(nreads, 1), dtype=CHAIN_DTYPE)
        vals = np.zeros(max(nreads, 1), dtype=np.uint64)
        cp = SpcParams(*(int(v) for v in (ChainParams() if chain_params is None else chain_params)))
        ap = SpaParams(*(int(v) for v in (AlignParams() if params is None else params)))
        _check(L.spa_align_batch(self._h, kind, k, w, _np_ptr(seqs), _np_ptr(offs), nreads, int(min_length), 1 if want_docs else 0,
                                 C.byref(cp), C.byref(ap), _np_ptr(rec), _np_ptr(chains), _np_ptr(vals)))
        return rec[:nreads], chains[:nreads], vals[:nreads]

    def align_stats(self) -> dict:
        """Of the most recent align_device / align_host call: reads, aligned reads, their gaps, the filled ones, table cells,
        the error and overflow flags, kernel time and the time of the four steps (count and scan, walk, fill, reduce)."""
        s = SpaAlignStats()
        _check(_spa().spa_last_align_stats(self._h, C.byref(s)))
        out = {f[0]: getattr(s, f[0]) for f in SpaAlignStats._fields_}
        out["step_ms"] = list(s.step_ms)
        return out

    # -- CIGARs (include/spumoni_cigar.h) -------------------------------------------
    def cigar_device(self, d_reads, d_read_offsets, d_matches, d_match_offsets, d_chains, d_pred, params=None, gap_capacity=None,
                     op_capacity=None, d_out=None, d_out_op_offsets=None, d_out_ops=None, stream=None):
        """align_device's records and, beside them, each read's path as merged entries (length << 4 | op, cigar.py) from the
        same inputs.  Returns (d_out int32 (reads, 12), d_out_op_offsets int64[reads + 1], d_out_ops int32[op_capacity]);
        gap_capacity defaults to the number of matches, which always suffices, op_capacity to the number of read
        characters plus twice the matches plus the reads, which suffices unless gaps of the text go unfilled in runs.
        params: (max_fill,) or None for the default."""
        import torch

        from .align import AlignParams

        L = _spg()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        dev = d_match_offsets.device
        nreads = d_match_offsets.numel() - 1
        if gap_capacity is None:
            gap_capacity = d_matches.numel() // 4
        if op_capacity is None:
            op_capacity = 2 * d_reads.numel() + 2 * (d_matches.numel() // 4) + max(nreads, 0)
        if d_out is None:
            d_out = torch.empty((max(nreads, 0), 12), dtype=torch.int32, device=dev)
        if d_out_op_offsets is None:
            d_out_op_offsets = torch.empty(max(nreads, 0) + 1, dtype=torch.int64, device=dev)
        if d_out_ops is None:
            d_out_ops = torch.empty(max(int(op_capacity), 1), dtype=torch.int32, device=dev)
        p = SpaParams(*(int(v) for v in (AlignParams() if params is None else params)))
        _check(L.spg_cigar_device(self._h, _t_ptr(d_reads), _t_ptr(d_read_offsets), _t_ptr(d_matches), _t_ptr(d_match_offsets), nreads,
                                  _t_ptr(d_chains), _t_ptr(d_pred), C.byref(p), int(gap_capacity), int(op_capacity), _t_ptr(d_out),
                                  _t_ptr(d_out_op_offsets), _t_ptr(d_out_ops), C.c_void_p(st.cuda_stream)))
        return d_out, d_out_op_offsets, d_out_ops

    def cigar_host(self, seqs, offs, min_length, chain_params=None, params=None, digest=None, want_docs=False):
        """spg_cigar_begin + spg_cigar_fetch: reads in, (records align.ALIGN_DTYPE[reads], op_offsets uint64[reads + 1],
        entries uint32[op_offsets[-1]], chains chain.CHAIN_DTYPE[reads], values uint64[reads]) out.  digest: (kind, k, w)
        or None."""
        from .align import ALIGN_DTYPE, AlignParams
        from .chain import CHAIN_DTYPE, ChainParams

        L = _spg()
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        nreads = offs.size - 1
        kind, k, w = digest if digest else (0, 0, 0)
        rec = np.zeros(max(nreads, 1), dtype=ALIGN_DTYPE)
        chains = np.zeros(max(nreads, 1), dtype=CHAIN_DTYPE)
        vals = np.zeros(max(nreads, 1), dtype=np.uint64)
        cp = SpcParams(*(int(v) for v in (ChainParams() if chain_params is None else chain_params)))
        ap = SpaParams(*(int(v) for v in (AlignParams() if params is None else params)))
        n = C.c_uint64(0)
        _check(L.spg_cigar_begin(self._h, kind, k, w, _np_ptr(seqs), _np_ptr(offs), nreads, int(min_length), 1 if want_docs else 0,
                                 C.byref(cp), C.byref(ap), _np_ptr(rec), _np_ptr(chains), _np_ptr(vals), C.byref(n)))
        op_offsets = np.zeros(max(nreads, 0) + 1, dtype=np.uint64)
        ops = np.zeros(max(n.value, 1), dtype=np.uint32)
        _check(L.spg_cigar_fetch(self._h, _np_ptr(op_offsets), _np_ptr(ops)))
        return rec[:nreads], op_offsets, ops[:n.value], chains[:nreads], vals[:nreads]

    def cigar_stats(self) -> dict:
        """Of the most recent cigar_device / cigar_host call: align_stats' counts, the entries, the words of path, the error and
        overflow flags, kernel time, the time of the five steps (plan, lane fills, wavefront fills with their walk back,
        emit, reduce) and the wavefronts' ticks of fill and walk back."""
        s = SpgCigarStats()
        _check(_spg().spg_last_cigar_stats(self._h, C.byref(s)))
        out = {f[0]: getattr(s, f[0]) for f in SpgCigarStats._fields_}
        out["step_ms"] = list(s.step_ms)
        return out

    # -- extended CIGARs (include/spumoni_extend.h) ----------------------------------
    def extend_device(self, d_reads, d_read_offsets, d_matches, d_match_offsets, d_chains, d_pred, params=None, extend_params=None,
                      gap_capacity=None, op_capacity=None, d_out=None, d_out_op_offsets=None, d_out_ops=None, d_out_ends=None,
                      want_ends=True, stream=None):
        """cigar_device's results with both ends of every alignment extended and the rest of the read soft-clipped
        (extend.py), from the same inputs.  Returns (d_out int32 (reads, 12), d_out_op_offsets int64[reads + 1], d_out_ops
        int32[op_capacity], d_out_ends int32 (2 * reads, 4) or None without want_ends); gap_capacity defaults to the
        number of matches, op_capacity to cigar_device's default plus two clips a read.  params: (max_fill,),
        extend_params: (max_extend, band, mismatch, indel), or None for the defaults."""
        import torch

        from .align import AlignParams
        from .extend import ExtendParams

        L = _spe()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        dev = d_match_offsets.device
        nreads = d_match_offsets.numel() - 1
        if gap_capacity is None:
            gap_capacity = d_matches.numel() // 4
        if op_capacity is None:
            op_capacity = 2 * d_reads.numel() + 2 * (d_matches.numel() // 4) + 3 * max(nreads, 0)
        if d_out is None:
            d_out = torch.empty((max(nreads, 0), 12), dtype=torch.int32, device=dev)
        if d_out_op_offsets is None:
            d_out_op_offsets = torch.empty(max(nreads, 0) + 1, dtype=torch.int64, device=dev)
        if d_out_ops is None:
            d_out_ops = torch.empty(max(int(op_capacity), 1), dtype=torch.int32, device=dev)
        if d_out_ends is None and want_ends:
            d_out_ends = torch.empty((2 * max(nreads, 0), 4), dtype=torch.int32, device=dev)
        p = SpaParams(*(int(v) for v in (AlignParams() if params is None else params)))
        ep = SpeParams(*(int(v) for v in (ExtendParams() if extend_params is None else extend_params)))
        _check(L.spe_extend_device(self._h, _t_ptr(d_reads), _t_ptr(d_read_offsets), _t_ptr(d_matches), _t_ptr(d_match_offsets), nreads,
                                   _t_ptr(d_chains), _t_ptr(d_pred), C.byref(p), C.byref(ep), int(gap_capacity), int(op_capacity),
                                   _t_ptr(d_out), _t_ptr(d_out_op_offsets), _t_ptr(d_out_ops), _t_ptr(d_out_ends),
                                   C.c_void_p(st.cuda_stream)))
        return d_out, d_out_op_offsets, d_out_ops, d_out_ends

    def extend_host(self, seqs, offs, min_length, chain_params=None, params=None, extend_params=None, digest=None, want_docs=False):
        """spe_extend_begin + spe_extend_fetch: reads in, cigar_host's tuple plus the ends out: (records
        align.ALIGN_DTYPE[reads], op_offsets uint64[reads + 1], entries uint32[op_offsets[-1]], chains
        chain.CHAIN_DTYPE[reads], values uint64[reads], ends extend.END_DTYPE[2 * reads]).  digest: (kind, k, w) or None."""
        from .align import ALIGN_DTYPE, AlignParams
        from .chain import CHAIN_DTYPE, ChainParams
        from .extend import END_DTYPE, ExtendParams

        L = _spe()
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        nreads = offs.size - 1
        kind, k, w = digest if digest else (0, 0, 0)
        rec = np.zeros(max(nreads, 1), dtype=ALIGN_DTYPE)
        chains = np.zeros(max(nreads, 1), dtype=CHAIN_DTYPE)
        vals = np.zeros(max(nreads, 1), dtype=np.uint64)
        ends = np.zeros(2 * max(nreads, 1), dtype=END_DTYPE)
        cp = SpcParams(*(int(v) for v in (ChainParams() if chain_params is None else chain_params)))
        ap = SpaParams(*(int(v) for v in (AlignParams() if params is None else params)))
        ep = SpeParams(*(int(v) for v in (ExtendParams() if extend_params is None else extend_params)))
        n = C.c_uint64(0)
        _check(L.spe_extend_begin(self._h, kind, k, w, _np_ptr(seqs), _np_ptr(offs), nreads, int(min_length), 1 if want_docs else 0,
                                  C.byref(cp), C.byref(ap), C.byref(ep), _np_ptr(rec), _np_ptr(chains), _np_ptr(vals), _np_ptr(ends),
                                  C.byref(n)))
        op_offsets = np.zeros(max(nreads, 0) + 1, dtype=np.uint64)
        ops = np.zeros(max(n.value, 1), dtype=np.uint32)
        _check(L.spe_extend_fetch(self._h, _np_ptr(op_offsets), _np_ptr(ops)))
        return rec[:nreads], op_offsets, ops[:n.value], chains[:nreads], vals[:nreads], ends[:2 * nreads]

    def extend_stats(self) -> dict:
        """Of the most recent extend_device / extend_host call: cigar_stats' counts, the ends looked at and extended, the
        band cells, the clipped characters, the error and overflow flags, kernel time and the time of the six steps (cigar's
        five, then the ends)."""
        s = SpeExtendStats()
        _check(_spe().spe_last_extend_stats(self._h, C.byref(s)))
        out = {f[0]: getattr(s, f[0]) for f in SpeExtendStats._fields_ if f[0] != "reserved"}
        out["step_ms"] = list(s.step_ms)
        return out

    # -- mappings (include/spumoni_map.h) ----------------------------------------------
    def set_sequences(self, seq_lengths, strands: int) -> None:
        """The sequence table (map.read_seq_table's lengths and strands): copied to the device and held in the handle."""
        lengths = np.ascontiguousarray(seq_lengths, dtype=np.uint64)
        _check(_spn().spn_set_sequences(self._h, _np_ptr(lengths), lengths.size, int(strands)))
        self._n_seqs = int(lengths.size)

    def map_device(self, d_alignments, d_op_offsets, d_ops, d_read_offsets, op_capacity=None, in_entries=None, d_out=None,
                   d_out_op_offsets=None, d_out_ops=None, stream=None):
        """extend_device's (d_out, d_out_op_offsets, d_out_ops) and the reads' offsets in, the mappings out (map.py):
        (d_out int32 (reads, 12), a view of map.MAPPING_DTYPE; d_out_op_offsets int64[reads + 1]; d_out_ops
        int32[op_capacity]).  in_entries defaults to d_ops' size, op_capacity to in_entries plus two a read."""
        import torch

        L = _spn()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        dev = d_read_offsets.device
        nreads = d_read_offsets.numel() - 1
        if in_entries is None:
            in_entries = d_ops.numel()
        if op_capacity is None:
            op_capacity = int(in_entries) + 2 * max(nreads, 0)
        if d_out is None:
            d_out = torch.empty((max(nreads, 0), 12), dtype=torch.int32, device=dev)
        if d_out_op_offsets is None:
            d_out_op_offsets = torch.empty(max(nreads, 0) + 1, dtype=torch.int64, device=dev)
        if d_out_ops is None:
            d_out_ops = torch.empty(max(int(op_capacity), 1), dtype=torch.int32, device=dev)
        _check(L.spn_map_device(self._h, _t_ptr(d_alignments), _t_ptr(d_op_offsets), _t_ptr(d_ops), int(in_entries),
                                _t_ptr(d_read_offsets), nreads, int(op_capacity), _t_ptr(d_out), _t_ptr(d_out_op_offsets),
                                _t_ptr(d_out_ops), C.c_void_p(st.cuda_stream)))
        return d_out, d_out_op_offsets, d_out_ops

    def map_host(self, seqs, offs, min_length, chain_params=None, params=None, extend_params=None, digest=None, want_docs=False):
        """spn_map_begin + spn_map_fetch: reads in, (mappings map.MAPPING_DTYPE[reads], op_offsets uint64[reads + 1],
        entries uint32[op_offsets[-1]], alignments align.ALIGN_DTYPE[reads]) out.  digest: (kind, k, w) or None."""
        from .align import ALIGN_DTYPE, AlignParams
        from .chain import ChainParams
        from .extend import ExtendParams
        from .map import MAPPING_DTYPE

        L = _spn()
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        nreads = offs.size - 1
        kind, k, w = digest if digest else (0, 0, 0)
        out = np.zeros(max(nreads, 1), dtype=MAPPING_DTYPE)
        rec = np.zeros(max(nreads, 1), dtype=ALIGN_DTYPE)
        cp = SpcParams(*(int(v) for v in (ChainParams() if chain_params is None else chain_params)))
        ap = SpaParams(*(int(v) for v in (AlignParams() if params is None else params)))
        ep = SpeParams(*(int(v) for v in (ExtendParams() if extend_params is None else extend_params)))
        n = C.c_uint64(0)
        _check(L.spn_map_begin(self._h, kind, k, w, _np_ptr(seqs), _np_ptr(offs), nreads, int(min_length), 1 if want_docs else 0,
                               C.byref(cp), C.byref(ap), C.byref(ep), _np_ptr(out), _np_ptr(rec), C.byref(n)))
        op_offsets = np.zeros(max(nreads, 0) + 1, dtype=np.uint64)
        ops = np.zeros(max(n.value, 1), dtype=np.uint32)
        _check(L.spn_map_fetch(self._h, _np_ptr(op_offsets), _np_ptr(ops)))
        return out[:nreads], op_offsets, ops[:n.value], rec[:nreads]

    def map_stats(self) -> dict:
        """Of the most recent map_device / map_host call: the reads, the mapped, cut and reverse-strand reads, the entries
        in and out, the characters that cuts clipped, the error and overflow flags, kernel time and the time of the two
        steps (locate and count, write)."""
        s = SpnMapStats()
        _check(_spn().spn_last_map_stats(self._h, C.byref(s)))
        out = {f[0]: getattr(s, f[0]) for f in SpnMapStats._fields_ if f[0] != "reserved"}
        out["step_ms"] = list(s.step_ms)
        return out

    # -- coverage (include/spumoni_cover.h) --------------------------------------------
    def cover_add_device(self, d_mappings, d_op_offsets, d_ops, d_diff, d_mism, d_seq_counts, in_entries=None, stream=None) -> None:
        """map_device's (d_out, d_out_op_offsets, d_out_ops) added to d_diff int32[G + 1], d_mism int32[G] and d_seq_counts
        int64[2 * n_seqs] (cover.py).  in_entries defaults to d_ops' size."""
        import torch

        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        nreads = d_op_offsets.numel() - 1
        if in_entries is None:
            in_entries = d_ops.numel()
        _check(_spd().spd_cover_add_device(self._h, _t_ptr(d_mappings), _t_ptr(d_op_offsets), _t_ptr(d_ops), int(in_entries), nreads,
                                           _t_ptr(d_diff), _t_ptr(d_mism), _t_ptr(d_seq_counts), C.c_void_p(st.cuda_stream)))

    def cover_finish_device(self, d_diff, d_mism, d_seq_counts, d_depth=None, d_out=None, stream=None):
        """(d_depth int32[G], d_out int64 (n_seqs, 6), a view of cover.SEQ_COVER_DTYPE) of the three arrays, which stay as
        they are."""
        import torch

        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        if d_depth is None:
            d_depth = torch.empty(d_mism.numel(), dtype=torch.int32, device=d_mism.device)
        if d_out is None:
            d_out = torch.empty((d_seq_counts.numel() // 2, 6), dtype=torch.int64, device=d_mism.device)
        _check(_spd().spd_cover_finish_device(self._h, _t_ptr(d_diff), _t_ptr(d_mism), _t_ptr(d_seq_counts), _t_ptr(d_depth),
                                              _t_ptr(d_out), C.c_void_p(st.cuda_stream)))
        return d_depth, d_out

    def cover_runs_device(self, d_depth, d_mism, min_depth, run_capacity, d_runs=None, d_count=None, stream=None):
        """(d_runs int64 (run_capacity, 4), a view of cover.RUN_DTYPE; d_count int64[1]): the runs of depth >= min_depth."""
        import torch

        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        if d_runs is None:
            d_runs = torch.empty((max(int(run_capacity), 1), 4), dtype=torch.int64, device=d_depth.device)
        if d_count is None:
            d_count = torch.empty(1, dtype=torch.int64, device=d_depth.device)
        _check(_spd().spd_cover_runs_device(self._h, _t_ptr(d_depth), _t_ptr(d_mism), int(min_depth), int(run_capacity), _t_ptr(d_runs),
                                            _t_ptr(d_count), C.c_void_p(st.cuda_stream)))
        return d_runs, d_count

    def cover_reset(self) -> None:
        """Allocates the handle's coverage arrays for the sequence table in force, or zeroes them."""
        _check(_spd().spd_cover_reset(self._h))

    def cover_add_host(self, seqs, offs, min_length, chain_params=None, params=None, extend_params=None, digest=None, want_docs=False):
        """spd_cover_add_batch: map_host's arguments; the mappings are added to the handle's arrays on the device and come
        back (map.MAPPING_DTYPE[reads]); the entries do not."""
        from .align import AlignParams
        from .chain import ChainParams
        from .extend import ExtendParams
        from .map import MAPPING_DTYPE

        L = _spd()
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        nreads = offs.size - 1
        kind, k, w = digest if digest else (0, 0, 0)
        out = np.zeros(max(nreads, 1), dtype=MAPPING_DTYPE)
        cp = SpcParams(*(int(v) for v in (ChainParams() if chain_params is None else chain_params)))
        ap = SpaParams(*(int(v) for v in (AlignParams() if params is None else params)))
        ep = SpeParams(*(int(v) for v in (ExtendParams() if extend_params is None else extend_params)))
        _check(L.spd_cover_add_batch(self._h, kind, k, w, _np_ptr(seqs), _np_ptr(offs), nreads, int(min_length), 1 if want_docs else 0,
                                     C.byref(cp), C.byref(ap), C.byref(ep), _np_ptr(out)))
        return out[:nreads]

    def cover_summary(self, n_seqs: int) -> np.ndarray:
        """cover.SEQ_COVER_DTYPE[n_seqs] of everything added since cover_reset, in table order."""
        from .cover import SEQ_COVER_DTYPE

        out = np.zeros(max(int(n_seqs), 1), dtype=SEQ_COVER_DTYPE)
        _check(_spd().spd_cover_summary(self._h, _np_ptr(out), int(n_seqs)))
        return out[:int(n_seqs)]

    def cover_runs(self, min_depth: int = 1) -> np.ndarray:
        """spd_cover_runs_begin + _fetch: cover.RUN_DTYPE[] of the runs of depth >= min_depth."""
        from .cover import RUN_DTYPE

        L = _spd()
        n = C.c_uint64(0)
        _check(L.spd_cover_runs_begin(self._h, int(min_depth), C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=RUN_DTYPE)
        _check(L.spd_cover_runs_fetch(self._h, _np_ptr(out)))
        return out[:n.value]

    def cover_depth(self, first: int, count: int):
        """(depth uint32[count], mism uint32[count]) of the positions [first, first + count) of the forward genome."""
        depth, mism = np.zeros(max(int(count), 1), dtype=np.uint32), np.zeros(max(int(count), 1), dtype=np.uint32)
        _check(_spd().spd_cover_depth(self._h, int(first), int(count), _np_ptr(depth), _np_ptr(mism)))
        return depth[:int(count)], mism[:int(count)]

    def cover_stats(self) -> dict:
        """Of the most recent cover_* calls: the reads, the mapped, added and skipped ones, intervals and atomic adds of the
        adds (since cover_reset for cover_add_host, of the last call for cover_add_device), the runs of the last runs
        call, the error and overflow flags and the time of the last add, finish and runs step."""
        s = SpdCoverStats()
        _check(_spd().spd_last_cover_stats(self._h, C.byref(s)))
        out = {f[0]: getattr(s, f[0]) for f in SpdCoverStats._fields_}
        out["step_ms"] = list(s.step_ms)
        return out

    # -- pileup and calls (include/spumoni_call.h) ------------------------------------------
    def pileup_add_device(self, d_mappings, d_op_offsets, d_ops, d_reads, d_read_offsets, d_alt, d_other, d_ins, d_ddiff, in_entries=None,
                          in_chars=None, stream=None) -> None:
        """map_device's (d_out, d_out_op_offsets, d_out_ops) and the reads' bytes (d_reads uint8, d_read_offsets int64[reads + 1])
        added to d_alt int32[4 * G], d_other int32[G], d_ins int32[G] and d_ddiff int32[G + 1] (call.py).  in_entries and
        in_chars default to d_ops' and d_reads' sizes."""
        import torch

        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        nreads = d_op_offsets.numel() - 1
        if in_entries is None:
            in_entries = d_ops.numel()
        if in_chars is None:
            in_chars = d_reads.numel()
        _check(_spl().spl_pileup_add_device(self._h, _t_ptr(d_mappings), _t_ptr(d_op_offsets), _t_ptr(d_ops), int(in_entries),
                                            _t_ptr(d_reads), _t_ptr(d_read_offsets), int(in_chars), nreads, _t_ptr(d_alt), _t_ptr(d_other),
                                            _t_ptr(d_ins), _t_ptr(d_ddiff), C.c_void_p(st.cuda_stream)))

    def pileup_finish_device(self, d_ddiff, d_del=None, stream=None):
        """d_del int32[G]: the running sum of d_ddiff, which stays as it is."""
        import torch

        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        if d_del is None:
            d_del = torch.empty(d_ddiff.numel() - 1, dtype=torch.int32, device=d_ddiff.device)
        _check(_spl().spl_pileup_finish_device(self._h, _t_ptr(d_ddiff), _t_ptr(d_del), C.c_void_p(st.cuda_stream)))
        return d_del

    def calls_device(self, d_depth, d_mism, d_alt, d_other, d_ins, d_del, min_depth=2, min_alt=2, min_permille=500, call_capacity=0,
                     d_calls=None, d_count=None, stream=None):
        """(d_calls int64 (call_capacity, 6), a view of call.CALL_DTYPE; d_count int64[1]): the calls of the arrays."""
        import torch

        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        if d_calls is None:
            d_calls = torch.empty((max(int(call_capacity), 1), 6), dtype=torch.int64, device=d_depth.device)
        if d_count is None:
            d_count = torch.empty(1, dtype=torch.int64, device=d_depth.device)
        _check(_spl().spl_calls_device(self._h, _t_ptr(d_depth), _t_ptr(d_mism), _t_ptr(d_alt), _t_ptr(d_other), _t_ptr(d_ins), _t_ptr(d_del),
                                       int(min_depth), int(min_alt), int(min_permille), int(call_capacity), _t_ptr(d_calls), _t_ptr(d_count),
                                       C.c_void_p(st.cuda_stream)))
        return d_calls, d_count

    def call_reset(self) -> None:
        """cover_reset, and the handle's pileup arrays allocated for the sequence table in force, or zeroed."""
        _check(_spl().spl_call_reset(self._h))

    def call_add_host(self, seqs, offs, min_length, chain_params=None, params=None, extend_params=None, digest=None, want_docs=False):
        """spl_call_add_batch: cover_add_host's arguments; the mappings are added to the handle's coverage and to its
        pileup on the device and come back (map.MAPPING_DTYPE[reads])."""
        from .align import AlignParams
        from .chain import ChainParams
        from .extend import ExtendParams
        from .map import MAPPING_DTYPE

        L = _spl()
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        nreads = offs.size - 1
        kind, k, w = digest if digest else (0, 0, 0)
        out = np.zeros(max(nreads, 1), dtype=MAPPING_DTYPE)
        cp = SpcParams(*(int(v) for v in (ChainParams() if chain_params is None else chain_params)))
        ap = SpaParams(*(int(v) for v in (AlignParams() if params is None else params)))
        ep = SpeParams(*(int(v) for v in (ExtendParams() if extend_params is None else extend_params)))
        _check(L.spl_call_add_batch(self._h, kind, k, w, _np_ptr(seqs), _np_ptr(offs), nreads, int(min_length), 1 if want_docs else 0,
                                    C.byref(cp), C.byref(ap), C.byref(ep), _np_ptr(out)))
        return out[:nreads]

    def calls(self, min_depth: int = 2, min_alt: int = 2, min_permille: int = 500) -> np.ndarray:
        """spl_calls_begin + _fetch: call.CALL_DTYPE[] in (sequence, position) order."""
        from .call import CALL_DTYPE

        L = _spl()
        n = C.c_uint64(0)
        _check(L.spl_calls_begin(self._h, int(min_depth), int(min_alt), int(min_permille), C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=CALL_DTYPE)
        _check(L.spl_calls_fetch(self._h, _np_ptr(out)))
        return out[:n.value]

    def pileup_counts(self, first: int, count: int):
        """(alt uint32 (count, 4), other, ins, del uint32[count]) of the positions [first, first + count) of the forward genome."""
        n = max(int(count), 1)
        alt, other, ins, dele = (np.zeros(4 * n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32),
                                 np.zeros(n, dtype=np.uint32))
        _check(_spl().spl_pileup_counts(self._h, int(first), int(count), _np_ptr(alt), _np_ptr(other), _np_ptr(ins), _np_ptr(dele)))
        return alt[:4 * int(count)].reshape(-1, 4), other[:int(count)], ins[:int(count)], dele[:int(count)]

    def call_stats(self) -> dict:
        """Of the most recent pileup and calls steps: the reads, the mapped, added and skipped ones, the 'X' columns, those
        of a byte outside ACGT, the 'I' and 'D' entries and the atomic adds of the adds (since call_reset for
        call_add_host, of the last call for pileup_add_device), the calls of the last calls step, the error and overflow
        flags and the time of the last add, finish and calls step."""
        s = SplCallStats()
        _check(_spl().spl_last_call_stats(self._h, C.byref(s)))
        out = {f[0]: getattr(s, f[0]) for f in SplCallStats._fields_ if f[0] != "reserved"}
        out["step_ms"] = list(s.step_ms)
        return out

    # -- consensus (include/spumoni_consensus.h) ----------------------------------------------
    def consensus_device(self, d_depth, d_alt, d_ins, d_del, min_depth=2, min_alt=2, min_permille=500, mask=ord("N"), line_width=60,
                         body_capacity=0, d_records=None, d_body=None, d_count=None, stream=None):
        """(d_records int64 (n_seqs, 6), a view of consensus.SEQ_DTYPE; d_body uint8[body_capacity] or None; d_count int64[1]):
        the consensus of the arrays (consensus.py).  n_seqs is d_records' when it is given, else the table's as set through
        set_sequences on this object."""
        import torch

        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        if d_records is None:
            d_records = torch.empty((self._n_seqs, 6), dtype=torch.int64, device=d_depth.device)
        if d_body is None and body_capacity:
            d_body = torch.empty(int(body_capacity), dtype=torch.uint8, device=d_depth.device)
        if d_count is None:
            d_count = torch.empty(1, dtype=torch.int64, device=d_depth.device)
        p = _sps_params(min_depth, min_alt, min_permille, mask, line_width)
        _check(_sps().sps_consensus_device(self._h, _t_ptr(d_depth), _t_ptr(d_alt), _t_ptr(d_ins), _t_ptr(d_del), C.byref(p),
                                           int(body_capacity), _t_ptr(d_records), _t_ptr(d_body), _t_ptr(d_count),
                                           C.c_void_p(st.cuda_stream)))
        return d_records, d_body, d_count

    def consensus(self, min_depth: int = 2, min_alt: int = 2, min_permille: int = 500, mask=ord("N"), line_width: int = 60):
        """sps_consensus_begin + _fetch on the handle's arrays of call_reset / call_add_host: (consensus.SEQ_DTYPE[n_seqs],
        body uint8[])."""
        from .consensus import SEQ_DTYPE

        L = _sps()
        n = C.c_uint64(0)
        p = _sps_params(min_depth, min_alt, min_permille, mask, line_width)
        _check(L.sps_consensus_begin(self._h, C.byref(p), C.byref(n)))
        records = np.zeros(max(self._n_seqs, 1), dtype=SEQ_DTYPE)
        body = np.zeros(max(n.value, 1), dtype=np.uint8)
        _check(L.sps_consensus_fetch(self._h, _np_ptr(records), _np_ptr(body)))
        return records[:self._n_seqs], body[:n.value]

    def consensus_stats(self) -> dict:
        """Of the most recent consensus: the positions and how they were decided, the insertion sites, the letters and the
        bytes of the body, the overflow flag and the time of the count, the scans and the write."""
        s = SpsConsensusStats()
        _check(_sps().sps_last_consensus_stats(self._h, C.byref(s)))
        out = {f[0]: getattr(s, f[0]) for f in SpsConsensusStats._fields_}
        out["step_ms"] = list(s.step_ms)
        return out

    def last_chunk_stats(self) -> dict:
        """Chunked walk of the last query: chunk size (0 = it ran the plain walk), characters walked a second
        time to join the chunks, reads that fell back to the plain walk."""
        o = (C.c_uint64 * 4)()
        _check(lib().spx_last_chunk_stats(self._h, C.byref(o)))
        return {"chunk_len": o[0], "chunks_bound": o[1], "rewalked_chars": o[2], "fallback_reads": o[3]}

    def last_stats(self) -> dict:
        s = SpxWalkStats()
        _check(lib().spx_last_walk_stats(self._h, C.byref(s)))
        return {f[0]: getattr(s, f[0]) for f in SpxWalkStats._fields_}


def digester(device: int = 0) -> "Index":
    """A minimal index handle, for callers that only want the device digestion (index builders)."""
    import torch

    from .synth import RawIndex

    z = torch.zeros(1, dtype=torch.int64)
    return Index.from_raw(RawIndex(heads=torch.zeros(1, dtype=torch.uint8), lens=torch.ones(1, dtype=torch.int64),
                                   thr=z, n=1), device)


def pinned_array(shape, dtype):
    """numpy array backed by spx_host_alloc (page-locked) memory; keep the returned owner alive."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = lib().spx_host_alloc(max(n, 1))
    if not p:
        raise SpxError(lib().spx_last_error().decode())
    buf = (C.c_char * max(n, 1)).from_address(p)
    arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    free = lib().spx_host_free

    class _Owner:
        def __del__(self_inner):
            try:
                free(p)
            except Exception:
                pass

    return arr, _Owner()


def pad_seqs(seqs):
    """Return a copy of seqs with the slack spx_query_batch_device asks for
    (readable for round_up(n, 4) + 32 bytes)."""
    import torch

    n = seqs.numel()
    padded = torch.zeros(((n + 3) // 4) * 4 + 32, dtype=torch.uint8, device=seqs.device)
    padded[:n] = seqs
    return padded


# ---- the document votes (include/spumoni_docvote.h) -----------------------------------------------------------------
DOCVOTE_EXPORTS = ["spv_votes_device", "spv_assign_batch", "spv_last_votes_stats"]
_SPV_READY = False


class SpvVotesStats(C.Structure):
    _fields_ = [("reads_short", C.c_uint64), ("reads_medium", C.c_uint64), ("reads_long", C.c_uint64),
                ("reads_empty", C.c_uint64), ("voting_positions", C.c_uint64), ("long_tiles", C.c_uint64),
                ("kernel_ms", C.c_float)]


def _spv() -> C.CDLL:
    """The library with the spv_* argtypes set (on first use)."""
    global _SPV_READY
    L = lib()
    if not hasattr(L, "spv_assign_batch"):
        raise SpxError(f"{LIB_PATH} has no document votes (spv_assign_batch): there is no CPU fallback")
    if not _SPV_READY:
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.spv_votes_device.argtypes = [vp, vp, vp, i32, vp, u64, u64, u64, vp, vp]
        L.spv_assign_batch.argtypes = [vp, i32, i32, u32, u32, vp, vp, u64, u64, vp, vp]
        L.spv_last_votes_stats.argtypes = [vp, C.POINTER(SpvVotesStats)]
        _SPV_READY = True
    return L


# ---- the matches (include/spumoni_mems.h) ---------------------------------------------------------------------------
MEMS_EXPORTS = ["spm_mems_device", "spm_mems_begin", "spm_mems_fetch", "spm_last_mems_stats"]
_SPM_READY = False


class SpmMemsStats(C.Structure):
    _fields_ = [("values", C.c_uint64), ("matches", C.c_uint64), ("written", C.c_uint64), ("longest", C.c_uint64),
                ("kernel_ms", C.c_float)]


def _spm() -> C.CDLL:
    """The library with the spm_* argtypes set (on first use)."""
    global _SPM_READY
    L = lib()
    if not hasattr(L, "spm_mems_begin"):
        raise SpxError(f"{LIB_PATH} has no match kernels (spm_mems_begin): there is no CPU fallback")
    if not _SPM_READY:
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.spm_mems_device.argtypes = [vp, vp, i32, vp, vp, vp, u64, u64, u64, vp, vp, u64, vp, vp]
        L.spm_mems_begin.argtypes = [vp, i32, u32, u32, vp, vp, u64, u64, i32, vp, vp, C.POINTER(u64)]
        L.spm_mems_fetch.argtypes = [vp, vp, vp]
        L.spm_last_mems_stats.argtypes = [vp, C.POINTER(SpmMemsStats)]
        _SPM_READY = True
    return L


# ---- the placements (include/spumoni_place.h) -----------------------------------------------------------------------
PLACE_EXPORTS = ["spp_place_device", "spp_place_batch", "spp_last_place_stats"]
_SPP_READY = False


class SppPlaceStats(C.Structure):
    _fields_ = [("values", C.c_uint64), ("placed", C.c_uint64), ("seed_values", C.c_uint64), ("extended_values", C.c_uint64),
                ("kernel_ms", C.c_float)]


def _spp() -> C.CDLL:
    """The library with the spp_* argtypes set (on first use)."""
    global _SPP_READY
    L = lib()
    if not hasattr(L, "spp_place_batch"):
        raise SpxError(f"{LIB_PATH} has no placement kernels (spp_place_batch): there is no CPU fallback")
    if not _SPP_READY:
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.spp_place_device.argtypes = [vp, vp, vp, i32, vp, vp, vp, u64, u64, u64, u32, u64, vp, vp]
        L.spp_place_batch.argtypes = [vp, i32, u32, u32, vp, vp, u64, u64, u32, u64, i32, vp, vp]
        L.spp_last_place_stats.argtypes = [vp, C.POINTER(SppPlaceStats)]
        _SPP_READY = True
    return L


# ---- the chains (include/spumoni_chain.h) ---------------------------------------------------------------------------
CHAIN_EXPORTS = ["spc_chain_device", "spc_chain_batch", "spc_last_chain_stats"]
_SPC_READY = False


class SpcParams(C.Structure):
    _fields_ = [("lookback", C.c_uint32), ("max_dist", C.c_uint32), ("max_gap", C.c_uint32), ("gap_penalty", C.c_uint32)]


class SpcChainStats(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("anchors", C.c_uint64), ("chained_reads", C.c_uint64), ("chain_anchors", C.c_uint64),
                ("candidates", C.c_uint64), ("kernel_ms", C.c_float)]


def _spc() -> C.CDLL:
    """The library with the spc_* argtypes set (on first use)."""
    global _SPC_READY
    L = lib()
    if not hasattr(L, "spc_chain_batch"):
        raise SpxError(f"{LIB_PATH} has no chain kernel (spc_chain_batch): there is no CPU fallback")
    if not _SPC_READY:
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.spc_chain_device.argtypes = [vp, vp, vp, vp, u64, C.POINTER(SpcParams), vp, vp, vp, vp]
        L.spc_chain_batch.argtypes = [vp, i32, u32, u32, vp, vp, u64, u64, i32, C.POINTER(SpcParams), vp, vp]
        L.spc_last_chain_stats.argtypes = [vp, C.POINTER(SpcChainStats)]
        _SPC_READY = True
    return L


# ---- the alignments (include/spumoni_align.h) -----------------------------------------------------------------------
ALIGN_EXPORTS = ["spa_align_device", "spa_align_batch", "spa_last_align_stats"]
_SPA_READY = False


class SpaParams(C.Structure):
    _fields_ = [("max_fill", C.c_uint32)]


class SpaAlignStats(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("aligned_reads", C.c_uint64), ("gaps", C.c_uint64), ("filled_gaps", C.c_uint64),
                ("cells", C.c_uint64), ("error", C.c_uint32), ("overflow", C.c_uint32), ("kernel_ms", C.c_float),
                ("step_ms", C.c_float * 4)]


def _spa() -> C.CDLL:
    """The library with the spa_* argtypes set (on first use)."""
    global _SPA_READY
    L = lib()
    if not hasattr(L, "spa_align_batch"):
        raise SpxError(f"{LIB_PATH} has no align kernels (spa_align_batch): there is no CPU fallback")
    if not _SPA_READY:
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.spa_align_device.argtypes = [vp, vp, vp, vp, vp, u64, vp, vp, C.POINTER(SpaParams), u64, vp, vp, vp, vp]
        L.spa_align_batch.argtypes = [vp, i32, u32, u32, vp, vp, u64, u64, i32, C.POINTER(SpcParams), C.POINTER(SpaParams), vp, vp, vp]
        L.spa_last_align_stats.argtypes = [vp, C.POINTER(SpaAlignStats)]
        _SPA_READY = True
    return L


# ---- the CIGARs (include/spumoni_cigar.h) ---------------------------------------------------------------------------
CIGAR_EXPORTS = ["spg_cigar_device", "spg_cigar_begin", "spg_cigar_fetch", "spg_last_cigar_stats"]
_SPG_READY = False


class SpgCigarStats(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("aligned_reads", C.c_uint64), ("gaps", C.c_uint64), ("filled_gaps", C.c_uint64),
                ("cells", C.c_uint64), ("entries", C.c_uint64), ("path_words", C.c_uint64), ("wave_fill_ticks", C.c_uint64),
                ("wave_back_ticks", C.c_uint64), ("error", C.c_uint32), ("overflow", C.c_uint32), ("kernel_ms", C.c_float),
                ("step_ms", C.c_float * 5)]


def _spg() -> C.CDLL:
    """The library with the spg_* argtypes set (on first use)."""
    global _SPG_READY
    L = lib()
    if not hasattr(L, "spg_cigar_begin"):
        raise SpxError(f"{LIB_PATH} has no cigar kernels (spg_cigar_begin): there is no CPU fallback")
    if not _SPG_READY:
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.spg_cigar_device.argtypes = [vp, vp, vp, vp, vp, u64, vp, vp, C.POINTER(SpaParams), u64, u64, vp, vp, vp, vp]
        L.spg_cigar_begin.argtypes = [vp, i32, u32, u32, vp, vp, u64, u64, i32, C.POINTER(SpcParams), C.POINTER(SpaParams), vp, vp, vp,
                                      C.POINTER(u64)]
        L.spg_cigar_fetch.argtypes = [vp, vp, vp]
        L.spg_last_cigar_stats.argtypes = [vp, C.POINTER(SpgCigarStats)]
        _SPG_READY = True
    return L


# ---- the extended CIGARs (include/spumoni_extend.h) -----------------------------------------------------------------
EXTEND_EXPORTS = ["spe_extend_device", "spe_extend_begin", "spe_extend_fetch", "spe_last_extend_stats"]
_SPE_READY = False


class SpeParams(C.Structure):
    _fields_ = [("max_extend", C.c_uint32), ("band", C.c_uint32), ("mismatch", C.c_uint32), ("indel", C.c_uint32)]


class SpeEnd(C.Structure):
    _fields_ = [("read_chars", C.c_uint32), ("text_chars", C.c_uint32), ("score", C.c_int32), ("edits", C.c_uint32)]


class SpeExtendStats(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("aligned_reads", C.c_uint64), ("gaps", C.c_uint64), ("filled_gaps", C.c_uint64),
                ("cells", C.c_uint64), ("entries", C.c_uint64), ("path_words", C.c_uint64), ("ends", C.c_uint64),
                ("extended_ends", C.c_uint64), ("band_cells", C.c_uint64), ("clipped", C.c_uint64), ("error", C.c_uint32),
                ("overflow", C.c_uint32), ("kernel_ms", C.c_float), ("step_ms", C.c_float * 6), ("reserved", C.c_uint32)]


def _spe() -> C.CDLL:
    """The library with the spe_* argtypes set (on first use)."""
    global _SPE_READY
    L = lib()
    if not hasattr(L, "spe_extend_begin"):
        raise SpxError(f"{LIB_PATH} has no extend kernels (spe_extend_begin): there is no CPU fallback")
    if not _SPE_READY:
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.spe_extend_device.argtypes = [vp, vp, vp, vp, vp, u64, vp, vp, C.POINTER(SpaParams), C.POINTER(SpeParams), u64, u64, vp, vp,
                                        vp, vp, vp]
        L.spe_extend_begin.argtypes = [vp, i32, u32, u32, vp, vp, u64, u64, i32, C.POINTER(SpcParams), C.POINTER(SpaParams),
                                       C.POINTER(SpeParams), vp, vp, vp, vp, C.POINTER(u64)]
        L.spe_extend_fetch.argtypes = [vp, vp, vp]
        L.spe_last_extend_stats.argtypes = [vp, C.POINTER(SpeExtendStats)]
        _SPE_READY = True
    return L


# ---- the mappings (include/spumoni_map.h) -------------------------------------------------------------------------
MAP_EXPORTS = ["spn_set_sequences", "spn_map_device", "spn_map_begin", "spn_map_fetch", "spn_last_map_stats"]
_SPN_READY = False


class SpnMapStats(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("mapped", C.c_uint64), ("cut_reads", C.c_uint64), ("reverse_reads", C.c_uint64),
                ("entries_in", C.c_uint64), ("entries_out", C.c_uint64), ("cut_chars", C.c_uint64), ("error", C.c_uint32),
                ("overflow", C.c_uint32), ("kernel_ms", C.c_float), ("step_ms", C.c_float * 2), ("reserved", C.c_uint32)]


def _spn() -> C.CDLL:
    """The library with the spn_* argtypes set (on first use)."""
    global _SPN_READY
    L = lib()
    if not hasattr(L, "spn_map_begin"):
        raise SpxError(f"{LIB_PATH} has no map kernels (spn_map_begin): there is no CPU fallback")
    if not _SPN_READY:
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.spn_set_sequences.argtypes = [vp, vp, u64, u32]
        L.spn_map_device.argtypes = [vp, vp, vp, vp, u64, vp, u64, u64, vp, vp, vp, vp]
        L.spn_map_begin.argtypes = [vp, i32, u32, u32, vp, vp, u64, u64, i32, C.POINTER(SpcParams), C.POINTER(SpaParams),
                                    C.POINTER(SpeParams), vp, vp, C.POINTER(u64)]
        L.spn_map_fetch.argtypes = [vp, vp, vp]
        L.spn_last_map_stats.argtypes = [vp, C.POINTER(SpnMapStats)]
        _SPN_READY = True
    return L


# ---- the coverage (include/spumoni_cover.h) ------------------------------------------------------------------------
COVER_EXPORTS = ["spd_cover_add_device", "spd_cover_finish_device", "spd_cover_runs_device", "spd_cover_reset", "spd_cover_add_batch",
                 "spd_cover_summary", "spd_cover_runs_begin", "spd_cover_runs_fetch", "spd_cover_depth", "spd_last_cover_stats"]
_SPD_READY = False


class SpdCoverStats(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("mapped", C.c_uint64), ("added", C.c_uint64), ("skipped", C.c_uint64),
                ("intervals", C.c_uint64), ("atomics", C.c_uint64), ("runs", C.c_uint64), ("error", C.c_uint32),
                ("overflow", C.c_uint32), ("kernel_ms", C.c_float), ("step_ms", C.c_float * 3)]


def _spd() -> C.CDLL:
    """The library with the spd_* argtypes set (on first use)."""
    global _SPD_READY
    L = _spn()
    if not hasattr(L, "spd_cover_add_batch"):
        raise SpxError(f"{LIB_PATH} has no coverage kernels (spd_cover_add_batch): there is no CPU fallback")
    if not _SPD_READY:
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.spd_cover_add_device.argtypes = [vp, vp, vp, vp, u64, u64, vp, vp, vp, vp]
        L.spd_cover_finish_device.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.spd_cover_runs_device.argtypes = [vp, vp, vp, u32, u64, vp, vp, vp]
        L.spd_cover_reset.argtypes = [vp]
        L.spd_cover_add_batch.argtypes = [vp, i32, u32, u32, vp, vp, u64, u64, i32, C.POINTER(SpcParams), C.POINTER(SpaParams),
                                          C.POINTER(SpeParams), vp]
        L.spd_cover_summary.argtypes = [vp, vp, u64]
        L.spd_cover_runs_begin.argtypes = [vp, u32, C.POINTER(u64)]
        L.spd_cover_runs_fetch.argtypes = [vp, vp]
        L.spd_cover_depth.argtypes = [vp, u64, u64, vp, vp]
        L.spd_last_cover_stats.argtypes = [vp, C.POINTER(SpdCoverStats)]
        _SPD_READY = True
    return L


# ---- the pileup and the calls (include/spumoni_call.h) ---------------------------------------------------------------
CALL_EXPORTS = ["spl_pileup_add_device", "spl_pileup_finish_device", "spl_calls_device", "spl_call_reset", "spl_call_add_batch",
                "spl_calls_begin", "spl_calls_fetch", "spl_pileup_counts", "spl_last_call_stats"]
_SPL_READY = False


class SplCallStats(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("mapped", C.c_uint64), ("added", C.c_uint64), ("skipped", C.c_uint64),
                ("x_columns", C.c_uint64), ("other_columns", C.c_uint64), ("insertions", C.c_uint64), ("deletions", C.c_uint64),
                ("atomics", C.c_uint64), ("calls", C.c_uint64), ("error", C.c_uint32), ("overflow", C.c_uint32),
                ("step_ms", C.c_float * 3), ("reserved", C.c_uint32)]


def _spl() -> C.CDLL:
    """The library with the spl_* argtypes set (on first use)."""
    global _SPL_READY
    L = _spd()
    if not hasattr(L, "spl_call_add_batch"):
        raise SpxError(f"{LIB_PATH} has no pileup kernels (spl_call_add_batch): there is no CPU fallback")
    if not _SPL_READY:
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.spl_pileup_add_device.argtypes = [vp, vp, vp, vp, u64, vp, vp, u64, u64, vp, vp, vp, vp, vp]
        L.spl_pileup_finish_device.argtypes = [vp, vp, vp, vp]
        L.spl_calls_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, u32, u32, u64, vp, vp, vp]
        L.spl_call_reset.argtypes = [vp]
        L.spl_call_add_batch.argtypes = [vp, i32, u32, u32, vp, vp, u64, u64, i32, C.POINTER(SpcParams), C.POINTER(SpaParams),
                                         C.POINTER(SpeParams), vp]
        L.spl_calls_begin.argtypes = [vp, u32, u32, u32, C.POINTER(u64)]
        L.spl_calls_fetch.argtypes = [vp, vp]
        L.spl_pileup_counts.argtypes = [vp, u64, u64, vp, vp, vp, vp]
        L.spl_last_call_stats.argtypes = [vp, C.POINTER(SplCallStats)]
        _SPL_READY = True
    return L


# ---- the consensus (include/spumoni_consensus.h) -------------------------------------------------------------------
CONSENSUS_EXPORTS = ["sps_consensus_device", "sps_consensus_begin", "sps_consensus_fetch", "sps_last_consensus_stats"]
_SPS_READY = False


class SpsParams(C.Structure):
    _fields_ = [("min_depth", C.c_uint32), ("min_alt", C.c_uint32), ("min_permille", C.c_uint32), ("line_width", C.c_uint32),
                ("mask", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class SpsConsensusStats(C.Structure):
    _fields_ = [("positions", C.c_uint64), ("kept", C.c_uint64), ("substituted", C.c_uint64), ("deleted", C.c_uint64),
                ("masked", C.c_uint64), ("ins_sites", C.c_uint64), ("letters", C.c_uint64), ("bytes", C.c_uint64),
                ("overflow", C.c_uint32), ("step_ms", C.c_float * 3)]


def _sps_params(min_depth, min_alt, min_permille, mask, line_width) -> SpsParams:
    """The parameters as the library takes them: the ranges are the library's to check, the fields' widths are checked here."""
    if isinstance(mask, (bytes, bytearray)):
        if len(mask) != 1:
            raise ValueError("mask must be one byte")
        mask = mask[0]
    vals = [int(min_depth), int(min_alt), int(min_permille), int(line_width)]
    if not (0 <= int(mask) <= 255) or any(v < 0 or v > 0xFFFFFFFF for v in vals):
        raise ValueError("min_depth, min_alt, min_permille and line_width must fit 32 bits, mask one byte")
    return SpsParams(vals[0], vals[1], vals[2], vals[3], int(mask))


def _sps() -> C.CDLL:
    """The library with the sps_* argtypes set (on first use)."""
    global _SPS_READY
    L = _spl()
    if not hasattr(L, "sps_consensus_begin"):
        raise SpxError(f"{LIB_PATH} has no consensus kernels (sps_consensus_begin): there is no CPU fallback")
    if not _SPS_READY:
        vp, u64 = C.c_void_p, C.c_uint64
        L.sps_consensus_device.argtypes = [vp, vp, vp, vp, vp, C.POINTER(SpsParams), u64, vp, vp, vp, vp]
        L.sps_consensus_begin.argtypes = [vp, C.POINTER(SpsParams), C.POINTER(u64)]
        L.sps_consensus_fetch.argtypes = [vp, vp, vp]
        L.sps_last_consensus_stats.argtypes = [vp, C.POINTER(SpsConsensusStats)]
        _SPS_READY = True
    return L


# ---- the index builder (include/spumoni_build.h) -------------------------------------------------------------------
_SPB_READY = False


def _spb() -> C.CDLL:
    """The library with the spb_* argtypes set (on first use: a library without the builder still loads for queries)."""
    global _SPB_READY
    L = lib()
    if not hasattr(L, "spb_build_from_text"):
        raise SpxError(f"{LIB_PATH} has no index builder (spb_build_from_text): there is no CPU fallback for the HIP path")
    if not _SPB_READY:
        vp, u64 = C.c_void_p, C.c_uint64
        L.spb_build_from_text.restype = vp
        L.spb_build_from_text.argtypes = [vp, u64, vp, C.c_uint32, C.c_int, C.c_int]
        L.spb_build_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        L.spb_build_copy.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
        L.spb_build_free.argtypes = [vp]
        _SPB_READY = True
    return L


def build_raw(text, doc_lengths=None, with_samples: bool = True, device: int = 0):
    """The run-length BWT, thresholds and SA samples of `text` (bytes >= 2, no terminator) built on the device:
    a synth.RawIndex of CPU tensors, field for field what synth.index_from_text(text, doc_lengths, with_samples) gives
    (document ids only when doc_lengths is given and with_samples)."""
    import torch

    from . import synth

    if isinstance(text, torch.Tensor):
        t = text.detach().to("cpu", torch.uint8).contiguous().numpy()
    else:
        t = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else
                                 np.asarray(text, dtype=np.uint8))
    L = _spb()
    dl = None if doc_lengths is None else np.ascontiguousarray(np.asarray(list(doc_lengths), dtype=np.uint64))
    h = L.spb_build_from_text(_np_ptr(t), t.size, _np_ptr(dl), 0 if dl is None else dl.size, 1 if with_samples else 0,
                              device)
    if not h:
        raise SpxError(L.spx_last_error().decode())
    try:
        n, r = C.c_uint64(), C.c_uint64()
        _check(L.spb_build_stats(h, C.byref(n), C.byref(r)))
        r = r.value
        heads = np.empty(r, dtype=np.uint8)
        lens, thr = np.empty(r, dtype=np.int64), np.empty(r, dtype=np.int64)
        ssa = esa = ds = de = None
        if with_samples:
            ssa, esa = np.empty(r, dtype=np.int64), np.empty(r, dtype=np.int64)
            if dl is not None:
                ds, de = np.empty(r, dtype=np.int64), np.empty(r, dtype=np.int64)
        _check(L.spb_build_copy(h, _np_ptr(heads), _np_ptr(lens), _np_ptr(thr), _np_ptr(ssa), _np_ptr(esa),
                                _np_ptr(ds), _np_ptr(de)))
    finally:
        L.spb_build_free(h)

    def tt(a):
        return None if a is None else torch.from_numpy(a)

    return synth.RawIndex(heads=tt(heads), lens=tt(lens), thr=tt(thr), n=n.value, ssa=tt(ssa), esa=tt(esa),
                          doc_start=tt(ds), doc_end=tt(de), text=torch.from_numpy(t.copy()))


# ---- reference text preparation (include/spumoni_reftext.h) -------------------------------------------------------
REFTEXT_EXPORTS = ["spr_text_from_fasta", "spr_text_stats", "spr_text_copy", "spr_text_names", "spr_text_free"]
_SPR_READY = False


def _spr() -> C.CDLL:
    """The library with the spr_* argtypes set (on first use)."""
    global _SPR_READY
    L = lib()
    if not hasattr(L, "spr_text_from_fasta"):
        raise SpxError(f"{LIB_PATH} has no text preparation (spr_text_from_fasta): there is no CPU fallback")
    if not _SPR_READY:
        vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        L.spr_text_from_fasta.restype = vp
        L.spr_text_from_fasta.argtypes = [vp, u64, vp, u32, C.c_int, C.c_int, u32, u32, u64, C.c_int]
        L.spr_text_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
        L.spr_text_copy.argtypes = [vp, vp, vp, vp, vp, vp]
        L.spr_text_names.argtypes = [vp, vp, vp, C.POINTER(u64)]
        L.spr_text_free.argtypes = [vp]
        _SPR_READY = True
    return L


def prepare_fasta(files, rev_comp: bool = True, digest_kind: int = 0, k: int = 4, w: int = 11, max_text: int = 0,
                  device: int = 0):
    """The text `spumoni build` indexes from FASTA file contents (a list of bytes, already inflated), prepared on the
    device: a dict with "text", "file_text_lengths", "fwd" (the sequences, case preserved, back to back), "seq_ends"
    and "seq_file" (numpy arrays), and "names" (a list of bytes: map.sequence_name of every sequence)."""
    data = np.frombuffer(b"".join(files), dtype=np.uint8)
    ends = np.ascontiguousarray(np.cumsum([len(f) for f in files]), dtype=np.uint64)
    L = _spr()
    h = L.spr_text_from_fasta(_np_ptr(data) if data.size else None, data.size, _np_ptr(ends), ends.size,
                              1 if rev_comp else 0, digest_kind, k, w, max_text, device)
    if not h:
        raise SpxError(L.spx_last_error().decode())
    try:
        nt, ns, nf = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(L.spr_text_stats(h, C.byref(nt), C.byref(ns), C.byref(nf)))
        out = {"text": np.empty(nt.value, dtype=np.uint8), "file_text_lengths": np.empty(ends.size, dtype=np.uint64),
               "fwd": np.empty(nf.value, dtype=np.uint8), "seq_ends": np.empty(ns.value, dtype=np.uint64),
               "seq_file": np.empty(ns.value, dtype=np.uint32)}
        _check(L.spr_text_copy(h, *[_np_ptr(out[x]) for x in ("text", "file_text_lengths", "fwd", "seq_ends",
                                                                "seq_file")]))
        nb = C.c_uint64()
        _check(L.spr_text_names(h, None, None, C.byref(nb)))
        names, name_ends = np.empty(nb.value, dtype=np.uint8), np.empty(ns.value, dtype=np.uint64)
        _check(L.spr_text_names(h, _np_ptr(names), _np_ptr(name_ends), None))
        cuts = [0] + name_ends.tolist()
        out["names"] = [names[a:b].tobytes() for a, b in zip(cuts, cuts[1:])]
    finally:
        L.spr_text_free(h)
    return out
