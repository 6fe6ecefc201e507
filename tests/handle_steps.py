"""The catalogue of steps that tests/test_gpu_used_handle.py and tests/test_used_handle_cpu.py run on long-lived handles.

A step is one call of one entry point of the C-ABI on one batch, together with what it must return.  The expectation comes
from the oracle alone (oracle.OracleIndex.pml / ms, oracle.classify, oracle.digest_batch) and, for the votes, the matches and
the text, from votes_reference, mems_reference and the formatter of tests/test_gpu_text.py (tests/text_lines.py) applied to the oracle's arrays (or
to crafted arrays where a pair needs values no index gives: all ids distinct, every position a start).  Nothing the library
returns ever enters an expectation.  build() computes all of it once; it needs no device and no library.

A step runs in three parts so that two steps can be enqueued back to back on one handle:
    job = step.prepare()        buffers, uploads, fences armed (device forms: on torch's current stream)
    job.launch(ix, stream)      options + the library's calls, nothing else: no synchronisation, no allocation
    got = job.collect()         waits for the step's stream, reads back, checks the fences -> dict of numpy arrays
and step.check_path(ix) asserts what the library reports about the path the call took; it is valid only while the step's
call is the handle's most recent one.  compare(name, got, step.want) holds every value of every key to the expectation.

Every device-form output sits in a DeviceFence: FENCE bytes of PATTERN on either side of the values (the values in front
of offs[0] count as fence too), the values themselves set to the pattern as well, so what is not written fails like what
is written wrongly.  Host forms get their class records in a HostFence.

Every step of the catalogue has a dirtier: the call that, run just before it on the same handle, leaves more bytes and
other content in exactly the scratch the step uses (the table below says which and why).  Catalogue.check_claims() asserts
from the expected
arrays that the two differ in the way the pair needs -- a pair cannot turn harmless unnoticed.  step.resize(k) is the same
step on the batch's first k reads (the expectation is a slice: every value depends on its own read only).
"""
import os

import numpy as np
import torch

from spumoni_amd import capi, synth
from spumoni_amd.align import ALIGN_DTYPE, GAP_DTYPE, UNALIGNED, UNFILLED, AlignParams, align_reference
from spumoni_amd.chain import CHAIN_DTYPE, NO_DOC, chain_reference
from spumoni_amd.cigar import OP_D, OP_EQ, OP_I, cigar_reference
from spumoni_amd.docvote import VOTE_DTYPE, votes_reference
from spumoni_amd.mems import MATCH_DTYPE, mems_reference
from spumoni_amd.place import PLACEMENT_DTYPE, UNPLACED, place_reference
from tests import cases
from tests import grid_cases as gc
from tests.test_gpu_align import Batch
from tests.test_gpu_place import _to_device
from tests.text_lines import _expect, _fill

PML, MS = capi.SPX_MODE_PML, capi.SPX_MODE_MS
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
N = ord("N")
FENCE = 64  # bytes of PATTERN on either side
PATTERN = 0xA5
K, W = 4, 11  # the digestion's (k, w)
N_STEPS = 61  # steps of the catalogue (the tests are parametrised over it before anything is built; build() must give as many)
OPTION_DEFAULTS = {"chunk_mode": 0, "chunk_shift": 0, "chunk_len": 0, "digest_kernel": 0, "digest_parked": 0}

# step family                          dirtier                                        the scratch they share; what the dirtier leaves there
# plain PML walk                       reads of a letter the index lacks              C_LEN_BITS (state-machine walk), S_LEN / S_DOC / S_CLASS: every character
#                                                                                     resets, all bits set, all lengths 0, against long matches with few resets
# chunked walk, nothing falls back     long reads in chunks of 32 that DO fall back   C_DESC .. C_FAIL of chunk_scr[]: open seams, read_fail set (asserted:
#                                                                                     fallback_reads > 0 when the dirtier is the handle's last call)
# chunked walk, reads fall back        the same reads with ten times the mismatches,  the same: descriptors, flags and seam records of chunks whose seams
#                                      other chunk size                               all closed
# chunked / plain walk of long         ragged random reads at another chunk size      the same: many short chunks of reads that reset all the time
# exact matches (period-20 text)
# MS + lengths on short reads          one MS read of 70 000 characters               S_LEN, S_PTR, S_CLASS: a read of 65536 values or more stores unstaged, 32 bit
# digestion of clean ACGT              reads that are half N, another forced kernel   digest_scr[]: `bad` flags and counts of reads the wavefront kernel redid
# digest + query, parked               the same call, concatenated, on longer reads   digest_scr[], S_SEQ: concatenated reads (and the reverse)
# votes on few documents               all ids of a long read distinct, 32 bit        vote_scr[] V_TILES / V_TABLE: full tile tables
# matches, one start per read          every position a start                         mems_scr[] M_BITS / M_PREFIX: a bitmap of ones
# text of 1-digit values               MS pointers of 13 digits, four times the size  S_LINE_BYTES .. S_TEXT: longer lines
# class records, every bin below       threshold 0 on more reads                      S_CLASS: every bin above
# placements, 16 bit, short reads      32 bit with reads above 2 048 values           the product's counters; the 16-lane path behind the whole-wavefront one
# place_host                           place_host on a read of 70 000 characters      place_scr[], stage_scr[]: 32-bit values of six times the characters
# chains with f and pred, <= 16        reads of 5 000 anchors with ids                the counters; the ring of 64 before the groups of 16 lanes
# chain_host                           chain_host at min_length 1 on noisier reads    M_OUT, M_MOFFS of mems_scr[], H_OUT of chain_scr[], stage_scr[]: four times the matches
# align_device, table in caller        every gap wave-sized and filled, four times    align_scr[] L_DESC, L_LIST: descriptors and a list full of other offsets
# buffers / in the scratch, capacity   the gaps                                       L_GAPS: the places of the read that does not fit must not keep the
# one short inside a middle read                                                      dirtier's sides
# align_host                           align_host on reads with ten times the edits   L_CHAINS, L_PRED, L_OUT
# cigar_device at max_fill 512,        max_fill 4 096, 20 traces in device memory     cigar_scr[] TB_TRACE at another stride, TB_PATH full of codes 2 and 3,
# nearly all '='; op_capacity short    (16 wavefronts), lopsided and empty-sided      TB_LIST filled from both ends; TB_OCNT, TB_POFFS: the read that does not
# of the last read                     gaps                                           fit comes back unaligned
# cigar_host                           cigar_host on reads with ten times the edits   TB_OOFFS, TB_OPS between spg_cigar_begin and spg_cigar_fetch


class Mismatch(AssertionError):
    pass


# ---- fences ----------------------------------------------------------------------------------------------------------
def check_fence(raw_bytes, lo, hi, what):
    """raw_bytes: the whole buffer as uint8; [lo, hi) are the values, every other byte must still be PATTERN"""
    outside = np.ones(raw_bytes.size, dtype=bool)
    outside[lo:hi] = False
    hit = np.flatnonzero(outside & (raw_bytes != PATTERN))
    if hit.size:
        at = int(hit[0])
        where = f"{lo - at} bytes in front of the values" if at < lo else f"{at - hi} bytes behind them"
        raise Mismatch(f"{what}: {hit.size} fence bytes written, the first {where}")


class DeviceFence:
    """`n` values of a torch dtype in device memory between two fences; .t is what the library gets (16-byte aligned).
    front: values in front of the first read's (offs[0] != 0) -- fence as well."""

    def __init__(self, what, n, dtype, front=0):
        self.what, self.n, self.front = what, int(n), int(front)
        self.item = torch.empty(0, dtype=dtype).element_size()
        body = max(16, (self.n * self.item + 15) // 16 * 16)
        self.buf = torch.empty(FENCE + body + FENCE, dtype=torch.uint8, device="cuda")
        self.buf.fill_(PATTERN)
        self.t = self.buf[FENCE: FENCE + body].view(dtype)
        assert self.t.data_ptr() % 16 == 0

    def values(self, np_dtype):
        h = self.buf.cpu().numpy()
        lo, hi = FENCE + self.front * self.item, FENCE + self.n * self.item
        check_fence(h, lo, hi, self.what)
        return h[lo:hi].copy().view(np_dtype)


class HostFence:
    """the same in host memory, for the class records of the host forms (capi: class_out)"""

    def __init__(self, what, nreads):
        self.what, self.n = what, int(nreads)
        self.buf = np.full(FENCE + self.n * 16 + FENCE, PATTERN, dtype=np.uint8)
        self.out = self.buf[FENCE: FENCE + self.n * 16].view(capi.CLASS_DTYPE)

    def values(self):
        check_fence(self.buf, FENCE, FENCE + self.n * 16, self.what)
        return self.out.copy()


# ---- the comparator ----------------------------------------------------------------------------------------------------
def compare(name, got, want):
    """every value of every key; raises Mismatch naming the step, the key and the first value that differs"""
    if set(got) != set(want):
        raise Mismatch(f"{name}: keys {sorted(got)} instead of {sorted(want)}")
    for key, w in want.items():
        g = got[key]
        if isinstance(w, bytes):
            if g != w:
                at = next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
                raise Mismatch(f"{name}: {key}: {len(g)} bytes against {len(w)}, the first difference at byte {at}: "
                               f"{g[max(at - 20, 0): at + 20]!r} against {w[max(at - 20, 0): at + 20]!r}")
            continue
        g, w = np.asarray(g), np.asarray(w)
        if g.shape != w.shape:
            raise Mismatch(f"{name}: {key}: shape {g.shape} instead of {w.shape}")
        for f in (w.dtype.names or (None,)):
            a, b = (g, w) if f is None else (g[f], w[f])
            bad = np.flatnonzero(a.astype(np.uint64) != b.astype(np.uint64))
            if bad.size:
                i = int(bad[0])
                raise Mismatch(f"{name}: {key}{'' if f is None else '.' + f}: {bad.size} of {a.size} values differ, the first at "
                               f"{i}: {int(a[i])} instead of {int(b[i])}")


# ---- steps ---------------------------------------------------------------------------------------------------------------
def set_options(ix, opts):
    for key, dflt in OPTION_DEFAULTS.items():
        ix.set_option(key, int(opts.get(key, dflt)))


class Job:
    def __init__(self, launch, collect):
        self._launch, self._collect, self.stream = launch, collect, None

    def launch(self, ix, stream=None):
        self.stream = stream
        self._launch(ix, stream)

    def collect(self):
        if self.stream is not None:
            self.stream.synchronize()
        return self._collect()


class Step:
    """name; index: which of the catalogue's indexes its handle is made from; form: "host" | "device"; chars: the
    characters (values) of its batch; want: the expectation; dirtier: name of its dirtier in Catalogue.dirtiers"""

    def __init__(self, family, nreads):
        self.family, self.nreads = family, nreads
        self.name, self.index, self.form, self.dirtier = family.name, family.index, family.form, family.dirtier
        self.chars, self.want = family.expect(nreads)

    def prepare(self):
        return self.family.prepare(self.nreads)

    def check_path(self, ix, fake=False):
        if not fake:
            self.family.path(ix, self)

    def resize(self, k):
        return Step(self.family, k)

    def sizes(self):
        """(large, small, medium) read counts of the grow-and-shrink order"""
        n = self.family.nreads
        return n, max(1, n // 8), max(2, n // 2)


class Family:
    """One entry point on one batch: expect(k) -> (chars, want) and prepare(k) -> Job for the batch's first k reads."""
    form = "host"
    dirtier = None

    def __init__(self, name, index, nreads):
        self.name, self.index, self.nreads = name, index, int(nreads)

    def path(self, ix, step):
        pass

    def step(self):
        return Step(self, self.nreads)


def _class_records(oracle_mod, lengths, offs, cls):
    _, a, b, s = oracle_mod.classify(lengths, offs, cls[0], cls[1])
    rec = np.zeros(len(offs) - 1, dtype=capi.CLASS_DTYPE)
    rec["above"], rec["below"], rec["sum_max"] = a, b, s
    return rec


def _upload(a, np_dtype):
    """an unsigned array on the device (torch has the signed types of the same width)"""
    signed = {np.uint16: np.int16, np.uint32: np.int32, np.uint64: np.int64}[np_dtype]
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np_dtype).view(signed).copy()).cuda()


class Query(Family):
    """spx_query_batch[16] / spx_query_batch_device[16].  full: the oracle's arrays of the whole batch."""

    def __init__(self, cat, name, index, batch, mode, form="host", bits=32, lengths=True, docs=False, cls=None, opts=None, front=0,
                 chunk=0, fallback=None, compact=1):
        super().__init__(name, index, len(batch[1]) - 1)
        self.cat, self.batch, self.mode, self.form, self.bits = cat, batch, mode, form, bits
        self.lengths, self.docs, self.cls, self.opts, self.front = lengths, docs, cls, dict(opts or {}), front
        self.chunk, self.fallback, self.compact = chunk, fallback, compact
        self.full = cat.oracle_values(index, batch, mode)
        if bits == 16:
            assert int(np.diff(batch[1]).max()) < 65536 and ("docs" not in self.full or int(self.full["docs"].max(initial=0)) < 65536)

    def expect(self, k):
        offs = self.batch[1][: k + 1]
        tot = int(offs[-1])
        want = {}
        if self.lengths:
            want["lengths"] = self.full["lengths"][:tot]
        if self.mode == MS:
            want["pointers"] = self.full["pointers"][:tot]
        if self.docs:
            want["docs"] = self.full["docs"][:tot]
        if self.cls:
            want["class"] = _class_records(self.cat.oracle, self.full["lengths"][:tot], offs, self.cls)
        return tot, want

    def prepare(self, k):
        seqs, offs = self.batch[0], self.batch[1][: k + 1]
        tot = int(offs[-1])
        seqs = seqs[:tot]
        cls = self.cls or (0, 0)
        if self.form == "host":
            hf = HostFence(self.name + " class", k) if self.cls else None
            res = {}

            def launch(ix, stream):
                set_options(ix, self.opts)
                res.update(ix.query_host(self.mode, seqs, offs, want_lengths=self.lengths, want_docs=self.docs, classify=self.cls,
                                         bits=self.bits, class_out=hf.out if hf else None))

            def collect():
                if hf:
                    res["class"] = hf.values()
                return res

            return Job(launch, collect)
        f0 = self.front
        vt, nt = (torch.int16, np.uint16) if self.bits == 16 else (torch.int32, np.uint32)
        d_seqs = torch.zeros(f0 + (tot + 3) // 4 * 4 + 64, dtype=torch.uint8, device="cuda")
        d_seqs[f0: f0 + tot] = torch.from_numpy(seqs.copy()).cuda()
        d_offs = torch.from_numpy(offs.astype(np.int64) + f0).cuda()
        fl = DeviceFence(self.name + " lengths", f0 + tot, vt, f0) if self.lengths else None
        fp = DeviceFence(self.name + " pointers", f0 + tot, torch.int64, f0) if self.mode == MS else None
        fd = DeviceFence(self.name + " docs", f0 + tot, vt, f0) if self.docs else None
        fc = DeviceFence(self.name + " class", 2 * k, torch.int64) if self.cls else None

        def launch(ix, stream):
            set_options(ix, self.opts)
            ix.query_device(self.mode, d_seqs, d_offs, tot, d_lengths=fl.t if fl else None, d_pointers=fp.t if fp else None,
                            d_docs=fd.t if fd else None, d_class=fc.t if fc else None, bin_width=cls[0], max_value_thr=cls[1],
                            stream=stream, narrow=self.bits == 16)

        def collect():
            got = {}
            if fl:
                got["lengths"] = fl.values(nt)
            if fp:
                got["pointers"] = fp.values(np.uint64)
            if fd:
                got["docs"] = fd.values(nt)
            if fc:
                got["class"] = fc.values(np.uint64).view(capi.CLASS_DTYPE).reshape(-1)
            return got

        return Job(launch, collect)

    def path(self, ix, step):
        assert ix.describe()["compact_rows"] == self.compact, self.name
        cs = ix.last_chunk_stats()
        assert cs["chunk_len"] == self.chunk, (self.name, cs)
        if self.fallback is True and step.nreads == self.nreads:
            assert cs["fallback_reads"] > 0, (self.name, cs)
        if self.fallback is False:
            assert cs["fallback_reads"] == 0, (self.name, cs)


class Digest(Family):
    """spx_digest_batch with a forced kernel"""

    def __init__(self, cat, name, index, batch, kind, kernel):
        super().__init__(name, index, len(batch[1]) - 1)
        self.batch, self.kind, self.kernel = batch, kind, kernel
        self.full = cat.oracle.digest_batch(kind, K, W, batch[0], batch[1])

    def expect(self, k):
        doffs = self.full[1][: k + 1]
        return int(self.batch[1][k]), {"digested": self.full[0][: int(doffs[-1])], "offsets": doffs}

    def prepare(self, k):
        offs = self.batch[1][: k + 1]
        seqs = self.batch[0][: int(offs[-1])]
        res = {}

        def launch(ix, stream):
            set_options(ix, {"digest_kernel": self.kernel})
            res["digested"], res["offsets"] = ix.digest_host(self.kind, K, W, seqs, offs)

        return Job(launch, lambda: res)


class DigestQuery(Family):
    """spx_digest_query_batch / _device[16]: PML lengths + document ids + class records at the digested offsets"""
    CLS = (5, 2)

    def __init__(self, cat, name, index, batch, kind, form="host", bits=32, parked=0):
        super().__init__(name, index, len(batch[1]) - 1)
        self.cat, self.batch, self.kind, self.form, self.bits, self.parked = cat, batch, kind, form, bits, parked
        dseqs, doffs = cat.oracle.digest_batch(kind, K, W, batch[0], batch[1])
        self.doffs = doffs
        self.full = cat.oracle_values(index, (dseqs, doffs.astype(np.int64)), PML)

    def expect(self, k):
        doffs = self.doffs[: k + 1]
        dt = int(doffs[-1])
        want = {"offsets": doffs, "lengths": self.full["lengths"][:dt], "docs": self.full["docs"][:dt],
                "class": _class_records(self.cat.oracle, self.full["lengths"][:dt], doffs, self.CLS)}
        return int(self.batch[1][k]), want

    def prepare(self, k):
        offs = self.batch[1][: k + 1].astype(np.uint64)
        tot = int(offs[-1])
        seqs = self.batch[0][:tot]
        dt = int(self.doffs[k])
        if self.form == "host":
            hf = HostFence(self.name + " class", k)
            res = {}

            def launch(ix, stream):
                set_options(ix, {"digest_parked": self.parked})
                res.update(ix.digest_query_host(PML, self.kind, K, W, seqs, offs, want_docs=True, classify=self.CLS, class_out=hf.out))

            def collect():
                res["class"] = hf.values()
                return res

            return Job(launch, collect)
        vt, nt = (torch.int16, np.uint16) if self.bits == 16 else (torch.int32, np.uint32)
        d_seqs = torch.zeros((tot + 15) // 16 * 16 + 64, dtype=torch.uint8, device="cuda")
        d_seqs[:tot] = torch.from_numpy(seqs.copy()).cuda()
        d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
        cap = int(capi.lib().spx_digest_capacity(self.kind, K, tot))
        fo = DeviceFence(self.name + " offsets", k + 1, torch.int64)
        work = (torch.zeros(cap + 64, dtype=torch.uint8, device="cuda"), fo.t)
        # (the outputs are sized for total_chars entries, as the header asks; the digested reads fill the first `dt`)
        fl = DeviceFence(self.name + " lengths", tot, vt)
        fd = DeviceFence(self.name + " docs", tot, vt)
        fc = DeviceFence(self.name + " class", 2 * k, torch.int64)

        def launch(ix, stream):
            set_options(ix, {"digest_parked": self.parked})
            ix.digest_query_device(PML, self.kind, K, W, d_seqs, d_offs, tot, d_lengths=fl.t, d_docs=fd.t, d_class=fc.t,
                                   bin_width=self.CLS[0], max_value_thr=self.CLS[1], stream=stream, work=work)

        def collect():
            return {"offsets": fo.values(np.uint64), "lengths": fl.values(nt)[:dt], "docs": fd.values(nt)[:dt],
                    "class": fc.values(np.uint64).view(capi.CLASS_DTYPE).reshape(-1)}

        return Job(launch, collect)


class Text(Family):
    """spx_query_text_begin / _fetch: the streams with the ids filled into the gaps, against the formatter over the oracle's
    arrays.  reserve: a spx_query_text_reserve hint (chars, reads) in front of the call."""
    KEYS = ("lengths", "pointers", "docs")

    def __init__(self, cat, name, index, batch, mode, streams, gaps=True, cls=None, digest=None, reserve=None):
        super().__init__(name, index, len(batch[1]) - 1)
        self.cat, self.batch, self.mode, self.streams, self.gaps, self.cls = cat, batch, mode, streams, gaps, cls
        self.digest, self.reserve = digest, reserve
        if digest:
            dseqs, doffs = cat.oracle.digest_batch(digest[0], K, W, batch[0], batch[1])
            self.voffs = doffs.astype(np.int64)
            self.full = cat.oracle_values(index, (dseqs, self.voffs), mode)
        else:
            self.voffs = np.asarray(batch[1], dtype=np.int64)
            self.full = cat.oracle_values(index, batch, mode)
        self.ids = [b"r%d%s" % (q, b" x" * (q % 3)) for q in range(self.nreads)]

    def expect(self, k):
        voffs = self.voffs[: k + 1]
        ids = self.ids[:k] if self.gaps else [None] * k
        want = {}
        for i, key in enumerate(self.KEYS):
            if self.streams & (1 << i):
                vals = self.full[key]
                if self.gaps:
                    want[key] = _expect(vals, voffs, ids)
                else:
                    want[key] = b"".join(b"".join(b"%d " % int(v) for v in vals[voffs[q]: voffs[q + 1]]) + b"\n" for q in range(k))
        if self.cls:
            want["class"] = _class_records(self.cat.oracle, self.full["lengths"][: int(voffs[-1])], voffs, self.cls)
        return int(self.batch[1][k]), want

    def prepare(self, k):
        offs = self.batch[1][: k + 1]
        seqs = self.batch[0][: int(offs[-1])]
        ids = self.ids[:k]
        gap = np.array([len(i) + 2 for i in ids], dtype=np.uint32) if self.gaps else None
        hf = HostFence(self.name + " class", k) if self.cls else None
        dg = (self.digest[0], K, W) if self.digest else (0, 0, 0)
        res = {}

        def launch(ix, stream):
            set_options(ix, {})
            if self.reserve:
                ix.reserve_text(self.mode, self.reserve[0], self.reserve[1], self.streams, classify=bool(self.cls), digest=dg[:2])
            got = ix.query_text(self.mode, seqs, offs, gap, self.streams, digest=dg, classify=self.cls,
                                class_out=hf.out if hf else None)
            for i, key in enumerate(self.KEYS):
                if self.streams & (1 << i):
                    res[key] = _fill(got["text"][i], got["line_start"][i], ids) if self.gaps else got["text"][i]
                else:
                    assert got["text"][i] is None

        def collect():
            if hf:
                res["class"] = hf.values()
            return res

        return Job(launch, collect)

    def path(self, ix, step):
        if step.nreads:
            assert all(len(v) > 0 for key, v in step.want.items() if key != "class"), self.name  # non-empty streams


def _vote_table(rec):
    return np.stack([rec[f] for f in VOTE_DTYPE.names], axis=1).astype(np.uint32).reshape(-1)


class Votes(Family):
    """spv_votes_device over uploaded arrays (L, D: the oracle's, or crafted), or -- chained -- over what a
    spx_query_batch_device16 call on the same batch wrote on the step's stream a moment ago; spv_assign_batch (form host)."""

    def __init__(self, cat, name, index, offs, L, D, bits, min_length, form="device", batch=None, paths=True):
        super().__init__(name, index, len(offs) - 1)
        self.offs, self.L, self.D, self.bits, self.min_length, self.form = np.asarray(offs, dtype=np.int64), L, D, bits, min_length, form
        self.batch, self.paths = batch, paths
        assert int(np.max(L, initial=0)) < (1 << bits) and int(np.max(D, initial=0)) < (1 << bits)

    def expect(self, k):
        offs = self.offs[: k + 1]
        rec = votes_reference(self.L, self.D, offs, self.min_length)
        if self.form == "host":
            return int(offs[-1]), {"records": rec, "values": np.diff(offs).astype(np.uint64)}
        return int(offs[-1]), {"votes": _vote_table(rec)}

    def prepare(self, k):
        offs = self.offs[: k + 1]
        tot = int(offs[-1])
        if self.form == "host":
            seqs = self.batch[0][:tot]
            res = {}

            def launch(ix, stream):
                set_options(ix, {"chunk_mode": 1})
                got = ix.assign_host(PML, seqs, offs.astype(np.uint64), self.min_length)
                res["records"] = got[list(VOTE_DTYPE.names)]
                res["values"] = got["values"]

            return Job(launch, lambda: res)
        vt, nt = (torch.int16, np.uint16) if self.bits == 16 else (torch.int32, np.uint32)
        d_offs = torch.from_numpy(offs.copy()).cuda()
        fo = DeviceFence(self.name + " votes", 4 * k, torch.int32)
        if self.batch is None:
            d_L, d_D = _upload(self.L[:tot], nt), _upload(self.D[:tot], nt)
            if d_L.numel() == 0:
                d_L, d_D = torch.zeros(8, dtype=vt, device="cuda"), torch.zeros(8, dtype=vt, device="cuda")

            def launch(ix, stream):
                ix.votes_device(d_L[:tot], d_D[:tot], d_offs, self.min_length, d_out=fo.t, stream=stream)
        else:
            seqs = self.batch[0][:tot]
            d_seqs = capi.pad_seqs(torch.from_numpy(seqs.copy()).cuda())
            fl = DeviceFence(self.name + " lengths", tot, vt)
            fd = DeviceFence(self.name + " docs", tot, vt)

            def launch(ix, stream):
                set_options(ix, {"chunk_mode": 1})
                # one stream: the votes read what the query wrote, the caller's own data, in stream order
                ix.query_device(PML, d_seqs, d_offs, tot, d_lengths=fl.t, d_docs=fd.t, stream=stream, narrow=self.bits == 16)
                ix.votes_device(fl.t[:tot], fd.t[:tot], d_offs, self.min_length, d_out=fo.t, stream=stream)

        return Job(launch, lambda: {"votes": fo.values(np.uint32)})

    def path(self, ix, step):
        st = ix.votes_stats()
        lens = np.diff(step.family.offs[: step.nreads + 1])
        assert st["reads_short"] + st["reads_medium"] + st["reads_long"] + st["reads_empty"] == lens.size, (self.name, st)
        assert st["reads_empty"] == int((lens == 0).sum()), (self.name, st)
        if self.paths and step.nreads == self.nreads:
            assert st["reads_short"] > 0 and st["reads_medium"] > 0 and st["reads_long"] > 0, (self.name, st)


class Mems(Family):
    """spm_mems_device over uploaded arrays (the oracle's MS lengths, pointers, document ids, or crafted ones), one call with
    the capacity the reference gives; spm_mems_begin / _fetch (form host)."""

    def __init__(self, cat, name, index, offs, L, P, D, bits, min_length, form="device", batch=None):
        super().__init__(name, index, len(offs) - 1)
        self.offs, self.L, self.P, self.D = np.asarray(offs, dtype=np.int64), L, P, D
        self.bits, self.min_length, self.form, self.batch = bits, min_length, form, batch
        assert int(np.max(L, initial=0)) < (1 << bits) and (D is None or int(np.max(D, initial=0)) < (1 << bits))

    def expect(self, k):
        offs = self.offs[: k + 1]
        ref = mems_reference(self.L, self.P, offs, self.min_length, self.D)
        want = {"match_offsets": ref[0], "records": ref[1]}
        if self.D is not None:
            want["docs"] = ref[2]
        if self.form == "host":
            want["values"] = np.diff(offs).astype(np.uint64)
        return int(offs[-1]), want

    def prepare(self, k):
        offs = self.offs[: k + 1]
        tot = int(offs[-1])
        if self.form == "host":
            seqs = self.batch[0][:tot]
            res = {}

            def launch(ix, stream):
                set_options(ix, {})
                got = ix.mems_host(seqs, offs.astype(np.uint64), self.min_length, want_docs=self.D is not None)
                res["match_offsets"], res["records"], res["values"] = got[0], got[1], got[-1]
                if self.D is not None:
                    res["docs"] = got[2]

            return Job(launch, lambda: res)
        nt = np.uint16 if self.bits == 16 else np.uint32
        n = int(mems_reference(self.L, self.P, offs, self.min_length)[1].size)
        pad = 8  # (uploaded arrays are never empty)
        zeros = np.zeros(pad, dtype=np.int64)
        d_L = _upload(np.r_[self.L[:tot], zeros], nt)
        d_P = _upload(np.r_[np.asarray(self.P[:tot], dtype=np.uint64), zeros.astype(np.uint64)], np.uint64)
        d_D = None if self.D is None else _upload(np.r_[self.D[:tot], zeros], nt)
        d_offs = torch.from_numpy(offs.copy()).cuda()
        fm = DeviceFence(self.name + " match offsets", k + 1, torch.int64)
        fr = DeviceFence(self.name + " records", 4 * n, torch.int32)
        fdoc = DeviceFence(self.name + " docs", n, torch.int32) if self.D is not None else None

        def launch(ix, stream):
            ix.mems_device(d_L[:tot], d_P[:tot], d_offs, self.min_length, d_docs=None if d_D is None else d_D[:tot], capacity=n,
                           d_match_offsets=fm.t, d_out=fr.t, d_out_docs=fdoc.t if fdoc else None, stream=stream)

        def collect():
            got = {"match_offsets": fm.values(np.uint64), "records": fr.values(np.uint32).view(MATCH_DTYPE).reshape(-1)}
            if fdoc:
                got["docs"] = fdoc.values(np.uint32)
            return got

        return Job(launch, collect)

    def path(self, ix, step):
        st = ix.mems_stats()
        n = step.want["records"].size
        assert st["matches"] == n and st["written"] == n and st["values"] == step.chars, (self.name, st, n)


class Product(Family):
    """What Place, Chain, Align and Cigar share: expect(k) computed once per k, the oracle's MS arrays of a host form's batch
    and the matches mems_reference makes of them (the library's own matches never enter an expectation)."""

    def __init__(self, cat, name, index, nreads, form, batch=None, min_length=0):
        super().__init__(name, index, nreads)
        self.cat, self.form, self.batch, self.min_length = cat, form, batch, min_length
        self._memo, self.seen = {}, {}
        self.ms = cat.oracle_values(index, batch, MS) if form == "host" else None

    def text(self):
        return self.cat.indexes[self.index]["text"]

    def expect(self, k):
        if k not in self._memo:
            self._memo[k] = self.compute(k)
        return self._memo[k]

    def host_reads(self, k):
        offs = np.asarray(self.batch[1][: k + 1], dtype=np.uint64)
        return self.batch[0][: int(offs[-1])], offs

    def matches(self, k):
        """(match_offsets, records) of the batch's first k reads"""
        m = mems_reference(self.ms["lengths"], self.ms["pointers"], np.asarray(self.batch[1][: k + 1], dtype=np.int64), self.min_length)
        return m[0], m[1]

    def host_job(self, call, keys):
        res = {}

        def launch(ix, stream):
            set_options(ix, {})
            res.update(zip(keys, call(ix)))

        return Job(launch, lambda: res)


def _pattern_behind(fence_values, written, what):
    """the places of a fenced output that the capacity covers and the call must leave alone"""
    tail = fence_values[written:].view(np.uint8)
    if (tail != PATTERN).any():
        raise Mismatch(f"{what}: written behind the {written} values that fit")
    return fence_values[:written]


class Place(Product):
    """spp_place_device over uploaded arrays (crafted: the rule is one on the arrays and the text), spp_place_batch (form
    host) against place_reference over the oracle's MS lengths and pointers."""

    def __init__(self, cat, name, index, offs, R, L, P, D, bits, params, form="device", batch=None):
        super().__init__(cat, name, index, len(offs) - 1, form, batch)
        self.offs, self.R, self.L, self.P, self.D, self.bits, self.params = np.asarray(offs, dtype=np.int64), R, L, P, D, bits, params
        if form == "host":
            self.R, self.L, self.P = batch[0], self.ms["lengths"], self.ms["pointers"]
        assert int(np.max(self.L, initial=0)) < (1 << bits) and (D is None or int(np.max(D, initial=0)) < (1 << bits))

    def compute(self, k):
        offs = self.offs[: k + 1]
        want = {"records": place_reference(self.R, self.L, self.P, offs.astype(np.uint64), self.text(), *self.params, docs=self.D)}
        if self.form == "host":
            want["values"] = np.diff(offs).astype(np.uint64)
        return int(offs[-1] - offs[0]), want

    def prepare(self, k):
        if self.form == "host":
            seqs, offs = self.host_reads(k)
            return self.host_job(lambda ix: ix.place_host(seqs, offs, *self.params), ("records", "values"))
        offs = self.offs[: k + 1]
        hi = int(offs[-1])
        d_R, d_L, d_P = _to_device(self.R[:hi], 8), _to_device(self.L[:hi], self.bits), _to_device(self.P[:hi], 64)
        d_D = None if self.D is None else _to_device(self.D[:hi], self.bits)
        d_offs = _to_device(offs, 64)
        fo = DeviceFence(self.name + " records", 8 * k, torch.int32)

        def launch(ix, stream):
            ix.place_device(d_R, d_L, d_P, d_offs, *self.params, d_docs=d_D, d_out=fo.t, total_values=hi, stream=stream)

        return Job(launch, lambda: {"records": fo.values(np.uint32).view(PLACEMENT_DTYPE).reshape(-1)})

    def path(self, ix, step):
        st = ix.place_stats()
        placed = int((step.want["records"]["ref_start"] != np.uint64(UNPLACED)).sum())
        assert st["values"] == step.chars and st["placed"] == placed, (self.name, st, placed)


class Chain(Product):
    """spc_chain_device over uploaded records (crafted anchors: the rule is one on the records) with f and pred of every
    anchor; spc_chain_batch (form host) against chain_reference over mems_reference over the oracle's MS arrays."""

    def __init__(self, cat, name, index, offs, rec, D, params=None, form="device", batch=None, min_length=0):
        nreads = len(batch[1]) - 1 if form == "host" else len(offs) - 1
        super().__init__(cat, name, index, nreads, form, batch, min_length)
        self.offs, self.rec, self.D, self.params = None if offs is None else np.asarray(offs, dtype=np.int64), rec, D, params

    def compute(self, k):
        if self.form == "host":
            mo, rec = self.matches(k)
            count = [0]
            chains, _, _ = chain_reference(mo, rec, self.params, count=count)
            self.seen[k] = dict(anchors=rec.size, candidates=count[0])
            return int(self.batch[1][k]), {"records": chains, "values": np.diff(self.batch[1][: k + 1]).astype(np.uint64)}
        offs = self.offs[: k + 1]
        lo, hi = int(offs[0]), int(offs[-1])
        count = [0]
        chains, score, pred = chain_reference(offs.astype(np.uint64), self.rec, self.params, self.D, count=count)
        self.seen[k] = dict(anchors=hi - lo, candidates=count[0])
        return hi - lo, {"records": chains, "score": score[lo:hi], "pred": pred[lo:hi]}

    def prepare(self, k):
        if self.form == "host":
            seqs, offs = self.host_reads(k)
            return self.host_job(lambda ix: ix.chain_host(seqs, offs, self.min_length, self.params), ("records", "values"))
        offs = self.offs[: k + 1]
        lo, hi = int(offs[0]), int(offs[-1])
        d_rec = torch.from_numpy(np.concatenate([self.rec[:hi], np.zeros(1, dtype=MATCH_DTYPE)]).view(np.int32).reshape(-1, 4).copy()).cuda()
        d_D = None if self.D is None else _upload(np.r_[self.D[:hi], 0], np.uint32)
        d_offs = torch.from_numpy(offs.copy()).cuda()
        fo = DeviceFence(self.name + " records", 12 * k, torch.int32)
        fs = DeviceFence(self.name + " score", hi, torch.int32, lo)
        fp = DeviceFence(self.name + " pred", hi, torch.int32, lo)

        def launch(ix, stream):
            ix.chain_device(d_rec, d_offs, self.params, d_match_docs=d_D, d_out=fo.t, d_out_score=fs.t, d_out_pred=fp.t, stream=stream)

        return Job(launch, lambda: {"records": fo.values(np.uint32).view(CHAIN_DTYPE).reshape(-1), "score": fs.values(np.uint32),
                                    "pred": fp.values(np.uint32)})

    def path(self, ix, step):
        st, chains, seen = ix.chain_stats(), step.want["records"], self.seen[step.nreads]
        assert st["reads"] == step.nreads and st["anchors"] == seen["anchors"] and st["candidates"] == seen["candidates"], (self.name, st, seen)
        assert st["chained_reads"] == int((chains["anchors"] > 0).sum()) and st["chain_anchors"] == int(chains["anchors"].sum()), (self.name, st)


UNALIGNED_REC = (UNALIGNED, 0, 0, 0, 0, 0, 0, 0, 0, NO_DOC)


class Align(Product):
    """spa_align_device over crafted reads, anchors, chains and pred (tests/test_gpu_align.py: Batch) on the index's text,
    the per-gap table in caller buffers or (table False) in the index's scratch; short: a gap capacity one below the end of
    a middle read's gaps -- that read and every later one with gaps comes back unaligned.  spa_align_batch (form host)
    against oracle MS -> mems_reference -> chain_reference -> align_reference."""
    reference = staticmethod(align_reference)
    TABLE = ("gap_offsets", "gaps")

    def __init__(self, cat, name, index, arrays, params=None, table=True, short=False, form="device", batch=None, min_length=0):
        nreads = len(batch[1]) - 1 if form == "host" else len(arrays[3]) - 1
        super().__init__(cat, name, index, nreads, form, batch, min_length)
        self.arrays, self.params, self.table, self.short = arrays, params, table, short

    def sliced(self, k):
        R, roffs, rec, moffs, chains, pred = self.arrays
        return R, roffs[: k + 1], rec, moffs[: k + 1], chains[:k], pred

    def refer(self, k):
        """(chars, the six arrays, the product's reference over them, align_reference's table, extra keys of a host form)"""
        if self.form == "host":
            seqs, offs = self.host_reads(k)
            mo, rec = self.matches(k)
            chains, _, pred = chain_reference(mo, rec)
            arrays, extra = (seqs, offs, rec, mo, chains, pred), {"chains": chains, "values": np.diff(offs.astype(np.int64)).astype(np.uint64)}
        else:
            arrays, extra = self.sliced(k), {}
        R, roffs, rec, moffs, chains, pred = arrays
        count = [0]
        table = align_reference(R, roffs, self.text(), moffs, rec, chains, pred, self.params, count=count)
        ref = table if self.reference is align_reference else self.reference(R, roffs, self.text(), moffs, rec, chains, pred, self.params)
        return int(roffs[-1]) - int(roffs[0]), arrays, ref, table, count[0], extra

    def gap_capacity(self, k, goffs):
        if not self.short:
            return self.arrays[2].size  # the number of records: always enough
        per_read = np.diff(goffs.astype(np.int64))
        cand = np.flatnonzero(per_read >= 2)
        q = int(cand[cand.size // 2])  # a middle read among those with two gaps or more
        return int(goffs[q + 1]) - 1

    def compute(self, k):
        chars, arrays, (want, goffs, gaps), _, cells, extra = self.refer(k)
        self.seen[k] = dict(goffs=goffs, gaps=gaps, cells=cells, cap=None, reference=want)
        if self.form == "host":
            return chars, dict(extra, records=want)
        cap = self.seen[k]["cap"] = self.gap_capacity(k, goffs)
        fits = (goffs[1:] <= cap) | (np.diff(goffs.astype(np.int64)) == 0)
        want = want.copy()
        want[~fits] = UNALIGNED_REC
        out = {"records": want}
        if self.table:
            out.update(gap_offsets=goffs, gaps=gaps)
        return chars, out

    def uploads(self, k):
        R, roffs, rec, moffs, chains, pred = self.sliced(k)
        n = rec.size
        return (torch.from_numpy(np.r_[R, np.zeros(8, dtype=np.uint8)]).cuda(),
                torch.from_numpy(np.asarray(roffs, dtype=np.uint64).view(np.int64).copy()).cuda(),
                torch.from_numpy(np.concatenate([rec, np.zeros(1, dtype=MATCH_DTYPE)]).view(np.int32).reshape(-1, 4).copy()).cuda()[:n],
                torch.from_numpy(np.asarray(moffs, dtype=np.uint64).view(np.int64).copy()).cuda(),
                torch.from_numpy(np.concatenate([chains, np.zeros(1, dtype=CHAIN_DTYPE)]).view(np.int32).reshape(-1, 12).copy()).cuda()[:k],
                torch.from_numpy(np.r_[pred, np.zeros(1, dtype=np.uint32)].view(np.int32).copy()).cuda()[:n])

    def prepare(self, k):
        if self.form == "host":
            seqs, offs = self.host_reads(k)
            return self.host_job(lambda ix: ix.align_host(seqs, offs, self.min_length, None, self.params), ("records", "chains", "values"))
        self.expect(k)
        cap, total = self.seen[k]["cap"], self.seen[k]["gaps"].size
        d = self.uploads(k)
        fo = DeviceFence(self.name + " records", 12 * k, torch.int32)
        fg = DeviceFence(self.name + " gap offsets", k + 1, torch.int64) if self.table else None
        ft = DeviceFence(self.name + " gaps", 4 * cap, torch.int32) if self.table else None
        p = capi.SpaParams(*(self.params or AlignParams()))

        def launch(ix, stream):
            st = stream if stream is not None else torch.cuda.current_stream()
            capi._check(capi._spa().spa_align_device(ix._h, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), k, d[4].data_ptr(),
                                                     d[5].data_ptr(), capi.C.byref(p), cap, fo.t.data_ptr(), fg.t.data_ptr() if fg else None,
                                                     ft.t.data_ptr() if ft else None, capi.C.c_void_p(st.cuda_stream)))

        def collect():
            got = {"records": fo.values(np.uint32).view(ALIGN_DTYPE).reshape(-1)}
            if self.table:
                got["gap_offsets"] = fg.values(np.uint64)
                got["gaps"] = _pattern_behind(ft.values(np.uint32), 4 * min(total, cap), self.name + " gaps").view(GAP_DTYPE).reshape(-1)
            return got

        return Job(launch, collect)

    def stats(self, ix):
        return ix.align_stats()

    def path(self, ix, step):
        st, seen, want = self.stats(ix), self.seen[step.nreads], step.want["records"]
        ok = int((want["ref_start"] != np.uint64(UNALIGNED)).sum())
        lost = ok < int((seen["reference"]["ref_start"] != np.uint64(UNALIGNED)).sum())
        assert st["reads"] == step.nreads and st["aligned_reads"] == ok and st["error"] == 0 and st["overflow"] == int(lost), (self.name, st, ok)
        assert lost == bool(self.short or getattr(self, "short_ops", False)), (self.name, lost)
        if not lost:
            gaps = seen["gaps"]
            assert st["gaps"] == gaps.size and st["filled_gaps"] == int((gaps["edits"] != UNFILLED).sum()) and st["cells"] == seen["cells"], (self.name, st)
        return st, lost


class Cigar(Align):
    """spg_cigar_device on the same kind of input, records, op offsets and entries; short_ops: an op capacity one below the
    entries -- the last read with entries does not fit, writes none and comes back unaligned while the offsets still count
    it.  spg_cigar_begin + spg_cigar_fetch (form host), the two calls together."""
    reference = staticmethod(cigar_reference)

    def __init__(self, cat, name, index, arrays, params=None, short_ops=False, form="device", batch=None, min_length=0):
        super().__init__(cat, name, index, arrays, params, form=form, batch=batch, min_length=min_length)
        self.short_ops = short_ops

    def compute(self, k):
        chars, arrays, (want, ooffs, ops), (_, goffs, gaps), cells, extra = self.refer(k)
        self.seen[k] = dict(goffs=goffs, gaps=gaps, cells=cells, reference=want, ooffs=ooffs, entries=ops.size)
        if self.form == "host":
            return chars, dict(extra, records=want, op_offsets=ooffs, entries=ops)
        R, _, rec, moffs, _, _ = arrays
        op_cap = int(ooffs[-1]) - 1 if self.short_ops else 2 * R.size + 2 * rec.size + moffs.size + 64
        fits = ooffs[1:] <= op_cap
        whole = int(ooffs[1:][fits].max(initial=0))
        self.seen[k].update(op_cap=op_cap, entries=whole)
        want = want.copy()
        want[~fits] = UNALIGNED_REC
        return chars, {"records": want, "op_offsets": ooffs, "entries": ops[:whole]}

    def prepare(self, k):
        if self.form == "host":
            seqs, offs = self.host_reads(k)
            return self.host_job(lambda ix: ix.cigar_host(seqs, offs, self.min_length, None, self.params),
                                 ("records", "op_offsets", "entries", "chains", "values"))
        self.expect(k)
        op_cap, whole = self.seen[k]["op_cap"], self.seen[k]["entries"]
        d = self.uploads(k)
        cap = self.arrays[2].size
        fo = DeviceFence(self.name + " records", 12 * k, torch.int32)
        ff = DeviceFence(self.name + " op offsets", k + 1, torch.int64)
        fe = DeviceFence(self.name + " entries", op_cap, torch.int32)

        def launch(ix, stream):
            ix.cigar_device(*d, self.params, gap_capacity=cap, op_capacity=op_cap, d_out=fo.t, d_out_op_offsets=ff.t, d_out_ops=fe.t, stream=stream)

        return Job(launch, lambda: {"records": fo.values(np.uint32).view(ALIGN_DTYPE).reshape(-1), "op_offsets": ff.values(np.uint64),
                                    "entries": _pattern_behind(fe.values(np.uint32), whole, self.name + " entries")})

    def stats(self, ix):
        return ix.cigar_stats()

    def path(self, ix, step):
        st, lost = super().path(ix, step)
        seen = self.seen[step.nreads]
        assert st["entries"] == seen["entries"], (self.name, st, seen["entries"])
        if not lost:
            assert st["path_words"] == gc.path_words(seen["gaps"], (self.params or AlignParams()).max_fill), (self.name, st)


# ---- batches -------------------------------------------------------------------------------------------------------------
def _concat(reads):
    offs = np.concatenate([[0], np.cumsum([r.size for r in reads])]).astype(np.int64)
    return (np.concatenate(reads).astype(np.uint8) if offs[-1] else np.zeros(0, dtype=np.uint8)), offs


def _cut(rng, text, m, every=0):
    """m characters of the text, a substitution every `every` characters or so (0: none)"""
    s = int(rng.integers(0, text.size - m)) if m < text.size else 0
    rd = np.resize(text[s:], m).copy() if m > text.size - s else text[s: s + m].copy()
    for _ in range(m // every if every else 0):
        rd[rng.integers(0, m)] = DNA[rng.integers(0, 4)]
    return rd


def _ends_on_the_grid(rng, text, nreads, grid):
    """reads of 0 .. 700 characters whose ends (in the concatenation) fall on multiples of `grid` and one either side; every
    third read random letters (N among them), the others cut from the text with substitutions"""
    reads, at = [], 0
    for q in range(nreads):
        m = int(rng.integers(0, 700)) if q % 11 else 0
        end = (at + m + grid // 2) // grid * grid + (q % 3 - 1)
        m = max(end - at, 0)
        rd = _cut(rng, text, m, 60) if q % 3 else np.r_[DNA, [N]].astype(np.uint8)[rng.integers(0, 5, size=m)]
        reads.append(rd)
        at += m
    return _concat(reads)


def _ragged(rng, raw, lens, seed, **kw):
    """reads of the given lengths for a statistical index (no text to cut from): the tails of simulated reads"""
    m = max(max(lens), 1)
    pool, _ = synth.simulate_reads(raw, len(lens), m, seed=seed, **kw)
    pool = pool.cpu().numpy().reshape(len(lens), m)
    return _concat([pool[q, m - ln:].copy() for q, ln in enumerate(lens)])


def resets(pml):
    """PML lengths that are 0 -- the characters at which the walk reset its counter -- per character"""
    z = np.asarray(pml) == 0
    return float(z.mean()) if z.size else 0.0


class Catalogue:
    """indexes: name -> dict(raw, text, wide); steps / dirtiers: name -> Step; claims: (step, dirtier, check) per pair."""

    def __init__(self, oracle_mod, device_forms=True, native_only=True):
        self.oracle, self.device_forms, self.native_only = oracle_mod, device_forms, native_only
        self.indexes, self.steps, self.dirtiers, self.claims = {}, {}, {}, {}
        self._orc, self._values = {}, {}

    # -- indexes and the oracle's arrays --
    def add_index(self, name, raw, text=None, wide=False, same_as=None):
        self.indexes[name] = dict(raw=raw, text=text, wide=wide)
        self._orc[name] = self._orc[same_as] if same_as else self.oracle.OracleIndex.from_raw(raw)

    def oracle_values(self, index, batch, mode):
        """lengths, docs (PML) / pointers, docs, lengths where the index holds its text (MS) of a batch: computed once"""
        key = (self.indexes[index]["raw"].n, id(batch[0]), mode)
        if key not in self._values:
            orc, text = self._orc[index], self.indexes[index]["text"]
            if mode == PML:
                ln, dc = orc.pml(batch[0], batch[1], want_docs=True)
                self._values[key] = (batch, {"lengths": ln, "docs": dc})
            else:
                self._values[key] = (batch, orc.ms(batch[0], batch[1], want_docs=True, text=text))
        return self._values[key][1]

    def handle(self, index):
        """a fresh handle of one of the indexes (needs the library)"""
        spec = self.indexes[index]
        old = os.environ.pop("SPX_ROWS_WIDE", None)
        if spec["wide"]:
            os.environ["SPX_ROWS_WIDE"] = "1"  # (read when an index is flattened: the general 16-byte rows)
        try:
            ix = capi.Index.from_raw(spec["raw"], 0)
        finally:
            os.environ.pop("SPX_ROWS_WIDE", None)
            if old is not None:
                os.environ["SPX_ROWS_WIDE"] = old
        if spec["text"] is not None:
            ix.set_text(torch.from_numpy(spec["text"].copy()))
        return ix

    def add(self, family, dirtier, claim=None, as_dirtier=False):
        if family.form == "device" and not self.device_forms:
            return
        if not self.native_only and isinstance(family, (Votes, Mems, Product)):
            return  # (the stand-in library of the CPU tier has no votes, no matches and none of the products built on them)
        family.dirtier = dirtier
        (self.dirtiers if as_dirtier else self.steps)[family.name] = family.step()
        if claim:
            self.claims[family.name] = claim

    def every(self):
        return list(self.steps.values())

    def dirtier_of(self, step):
        return self.dirtiers[step.dirtier]

    def check_claims(self):
        """every pair differs in the way it was chosen for; returns the number of pairs checked"""
        n = 0
        for step in self.every():
            d = self.dirtier_of(step)
            assert d.index == step.index, (step.name, d.name)  # one handle
            assert 4 * step.chars <= d.chars <= max(10 * step.chars, 1) and d.chars <= 400_000, (step.name, step.chars, d.name, d.chars)
            assert step.chars <= 40_000, (step.name, step.chars)
            self.claims[step.name](step, d)
            n += 1
        return n


def build(oracle_mod, device_forms=True, native_only=True):
    """The catalogue.  device_forms False: host forms only; native_only False: only what tests/fake_device answers."""
    cat = Catalogue(oracle_mod, device_forms, native_only)
    rng = np.random.default_rng(2024)
    add = cat.add

    # ---- index 1: a real BWT of 9 000 characters, four documents, with its text; compact rows and general rows ----
    raw, text = cases.real_case(7, 9000, list(b"ACGT"), ndocs=4)
    cat.add_index("real", raw, text)
    cat.add_index("real_wide", raw, text, wide=True, same_as="real")
    lens = [0, 1, 700, 699, 0, 63, 64, 65, 511, 512, 513] + [int(x) for x in rng.integers(200, 700, size=60)]
    match = _concat([_cut(rng, text, m) for m in lens])  # long exact matches: few resets
    absent = _concat([np.full(int(m), N, dtype=np.uint8) for m in rng.integers(300, 900, size=260)])  # every character resets
    short = _concat([_cut(rng, text, m, 40) if q % 2 else DNA[rng.integers(0, 4, size=m)]
                     for q, m in enumerate([0, 0, 1, 2, 149] + [int(x) for x in rng.integers(0, 150, size=140)])])
    many = _concat([_cut(rng, text, int(m), 50) for m in rng.integers(20, 200, size=640)])
    big_ms = _concat([np.tile(text, 9)[1234: 1234 + 70000]])

    def few_resets(step, d):  # resets per character: 1.0 against < 0.05
        a = cat.oracle_values(step.index, step.family.batch, PML)["lengths"]
        b = cat.oracle_values(d.index, d.family.batch, PML)["lengths"]
        assert resets(a) < 0.05 and resets(b) == 1.0, (step.name, resets(a), resets(b))

    def staged(step, d):  # every read of the step stages its lengths, the dirtier's read cannot
        assert int(np.diff(step.family.batch[1]).max()) < 65536 <= int(np.diff(d.family.batch[1]).max())
        assert int(d.want["lengths"].max()) > 4 * int(step.want["lengths"].max())

    def all_below(step, d):
        assert step.want["class"]["above"].sum() == 0 and step.want["class"]["below"].sum() > 0
        assert d.want["class"]["below"].sum() == 0 and d.want["class"]["above"].sum() > 0 and d.nreads >= 4 * step.nreads

    top = int(cat.oracle_values("real", match, PML)["lengths"].max()) + 1
    for ixname, compact in (("real", 1), ("real_wide", 0)):
        sfx = "" if compact else " (general rows)"
        add(Query(cat, "dirty: absent letter, PML 32 + docs + class" + sfx, ixname, absent, PML, docs=True, cls=(64, 1), compact=compact), None,
            as_dirtier=True)
        add(Query(cat, "dirty: absent letter, device PML 32 + docs + class" + sfx, ixname, absent, PML, "device", docs=True, cls=(64, 1),
                  compact=compact), None, as_dirtier=True)
        add(Query(cat, "query_host PML 32 + docs + class" + sfx, ixname, match, PML, docs=True, cls=(64, 20), compact=compact),
            "dirty: absent letter, PML 32 + docs + class" + sfx, few_resets)
        add(Query(cat, "query_device PML 16, offs[0] = 0" + sfx, ixname, match, PML, "device", bits=16, compact=compact),
            "dirty: absent letter, device PML 32 + docs + class" + sfx, few_resets)
        add(Query(cat, "query_device PML 32, offs[0] = 37" + sfx, ixname, match, PML, "device", front=37, docs=True, cls=(150, 9),
                  compact=compact), "dirty: absent letter, device PML 32 + docs + class" + sfx, few_resets)
    add(Query(cat, "query_host PML 16 + class", "real", match, PML, bits=16, cls=(7, 30)), "dirty: absent letter, PML 32 + docs + class",
        few_resets)
    add(Query(cat, "dirty: class records at threshold 0", "real", many, PML, lengths=False, cls=(8, 0)), None, as_dirtier=True)
    add(Query(cat, "query_host PML class only, every bin below", "real", short, PML, lengths=False, cls=(8, top)),
        "dirty: class records at threshold 0", all_below)
    add(Query(cat, "dirty: one MS read of 70 000 characters", "real", big_ms, MS, docs=True, cls=(64, 5), opts={"chunk_mode": 1}), None,
        as_dirtier=True)
    add(Query(cat, "dirty: one MS read of 70 000 characters, device", "real", big_ms, MS, "device", docs=True, cls=(64, 5),
              opts={"chunk_mode": 1}), None,
        as_dirtier=True)
    add(Query(cat, "query_host MS pointers + lengths + docs + class", "real", short, MS, docs=True, cls=(20, 6)),
        "dirty: one MS read of 70 000 characters", staged)
    add(Query(cat, "query_host MS pointers + docs", "real", short, MS, lengths=False, docs=True),
        "dirty: one MS read of 70 000 characters", lambda step, d: staged(cat.steps["query_host MS pointers + lengths + docs + class"], d))
    add(Query(cat, "query_device MS + lengths + docs 32", "real", short, MS, "device", docs=True),
        "dirty: one MS read of 70 000 characters, device", staged)
    add(Query(cat, "query_device MS + lengths + docs 16", "real", short, MS, "device", bits=16, docs=True),
        "dirty: one MS read of 70 000 characters, device", staged)

    # the chunked walk on this index: chunks of 32 characters, read ends on the grid and one either side
    grid32 = _ends_on_the_grid(rng, text, 90, 32)
    assert {int(e) % 32 for e in grid32[1][1:]} >= {0, 1, 31} and grid32[1][-1] <= 40_000

    def resets_everywhere(step, d):
        b = cat.oracle_values(d.index, d.family.batch, PML)["lengths"]
        assert resets(b) == 1.0 and resets(cat.oracle_values(step.index, step.family.batch, PML)["lengths"]) < 0.5

    add(Query(cat, "dirty: absent letter in chunks of 64, PML + docs", "real", absent, PML, docs=True, opts={"chunk_mode": 2, "chunk_len": 64},
              chunk=64), None, as_dirtier=True)
    add(Query(cat, "chunk_shift 5, ragged ends, device PML 16 + docs", "real", grid32, PML, "device", bits=16, docs=True,
              opts={"chunk_mode": 2, "chunk_shift": 5}, chunk=32), "dirty: absent letter in chunks of 64, PML + docs", resets_everywhere)
    add(Query(cat, "chunk_shift 5, ragged ends, host MS + docs", "real", grid32, MS, lengths=False, docs=True,
              opts={"chunk_mode": 2, "chunk_shift": 5}, chunk=32), "dirty: absent letter in chunks of 64, PML + docs", resets_everywhere)

    # ---- index 2: the period-20 text of tests/test_gpu_chunked.py::test_reads_that_never_jump_fall_back ----
    # Its long reads are exact matches of thousands of characters (never_jumps() asserts that on the oracle's MS lengths), but
    # at chunks of 96 they do not fall back: the BWT of a period-20 text is 21 runs, the oracle counts 152 jumps in the 3 000
    # characters of the first read -- one per period, each to the end of a run, where a chunk's speculative walk lands too -- so
    # every seam closes at its first checkpoint (on an MI355X: fallback_reads 0, rewalked_chars 1376 of 8300).  These steps
    # assert chunk_len; the steps that fall back, and the pair around them, are on index 3.
    unit = np.frombuffer(b"ACGTTGCAAGGCTTAACCGT", dtype=np.uint8)
    ptext = np.tile(unit, 400)
    cat.add_index("period20", synth.index_from_text(torch.from_numpy(ptext.copy()), doc_lengths=[3000, 5000]), ptext)
    nj = [ptext[7:3007], ptext[100:1500], np.full(900, N, dtype=np.uint8), np.full(1000, ord("A"), dtype=np.uint8), ptext[13:2013].copy()]
    nj[4][::97] = ord("T")
    never = _concat(nj)
    ragged5 = _concat([np.r_[DNA, [N]].astype(np.uint8)[rng.integers(0, 5, size=int(m))] for m in rng.integers(100, 900, size=80)])

    def never_jumps(step, d):  # matches of a thousand characters and more against matches of a few (the MS lengths say so)
        a = cat.oracle_values(step.index, step.family.batch, MS)["lengths"]
        b = cat.oracle_values(d.index, d.family.batch, MS)["lengths"]
        assert int(a.max()) >= 1000 and int(b.max()) < 100, (step.name, int(a.max()), int(b.max()))

    for mode, tag, kw in ((PML, "PML + docs", dict(docs=True)), (MS, "MS + docs", dict(docs=True, lengths=False))):
        add(Query(cat, f"dirty: ragged random reads in chunks of 48, {tag}", "period20", ragged5, mode, opts={"chunk_mode": 2, "chunk_len": 48},
                  chunk=48, **kw), None, as_dirtier=True)
        add(Query(cat, f"chunk_len 96, reads that never jump, {tag}", "period20", never, mode, opts={"chunk_mode": 2, "chunk_len": 96},
                  chunk=96, **kw), f"dirty: ragged random reads in chunks of 48, {tag}", never_jumps)
        add(Query(cat, f"plain walk of the reads that never jump, {tag}", "period20", never, mode, opts={"chunk_mode": 1}, **kw),
            f"dirty: ragged random reads in chunks of 48, {tag}", never_jumps)

    # ---- index 3: a statistical index of 2^16 runs over 253 letters, ten documents: long reads, the votes ----
    sraw = synth.statistical_rlbwt(1 << 16, 253, 8.0, seed=6, zipf=1.0, with_samples=True, n_docs=10)
    cat.add_index("stat", sraw)
    vlens = [63, 64, 65, 2047, 2048, 2049, 3000, 0, 1, 0] + [int(x) for x in rng.integers(2, 64, size=40)] + \
            [int(x) for x in rng.integers(100, 1500, size=10)]
    vbatch = _ragged(rng, sraw, vlens, seed=31)
    vv = cat.oracle_values("stat", vbatch, PML)
    distinct_offs = np.arange(3) * 65536
    dL = np.full(2 * 65536, 7)
    dD = np.concatenate([np.random.default_rng(s).permutation(65536) for s in (1, 2)])

    def tiles_full(step, d):  # few documents per read against one vote per document
        assert int(d.want["votes"].reshape(-1, 4)[:, 2].max()) == 1 and int(d.want["votes"].reshape(-1, 4)[:, 0].min()) == 65536
        tbl = _vote_table(votes_reference(vv["lengths"], vv["docs"], vbatch[1], step.family.min_length)).reshape(-1, 4)
        assert len(set(vv["docs"].tolist())) <= 10 and int(tbl[:, 2].max()) > 100

    add(Votes(cat, "dirty: votes, all ids of a long read distinct, 32 bit", "stat", distinct_offs, dL, dD, 32, 0, paths=False), None,
        as_dirtier=True)
    add(Votes(cat, "votes_device 32 over the oracle's arrays", "stat", vbatch[1], vv["lengths"], vv["docs"], 32, 2),
        "dirty: votes, all ids of a long read distinct, 32 bit", tiles_full)
    add(Votes(cat, "votes_device 16 over what query_device16 wrote", "stat", vbatch[1], vv["lengths"], vv["docs"], 16, 2, batch=vbatch),
        "dirty: votes, all ids of a long read distinct, 32 bit", tiles_full)

    def every_position_votes(step, d):  # voters per value 1.0 (min_length 0) on five times the reads, against a threshold that leaves positions out
        assert (d.want["records"]["voters"] == d.want["values"]).all() and d.nreads >= 5 * step.nreads
        assert (step.want["records"]["voters"] < step.want["values"]).any() and step.want["records"]["voters"].any()

    vmany = _ragged(rng, sraw, [int(x) for x in rng.integers(100, 700, size=300)], seed=32)
    vm = cat.oracle_values("stat", vmany, PML)
    add(Votes(cat, "dirty: assign_host on more and longer reads", "stat", vmany[1], vm["lengths"], vm["docs"], 32, 0, "host", vmany,
              paths=False), None, as_dirtier=True)
    add(Votes(cat, "assign_host", "stat", vbatch[1], vv["lengths"], vv["docs"], 32, 2, "host", vbatch),
        "dirty: assign_host on more and longer reads", every_position_votes)
    # Long reads simulated from the index itself, half of them following its runs with a mismatch every fifty characters.  In chunks of
    # 32 a share of them keeps a seam open through every round and is walked again the plain way (fallback_reads > 0, asserted:
    # tests/test_gpu_dynamic_deal.py has the same kind of batch); in chunks of 176 a seam left open closes in the next round
    # and nothing falls back (tests/test_gpu_chunked.py).  The step that falls back runs behind the same kind of reads with
    # ten times the mismatches at another chunk size (seams that all close); the step where nothing falls back runs behind a
    # batch that does -- read_fail, open seams and flags left in the scratch it uses.
    long_reads = _ragged(rng, sraw, [2200] * 16, seed=16)
    long5 = _ragged(rng, sraw, [2200] * 70, seed=17, f_mis=0.2)
    long5_open = _ragged(rng, sraw, [2200] * 70, seed=18)

    def jumps_per_character(batch):  # per read, counted by the oracle's own walk
        orc = cat._orc["stat"]
        return np.array([orc.stats(batch[0][a:b], np.array([0, b - a]))["jumps"] / (b - a) for a, b in zip(batch[1][:-1], batch[1][1:])])

    def mismatches(step, d):  # reads of the step that jump less than once in five characters (a seam can stay open); every read of the dirtier jumps more than once in four
        a, b = jumps_per_character(step.family.batch), jumps_per_character(d.family.batch)
        assert (a < 0.2).sum() >= 4 and b.min() > 0.25, (step.name, np.sort(a)[:6], b.min())

    def open_seams(step, d):  # a quarter of the dirtier's reads jump less than once in five characters, and it runs in chunks of 32: asserted to fall back
        b = jumps_per_character(d.family.batch)
        assert (b < 0.2).sum() >= d.nreads // 4 and d.family.chunk == 32 and d.family.fallback is True, (step.name, np.sort(b)[:6])

    for mode, tag, kw in ((PML, "PML + docs + class", dict(docs=True, cls=(150, 5))), (MS, "MS + docs", dict(docs=True, lengths=False))):
        add(Query(cat, f"dirty: long reads with many mismatches in chunks of 48, {tag}", "stat", long5, mode,
                  opts={"chunk_mode": 2, "chunk_len": 48}, chunk=48, **kw), None, as_dirtier=True)
        add(Query(cat, f"dirty: long reads in chunks of 32 that fall back, {tag}", "stat", long5_open, mode, "device",
                  opts={"chunk_mode": 2, "chunk_shift": 5}, chunk=32, fallback=True, **kw), None, as_dirtier=True)
        add(Query(cat, f"chunk_shift 5, long reads that fall back, host {tag}", "stat", long_reads, mode, opts={"chunk_mode": 2, "chunk_shift": 5},
                  chunk=32, fallback=True, **kw), f"dirty: long reads with many mismatches in chunks of 48, {tag}", mismatches)
        add(Query(cat, f"long reads in chunks of 176, nothing falls back, device {tag}", "stat", long_reads, mode, "device",
                  opts={"chunk_mode": 2, "chunk_len": 176}, chunk=176, fallback=False, **kw),
            f"dirty: long reads in chunks of 32 that fall back, {tag}", open_seams)

    # ---- the matches: the oracle's MS arrays on index 1, and crafted arrays for the pair of the table ----
    mlens = [63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 0, 1] + [int(x) for x in rng.integers(10, 300, size=20)]
    mbatch = _concat([_cut(rng, text, m, 25) for m in mlens])
    mv = cat.oracle_values("real", mbatch, MS)
    craft_offs = np.r_[0, np.cumsum([63, 64, 0, 0, 1, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 0, 5])]
    falling = np.zeros(int(craft_offs[-1]), dtype=np.int64)
    for o, e in zip(craft_offs[:-1], craft_offs[1:]):
        falling[o:e] = np.arange(e - o, 0, -1) + 16
    const_offs = np.r_[0, np.cumsum(rng.integers(100, 1200, size=100))]
    const_offs = const_offs[: int(np.searchsorted(const_offs, 90_000))]
    constant = np.full(int(const_offs[-1]), 21)
    cP = rng.integers(0, 1 << 40, size=constant.size).astype(np.uint64)
    cD = rng.integers(0, 5, size=constant.size)

    def one_start_per_read(step, d):  # matches per value: reads / values against 1.0
        assert d.want["records"].size == d.chars
        if step.family.L is falling:
            assert step.want["records"].size == int((np.diff(craft_offs) > 0).sum())
        assert step.want["records"].size < step.chars / 4

    for bits in (16, 32):
        add(Mems(cat, f"dirty: matches, every position a start, {bits} bit", "real", const_offs, constant, cP, cD, bits, 4), None,
            as_dirtier=True)
        add(Mems(cat, f"mems_device {bits}, one start per read", "real", craft_offs, falling, cP, None, bits, 4),
            f"dirty: matches, every position a start, {bits} bit", one_start_per_read)
        for docs in (True, False):
            add(Mems(cat, f"mems_device {bits} over the oracle's MS arrays, {'with' if docs else 'without'} docs", "real", mbatch[1],
                     mv["lengths"], mv["pointers"], mv["docs"] if docs else None, bits, 8),
                f"dirty: matches, every position a start, {bits} bit", one_start_per_read)
    mmany = _concat([_cut(rng, text, int(m), 9) for m in rng.integers(100, 500, size=200)])
    mm = cat.oracle_values("real", mmany, MS)
    add(Mems(cat, "dirty: mems_host, a start every few characters", "real", mmany[1], mm["lengths"], mm["pointers"], mm["docs"], 32, 1, "host",
             mmany), None, as_dirtier=True)

    def more_matches(step, d):
        assert d.want["records"].size > 8 * step.want["records"].size > 0, (step.name, d.want["records"].size, step.want["records"].size)

    add(Mems(cat, "mems_host", "real", mbatch[1], mv["lengths"], mv["pointers"], mv["docs"], 32, 8, "host", mbatch),
        "dirty: mems_host, a start every few characters", more_matches)

    # ---- the vectors as text on index 1 ----
    mixed = cases.reads_mixed(rng, text, list(b"ACGT"), 150, 450, [N])
    mixed4 = cases.reads_mixed(rng, text, list(b"ACGT"), 560, 600, [N])
    L_, P_, D_ = capi.SPX_TEXT_LENGTHS, capi.SPX_TEXT_POINTERS, capi.SPX_TEXT_DOCS

    def text_bytes(s):
        return sum(len(v) for key, v in s.want.items() if key != "class")

    def longer_lines(step, d):  # bytes of text per character of the batch: more streams, or values of more digits
        assert text_bytes(d) / d.chars > 1.5 * text_bytes(step) / step.chars, (step.name, text_bytes(d) / d.chars, text_bytes(step) / step.chars)

    def more_text(step, d):  # the same streams: every one of them four times as long
        assert set(d.want) >= set(step.want) - {"class"}
        assert all(len(d.want[key]) >= 4 * len(v) > 0 for key, v in step.want.items() if key != "class"), step.name

    add(Text(cat, "dirty: text, MS with all three streams on four times the characters", "real", mixed4, MS, L_ | P_ | D_), None, as_dirtier=True)
    add(Text(cat, "query_text PML lengths + docs + class with gaps", "real", mixed, PML, L_ | D_, cls=(20, 6)),
        "dirty: text, MS with all three streams on four times the characters", longer_lines)
    add(Text(cat, "query_text MS with all three streams", "real", mixed, MS, L_ | P_ | D_),
        "dirty: text, MS with all three streams on four times the characters", more_text)
    add(Text(cat, "query_text after a reserve_text hint smaller than the batch", "real", mixed, PML, L_ | D_, cls=(33, 2), reserve=(16, 1)),
        "dirty: text, MS with all three streams on four times the characters", longer_lines)

    # ---- index 4: 2^40 - 3 positions (general rows): text of 1-digit values against MS pointers of 13 digits ----
    wraw, wletters = cases.wide_case(0, n_docs=300)
    cat.add_index("wide40", wraw, None, wide=True)
    w_small = synth.simulate_reads(wraw, 150, 60, seed=5, positive_fraction=0.0)
    w_small = (w_small[0].numpy(), w_small[1].numpy())
    w_big = cases.wide_reads(wraw, wletters, 3, nreads=200, length=60)

    def digits(step, d):  # 1-digit values against pointers of 13 digits, four times the values
        a, b = cat.oracle_values(step.index, step.family.batch, PML)["lengths"], d.family.full["pointers"]
        assert (a < 10).mean() > 0.9 and int(np.median(b)) >= (1 << 32) and int(b[b < (1 << 63)].max()) >= 10 ** 12, (step.name, (a < 10).mean())
        assert d.chars >= 4 * step.chars

    add(Text(cat, "dirty: text, MS pointers of 13 digits", "wide40", w_big, MS, P_), None, as_dirtier=True)
    add(Text(cat, "query_text PML, 1-digit values, no gaps", "wide40", w_small, PML, L_, gaps=False),
        "dirty: text, MS pointers of 13 digits", digits)

    # ---- indexes 5 and 6: over the digested genome (-m and -a), queried with DNA reads ----
    genome = cases.repetitive_text(rng, 30000, list(b"ACGT"))
    dlens = [0, 3, 239, 240, 241, 4095, 4096, 9000] + [int(x) for x in rng.integers(20, 400, size=30)]
    clean = _concat([_cut(rng, genome, m) if q % 2 else DNA[rng.integers(0, 4, size=m)] for q, m in enumerate(dlens)])
    halfn = [DNA[rng.integers(0, 4, size=int(m))].copy() for m in rng.integers(200, 3000, size=80)]
    for r_ in halfn:
        r_[rng.random(r_.size) < 0.5] = N
    halfn = _concat(halfn)
    dq_reads = cases.reads_mixed(rng, genome, list(b"ACGT"), 120, 400, [N])
    dq_long = cases.reads_mixed(rng, genome, list(b"ACGT"), 260, 900, [N])

    def longer_digested_reads(step, d):  # digested values per read, and in all: what the digestion parks and the walk takes
        a, b = np.diff(step.want["offsets"].astype(np.int64)), np.diff(d.want["offsets"].astype(np.int64))
        assert b.mean() > 1.5 * a.mean() and b.max() > 1.5 * a.max() and b.sum() >= 4 * a.sum() > 0, (step.name, a.mean(), b.mean())

    def half_n(step, d):  # no character outside ACGT against every other one
        a, b = step.family.batch[0], d.family.batch[0]
        assert np.isin(a, DNA).all() and 0.4 < (b == N).mean() < 0.6
        assert d.want["digested"].size / d.chars < 0.5 * step.want["digested"].size / step.chars  # (a window with an N gives nothing)

    for kind, tag in ((capi.SPX_DIGEST_PROMOTED, "-m"), (capi.SPX_DIGEST_DNA, "-a")):
        dtext = oracle_mod.digest(kind, K, W, genome)
        name = "digested " + tag
        cat.add_index(name, synth.index_from_text(torch.from_numpy(dtext.copy()), doc_lengths=[dtext.size // 2, dtext.size - dtext.size // 2]),
                      dtext)
        for kernel in (2, 3):
            add(Digest(cat, f"dirty: digest_host {tag}, half N, kernel {kernel}", name, halfn, kind, kernel), None, as_dirtier=True)
        for kernel in (1, 2, 3, 0):
            add(Digest(cat, f"digest_host {tag}, kernel {kernel}", name, clean, kind, kernel),
                f"dirty: digest_host {tag}, half N, kernel {2 if kernel == 3 else 3}", half_n)
        add(DigestQuery(cat, f"dirty: digest_query_host {tag} on longer reads", name, dq_long, kind), None, as_dirtier=True)
        add(DigestQuery(cat, f"digest_query_host {tag}, PML + docs + class", name, dq_reads, kind),
            f"dirty: digest_query_host {tag} on longer reads", longer_digested_reads)
    m_ = "digested -m"
    add(DigestQuery(cat, "dirty: digest_query_device 32, concatenated, longer reads", m_, dq_long, 1, "device", 32, parked=1), None,
        as_dirtier=True)
    add(DigestQuery(cat, "dirty: digest_query_device 32, parked, longer reads", m_, dq_long, 1, "device", 32, parked=2), None, as_dirtier=True)
    for bits in (16, 32):
        add(DigestQuery(cat, f"digest_query_device {bits}, parked", m_, dq_reads, 1, "device", bits, parked=2),
            "dirty: digest_query_device 32, concatenated, longer reads", longer_digested_reads)
        add(DigestQuery(cat, f"digest_query_device {bits}, concatenated", m_, dq_reads, 1, "device", bits, parked=1),
            "dirty: digest_query_device 32, parked, longer reads", longer_digested_reads)
    add(Text(cat, "dirty: text with -m digestion on longer reads", m_, dq_long, PML, L_ | D_, digest=(1,)), None, as_dirtier=True)
    add(Text(cat, "query_text PML with -m digestion", m_, dq_reads, PML, L_, digest=(1,)),
        "dirty: text with -m digestion on longer reads", longer_lines)
    # ---- place, chain, align, cigar: crafted arrays over index 1's text (the kernels read the text alone), and its host batches ----
    def both(step_family, dirt_family, claim):
        add(dirt_family, None, as_dirtier=True)
        add(step_family, dirt_family.name, claim)

    lens16 = np.r_[[0, 1, 2047, 2048, 300], rng.integers(0, 400, size=75)]
    lens32 = np.r_[[2049, 2500, 5000, 3000, 0], rng.integers(0, 2000, size=80)]
    p16 = gc.place_batch(rng, text, lens16, np.flatnonzero(lens16 >= 40)[::2], 5)
    p32 = gc.place_batch(rng, text, lens32, np.flatnonzero(lens32 >= 40)[::2], 0)

    def both_place_paths(step, d):  # reads of up to 2 048 values (a group of 16 lanes), 16 bit, behind reads above that, 32 bit
        assert int(np.diff(step.family.offs).max()) == 2048 and step.family.bits == 16 and d.family.bits == 32
        assert int((np.diff(d.family.offs) > 2048).sum()) >= 4
        for s in (step, d):
            ok = s.want["records"]["ref_start"] != np.uint64(UNPLACED)
            assert ok.sum() >= 20 and (~ok).sum() >= 20, s.name

    both(Place(cat, "place_device 16", "real", p16[4], p16[0], p16[1], p16[2], p16[3], 16, (gc.MIN_SEED, 4, 16)),
         Place(cat, "dirty: place_device 32 with reads above 2 048 values", "real", p32[4], p32[0], p32[1], p32[2], None, 32, (gc.MIN_SEED, 4, 16)),
         both_place_paths)

    def wide_values(step, d):  # a read of 65 536 values or more is staged in 32 bits; six times the characters
        assert int(np.diff(step.family.offs).max()) < 65536 <= int(np.diff(d.family.offs).max()) and d.chars >= 6 * step.chars
        assert (step.want["records"]["ref_start"] != np.uint64(UNPLACED)).sum() >= step.nreads // 2

    both(Place(cat, "place_host", "real", mbatch[1], None, None, None, None, 32, (20, 4, 16), "host", mbatch),
         Place(cat, "dirty: place_host on a read of 70 000 characters", "real", big_ms[1], None, None, None, None, 32, (20, 4, 16), "host", big_ms),
         wide_values)

    c16 = gc.chain_batch(rng, rng.integers(0, 17, size=700), front=3)
    c5000 = gc.chain_batch(rng, [5000] * 6, front=1, n_docs=2)

    def long_path_first(step, d):  # groups of 16 lanes against the whole wavefront with its ring of 64, with ids
        assert int(np.diff(step.family.offs).max()) == 16 and int(np.diff(d.family.offs).min()) == 5000 and d.family.D is not None
        assert int(d.want["records"]["anchors"].min()) > 64 and int((step.want["records"]["anchors"] > 1).sum()) > step.nreads // 2

    both(Chain(cat, "chain_device with f and pred", "real", c16[0], c16[1], None),
         Chain(cat, "dirty: chain_device, reads of 5 000 anchors with ids", "real", c5000[0], c5000[1], c5000[2]), long_path_first)

    def four_times_the_matches(step, d):
        a, b = step.family.seen[step.nreads]["anchors"], d.family.seen[d.nreads]["anchors"]
        assert b >= 4 * a > 0 and int((step.want["records"]["anchors"] > 1).sum()) >= 10, (step.name, a, b)

    both(Chain(cat, "chain_host", "real", None, None, None, None, "host", mbatch, 8),
         Chain(cat, "dirty: chain_host at min_length 1 on noisier reads", "real", None, None, None, None, "host", mmany, 1), four_times_the_matches)

    def crafted_reads(shapes, per_read, empty_every=0, mutate=0.3, front=0):
        """a Batch over index 1's text: reads of `per_read` gaps each in the order of `shapes` (a shape may carry its read's own
        share of replaced characters as a third value), an anchor-less read now and then"""
        B = Batch(front=front)
        for n_, i in enumerate(range(0, len(shapes), per_read)):
            mine = [(int(s[0]), int(s[1])) for s in shapes[i:i + per_read]]
            room = sum(b for _, b in mine) + 12 * (len(mine) + 1)
            B.add(text, rng, int(rng.integers(0, text.size - room)), mine, mutate=shapes[i][2] if len(shapes[i]) > 2 else mutate)
            if empty_every and n_ % empty_every == 0:
                B.add_empty()
        return B.arrays()

    a_small = crafted_reads(rng.integers(0, 25, size=(260, 2)), 2, empty_every=4, front=2)
    wave_shapes = gc.SMALL_WAVE * 270 + gc.LARGE_WAVE * 4
    a_wave = crafted_reads([wave_shapes[i] for i in rng.permutation(len(wave_shapes))], 6)

    def lists_full(step, d):  # every gap of the dirtier is listed for a wavefront and filled: four times the gaps
        sg, dg = step.family.seen[step.nreads]["gaps"], d.family.seen[d.nreads]["gaps"]
        assert gc.wave_sized(dg, 512).all() and (dg["edits"] != UNFILLED).all() and dg.size >= 4 * sg.size > 100, (step.name, sg.size, dg.size)
        assert min(int(gc.wave_sized(sg, 512).sum()), int((~gc.wave_sized(sg, 512)).sum())) >= 50  # the step has gaps for a lane, too

    def one_short_in_the_middle(step, d):
        lists_full(step, d)
        seen = step.family.seen[step.nreads]
        q = int(np.searchsorted(seen["goffs"], seen["cap"], side="right")) - 1  # the read the capacity ends in
        assert int(seen["goffs"][q]) < seen["cap"] == int(seen["goffs"][q + 1]) - 1 and step.nreads // 4 < q < 3 * step.nreads // 4
        lost = (step.want["records"]["ref_start"] == np.uint64(UNALIGNED)) & (seen["reference"]["ref_start"] != np.uint64(UNALIGNED))
        assert lost[q] and not lost[:q].any() and lost.sum() >= 10

    add(Align(cat, "dirty: align_device, every gap wave-sized and filled", "real", a_wave), None, as_dirtier=True)
    add(Align(cat, "align_device, table in caller buffers", "real", a_small), "dirty: align_device, every gap wave-sized and filled", lists_full)
    add(Align(cat, "align_device, table in the scratch, capacity one short in a middle read", "real", a_small, table=False, short=True),
        "dirty: align_device, every gap wave-sized and filled", one_short_in_the_middle)

    def ten_times_the_edits(step, d):
        a, b = int(step.want["records"]["edits"].sum()), int(d.want["records"]["edits"].sum())
        assert b >= 10 * a > 0 and (step.want["records"]["anchors"] > 1).sum() >= 10, (step.name, a, b)

    both(Align(cat, "align_host", "real", None, form="host", batch=mbatch, min_length=8),
         Align(cat, "dirty: align_host on reads with ten times the edits", "real", None, form="host", batch=mmany, min_length=6), ten_times_the_edits)

    equal = [(3, 3), (17, 17), (20, 20), (40, 40), (1, 1), (64, 64), (2, 2), (33, 33)] * 14
    equal[20:20] = [(300, 300), (5, 5)]  # two traces in device memory, all '=' too
    equal[90:90] = [(300, 300), (18, 18)]
    equal[50:50] = [(6, 7, 0.3), (20, 18), (3, 3, 0.3), (17, 30)]  # the few reads with edits
    g_step = crafted_reads(equal, 2, empty_every=5, mutate=0.0)
    lopsided = [(1100, 17), (17, 1100), (200, 0), (0, 200)] * 10 + [(1100, 17)] * 10 + [(1, 300), (300, 1), (150, 0)] * 4
    g_dirty = crafted_reads([lopsided[i] for i in rng.permutation(len(lopsided))], 3, mutate=0.5)

    def op_lengths(step):
        e = step.want["entries"]
        return {op: int((e[(e & 15) == op] >> 4).sum()) for op in (OP_EQ, OP_I, OP_D)}, int((e >> 4).sum())

    def other_stride(step, d):  # nearly all '=' at max_fill 512 behind paths of 'I' and 'D' at max_fill 4 096 with 20 traces in device memory
        sg, dg = step.family.seen[step.nreads]["gaps"], d.family.seen[d.nreads]["gaps"]
        assert step.family.params is None and d.family.params == AlignParams(4096)
        far = gc.wave_sized(dg, 4096) & (gc.trace_words(dg) > gc.TRACE_LDS_WORDS)
        assert int(far.sum()) >= 17 > gc.grid_global(4096, d.family.arrays[2].size) == 16 and (dg["edits"] != UNFILLED).all()
        assert int((gc.wave_sized(dg, 4096) & ~far).sum()) >= 10 and int(((dg["a"] == 0) != (dg["b"] == 0)).sum()) >= 20
        assert int((gc.wave_sized(sg, 512) & (gc.trace_words(sg) > gc.TRACE_LDS_WORDS)).sum()) == 2
        (s_ops, s_all), (d_ops, d_all) = op_lengths(step), op_lengths(d)
        assert s_ops[OP_EQ] >= 0.95 * s_all and s_ops[OP_EQ] < s_all and d_ops[OP_I] + d_ops[OP_D] >= 0.5 * d_all, (step.name, s_ops, d_ops)

    def last_read_does_not_fit(step, d):
        seen = step.family.seen[step.nreads]
        lost = (step.want["records"]["ref_start"] == np.uint64(UNALIGNED)) & (seen["reference"]["ref_start"] != np.uint64(UNALIGNED))
        assert seen["op_cap"] == int(seen["ooffs"][-1]) - 1 and lost.sum() == 1 and 0 < step.want["entries"].size <= seen["op_cap"]
        assert int(d.want["op_offsets"][-1]) > 4 * int(seen["ooffs"][-1]) and d.nreads < step.nreads  # other offsets, fewer reads

    add(Cigar(cat, "dirty: cigar_device at max_fill 4 096, traces in device memory, lopsided gaps", "real", g_dirty, AlignParams(4096)), None,
        as_dirtier=True)
    add(Cigar(cat, "cigar_device, max_fill 512, nearly all '='", "real", g_step),
        "dirty: cigar_device at max_fill 4 096, traces in device memory, lopsided gaps", other_stride)
    add(Cigar(cat, "cigar_device, op_capacity short of the last read", "real", g_step, short_ops=True),
        "dirty: cigar_device at max_fill 4 096, traces in device memory, lopsided gaps", last_read_does_not_fit)
    both(Cigar(cat, "cigar_host", "real", None, form="host", batch=mbatch, min_length=8),
         Cigar(cat, "dirty: cigar_host on reads with ten times the edits", "real", None, form="host", batch=mmany, min_length=6),
         ten_times_the_edits)

    for s in list(cat.steps.values()) + list(cat.dirtiers.values()):
        assert s.dirtier is None or s.dirtier in cat.dirtiers, (s.name, s.dirtier)
    return cat


# ---- orders on one handle ----------------------------------------------------------------------------------------------
class Bench:
    """One long-lived handle per index of the catalogue (made on first use), and the streams the device forms rotate over."""
    turn = 0

    def __init__(self, cat, fake=False, clones=False):
        self.cat, self.fake, self.clones = cat, fake, clones
        self.handles, self.sources, self.ran = {}, {}, 0
        self.streams = [None]
        if cat.device_forms:
            self.streams = [torch.cuda.current_stream(), torch.cuda.Stream(), torch.cuda.Stream()]

    def handle(self, index):
        if index not in self.handles:
            ix = self.cat.handle(index)
            if self.clones:  # the steps run on a second query context of the same device; its source stays in use
                self.sources[index] = ix
                ix = ix.clone(0)
            self.handles[index] = ix
        return self.handles[index]

    def next_stream(self, step):
        if step.form != "device":
            return None  # host forms run on the handle's own stream
        Bench.turn += 1  # (the rotation goes on from bench to bench: every order sees all three streams)
        return self.streams[Bench.turn % len(self.streams)]

    def run(self, steps, handles=None):
        """Prepares all of `steps`, then launches them back to back -- nothing waits between one launch and the next, each device
        form on the next stream of the rotation -- then collects and compares them in launch order.  The path of the last step
        launched on each handle is asserted (the library reports its most recent call)."""
        jobs = [s.prepare() for s in steps]
        if self.cat.device_forms:
            torch.cuda.synchronize()  # the caller's own data: inputs uploaded, fences armed
        used = []
        for s, job in zip(steps, jobs):
            ix = handles[s.index] if handles else self.handle(s.index)
            job.launch(ix, self.next_stream(s))
            used.append(ix)
        last = {id(ix): i for i, ix in enumerate(used)}
        for i, (s, job) in enumerate(zip(steps, jobs)):
            compare(s.name, job.collect(), s.want)
            if last[id(used[i])] == i:
                s.check_path(used[i], self.fake)
            self.ran += 1

    def close(self):
        for ix in list(self.handles.values()) + list(self.sources.values()):
            ix.close()
        self.handles, self.sources = {}, {}


def run_fresh(cat, step, fake=False):
    """(a) the step on a handle nothing else has used"""
    b = Bench(cat, fake)
    try:
        b.run([step])
    finally:
        b.close()


def run_pair(cat, step, fake=False):
    """(b) dirtier then step, and step then dirtier, each order on one handle of its own"""
    d = cat.dirtier_of(step)
    for order in ((d, step), (step, d)):
        b = Bench(cat, fake)
        try:
            b.run(list(order))
        finally:
            b.close()


def run_sizes(cat, step, fake=False):
    """(c) large, small, medium on one handle: its scratch exceeds, then falls short of, what a call needs"""
    big, small, medium = step.sizes()
    sized = [step.resize(k) for k in (big, small, medium)]
    assert sized[0].chars > sized[2].chars > sized[1].chars, (step.name, [s.chars for s in sized])  # down, then up again
    b = Bench(cat, fake)
    try:
        for s in sized:
            b.run([s])
    finally:
        b.close()


def run_sequence(cat, seed, fake=False):
    """(d) a seeded permutation of the whole catalogue, every step behind its dirtier or in front of it, on one set of
    handles from start to end; odd seeds run it on same-device clones whose sources take the catalogue's steps, in
    catalogue order, between the clones' (main thread, no second thread).  Returns the number of calls compared."""
    rng = np.random.default_rng(1000 + seed)
    steps = cat.every()
    order = [steps[i] for i in rng.permutation(len(steps))]
    b = Bench(cat, fake, clones=seed % 2 == 1)
    try:
        for i, s in enumerate(order):
            d = cat.dirtier_of(s)
            group = [d, s] if rng.random() < 0.7 else [s, d]
            b.run(group)
            if b.clones:
                other = steps[i % len(steps)]
                b.handle(other.index)
                b.run([other], handles=b.sources)
        return b.ran
    finally:
        b.close()
