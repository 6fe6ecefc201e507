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
from spumoni_amd.docvote import VOTE_DTYPE, votes_reference
from spumoni_amd.mems import MATCH_DTYPE, mems_reference
from tests import cases
from tests.text_lines import _expect, _fill

PML, MS = capi.SPX_MODE_PML, capi.SPX_MODE_MS
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
N = ord("N")
FENCE = 64  # bytes of PATTERN on either side
PATTERN = 0xA5
K, W = 4, 11  # the digestion's (k, w)
N_STEPS = 51  # steps of the catalogue (the tests are parametrised over it before anything is built; build() must give as many)
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
        if not self.native_only and isinstance(family, (Votes, Mems)):
            return  # (the stand-in library of the CPU tier has no votes and no matches)
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
