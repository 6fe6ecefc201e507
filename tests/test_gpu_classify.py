"""-m gpu: the bin-max classifier (spx_class: sum_max_bin_values, bins_above, bins_below) on every path that computes it,
against the oracle's classifier over the ORACLE's lengths, over bin widths 1 .. 2^63 and thresholds 0 .. 2^64 - 1.

The library computes the class records in five places: fused into k_walk_fast (plain PML walk over compact rows; dealt by
lane index, or on demand once a batch has more reads than lanes; with and without out_lengths; 16- and 32-bit), fused into
the state-machine walk k_walk_lanes (general 16-byte rows, fallback reads, SPX_OLD_WALK=1), k_classify_reads and
k_classify_tiles behind the chunked walk (bin_width < 8 / >= 8), and inside k_ms_extend (MS mode with lengths); and it hands
them out through the text path and through digest + query in one call as well.  One test (group) per path, each on the
grid tests/cases.py: CLASSIFY_WIDTHS x classify_thresholds (widths around the 8 values of a 16-byte load, the 64-character
flush word, the tiles of 256 and 512, a read's length, 2^16, 2^32; thresholds 0, 1, median, max, max + 1 and around 2^16,
2^32, 2^64) or on the part of it the docstring names.  tests/test_classify_cpu.py holds the oracle's classifier to the rule
restated in Python integers over the same grid and checks the batch's conditions where no GPU is needed.

The class records are written into a buffer with four records of a pattern in front and behind, which must come back
untouched; the records themselves are set to the pattern before every call, so a record that is not written fails too."""
import numpy as np
import pytest
import torch

from spumoni_amd import capi, synth
from tests import cases

pytestmark = pytest.mark.gpu

W = cases.CLASSIFY_WIDTHS
FENCE = 4
PATTERN = 0x5A5A5A5A5A5A5A5A
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)


class _DeviceRecords:
    """nreads class records in device memory, FENCE records of PATTERN on either side; .out is what the library gets"""

    def __init__(self, nreads):
        self.n = nreads
        self.buf = torch.empty((nreads + 2 * FENCE, 2), dtype=torch.int64, device="cuda")
        self.out = self.buf[FENCE:]  # (16-byte aligned: a record has 16 bytes)

    def arm(self):
        self.buf.fill_(PATTERN)

    def records(self):
        torch.cuda.synchronize()
        h = self.buf.cpu().numpy()
        assert (h[:FENCE] == PATTERN).all() and (h[FENCE + self.n:] == PATTERN).all(), "class records written outside [0, nreads)"
        return h[FENCE: FENCE + self.n].copy().view(capi.CLASS_DTYPE).reshape(-1)


class _HostRecords:
    """the same in host memory, for the host-buffer entry points (capi: class_out)"""

    def __init__(self, nreads):
        self.n = nreads
        self.buf = np.zeros(nreads + 2 * FENCE, dtype=capi.CLASS_DTYPE)
        self.out = self.buf[FENCE:]

    def arm(self):
        self.buf.view(np.uint64)[:] = PATTERN

    def records(self):
        h = self.buf.view(np.uint64).reshape(-1, 2)
        assert (h[:FENCE] == PATTERN).all() and (h[FENCE + self.n:] == PATTERN).all(), "class records written outside [0, nreads)"
        return self.buf[FENCE: FENCE + self.n].copy()


def _hold(oracle_mod, ix, batch, pairs, lengths, run, rec):
    """run(ix, w, thr, rec.out) for every (w, thr) of `pairs`; the records must be oracle.classify(lengths, offs, w, thr),
    `lengths` being the ORACLE's values of `batch` = (seqs, offs), read by read: above, below and sum_max.  Returns the
    records per pair."""
    _, offs = batch
    m = np.diff(np.asarray(offs, dtype=np.int64))
    seen = {}
    for w, thr in pairs:
        rec.arm()
        run(ix, w, thr, rec.out)
        got = rec.records()
        _, a, b, s = oracle_mod.classify(lengths, offs, w, thr)
        bad = np.flatnonzero((got["above"] != a) | (got["below"] != b) | (got["sum_max"] != s))
        if bad.size:
            q = int(bad[0])
            raise AssertionError(f"bin_width {w}, max_value_thr {thr}: {bad.size} of {m.size} reads differ; read {q} of {int(m[q])} "
                                 f"values: got above / below / sum {int(got['above'][q])} / {int(got['below'][q])} / "
                                 f"{int(got['sum_max'][q])}, oracle {int(a[q])} / {int(b[q])} / {int(s[q])}")
        seen[(w, thr)] = got
    return seen


def _pml_device(d_seqs, d_offs, total, bits, with_lengths, chunked):
    """spx_query_batch_device[16] in PML mode; after every call: the chunked walk ran, or did not"""
    d_len = torch.empty(total + 8, dtype=torch.int16 if bits == 16 else torch.int32, device="cuda") if with_lengths else None

    def run(ix, w, thr, d_cls):
        ix.query_device(capi.SPX_MODE_PML, d_seqs, d_offs, total, d_lengths=d_len, d_class=d_cls, bin_width=w, max_value_thr=thr,
                        narrow=bits == 16)
        torch.cuda.synchronize()
        assert (ix.last_chunk_stats()["chunk_len"] != 0) == chunked

    return run


def _on_device(seqs, offs):
    return capi.pad_seqs(torch.from_numpy(seqs).cuda()), torch.from_numpy(np.asarray(offs, dtype=np.int64)).cuda(), int(offs[-1])


@pytest.fixture(scope="module")
def case(oracle_mod):
    """The index (text, SA samples, documents), the batch, the oracle's PML and MS lengths of it, the grid's thresholds for
    either, and the conditions the batch has to meet (tests/cases.py: classify_conditions)."""
    raw, text, seqs, offs = cases.classify_case()
    orc = oracle_mod.OracleIndex.from_raw(raw)
    c = dict(raw=raw, text=text, seqs=seqs, offs=offs, orc=orc, pml=orc.pml(seqs, offs), ms=orc.ms(seqs, offs, text=text)["lengths"])
    for key in ("pml", "ms"):
        cases.classify_conditions(oracle_mod, c[key], offs)
        c["T_" + key], c["med_" + key], _ = cases.classify_thresholds(c[key])
    return c


def _grid(widths, thresholds):
    return [(w, t) for w in widths for t in thresholds]


# ---- 1. k_walk_fast, dealt by lane index ---------------------------------------------------------------------------
def test_walk_fast_dealt_by_lane(oracle_mod, case):
    """Plain PML walk over compact rows ("chunk_mode" 1: never chunked; fewer reads than lanes, so every lane has one read
    or none): the whole grid through spx_query_batch_device and _device16, with d_lengths and with the classes alone -- four
    forms of the kernel, which must also agree among themselves."""
    ix = capi.Index.from_raw(case["raw"], 0)
    ix.set_option("chunk_mode", 1)
    assert ix.describe()["compact_rows"] == 1
    batch = (case["seqs"], case["offs"])
    d_seqs, d_offs, total = _on_device(*batch)
    rec = _DeviceRecords(case["offs"].size - 1)
    pairs = _grid(W, case["T_pml"])
    seen = [_hold(oracle_mod, ix, batch, pairs, case["pml"], _pml_device(d_seqs, d_offs, total, bits, with_lengths, False), rec)
            for bits in (32, 16) for with_lengths in (True, False)]
    for other in seen[1:]:
        assert all(np.array_equal(other[p], seen[0][p]) for p in pairs)


# ---- 1b. k_walk_fast, dealt on demand ------------------------------------------------------------------------------
def test_walk_fast_dealt_on_demand(oracle_mod, case):
    """More reads than lanes ("waves_per_cu" 4: one block of 256 threads per CU; lanes + 2 * 64 + 5 reads of 0 .. 40
    characters, two in three cut from the indexed text): after the first round the wavefronts claim reads from a counter and
    hand them to the lanes that end one, and a lane's bin state is set up anew for every read it is handed.  Nothing reports
    the deal: launch_lanes chooses it for a plain k_walk_fast launch whose reads outnumber the resident lanes.  Widths 1, 7,
    64 and 2^32 + 1, thresholds 1 and the median; the oracle's PML runs once."""
    text = case["text"]
    nlanes = torch.cuda.get_device_properties(0).multi_processor_count * 256
    n = nlanes + 2 * 64 + 5
    rng = np.random.default_rng(41)
    m = rng.integers(0, 41, size=n)
    m[nlanes - 70: nlanes + 70: 3] = 0  # (empty reads where the deal changes hands)
    offs = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
    seqs = DNA[rng.integers(0, 4, size=int(offs[-1]))]
    starts = rng.integers(0, text.size - 40, size=n)
    for q in range(n):
        if q % 3 == 0:
            continue
        seqs[offs[q]: offs[q + 1]] = text[starts[q]: starts[q] + m[q]]
    want = case["orc"].pml(seqs, offs)
    _, med, _ = cases.classify_thresholds(want)
    _, a, b, _ = oracle_mod.classify(want, offs, 7, med)
    assert med > 1 and ((a > 0) & (b > 0)).any() and ((a + b > 1) & (m % 7 != 0)).any()
    ix = capi.Index.from_raw(case["raw"], 0)
    ix.set_option("waves_per_cu", 4)
    ix.set_option("chunk_mode", 1)
    assert ix.describe()["compact_rows"] == 1 and n > nlanes
    d_seqs, d_offs, total = _on_device(seqs, offs)
    rec = _DeviceRecords(n)
    pairs = _grid([1, 7, 64, (1 << 32) + 1], [1, med])
    seen = [_hold(oracle_mod, ix, (seqs, offs), pairs, want, _pml_device(d_seqs, d_offs, total, bits, with_lengths, False), rec)
            for bits, with_lengths in ((32, True), (16, True), (32, False))]
    for other in seen[1:]:
        assert all(np.array_equal(other[p], seen[0][p]) for p in pairs)


# ---- 2. k_walk_lanes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 16])
def test_state_machine_walk_on_general_rows(oracle_mod, case, bits, monkeypatch):
    """The same index flattened into the general 16-byte rows (SPX_ROWS_WIDE=1), which only k_walk_lanes walks: the whole
    grid.  (tests/test_gpu_old_walk.py runs this module with SPX_OLD_WALK=1, where k_walk_lanes takes the compact rows of
    every other test here as well.)"""
    monkeypatch.setenv("SPX_ROWS_WIDE", "1")
    ix = capi.Index.from_raw(case["raw"], 0)
    assert ix.describe()["compact_rows"] == 0
    batch = (case["seqs"], case["offs"])
    d_seqs, d_offs, total = _on_device(*batch)
    rec = _DeviceRecords(case["offs"].size - 1)
    _hold(oracle_mod, ix, batch, _grid(W, case["T_pml"]), case["pml"], _pml_device(d_seqs, d_offs, total, bits, True, False), rec)


# ---- 3. / 4. k_classify_reads, k_classify_tiles behind the chunked walk ----------------------------------------------
@pytest.fixture(scope="module")
def long_case(case):
    """24 reads of 1000 .. 2200 characters for the chunked walk: every third of random letters, the others cut from the text
    with a substitution every 150 characters and a stretch of random letters"""
    rng = np.random.default_rng(43)
    text = case["text"]
    reads = []
    for q in range(24):
        m = int(rng.integers(1000, 2201)) if q > 1 else (1000, 2200)[q]
        rd = DNA[rng.integers(0, 4, size=m)]
        if q % 3:
            s = int(rng.integers(0, text.size - m))
            rd = text[s: s + m].copy()
            rd[rng.integers(0, m, size=m // 150)] = DNA[rng.integers(0, 4, size=m // 150)]
            at = int(rng.integers(0, m - 300))
            rd[at: at + 300] = DNA[rng.integers(0, 4, size=300)]
        reads.append(rd)
    offs = np.concatenate([[0], np.cumsum([r.size for r in reads])]).astype(np.int64)
    seqs = np.concatenate(reads)
    return seqs, offs, case["orc"].pml(seqs, offs)


@pytest.mark.parametrize("bits", [32, 16])
def test_classifier_kernels_behind_the_chunked_walk(oracle_mod, case, long_case, bits):
    """"chunk_mode" 2 and chunks of 128 characters: the walk writes the lengths, k_classify_reads (bin_width < 8) or
    k_classify_tiles (>= 8) reads them back.  test_gpu_chunked.py sweeps the widths up to 5000 at thresholds 1 and 5; here
    7 and 8 (either side of the switch) and every width of the grid from 65535 on, against every threshold.  Reads in which a
    seam stays open are walked again by k_walk_lanes, which writes their records anew: at most the reads cut from the text
    (the random ones reset every few characters), so the records of the others are the classifier kernels'."""
    seqs, offs, want = long_case
    cases.classify_conditions(oracle_mod, want, offs)
    T, _, _ = cases.classify_thresholds(want)
    ix = capi.Index.from_raw(case["raw"], 0)
    ix.set_option("chunk_mode", 2)
    ix.set_option("chunk_len", 128)
    assert ix.describe()["compact_rows"] == 1
    d_seqs, d_offs, total = _on_device(seqs, offs)
    rec = _DeviceRecords(offs.size - 1)
    pairs = _grid([7, 8] + [w for w in W if w >= 65535], T)
    _hold(oracle_mod, ix, (seqs, offs), pairs, want, _pml_device(d_seqs, d_offs, total, bits, True, True), rec)
    cs = ix.last_chunk_stats()
    assert cs["chunk_len"] == 128 and cs["fallback_reads"] <= sum(1 for q in range(offs.size - 1) if q % 3)


# ---- 5. k_ms_extend ------------------------------------------------------------------------------------------------
def _ms_host(bits):
    def run(ix, w, thr, cls):
        ix.query_host(capi.SPX_MODE_MS, run.seqs, run.offs, want_lengths=True, classify=(w, thr), bits=bits, class_out=cls)

    return run


@pytest.mark.parametrize("bits", [32, 16])
def test_ms_extension(oracle_mod, case, bits):
    """SPX_MODE_MS with lengths on an index that holds its text: k_ms_extend computes the MS lengths over ascending indices
    and the class records with them (whenever out_lengths and out_class are given in MS mode: nothing else does).  The whole
    grid through spx_query_batch / _batch16; the lengths go through the narrow or the staged store (every read < 65536)."""
    ix = capi.Index.from_raw(case["raw"], 0)
    run = _ms_host(bits)
    run.seqs, run.offs = case["seqs"], case["offs"]
    rec = _HostRecords(case["offs"].size - 1)
    _hold(oracle_mod, ix, (case["seqs"], case["offs"]), _grid(W, case["T_ms"]), case["ms"], run, rec)


def test_ms_extension_unstaged_lengths(oracle_mod, case):
    """One read of 70 000 characters (cut from a tiled copy of the text) behind the batch: a read of 65536 values or more
    stores its lengths one by one.  Widths 1, 64, 65536, the read's length and its neighbours, 2^32 + 1; thresholds 0,
    the median, max + 1 and 2^32."""
    text = case["text"]
    big = np.tile(text, 70000 // text.size + 2)[1234: 1234 + 70000]
    seqs = np.concatenate([case["seqs"], big])
    offs = np.concatenate([case["offs"], [case["offs"][-1] + big.size]]).astype(np.int64)
    want = case["orc"].ms(seqs, offs, text=text)["lengths"]
    _, med, mx = cases.classify_thresholds(want)
    ix = capi.Index.from_raw(case["raw"], 0)
    run = _ms_host(32)
    run.seqs, run.offs = seqs, offs
    rec = _HostRecords(offs.size - 1)
    pairs = _grid([1, 64, 65536, 69999, 70000, 70001, (1 << 32) + 1], [0, med, mx + 1, 1 << 32])
    seen = _hold(oracle_mod, ix, (seqs, offs), pairs, want, run, rec)
    last = seen[(64, med)][-1]
    assert last["above"] + last["below"] == 70000 // 64 and last["above"] > 0 and last["below"] > 0
    assert np.array_equal(ix.query_host(capi.SPX_MODE_MS, seqs, offs)["lengths"], want)


# ---- the composite entry points --------------------------------------------------------------------------------------
COMPOSITE_W = [1, 64, 150, (1 << 32) + 1]


@pytest.mark.parametrize("mode", [capi.SPX_MODE_PML, capi.SPX_MODE_MS])
def test_text_path(oracle_mod, case, mode):
    """spx_query_text_begin with out_class, _fetch: the class records travel with the text of the output files.  PML (the
    walk's classifier) and MS (k_ms_extend's); widths 1, 64, 150, 2^32 + 1, thresholds 0, the median, 2^32.  Nothing is forced:
    the batch is too small for the chunked walk to be chosen, which the chunk statistics confirm."""
    pml = mode == capi.SPX_MODE_PML
    want, med = (case["pml"], case["med_pml"]) if pml else (case["ms"], case["med_ms"])
    ix = capi.Index.from_raw(case["raw"], 0)
    streams = capi.SPX_TEXT_LENGTHS | (0 if pml else capi.SPX_TEXT_POINTERS)
    offs = case["offs"]
    first = b"".join(b"%d " % int(v) for v in want[offs[3]: offs[4]]) + b"\n"  # (reads 0 .. 2 are empty)

    def run(ix, w, thr, cls):
        got = ix.query_text(mode, case["seqs"], offs, None, streams, classify=(w, thr), class_out=cls)
        assert got["text"][0].startswith(b"\n\n\n" + first)
        assert ix.last_chunk_stats()["chunk_len"] == 0

    _hold(oracle_mod, ix, (case["seqs"], offs), _grid(COMPOSITE_W, [0, med, 1 << 32]), want, run, _HostRecords(offs.size - 1))


@pytest.mark.parametrize("kind", [capi.SPX_DIGEST_PROMOTED, capi.SPX_DIGEST_DNA])
def test_digest_and_query_in_one_call(oracle_mod, kind):
    """spx_digest_query_batch (run -m / -a): reads are digested on the device and walked in the same call; the bins are
    bins of the DIGESTED read, so the expected records are the oracle's over the oracle's digestion and its offsets.  PML and
    MS with lengths; widths 1, 64, 150, 2^32 + 1, thresholds 0, the median, 2^32."""
    rng = np.random.default_rng(50 + kind)
    genome = cases.repetitive_text(rng, 12000, list(b"ACGT"))
    k, w = 4, 11
    dtext = oracle_mod.digest(kind, k, w, genome)
    raw = synth.index_from_text(torch.from_numpy(dtext.copy()), doc_lengths=[dtext.size // 2, dtext.size - dtext.size // 2])
    orc = oracle_mod.OracleIndex.from_raw(raw)
    m = rng.integers(0, 1500, size=60)
    m[:8] = [0, 0, 1, k - 1, k, w + k - 2, w + k - 1, 1499]
    reads = []
    for q, ln in enumerate(m):
        s = int(rng.integers(0, genome.size - 1500))
        rd = genome[s: s + ln].copy() if q % 3 else DNA[rng.integers(0, 4, size=ln)]
        rd[rng.random(ln) < 0.01] = ord("N")
        reads.append(rd)
    seqs = np.concatenate(reads).astype(np.uint8)
    offs = np.concatenate([[0], np.cumsum(m)]).astype(np.uint64)
    dseqs, doffs = oracle_mod.digest_batch(kind, k, w, seqs, offs)
    doffs = doffs.astype(np.int64)
    ix = capi.Index.from_raw(raw, 0)
    for mode in (capi.SPX_MODE_PML, capi.SPX_MODE_MS):
        want = orc.pml(dseqs, doffs) if mode == capi.SPX_MODE_PML else orc.ms(dseqs, doffs, text=dtext)["lengths"]
        _, med, mx = cases.classify_thresholds(want)
        _, a, b, _ = oracle_mod.classify(want, doffs, 64, med)
        assert 0 < med < mx and (a + b > 1).any() and a.any() and b.any()

        def run(ix, bw, thr, cls):
            got = ix.digest_query_host(mode, kind, k, w, seqs, offs, classify=(bw, thr), class_out=cls)
            assert np.array_equal(got["offsets"].astype(np.int64), doffs)

        _hold(oracle_mod, ix, (dseqs, doffs), _grid(COMPOSITE_W, [0, med, 1 << 32]), want, run, _HostRecords(offs.size - 1))
