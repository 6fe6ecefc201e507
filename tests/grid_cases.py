"""The batches of tests/test_gpu_full_grids.py and tests/test_full_grid_cases_cpu.py: shapes at which a wavefront of the chain,
place, align and cigar kernels does a second unit of work, each with its expectation.

Every one of these kernels caps its grid and loops above the cap (spx_chain.hip: 4096 blocks and chunk_reads; spx_place.hip:
8192 blocks and a grid stride; spx_align.hip / spx_cigar.hip: min(gap_capacity, 4096) wavefronts over the listed gaps, fewer
for the traces in device memory; 1024 blocks in the reduction and the plan).  A case is built from a seed, needs neither a
device nor the library, and carries

    want       what chain_reference, place_reference, align_reference and cigar_reference give for it -- nothing else;
    reaches()  assertions, on the reference's answer alone, that the batch is in the regime it exists for;
    cells      the table cells the references filled (align.py: `count`), seconds: what they took.

Cases are built once per process (case(name)) and nothing changes them afterwards.  A case stays at or below MAX_CELLS table
cells: 1.76e6 cells took align_reference 1.1 s and cigar_reference 2.4 s, 1.9e7 took 9.6 s and 16 s.
"""
import time

import numpy as np

from spumoni_amd.align import UNALIGNED, UNFILLED, AlignParams, align_reference
from spumoni_amd.chain import ChainParams, chain_reference
from spumoni_amd.cigar import OP_D, OP_EQ, OP_I, OP_X, cigar_reference
from spumoni_amd.mems import MATCH_DTYPE, mems_reference
from spumoni_amd.place import UNPLACED, place_reference
from tests.test_gpu_align import LETTERS, N_TEXT, RUN_A, Batch

MAX_CELLS = 3_000_000
MAX_SECONDS = 30.0  # per case, for all of its references: ten times what MAX_CELLS cost where the figures above were taken
LANE_MAX = 16  # sides up to this are one lane's table
TRACE_LDS_WORDS = 2048  # a * ceil(b / 16) words up to this are traced in LDS
TRACE_BUDGET = 64 << 20

_TEXT = []


def text():
    """The text of tests/test_gpu_align.py: 2 000 000 random letters with a run of 'A'."""
    if not _TEXT:
        t = LETTERS[np.random.default_rng(100).integers(0, 4, N_TEXT)].copy()
        t[RUN_A:RUN_A + 5000] = ord("A")
        t.setflags(write=False)
        _TEXT.append(t)
    return _TEXT[0]


class Case:
    def __init__(self, name, **kw):
        self.name, self.cells, self.seconds = name, 0, 0.0
        self.__dict__.update(kw)


def _timed(case, fn, *args, **kw):
    t0 = time.perf_counter()
    out = fn(*args, **kw)
    case.seconds += time.perf_counter() - t0
    return out


# ---- 1. chain: chunk_reads 4 / 4 / 8 / 8 / 12 ---------------------------------------------------------------------------
CHAIN_SIZES = {65_535: 4, 65_536: 4, 65_537: 8, 131_072: 8, 131_073: 12}  # nreads -> chunk_reads = 4 * ceil(nreads / 65536)


def chain_batch(rng, counts, front=0, step=40, spread=3, y0=1000, n_docs=0):
    """tests/test_gpu_chain.py's _batch without its loop over the reads: anchors that mostly follow a diagonal with small
    indels, some out of order, some overlapping, half of the lengths equal; `front` records in front and 3 behind."""
    counts = np.asarray(counts, dtype=np.int64)
    offs = front + np.r_[0, np.cumsum(counts)]
    n, tot = int(offs[-1]) + 3, int(counts.sum())
    x, y, l = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), rng.integers(1, 60, n)
    l[rng.random(n) < 0.5] = 20
    read_of = np.repeat(np.arange(counts.size), counts)
    xs = rng.integers(0, step * np.maximum(counts[read_of], 1))
    xs = xs[np.lexsort((xs, read_of))]  # sorted inside every read
    drift = np.cumsum(rng.integers(-spread, spread + 1, tot))
    start = offs[:-1][read_of] - front  # the read's first anchor among the batch's
    drift = drift - np.r_[0, drift][start]
    ys = y0 + rng.integers(0, 1000, counts.size)[read_of] + xs + drift
    swap = rng.random(tot) < 0.08
    ys[swap] = y0 + rng.integers(0, 3000, int(swap.sum()))
    x[front:front + tot], y[front:front + tot] = xs, ys
    rec = np.zeros(n, dtype=MATCH_DTYPE)
    rec["read_pos"], rec["ref_pos"], rec["length"] = x, y, l
    return offs.astype(np.uint64), rec, (rng.integers(0, n_docs, n) if n_docs else None)


def _chain_case(nreads):
    rng = np.random.default_rng(nreads)
    chunk = 4 * -(-nreads // 65_536)
    counts = rng.integers(0, 7, nreads)
    trip = chunk * 1000 + 4  # the first quad of a chunk's second trip where a chunk is more than one quad
    planted = {trip: 200, 20_000: 17, 20_001: 64}  # (20 000 and 20 001: two reads of one quad)
    if nreads > 65_536:
        planted[65_536] = 65
    planted[nreads - 1] = 200  # (of 65 537 reads the last one is read 65 536)
    for q, h in planted.items():
        counts[q] = h
    docs = nreads == 65_537
    c = Case(f"chain {nreads}", product="chain", nreads=nreads, chunk=chunk, planted=planted, table=True)
    c.offs, c.rec, c.D = chain_batch(rng, counts, front=nreads % 3, n_docs=3 if docs else 0)
    if docs:  # nine anchors in ten carry their read's id, the others break the chains
        lo, hi = int(c.offs[0]), int(c.offs[-1])
        c.D[lo:hi] = np.where(rng.random(hi - lo) < 0.9, np.repeat(np.arange(nreads), counts) % 3, c.D[lo:hi])
    c.count = [0]
    c.want = _timed(c, chain_reference, c.offs, c.rec, None, c.D, count=c.count)

    def reaches():
        chains = c.want[0]
        assert chunk == CHAIN_SIZES[nreads] and (chunk // 4 - 1) * 65_536 < nreads <= (chunk // 4) * 65_536
        assert chunk == 4 or trip % chunk == 4  # the second trip of wavefront 1000
        assert 20_000 // 4 == 20_001 // 4
        anchors = np.diff(c.offs.astype(np.int64))
        assert all(int(anchors[q]) == h for q, h in planted.items())
        assert int(chains["anchors"][nreads - 1]) > 64 and int(chains["anchors"][trip]) > 64  # the ring wrapped inside one chain
        assert int(chains["anchors"][20_001]) > 16 and (nreads <= 65_536 or int(chains["anchors"][65_536]) > 16)
        assert int(chains["anchors"][20_000]) >= 2
        assert (anchors[anchors <= 6] >= 0).all() and int((anchors > 6).sum()) == len(planted)

    c.reaches = reaches
    return c


# ---- 2. place: one, two and three trips of the grid ---------------------------------------------------------------------
PLACE_SIZES = {131_072: (16, 1, 70_001), 131_073: (32, 2, 131_072), 262_145: (16, 3, 200_001)}  # nreads -> (bits, trips, the long read)
MIN_SEED = 6


def place_batch(rng, T, lens, seeded, front, min_seed=MIN_SEED):
    """Reads of lens[q] values whose lengths all lie below min_seed, but for the reads in `seeded` (each at least min_seed
    long): those lie on a diagonal of the text with a substitution in twenty characters, pointers on the diagonal, and have
    one exact seed of min_seed .. 60 values that ends inside the read.  `front` values in front of the batch, 9 behind."""
    offs = (front + np.r_[0, np.cumsum(lens)]).astype(np.uint64)
    tot = int(offs[-1]) + 9
    R = LETTERS[rng.integers(0, 4, tot)]
    L = rng.integers(0, min_seed, tot)  # below min_seed: a read is placed only where a seed is planted
    P = rng.integers(0, T.size, tot).astype(np.uint64)
    D = rng.choice([0, 1, 255, 256, 65535], size=tot)
    for q in np.asarray(seeded).tolist():
        o, m = int(offs[q]), int(lens[q])
        d = int(rng.integers(0, T.size - m))
        s = int(rng.integers(0, m - min_seed + 1))
        sl = int(rng.integers(min_seed, min(m - s, 60) + 1))
        keep = rng.random(m) >= 0.05
        keep[s:s + sl] = True  # a seed is an exact match
        R[o:o + m] = np.where(keep, T[d:d + m], R[o:o + m])
        P[o:o + m] = d + np.arange(m)
        L[o + s] = sl
    return R, L, P, D, offs


def _place_case(nreads):
    bits, trips, long_q = PLACE_SIZES[nreads]
    rng = np.random.default_rng(nreads)
    T = text()
    lens = rng.integers(0, 12, nreads)
    must = [q for q in (nreads - 4, nreads - 3, nreads - 2, nreads - 1, 131_072) if q < nreads and q != long_q]
    lens[must] = rng.integers(MIN_SEED, 12, len(must))
    lens[long_q] = 2500  # more than 2048 values: the whole wavefront
    seeded = np.flatnonzero((lens >= MIN_SEED) & (rng.random(nreads) < 6000 / nreads))  # (half of the reads are that long)
    seeded = np.union1d(seeded, must + [long_q])
    R, L, P, D, offs = place_batch(rng, T, lens, seeded, 5)
    c = Case(f"place {nreads}", product="place", nreads=nreads, bits=bits, R=R, L=L, P=P, D=D, offs=offs, params=(MIN_SEED, 4, 16))
    c.want = _timed(c, place_reference, R, L, P, offs, T, *c.params, docs=D)

    def reaches():
        assert -(-nreads // 131_072) == trips and int(lens[long_q]) > 2048 and (trips == 1 or long_q >= 131_072)
        ok = c.want["ref_start"] != np.uint64(UNPLACED)
        assert ok[must].all() and ok[long_q] and ok[nreads - 4:].all()
        assert np.array_equal(np.flatnonzero(ok), seeded) and 2000 < seeded.size < 4000
        assert int(lens[lens <= 11].max()) == 11 and int((lens > 11).sum()) == 1

    c.reaches = reaches
    return c


# ---- 3 .. 6: align and cigar on crafted chains --------------------------------------------------------------------------
def wave_sized(gaps, max_fill):
    """The gaps of a table that k_fill_small / k_trace_small hand to a wavefront."""
    a, b = gaps["a"].astype(np.int64), gaps["b"].astype(np.int64)
    return (a >= 1) & (b >= 1) & (a <= max_fill) & (b <= max_fill) & ((a > LANE_MAX) | (b > LANE_MAX))


def trace_words(gaps):
    return gaps["a"].astype(np.int64) * ((gaps["b"].astype(np.int64) + 15) // 16)


def path_words(gaps, max_fill):
    """Words of path the filled gaps with a table need: ceil((a + b) / 16) each (include/spumoni_cigar.h)."""
    a, b = gaps["a"].astype(np.int64), gaps["b"].astype(np.int64)
    tabled = (a >= 1) & (b >= 1) & (a <= max_fill) & (b <= max_fill) & ~((a == 1) & (b == 1))
    return int(((a + b + 15) // 16)[tabled].sum())


def grid_global(max_fill, cap):
    """Wavefronts of the launch that traces in device memory (spx_cigar.hip: cigar_reserve)."""
    return max(min(max(TRACE_BUDGET // (4 * max_fill * ((max_fill + 15) // 16)), 1), 4096, cap), 1)


def _references(c, cigar=True):
    """align_reference and (cigar) cigar_reference of c.arrays at c.params, timed; the cells from the gap table."""
    R, roffs, rec, moffs, chains, pred = c.arrays
    T = text()
    c.count = [0]
    c.align = _timed(c, align_reference, R, roffs, T, moffs, rec, chains, pred, c.params, count=c.count)
    c.cells = c.count[0]
    c.cigar = _timed(c, cigar_reference, R, roffs, T, moffs, rec, chains, pred, c.params) if cigar else None
    c.path_words = path_words(c.align[2], (c.params or AlignParams()).max_fill)
    return c


def _reads_of(rng, shapes, per_read, front=0):
    """A Batch whose reads take `per_read` of the gap shapes each, in the order given, at random places of the text."""
    B = Batch(front=front)
    T = text()
    for i in range(0, len(shapes), per_read):
        B.add(T, rng, int(rng.integers(0, 1_900_000 - 600 * per_read)), [tuple(s) for s in shapes[i:i + per_read]])
    return B


SMALL_WAVE = [(17, 1), (1, 17), (17, 2), (18, 18), (24, 17)]
LARGE_WAVE = [(64, 65), (65, 64), (129, 20), (20, 129), (128, 16)]
DEVICE_TRACE = [(129, 241), (121, 257), (257, 129)]  # the smallest gaps with a * ceil(b / 16) > 2048
DEVICE_TRACE_MORE = [(300, 200), (513, 65)]


def _wave_case():
    rng = np.random.default_rng(3)
    n = 8600
    shapes = [SMALL_WAVE[i] for i in rng.integers(0, len(SMALL_WAVE), n)]
    for i in rng.choice(n, n // 50, replace=False):  # the sizes in random order along the reads
        shapes[i] = LARGE_WAVE[int(rng.integers(0, len(LARGE_WAVE)))]
    c = Case("every wavefront fills two gaps", product="align+cigar", params=None, cap=None)
    c.arrays = _reads_of(rng, shapes, 10, front=2).arrays()
    _references(c)

    def reaches():
        gaps = c.align[2]
        wave = wave_sized(gaps, 512) & (gaps["edits"] != UNFILLED)
        assert int(wave.sum()) >= 8192 + 100 and wave.all()  # two trips for each of the 4096 wavefronts
        assert int((wave & (gaps["a"].astype(np.int64) * gaps["b"] >= 2048)).sum()) >= 100
        assert int(trace_words(gaps).max()) <= TRACE_LDS_WORDS  # cigar traces all of them in LDS
        assert c.arrays[2].size > gaps.size  # gap_capacity (the number of records) is generous

    c.reaches = reaches
    return c


def _trace_case(max_fill, n):
    rng = np.random.default_rng(max_fill)
    shapes = [DEVICE_TRACE[i % 3] for i in range(n - 8)] + DEVICE_TRACE_MORE * 4
    shapes = [shapes[i] for i in rng.permutation(n)]
    c = Case(f"device-memory traces reused, max_fill {max_fill}", product="cigar", params=AlignParams(max_fill), cap=None)
    c.arrays = _reads_of(rng, shapes, 4).arrays()
    _references(c)

    def reaches():
        gaps = c.align[2]
        far = wave_sized(gaps, max_fill) & (trace_words(gaps) > TRACE_LDS_WORDS) & (gaps["edits"] != UNFILLED)
        grid = grid_global(max_fill, c.arrays[2].size)
        assert grid == {4096: 16, 2048: 64}[max_fill] and int(far.sum()) == n > grid
        assert {int(e) & 15 for e in c.cigar[2]} == {OP_EQ, OP_X, OP_I, OP_D}

    c.reaches = reaches
    return c


def _ends_case(n_lds, n_dev):
    rng = np.random.default_rng(100 * n_lds + n_dev)
    lds = [(64, 65), (129, 20), (17, 2), (24, 17), (1, 17)]
    shapes = [lds[i % len(lds)] for i in range(n_lds)] + [DEVICE_TRACE[i % 3] for i in range(n_dev)]
    shapes = [shapes[i] for i in rng.permutation(len(shapes))]
    c = Case(f"the list's two ends meet, {n_lds} + {n_dev}", product="align+cigar", params=None, cap=n_lds + n_dev)
    c.arrays = _reads_of(rng, shapes, 5).arrays()
    _references(c)

    def reaches():
        gaps = c.align[2]
        wave = wave_sized(gaps, 512) & (gaps["edits"] != UNFILLED)
        far = trace_words(gaps) > TRACE_LDS_WORDS
        assert gaps.size == c.cap == int(c.align[1][-1]) and wave.all()  # total == cap, every gap on a list
        assert (int((wave & ~far).sum()), int((wave & far).sum())) == (n_lds, n_dev)
        return n_lds, n_dev

    c.reaches = reaches
    return c


REDUCE_SIZES = [262_144, 262_145, 262_400]


def _reduce_case(nreads, cap=None, name=None):
    """Nearly all reads without anchors; about 200 chained with small gaps, some among the first 256 reads, and the last."""
    rng = np.random.default_rng(nreads)
    T = text()
    chained = set(rng.choice(nreads, min(190, nreads // 4), replace=False).tolist()) | {0, 3, 63, 64, 200, 255, nreads - 1}
    B = Batch(front=nreads % 3)
    for q in range(nreads):
        if q in chained:
            h = int(rng.integers(1, 7))
            B.add(T, rng, int(rng.integers(0, 1_900_000)), [(int(a), int(b)) for a, b in rng.integers(0, 24, (h - 1, 2))])
        else:
            B.add_empty(1)
    c = Case(name or f"reduce and plan over {nreads} reads", product="align+cigar", params=None, cap=cap, nreads=nreads)
    c.arrays = B.arrays()
    _references(c)

    def reaches():
        want, goffs, gaps = c.align
        ok = np.flatnonzero(want["ref_start"] != np.uint64(UNALIGNED))
        assert sorted(chained) == ok.tolist() and ok[0] == 0 and ok[-1] == nreads - 1 and (ok < 256).sum() >= 6
        assert int((gaps["edits"] != UNFILLED).sum()) == gaps.size > 100 and c.cells > 0
        if cap is None:
            assert nreads >= 262_144  # 1024 blocks of 256 lanes
        else:
            assert cap + 1 > 262_144 > nreads and cap > gaps.size  # the plan's span is cap + 1

    c.reaches = reaches
    return c


# ---- 7. the host forms past the chain cap --------------------------------------------------------------------------------
HOST_READS, HOST_MIN_LENGTH, HOST_MIN_SEED = 70_000, 12, 30


def host_batch():
    """A text of 100 000 random letters and 70 000 reads of 36 .. 44 characters cut from it: a third exact, a third with one
    substitution in the middle, a sixth with one character of the text left out and a sixth with two substitutions."""
    rng = np.random.default_rng(7)
    T = LETTERS[rng.integers(0, 4, 100_000)].copy()
    lens = rng.integers(36, 45, HOST_READS)
    at = rng.integers(0, T.size - 50, HOST_READS)
    offs = np.r_[0, np.cumsum(lens)].astype(np.uint64)
    read_of = np.repeat(np.arange(HOST_READS), lens)
    pos = np.arange(int(offs[-1])) - offs[:-1].astype(np.int64)[read_of]
    kind = rng.integers(0, 6, HOST_READS)
    mid = lens // 2
    skip = (kind[read_of] == 2) & (pos >= mid[read_of])  # a character of the text left out
    seqs = T[at[read_of] + pos + skip].copy()
    other = np.zeros(256, dtype=np.uint8)
    other[LETTERS] = np.roll(LETTERS, 1)
    for k, where in ((1, mid), (3, mid), (4, mid - 9), (4, mid + 8)):  # the substitutions
        i = offs[:-1].astype(np.int64)[kind == k] + where[kind == k]
        seqs[i] = other[seqs[i]]
    return T, seqs, offs


def host_expectation(oracle_mod, raw, T, seqs, offs):
    """Oracle MS -> mems_reference -> chain_reference -> align_reference / cigar_reference, and place_reference."""
    c = Case("host forms on 70 000 reads", product="host", nreads=HOST_READS)
    ms = _timed(c, oracle_mod.OracleIndex.from_raw(raw).ms, seqs, offs, want_docs=False, text=T)
    c.m = _timed(c, mems_reference, ms["lengths"], ms["pointers"], offs, HOST_MIN_LENGTH, None)
    c.chain_count, c.count = [0], [0]
    c.chains, _, c.pred = _timed(c, chain_reference, c.m[0], c.m[1], None, None, count=c.chain_count)
    c.align = _timed(c, align_reference, seqs, offs, T, c.m[0], c.m[1], c.chains, c.pred, None, count=c.count)
    c.cigar = _timed(c, cigar_reference, seqs, offs, T, c.m[0], c.m[1], c.chains, c.pred, None)
    c.place = _timed(c, place_reference, seqs, ms["lengths"], ms["pointers"], offs, T, HOST_MIN_SEED)
    c.cells = c.count[0]

    def reaches():
        assert 4 * -(-HOST_READS // 65_536) == 8  # chunk_reads
        assert int((c.chains["anchors"] >= 2).sum()) > HOST_READS // 3 and int((c.align[2]["edits"] != UNFILLED).sum()) > HOST_READS // 3
        placed = int((c.place["ref_start"] != np.uint64(UNPLACED)).sum())
        assert HOST_READS // 4 < placed < HOST_READS
        assert {int(e) & 15 for e in c.cigar[2]} >= {OP_EQ, OP_X, OP_D}

    c.reaches = reaches
    return c


# ---- the table ------------------------------------------------------------------------------------------------------------
BUILDERS = {}
for _n in CHAIN_SIZES:
    BUILDERS[f"chain-{_n}"] = (_chain_case, _n)
for _n in PLACE_SIZES:
    BUILDERS[f"place-{_n}"] = (_place_case, _n)
BUILDERS["wave-two-gaps"] = (_wave_case,)
BUILDERS["trace-4096"] = (_trace_case, 4096, 48)
BUILDERS["trace-2048"] = (_trace_case, 2048, 70)
ENDS = [(20, 20), (40, 0), (0, 40), (1, 0)]
for _a, _b in ENDS:
    BUILDERS[f"ends-{_a}-{_b}"] = (_ends_case, _a, _b)
for _n in REDUCE_SIZES:
    BUILDERS[f"reduce-{_n}"] = (_reduce_case, _n)
BUILDERS["plan-span"] = (_reduce_case, 1000, 300_000, "the plan's span is gap_capacity + 1")
NAMES = list(BUILDERS)
_BUILT = {}


def case(name):
    if name not in _BUILT:
        fn, *args = BUILDERS[name]
        _BUILT[name] = fn(*args)
    return _BUILT[name]
