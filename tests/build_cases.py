"""A catalogue of texts for the index builder (spx_build.hip) and its specification (synth.index_from_text), chosen
from the builder's code: thread blocks of 256, range-minimum blocks of 64 positions under a sparse table, PLCP chunks
of 4 096 positions (256 chunks per block of k_plcp), 8-byte windows, prefix doubling from 8 characters, 65 535
documents.  Used by tests/test_build_spec_cpu.py and tests/test_gpu_build.py.

A case makes (text, doc_lengths, with_samples) from a seed and names what the text has to reach: `unmet(ref)` lists
the conditions that the first-principles answer (brute.BruteIndex: n, sa, lcp and the seven fields) does NOT meet, and
`reaches(ref)` is `not unmet(ref)`.  Both look at the reference's answer alone, so a case that stops reaching its
path fails by name instead of passing on something easier.  Here n = len(text) + 1."""
import dataclasses
from typing import Callable, Optional

import numpy as np

from tests import brute

BT = 256  # threads per block of every kernel
RMQ = 64  # positions per range-minimum block
CHUNK = 4096  # text positions per thread of k_plcp
MAX_DOCS = 65535
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)


@dataclasses.dataclass
class Case:
    name: str
    make: Callable  # seed -> (text u8, doc_lengths or None, with_samples)
    unmet: Callable  # BruteIndex -> list of the conditions that do not hold
    seed: int = 0

    def inputs(self):
        text, docs, samples = self.make(self.seed)
        return np.ascontiguousarray(text, dtype=np.uint8), docs, samples

    def reaches(self, ref) -> bool:
        return not self.unmet(ref)


_REFERENCES = {}


def reference(case: Case):
    """(text, doc_lengths, with_samples, brute.BruteIndex) of a case, computed once per process; nobody writes to it."""
    if case.name not in _REFERENCES:
        text, docs, samples = case.inputs()
        _REFERENCES[case.name] = (text, docs, samples, brute.BruteIndex(text, docs, samples))
    return _REFERENCES[case.name]


def _conditions(**named):
    return [k for k, ok in named.items() if not ok]


def random_dna(length, seed):
    """What every `reaches` has to tell from its own text."""
    return DNA[np.random.default_rng(seed).integers(0, 4, size=length)]


# ---- sizes --------------------------------------------------------------------------------------------------------
SIZE_POINTS = (64, 128, 256, 512, 4096, 8192, 12288, 65536)
BIG_POINT = 1 << 20


def _binary_with_repeats(length, seed):
    """Four copies of a random text over two letters, three characters changed: matches of about an eighth of it."""
    rng = np.random.default_rng(seed)
    base = np.array([67, 71], dtype=np.uint8)[rng.integers(0, 2, size=max(1, (length + 3) // 4))]
    text = np.tile(base, 4)[:length].copy()
    for p in rng.integers(0, length, size=3):
        text[p] = 67 + 71 - text[p]
    return text


def _size_case(n, kind):
    def make(seed):
        text = random_dna(n - 1, seed) if kind == "dna" else _binary_with_repeats(n - 1, seed)
        return text, [(n - 1) // 3, n - 1 - 2 * ((n - 1) // 3), (n - 1) // 3], True

    def unmet(ref):
        c = _conditions(n=ref.n == n, three_documents=set(ref.doc_start.tolist()) | set(ref.doc_end.tolist()) == {0, 1, 2}, letters=np.unique(ref.heads).size == (5 if kind == "dna" else 3))
        if kind == "binary":  # three changes cut the 3/4 of the text that repeats into at most 7 pieces
            c += _conditions(long_repeats=int(ref.lcp.max()) >= (n - 1) // 16)
        return c

    return Case(f"size_{kind}_{n}", make, unmet, seed=n)


def _size_cases():
    out = [_size_case(p + d, kind) for p in SIZE_POINTS for d in (-1, 0, 1) for kind in ("dna", "binary")]
    return out + [_size_case(BIG_POINT + d, "dna") for d in (-1, 0, 1)]


# ---- tail: the text's length modulo 8 -----------------------------------------------------------------------------
TAIL_U = 4100  # U U U[:j]: the suffix at |U| is a prefix of the text that ends at the terminator, longer than a chunk


def _tail_case(j):
    def make(seed):
        rng = np.random.default_rng(seed)
        u = rng.integers(2, 256, size=TAIL_U).astype(np.uint8)
        u[7], u[1000], u[-1] = 2, 255, 255
        return np.concatenate([u, u, u[:j]]), None, True

    def unmet(ref):
        n = ref.n
        sa = ref.sa.astype(np.int64)
        lcp = ref.lcp.astype(np.int64)
        at_end = lcp[1:] == n - 1 - np.maximum(sa[:-1], sa[1:])  # the common prefix stops at the terminator
        return _conditions(n_mod_8=n % 8 == (2 * TAIL_U + j + 1) % 8,
                           ends_at_terminator=bool((at_end & (lcp[1:] >= TAIL_U)).any()),
                           bytes_2_and_255=bool((ref.heads == 2).any() and (ref.heads == 255).any()))

    return Case(f"tail_{j}", make, unmet, seed=100 + j)


# ---- repeat lengths -----------------------------------------------------------------------------------------------
REPEAT_LENGTHS = (7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097, 9000)
NATURAL = 7  # the background's own LCP stays below this


def _repeat_case(ell, at_border):
    """A background over letters 2 .. 201 and one repeat of `ell` letters planted twice, every copy between four
    letters (202 .. 205) that occur once: the two copies match for exactly `ell`, nothing else for 7 or more.  The
    copy that sorts later (205 follows it, 203 the other) carries PLCP ell - k at its k-th position; `at_border`
    starts it 6 positions before a multiple of 4 096."""
    p1 = 100
    p2 = p1 + ell + 50
    if at_border:
        p2 = (p2 + 6 + CHUNK - 1) // CHUNK * CHUNK - 6
    length = max(20_000, p2 + ell + 100)

    def make(seed):
        rng = np.random.default_rng(seed)
        text = rng.integers(2, 202, size=length).astype(np.uint8)
        rep = rng.integers(2, 202, size=ell).astype(np.uint8)
        text[p1: p1 + ell] = rep
        text[p2: p2 + ell] = rep
        text[p1 - 1], text[p1 + ell], text[p2 - 1], text[p2 + ell] = 202, 203, 204, 205
        return text, [length], True

    def unmet(ref):
        lcp = ref.lcp.astype(np.int64)
        sa = ref.sa.astype(np.int64)
        long_ = np.flatnonzero(lcp >= NATURAL)
        # the planted pair alone is long: positions k = 0 .. ell - 7 of the copies, each with LCP ell - k
        pair = sa[long_] - sa[long_ - 1]
        c = _conditions(longest=int(lcp.max()) == ell, once=int((lcp == ell).sum()) == 1,
                        background_below_7=long_.size == ell - NATURAL + 1 and bool((np.abs(pair) == p2 - p1).all()),
                        lengths=np.array_equal(np.sort(lcp[long_]), np.arange(NATURAL, ell + 1)))
        if at_border:
            plcp = np.empty(ref.n, dtype=np.int64)
            plcp[sa] = lcp
            border = p2 + 6
            c += _conditions(border=border % CHUNK == 0, long_on_both_sides=plcp[border - 1] >= 4000 and plcp[border] >= 4000)
        return c

    return Case(f"repeat_{ell}" + ("_at_border" if at_border else ""), make, unmet, seed=ell)


# ---- chunk starts ---------------------------------------------------------------------------------------------------
CHUNK_STARTS = 10  # PLCP 0 .. 9 at the first position of chunks 1 .. 10: below, at and past one 8-byte window


def _chunk_start_make(seed):
    """A background over letters 2 .. 201; at position (v + 1) * 4 096 the letter 210 + v, found nowhere else, v + 1
    times and then a smaller letter: of these suffixes the shorter stretch sorts first, so the one at the chunk's
    first position follows the one after it and shares exactly v letters with it.  A PLCP of 0 is otherwise rare (one
    position per letter), so a chunk that starts from a wrong length is told only here."""
    rng = np.random.default_rng(seed)
    text = rng.integers(2, 202, size=(CHUNK_STARTS + 1) * CHUNK + 100).astype(np.uint8)
    for v in range(CHUNK_STARTS):
        at = (v + 1) * CHUNK
        text[at: at + v + 1] = 210 + v
    return text, [text.size], True


def _chunk_start_unmet(ref):
    plcp = np.empty(ref.n, dtype=np.int64)
    plcp[ref.sa.astype(np.int64)] = ref.lcp
    return _conditions(chunks=ref.n > (CHUNK_STARTS + 1) * CHUNK,
                       plcp_0_to_9_at_chunk_starts=plcp[CHUNK: (CHUNK_STARTS + 1) * CHUNK: CHUNK].tolist() == list(range(CHUNK_STARTS)))


# ---- long threshold intervals ---------------------------------------------------------------------------------------
def threshold_intervals(ref):
    """(lo, hi) of every run that has a threshold: (end of the previous run of its letter, its own start]."""
    starts = np.cumsum(ref.lens) - ref.lens
    ends = starts + ref.lens - 1
    order = np.argsort(ref.heads, kind="stable")
    hs = ref.heads[order]
    same = hs[1:] == hs[:-1]
    return ends[order[:-1]][same] + 1, starts[order[1:]][same]


def interval_census(ref):
    """What the range-minimum query of k_thresholds meets on this answer: the middle parts in blocks, the sparse
    levels, and where the first of several equal minima lies in intervals of three or more blocks."""
    lo, hi = threshold_intervals(ref)
    bl, bh = lo // RMQ, hi // RMQ
    middle = np.where(bh > bl, bh - bl - 1, -1)  # -1: one block, 0: two partial blocks
    levels = set(int(np.floor(np.log2(m))) for m in np.unique(middle[middle >= 1]).tolist())
    tied = {"left": 0, "middle": 0, "right": 0}
    lcp = ref.lcp
    for a, b in zip(lo[middle >= 1].tolist(), hi[middle >= 1].tolist()):
        seg = lcp[a: b + 1]
        where = np.flatnonzero(seg == seg.min())
        if where.size > 1:
            blk = (a + int(where[0])) // RMQ
            tied["left" if blk == a // RMQ else "right" if blk == b // RMQ else "middle"] += 1
    return dict(middle=middle, levels=levels, tied=tied)


# exponent and seed chosen on the CPU so that the reference meets the conditions below: the rare one is a first minimum
# in the right partial block (0 .. 9 of some 7 000 tied intervals over exponents 1.1, 1.3, 1.5 and seeds 0 .. 11; 9 here)
ZIPF_LENGTH, ZIPF_EXPONENT, ZIPF_SEED = 70_000, 1.5, 4


def _zipf_make(seed):
    """Letters 2 .. 252 by a Zipf law (2 the most frequent), and letters 254 and 255 twice each: 255 in front of
    seven 2s (the BWT's first positions) and in front of 254 (its last four); 254 in front of seven 2s and in front
    of a letter whose suffixes lie some three quarters into the BWT."""
    rng = np.random.default_rng(seed)
    p = np.arange(1, 252, dtype=np.float64) ** -ZIPF_EXPONENT
    p /= p.sum()
    text = (2 + rng.choice(251, size=ZIPF_LENGTH, p=p)).astype(np.uint8)
    three_quarters = 2 + int(np.searchsorted(np.cumsum(p), 0.75))
    low = [2] * 7
    for at, piece in ((10_000, [255] + low), (30_000, [254] + low), (50_000, [255, 254, three_quarters])):
        text[at: at + len(piece)] = piece
    return text, [ZIPF_LENGTH], True


def _zipf_unmet(ref):
    cen = interval_census(ref)
    nb = (ref.n + RMQ - 1) // RMQ
    top = int(np.floor(np.log2(nb - 2)))
    mids = set(cen["middle"].tolist())
    return _conditions(every_sparse_level=cen["levels"] >= set(range(top + 1)),
                       middle_0_1_2_4_8_16=mids >= {0, 1, 2, 4, 8, 16},
                       hundred_tied=sum(cen["tied"].values()) >= 100,
                       first_minimum_in_every_part=min(cen["tied"].values()) >= 5)


# ---- documents ----------------------------------------------------------------------------------------------------
DOCS_LENGTH = 70_000


def _docs_lengths(first_empty):
    """65 535 documents over 70 000 characters: three empty (the last one, one in the middle and the first -- or,
    with the first holding a character, the second), one of 4 469, all others of one character."""
    d = np.ones(MAX_DOCS, dtype=np.int64)
    d[0 if first_empty else 1] = 0
    d[MAX_DOCS // 2] = 0
    d[-1] = 0
    d[40_000] = DOCS_LENGTH - (MAX_DOCS - 4)
    assert int(d.sum()) == DOCS_LENGTH
    return d.tolist()


def _docs_text(seed):
    return np.random.default_rng(seed).integers(2, 202, size=DOCS_LENGTH).astype(np.uint8)


def _docs_case(name, docs, samples, first_empty=True):
    def make(seed):
        return _docs_text(seed), (_docs_lengths(first_empty) if docs else None), samples

    def unmet(ref):
        c = _conditions(n=ref.n == DOCS_LENGTH + 1, none_without_samples=samples or ref.ssa is None,
                        no_ids_without_documents=docs and samples or ref.doc_start is None)
        if docs and samples:
            ids = np.concatenate([ref.doc_start, ref.doc_end])
            samp = np.concatenate([ref.ssa, ref.esa])
            # an empty first document owns no position: the smallest id is then 1
            c += _conditions(first_id=int(ids.min()) == (1 if first_empty else 0), last_id=int(ids.max()) == MAX_DOCS - 1,
                             many_ids=np.unique(ids).size > 30_000,
                             # (200 letters: a sample at all but a few positions, so nearly each of the 65 532 documents that hold one)
                             nearly_every_id=np.unique(ids).size >= MAX_DOCS - 13,
                             terminator_in_last=bool((samp == ref.n - 1).any()) and bool((ids[samp == ref.n - 1] == MAX_DOCS - 1).all()))
        return c

    return Case(name, make, unmet, seed=65535)


# ---- extremes -----------------------------------------------------------------------------------------------------
def _fibonacci(length):
    a, b = b"C", b"CG"
    while len(b) < length:
        a, b = b, b + a
    return np.frombuffer(b[:length], dtype=np.uint8).copy()


def _extreme_cases():
    def one_letter(seed):
        return np.full(50_000, 65, dtype=np.uint8), [50_000], True

    def period_2(seed):
        return np.tile(np.array([67, 71], dtype=np.uint8), 25_000), [50_000], True

    def fibonacci(seed):
        return _fibonacci(46_368), [46_368], True

    def byte_255(seed):
        return np.full(3_000, 255, dtype=np.uint8), [3_000], True

    def smallest_tail(seed):
        return np.concatenate([random_dna(9_991, seed), np.full(9, 65, dtype=np.uint8)]), [10_000], True

    def sa_head(ref, k):  # the k shortest suffixes come first, by length
        return np.array_equal(ref.sa[: k + 1], ref.n - 1 - np.arange(k + 1))

    return [
        Case("one_letter", one_letter, lambda ref: _conditions(runs=ref.r == 2, lcp=int(ref.lcp.max()) == ref.n - 2)),
        Case("period_2", period_2, lambda ref: _conditions(runs=ref.r <= 4, lcp=int(ref.lcp.max()) == ref.n - 3)),
        Case("fibonacci", fibonacci, lambda ref: _conditions(
            runs=ref.r <= 64, lcp=int(ref.lcp.max()) > 4 * CHUNK,
            every_chunk_starts_long=int(np.sort(ref.lcp)[ref.n // 2]) > CHUNK)),
        Case("byte_255", byte_255, lambda ref: _conditions(runs=ref.r == 2, letter=int(ref.heads.max()) == 255,
                                                          lcp=int(ref.lcp.max()) == ref.n - 2)),
        Case("smallest_tail", smallest_tail, lambda ref: _conditions(nine=sa_head(ref, 9), not_ten=not sa_head(ref, 10)), seed=9),
    ]


def _all_cases():
    cases = _size_cases()
    cases += [_tail_case(j) for j in range(8)]
    cases += [_repeat_case(ell, False) for ell in REPEAT_LENGTHS]
    cases += [_repeat_case(ell, True) for ell in REPEAT_LENGTHS if ell >= 4095]
    cases += [Case("chunk_starts_0_to_9", _chunk_start_make, _chunk_start_unmet, seed=4096)]
    cases += [Case("zipf_long_intervals", _zipf_make, _zipf_unmet, seed=ZIPF_SEED)]
    cases += [_docs_case("documents_65535", True, True), _docs_case("documents_65535_first_holds_one", True, True, first_empty=False),
              _docs_case("documents_none", False, True), _docs_case("documents_no_samples", False, False)]
    cases += _extreme_cases()
    return cases


CASES = _all_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SMALLEST, LARGEST = BY_NAME["size_dna_63"], BY_NAME[f"size_dna_{BIG_POINT + 1}"]
# the families whose `reaches` must fail on random DNA of the same length (shown by test_build_spec_cpu.py)
TOLD_FROM_DNA = ["tail_3", "repeat_16", "repeat_4097_at_border", "chunk_starts_0_to_9", "zipf_long_intervals", "documents_65535"]
