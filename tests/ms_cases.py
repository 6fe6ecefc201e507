"""A catalogue of (text, documents, reads) for the query path in MS mode -- the walk (spx_walk_fast.inc, k_walk_lanes, the
chunked passes) and k_ms_extend -- held to matching statistics from first principles (tests/brute_ms.c over the suffix
array of tests/brute_index.c).  Used by tests/test_ms_math_cpu.py (the oracle) and tests/test_gpu_ms_math.py (HIP).

The index of a case is the BruteIndex fields as a synth.RawIndex: neither synth.index_from_text nor the HIP builder is
in the loop, so a failure names the query path.  Alphabets are below 128 (bytes >= 128 never take the reference's match
branch, SURVEY Appendix C1, and the equality with the mathematics fails there by design).

What the cases are chosen from:
  k_ms_extend      8-byte compares at any byte address, clamped at the read's end and at the text's end (read lengths
                   and n_text over every residue mod 8, a read that ends where the next read goes on like the text, the
                   text's suffix as the batch's last read); the `l - 1` carry along a match (matches far longer than a
                   read of the old test: 1 000 .. 66 000); a wavefront loops to its longest read (one read of 5 000
                   among 63 short ones, aligned to 64 reads); tiles of 16 pointers; lengths staged below 65 536 values
                   and stored one by one above; the 16-bit entry point up to reads of 65 535
  the walks        `pos < thr` where several positions tie for the smallest LCP; offsets inside a run past the 126 the
                   rows' cumulative lengths hold, and runs of 2^16 positions, laid out as pieces; the 64-character
                   flush word and 16-character checkpoints (read lengths around 8, 16, 32, 64); empty reads in runs;
                   more reads than a launch has lanes, dealt on demand (140 000 short reads)
  spx_flatten      compact rows unless a run has 2^16 positions; general rows, escaped slots and no pieces by knobs

A case names what it has to reach: `unmet(text, sa, lcp, true_ms)` lists the conditions that the first-principles
answers do NOT meet and `reaches(...)` is `not unmet(...)`; both look at the text, its suffix and LCP arrays, the reads
and the true matching statistics alone."""
import dataclasses
from typing import Callable

import numpy as np
import torch

from spumoni_amd import synth
from tests import brute, build_cases, cases

DNA = list(b"ACGT")
LENGTHS = [0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1000, 2200]
SHORT_LENGTHS = [0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65]
RATES = (0.003, 0.03, 0.15)
SUFFIXES = (1, 7, 8, 9, 16, 500)
LONG_MATCH = 66_000


# ---- texts ----------------------------------------------------------------------------------------------------------
def _thirds(n):
    return [n // 3, n - 2 * (n // 3), n // 3]


def _repetitive(n, letters, seed):
    return lambda: (cases.repetitive_text(np.random.default_rng(seed), n, letters), _thirds(n))


def _binary():
    text = build_cases._binary_with_repeats(20_000, 5)
    return text, _thirds(text.size)


def _zipf():
    """Letters 2 .. 126 by a Zipf law (exponent 1.2), 20 000 characters, the first 3 000 repeated at 12 000."""
    rng = np.random.default_rng(12)
    p = np.arange(1, 126, dtype=np.float64) ** -1.2
    text = (2 + rng.choice(125, size=20_000, p=p / p.sum())).astype(np.uint8)
    text[12_000:15_000] = text[:3_000]
    return text, _thirds(text.size)


PIECES_RUN = 66_000


def _pieces():
    """One letter 66 000 times in a row inside random DNA: the suffixes that start inside it are neighbours, so the BWT
    has a run of nearly as many positions."""
    rng = np.random.default_rng(21)
    side = lambda: np.asarray(DNA, dtype=np.uint8)[rng.integers(0, 4, size=3_000)]
    a, b = side(), side()
    a[-1], b[0] = ord("C"), ord("G")
    text = np.concatenate([a, np.full(PIECES_RUN, ord("A"), dtype=np.uint8), b])
    return text, _thirds(text.size)


def _period():
    """A unit of 20 letters 400 times: BWT runs of 400 positions, past the 126 that a row's cumulative lengths hold."""
    text = np.tile(np.frombuffer(b"ACGTTGCAAGGCTTAACCGT", dtype=np.uint8), 400)
    return text, _thirds(text.size)


def _long():
    """Random DNA with its first 1 000 characters repeated at 69 000: the text of the read that matches 66 000."""
    text = build_cases.random_dna(70_000, 70).copy()
    text[69_000:] = text[:1_000]
    return text, _thirds(text.size)


def _tail(j):
    def make():
        text = cases.repetitive_text(np.random.default_rng(40), 4096 + 7, DNA)[: 4096 + j]
        return text, _thirds(text.size)

    return make


TEXTS = {
    "rep_4096": _repetitive(4096, DNA, 31), "rep_65534": _repetitive(65534, DNA, 36), "rep_65535": _repetitive(65535, DNA, 32), "rep_65536": _repetitive(65536, DNA, 33),
    "rep_65537": _repetitive(65537, DNA, 34), "acgtn": _repetitive(30_000, list(b"ACGTN"), 35), "binary": _binary, "zipf": _zipf,
    "pieces": _pieces, "period": _period, "long": _long,
}
TEXTS.update({f"tail_{j}": _tail(j) for j in range(8)})
_TEXTS_MADE, _TEXT_REFS = {}, {}


def text_of(key):
    """(text, doc_lengths) of a text, made once per process; nobody writes to it."""
    if key not in _TEXTS_MADE:
        text, docs = TEXTS[key]()
        text = np.ascontiguousarray(text, dtype=np.uint8)
        assert int(text.max()) < 128 and int(text.min()) >= 2
        _TEXTS_MADE[key] = (text, docs)
    return _TEXTS_MADE[key]


def text_reference(key):
    """(text, doc_lengths, brute.BruteIndex) of a text, computed once per process; nobody writes to it."""
    if key not in _TEXT_REFS:
        text, docs = text_of(key)
        _TEXT_REFS[key] = (text, docs, brute.BruteIndex(text, docs))
    return _TEXT_REFS[key]


def raw_index(ref, with_text=None):
    """The first-principles index as a synth.RawIndex (CPU tensors)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int64))
    return synth.RawIndex(heads=torch.from_numpy(ref.heads.copy()), lens=t(ref.lens), thr=t(ref.thr), n=ref.n, ssa=t(ref.ssa),
                          esa=t(ref.esa), doc_start=t(ref.doc_start), doc_end=t(ref.doc_end),
                          text=None if with_text is None else torch.from_numpy(with_text.copy()))


# ---- reads ----------------------------------------------------------------------------------------------------------
def _letters_of(text):
    return np.unique(text)


def _absent(text):
    return ord("N") if ord("N") not in set(text.tolist()) and ord("A") in set(text.tolist()) else (
        ord("Z") if ord("Z") not in set(text.tolist()) else 127)


def _substring(rng, text, m, rate, letters):
    m = min(m, text.size - 1)
    s = int(rng.integers(0, text.size - m + 1))
    rd = text[s: s + m].copy()
    hit = rng.random(m) < rate
    rd[hit] = letters[rng.integers(0, letters.size, size=int(hit.sum()))]
    return rd


def _random(rng, m, letters):
    return letters[rng.integers(0, letters.size, size=m)]


EMPTY = np.zeros(0, dtype=np.uint8)


def _adjacent(rng, text):
    """Pairs of reads that are consecutive pieces of the text, the first of every length mod 8: k_ms_extend's last
    8-byte compare of the first read looks at the second read's characters, which go on like the text."""
    out = []
    for j in range(8):
        la = 40 + j
        s = int(rng.integers(0, text.size - la - 48))
        out += [text[s: s + la].copy(), text[s + la: s + la + 40].copy()]
    return out


def _with_absent(rng, text, letters, lengths):
    out, z = [], _absent(text)
    for m in lengths:
        rd = _substring(rng, text, m, 0.0, letters)
        rd[rng.integers(0, rd.size, size=1 + rd.size // 300)] = z
        out.append(rd)
    return out


def _group_of_64(rng, text, letters, long_len):
    """63 reads of <= 20 characters and one of `long_len` (lane 37 of its wavefront)."""
    out = [_substring(rng, text, int(rng.integers(0, 21)), 0.03, letters) for _ in range(64)]
    out[37] = _substring(rng, text, long_len, 0.003, letters)
    return out


def standard_reads(text, seed, lengths=LENGTHS, group_long=5000, last_suffix=500, more=()):
    """The read classes of the module's docstring over one text; returns (reads, marks): marks names the read
    indices the conditions look at."""
    rng = np.random.default_rng(seed)
    letters = _letters_of(text)
    reads, marks = [EMPTY] * 3, {}
    for rate in RATES:
        reads += [_substring(rng, text, m, rate, letters) for m in lengths]
    reads += [_random(rng, m, letters) for m in lengths]
    if 1000 in lengths:
        reads.append(_substring(rng, text, 1500, 0.0, letters))  # one exact match far longer than eight bytes
    reads += list(more)
    marks["adjacent"] = len(reads)
    reads += _adjacent(rng, text)
    reads += _with_absent(rng, text, letters, [9, 33, 64, 200, 1000][: 5 if 1000 in lengths else 3])
    marks["suffix_mid"] = len(reads)
    reads += [text[text.size - k:].copy() for k in SUFFIXES if k < text.size]
    reads += [EMPTY] * ((-len(reads)) % 64)  # (a run of empty reads: the group below is one wavefront of k_ms_extend)
    marks["group"] = len(reads)
    marks["group_long"] = min(group_long, text.size - 10)
    reads += _group_of_64(rng, text, letters, marks["group_long"])
    reads += [_random(rng, 12, letters), EMPTY, EMPTY]
    marks["suffix_last"] = len(reads)
    reads.append(text[text.size - min(last_suffix, text.size - 1):].copy())
    return reads, marks


def batch(reads):
    offs = np.concatenate([[0], np.cumsum([r.size for r in reads])]).astype(np.int64)
    seqs = np.concatenate(reads).astype(np.uint8) if offs[-1] else np.zeros(0, dtype=np.uint8)
    return seqs, offs


# ---- cases ----------------------------------------------------------------------------------------------------------
def _conditions(**named):
    return [k for k, ok in named.items() if not ok]


def run_lengths(text, sa):
    """The lengths of the BWT's runs, from the text and its suffix array."""
    t = np.concatenate([text, np.zeros(1, dtype=np.uint8)])
    bwt = t[(sa.astype(np.int64) - 1) % t.size]
    cut = np.flatnonzero(np.concatenate([[True], bwt[1:] != bwt[:-1], [True]]))
    return np.diff(cut)


def tied_minima(text, sa, lcp):
    """The largest number of positions that share the smallest LCP of one threshold interval."""
    t = np.concatenate([text, np.zeros(1, dtype=np.uint8)])
    bwt = t[(sa.astype(np.int64) - 1) % t.size]
    starts = np.flatnonzero(np.concatenate([[True], bwt[1:] != bwt[:-1]]))
    ends = np.concatenate([starts[1:], [t.size]]) - 1
    last_end, best = {}, 0
    for s, e in zip(starts.tolist(), ends.tolist()):
        c = int(bwt[s])
        if c in last_end and s - last_end[c] >= 3:
            seg = lcp[last_end[c] + 1: s + 1]
            best = max(best, int((seg == seg.min()).sum()))
        last_end[c] = e
    return best


def suffix_is_unique(sa, lcp, n_text, k):
    """text[n_text - k:] occurs once: the suffix after it in the suffix array does not begin with it."""
    rank = int(np.flatnonzero(sa == n_text - k)[0])
    return rank + 1 >= sa.size or int(lcp[rank + 1]) < k


@dataclasses.dataclass
class Case:
    name: str
    text_key: str
    make_reads: Callable  # text -> (list of reads, marks)
    extra: Callable = None  # (case, text, sa, lcp, ms) -> unmet conditions beyond the common ones
    _made: tuple = None

    def reads(self):
        """(seqs, offs, marks), made once; nobody writes to them."""
        if self._made is None:
            rd, marks = self.make_reads(text_of(self.text_key)[0])
            self._made = (rd if isinstance(rd, tuple) else batch(rd)) + (marks,)  # (a list of reads, or seqs and offs)
        return self._made

    def in_alphabet(self):
        """One flag per read: every character occurs in the text."""
        text = text_of(self.text_key)[0]
        seqs, offs, _ = self.reads()
        have = np.zeros(256, dtype=bool)
        have[text] = True
        bad = np.concatenate([[0], np.cumsum(~have[seqs])])
        return bad[offs[1:]] == bad[offs[:-1]]

    def unmet(self, text, sa, lcp, true_ms):
        seqs, offs, marks = self.reads()
        m = np.diff(offs)
        ok = self.in_alphabet()
        c = _conditions(below_128=int(text.max()) < 128 and (seqs.size == 0 or int(seqs.max()) < 128),
                        absent_in_a_tenth_at_most=int((~ok).sum()) * 10 <= ok.size,
                        values=true_ms.size == int(offs[-1]))
        if "suffix_last" in marks:
            q = marks["suffix_last"]
            k = int(m[q])
            c += _conditions(last_read_is_the_texts_suffix=q == m.size - 1 and np.array_equal(seqs[offs[q]:], text[text.size - k:]),
                             its_first_value_is_its_length=int(true_ms[offs[q]]) == k)
        if "suffix_mid" in marks:
            q0 = marks["suffix_mid"]
            ks = [k for k in SUFFIXES if k < text.size]
            c += _conditions(suffixes_inside_the_batch=all(
                int(m[q0 + i]) == k and int(true_ms[offs[q0 + i]]) == k and np.array_equal(seqs[offs[q0 + i]: offs[q0 + i + 1]], text[text.size - k:])
                for i, k in enumerate(ks)))
        if "adjacent" in marks:
            q0 = marks["adjacent"]
            firsts = [q0 + 2 * j for j in range(8)]
            # the first read's last position alone is a match of 1; the text's occurrence goes on for what the next read holds
            t = text.tobytes()
            c += _conditions(adjacent_every_length_mod_8=sorted(int(m[q]) % 8 for q in firsts) == list(range(8)),
                             last_value_is_1=all(int(true_ms[offs[q + 1] - 1]) == 1 for q in firsts),
                             goes_on_into_the_next_read=all(t.find(seqs[offs[q]: offs[q + 1] + 8].tobytes()) >= 0 and m[q + 1] >= 8 for q in firsts),
                             in_the_middle=0 < q0 and firsts[-1] + 2 < m.size)
        if "group" in marks:
            q0 = marks["group"]
            g = m[q0: q0 + 64]
            c += _conditions(group_is_one_wavefront=q0 % 64 == 0 and g.size == 64,
                             one_long_among_short=int(g.max()) == marks["group_long"] >= 500 and int(np.sort(g)[-2]) <= 20,
                             empty_reads_in_a_run=bool(((m[:-2] == 0) & (m[1:-1] == 0) & (m[2:] == 0)).any()))
        if self.extra:
            c += self.extra(self, text, sa, lcp, true_ms)
        return c

    def reaches(self, text, sa, lcp, true_ms):
        return not self.unmet(text, sa, lcp, true_ms)


def _standard_extra(case, text, sa, lcp, ms):
    seqs, offs, marks = case.reads()
    m = np.diff(offs)
    return _conditions(every_length=set(LENGTHS) <= set(m.tolist()),
                       long_matches=int(ms.max()) >= 1000,  # (the old test's reads end at 29 characters)
                       short_matches_too=bool((ms <= 16).any()))


def _standard(name, key, seed, extra=None, **kw):
    def both(case, text, sa, lcp, ms):
        return _standard_extra(case, text, sa, lcp, ms) + (extra(case, text, sa, lcp, ms) if extra else [])

    return Case(name, key, lambda text: standard_reads(text, seed, **kw), both)


def _size_extra(n):
    return lambda case, text, sa, lcp, ms: _conditions(n_text=text.size == n, many_runs=run_lengths(text, sa).size >= 500,
                                                       compact_rows=int(run_lengths(text, sa).max()) < 65536)


def _binary_extra(case, text, sa, lcp, ms):
    # (an interval's tied minima are the borders between the children of one suffix-tree node: over two letters and the
    # terminator there are at most two, so the three or more are asked of the texts over four letters and over 125)
    return _conditions(two_letters=np.unique(text).size == 2, two_tied_minima=tied_minima(text, sa, lcp) == 2,
                       long_repeats=int(lcp.max()) >= text.size // 16)


def _tied_extra(case, text, sa, lcp, ms):
    return _conditions(three_tied_minima=tied_minima(text, sa, lcp) >= 3)


def _zipf_extra(case, text, sa, lcp, ms):
    return _conditions(hundred_letters=np.unique(text).size >= 100, many_tied_minima=tied_minima(text, sa, lcp) >= 16)


def _period_extra(case, text, sa, lcp, ms):
    rl = run_lengths(text, sa)
    return _conditions(offsets_past_126=127 < int(rl.max()) < 65536)


def _pieces_reads(text):
    at = 3_000  # into the run, out of it, inside it, its first letter
    more = [text[at - 40: at + 300].copy(), text[at + PIECES_RUN - 300: at + PIECES_RUN + 40].copy(),
            np.full(3_000, ord("A"), dtype=np.uint8), text[at - 10: at + 1].copy()]
    return standard_reads(text, 51, more=more)


def _pieces_extra(case, text, sa, lcp, ms):
    return _conditions(run_of_2_to_the_16=int(run_lengths(text, sa).max()) >= 65536)


def _whole_reads(front, behind):
    def make(text):
        rng = np.random.default_rng(61)
        letters = _letters_of(text)
        short = lambda: [_substring(rng, text, m, 0.03, letters) for m in (9, 33, 64)]
        reads = short()
        marks = {"whole": len(reads)}
        if front or behind:
            reads += [np.concatenate([letters[:1], text]), EMPTY, np.concatenate([text, letters[-1:]])]
        else:
            reads += [text.copy()]
        return reads + short(), marks

    return make


def _whole_extra(plus):
    def extra(case, text, sa, lcp, ms):
        seqs, offs, marks = case.reads()
        q = marks["whole"]
        m = np.diff(offs)
        if not plus:
            return _conditions(sixteen_bit_limit=text.size == 65535 == int(m.max()), whole_text_matches=int(ms[offs[q]]) == text.size)
        return _conditions(read_length=int(m[q]) == plus == int(m[q + 2]) == text.size + 1,
                           letter_in_front=int(ms[offs[q] + 1]) == text.size and int(ms[offs[q]]) < text.size,
                           letter_behind=int(ms[offs[q + 2]]) == text.size)

    return extra


def _long_reads(text):
    rng = np.random.default_rng(71)
    letters = _letters_of(text)
    short = lambda: [_substring(rng, text, m, 0.03, letters) for m in (9, 33, 64, 1000)]
    big = np.concatenate([_random(rng, 60, letters), text[2_000: 2_000 + LONG_MATCH], _random(rng, 60, letters)])
    return short() + [EMPTY, big] + short(), {"big": 5}


def _long_extra(case, text, sa, lcp, ms):
    seqs, offs, marks = case.reads()
    q = marks["big"]
    return _conditions(text_of_70000=text.size >= 70_000, read_past_16_bits=int(offs[q + 1] - offs[q]) >= 65536,
                       match_past_16_bits=int(ms[offs[q]: offs[q + 1]].max()) >= 65536)


DEALT_READS = 140_000  # more than twice the 65 536 lanes of a plain launch at four wavefronts per CU on 256 CUs


def _dealt_reads(text):
    """Short reads, more of them than a launch has lanes: k_walk_fast deals all but the first round on demand.  Lengths
    from a Pareto tail (most reads a few characters, some hundreds), empty reads in runs of 70 and 300."""
    rng = np.random.default_rng(95)
    letters = _letters_of(text)
    lens = np.minimum(600, np.floor(5.0 * rng.pareto(1.1, size=DEALT_READS))).astype(np.int64)
    lens[1000:1070] = 0
    lens[90_000:90_300] = 0
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    kind = rng.integers(0, 50, size=DEALT_READS)  # < 10: random letters; the others cut from the text, 3 % substituted
    read_of = np.repeat(np.arange(DEALT_READS), lens)
    start = rng.integers(0, text.size - lens + 1)
    seqs = text[start[read_of] + np.arange(int(offs[-1])) - offs[read_of]].copy()
    hit = (kind[read_of] < 10) | (rng.random(seqs.size) < 0.03)
    seqs[hit] = letters[rng.integers(0, letters.size, size=int(hit.sum()))]
    marked = np.flatnonzero((kind == 49) & (lens > 0))  # one read in fifty holds a letter the text lacks
    seqs[offs[marked] + rng.integers(0, lens[marked])] = _absent(text)
    return (seqs, offs), {}


def _dealt_extra(case, text, sa, lcp, ms):
    m = np.diff(case.reads()[1])
    return _conditions(more_reads_than_lanes=m.size >= DEALT_READS, heavy_tail=int(m.max()) >= 500 and float(np.median(m)) <= 10,
                       empty_reads_in_runs=bool((m[1000:1070] == 0).all() and (m[90_000:90_300] == 0).all()))


def _tail_reads(k):
    def make(text):
        return standard_reads(text, 80 + k, lengths=SHORT_LENGTHS, group_long=600, last_suffix=k)

    return make


def _tail_extra(j, k):
    def extra(case, text, sa, lcp, ms):
        c = _conditions(n_text_mod_8=text.size % 8 == j)
        if k == 500:  # wherever a right answer points, pointer + length is the text's end
            c += _conditions(suffix_occurs_once=suffix_is_unique(sa, lcp, text.size, k))
        return c

    return extra


def _all_cases():
    out = [_standard(f"repetitive_{n}", f"rep_{n}", n, _size_extra(n)) for n in (4096, 65535, 65536, 65537)]
    out += [_standard("acgtn_30000", "acgtn", 5, _tied_extra), _standard("binary_tied_minima", "binary", 6, _binary_extra),
            _standard("zipf_125_letters", "zipf", 7, _zipf_extra), _standard("period_20_runs_of_400", "period", 8, _period_extra),
            Case("pieces_run_of_66000", "pieces", _pieces_reads, lambda *a: _standard_extra(*a) + _pieces_extra(*a)),
            Case("whole_text_65535", "rep_65535", _whole_reads(False, False), _whole_extra(0)),
            # a letter in front of the whole text, and behind it: reads of 65 535 (the 16-bit entry point's last) and of 65 536
            Case("whole_text_65534_and_a_letter", "rep_65534", _whole_reads(True, True), _whole_extra(65535)),
            Case("whole_text_and_a_letter", "rep_65535", _whole_reads(True, True), _whole_extra(65536)),
            Case("match_of_66000", "long", _long_reads, _long_extra),
            Case("dealt_on_demand", "rep_4096", _dealt_reads, _dealt_extra)]
    out += [Case(f"tail_{j}_suffix_{k}", f"tail_{j}", _tail_reads(k), _tail_extra(j, k)) for j in range(8) for k in SUFFIXES]
    return out


CASES = _all_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
UNIQUE_SUFFIX = [c.name for c in CASES if c.name.startswith("tail_") and int(c.name.rsplit("_", 1)[1]) == 500]
LONG_READS = [c.name for c in CASES if int(np.diff(c.reads()[1]).max()) >= 1000]  # what the chunked walk is asked on
_ANSWERS = {}


def reference(case):
    """(text, doc_lengths, BruteIndex, seqs, offs, true_ms) of a case, computed once per process."""
    if case.name not in _ANSWERS:
        text, docs, ref = text_reference(case.text_key)
        seqs, offs, _ = case.reads()
        _ANSWERS[case.name] = (text, docs, ref, seqs, offs, brute.brute_ms(text, ref.sa, seqs, offs))
    return _ANSWERS[case.name]


# ---- what is asserted -----------------------------------------------------------------------------------------------
def occurrences_wrong(text, seqs, offs, lengths, pointers, which):
    """The positions i (global) of the reads `which` with lengths[i] > 0 whose pointer does not name an occurrence:
    text[p: p + l] != read[i: i + l] or p + l > n_text.  A position whose pointer and length continue the one before in
    its read (p + 1, l - 1) is covered by that one; only the others are compared, character by character: the first 64
    characters of all of them at once, what lies behind them one position at a time."""
    L = np.asarray(lengths).astype(np.int64)
    P = np.asarray(pointers).astype(np.uint64)
    offs = np.asarray(offs).astype(np.int64)
    n_text, tot = text.size, int(offs[-1])
    if tot == 0:
        return []
    head = np.ones(tot, dtype=bool)
    head[1:] = (P[1:] != P[:-1] + np.uint64(1)) | (L[1:] != L[:-1] - 1)
    head[offs[:-1][np.diff(offs) > 0]] = True
    at = np.flatnonzero(head & (L > 0) & np.repeat(np.asarray(which, dtype=bool), np.diff(offs)))
    p, l = P[at], L[at]
    bad = (p >= np.uint64(n_text)) | (p.astype(np.int64) + l > n_text)
    at_ok, p_ok, l_ok = at[~bad], p[~bad].astype(np.int64), l[~bad]
    wrong = np.zeros(at_ok.size, dtype=bool)
    for d in range(int(min(64, l_ok.max())) if l_ok.size else 0):
        live = np.flatnonzero(l_ok > d)
        wrong[live] |= text[p_ok[live] + d] != seqs[at_ok[live] + d]
    for j in np.flatnonzero(l_ok > 64).tolist():
        i, pi, li = int(at_ok[j]), int(p_ok[j]), int(l_ok[j])
        wrong[j] |= not np.array_equal(text[pi + 64: pi + li], seqs[i + 64: i + li])
    return sorted(at[bad].tolist() + at_ok[wrong].tolist())


def last_suffix_ends_the_text(case, lengths, pointers):
    """UNIQUE_SUFFIX cases: the batch's last read is the text's suffix of 500 characters and occurs once, so at its first
    position pointer + length is n_text."""
    text, _, _, _, offs, _ = reference(case)
    at = int(offs[case.reads()[2]["suffix_last"]])
    return int(pointers[at]) + int(lengths[at]) == text.size and int(lengths[at]) == int(offs[-1]) - at


def check_answers(case, lengths, pointers, pml=None):
    """Section by section what a query in MS mode owes the mathematics.  Returns the number of positions compared."""
    text, _, _, seqs, offs, ms = reference(case)
    ok = case.in_alphabet()
    per_value = np.repeat(ok, np.diff(offs))
    L = np.asarray(lengths).astype(np.int64)
    assert L.size == ms.size
    wrong = np.flatnonzero((L != ms) & per_value)
    assert wrong.size == 0, (case.name, "lengths differ from the matching statistics at", wrong[:10].tolist(), L[wrong[:10]].tolist(),
                             ms[wrong[:10]].tolist(), int(wrong.size))
    over = np.flatnonzero(L > ms)
    assert over.size == 0, (case.name, "lengths above the matching statistics at", over[:10].tolist())
    bad = occurrences_wrong(text, seqs, offs, L, pointers, ok)
    assert not bad, (case.name, "pointers that name no occurrence at", bad[:10], len(bad))
    if pml is not None:
        over = np.flatnonzero(np.asarray(pml).astype(np.int64) > ms)
        assert over.size == 0, (case.name, "PML above the matching statistics at", over[:10].tolist())
    return int(per_value.sum())
