"""Shared builders of (index, reads) parity cases (used by CPU and GPU tests)."""
import numpy as np
import torch

from spumoni_amd import synth


def reads_mixed(rng, text, letters, nreads, maxlen, extra_letters=()):
    """ragged reads: substrings with errors, random, with absent letters; some empty."""
    reads = []
    pool = list(letters) + list(extra_letters)
    for q in range(nreads):
        m = int(rng.integers(0, maxlen)) if q % 17 else 0  # every 17th read is empty
        kind = rng.integers(0, 3)
        if m == 0:
            rd = np.zeros(0, dtype=np.uint8)
        elif kind == 0 and text is not None and text.size > m:
            s = int(rng.integers(0, text.size - m))
            rd = text[s : s + m].copy()
            for _ in range(int(rng.integers(0, 4))):
                rd[rng.integers(0, m)] = letters[rng.integers(0, len(letters))]
        elif kind == 1:
            rd = np.asarray(letters, dtype=np.uint8)[rng.integers(0, len(letters), size=m)]
        else:
            rd = np.asarray(pool, dtype=np.uint8)[rng.integers(0, len(pool), size=m)]
        reads.append(rd.astype(np.uint8))
    offs = np.concatenate([[0], np.cumsum([r.size for r in reads])]).astype(np.int64)
    seqs = np.concatenate(reads) if reads else np.zeros(0, dtype=np.uint8)
    return seqs, offs


def repetitive_text(rng, n, letters):
    letters = np.asarray(letters, dtype=np.uint8)
    base = letters[rng.integers(0, letters.size, size=max(8, n // 5))]
    parts, tot = [], 0
    while tot < n:
        p = base.copy()
        for _ in range(int(rng.integers(0, 6))):
            p[rng.integers(0, p.size)] = letters[rng.integers(0, letters.size)]
        p = p[int(rng.integers(0, p.size // 2)) :]
        parts.append(p)
        tot += p.size
    return np.concatenate(parts)[:n]


def real_case(seed, n, letters, ndocs=3, device="cpu"):
    rng = np.random.default_rng(seed)
    text = repetitive_text(rng, n, letters)
    cuts = sorted(rng.choice(np.arange(1, n), size=ndocs - 1, replace=False).tolist())
    doc_lengths = np.diff([0] + cuts + [n]).tolist()
    raw = synth.index_from_text(torch.from_numpy(text).to(device), doc_lengths=doc_lengths)
    return raw, text


# ---- indexes whose packed fields are full: n at the 40-bit limit, 16-bit document ids (test_gpu_field_widths.py) ----
N_LIMIT = (1 << 40) - 3  # the largest BWT length the flatten step accepts (spx_flatten.hip: n > MASK40 - 2 is refused)
WIDE_ALPHABETS = [list(b"ACGT"), list(b"ACGTN"), [3, 4, 5, 90, 127, 128, 129, 200, 255], [2, 60, 126, 127, 128, 254, 255],
                  list(b"ACGTNRY"), [5, 6, 7, 8, 9, 10]]


def wide_case(seed, n=N_LIMIT, r=3000, n_docs=65536, share=0.05):
    """A statistical index of `r` runs and exactly `n` positions: neighbours distinct, one terminator run, most runs
    1-5 long, `share` of them between 2^16 and 2^38 (the exponent is drawn, so every magnitude occurs; the largest are
    halved until the others fit into n - 2^39), one topped up by at least 2^39 so that the lengths add up to n: that run has
    a 40-bit length and holds half of all positions.  Thresholds, samples and document ids from synth.raw_from_runs; then
    the corners a random draw does not hit are written over the neighbours of every seventh (samples) or fourth (document ids) long run: samples n-1, 0 (the MS `sample--`
    wrap), single bits 24, 31, 32, 39 and their neighbours; document ids 0, 255, 256, 32768, 65535 (n_docs permitting).
    Returns (raw, letters)."""
    rng = np.random.default_rng(seed)
    letters = WIDE_ALPHABETS[seed % len(WIDE_ALPHABETS)]
    sigma = len(letters)
    idx = np.cumsum(rng.integers(1, sigma, size=r)) % sigma  # steps of 1 .. sigma-1: neighbours differ
    heads = np.asarray(letters, dtype=np.uint8)[idx].copy()
    lens = rng.integers(1, 6, size=r).astype(np.int64)
    big = np.flatnonzero(rng.random(r) < share)
    big = big[big != r // 2]
    assert big.size >= 8
    e = rng.integers(16, 38, size=big.size)
    lens[big] = (1 << e) + (rng.random(big.size) * (1 << e)).astype(np.int64)
    heads[r // 2], lens[r // 2] = 0, 1
    room = 1 << 39  # what the top-up adds at least: the longest run has 2^39 positions or more, a 40-bit length
    assert n > (1 << 38)
    while int(lens.sum()) > n - room:
        j = big[np.argmax(lens[big])]
        lens[j] //= 2
    top = big[int(rng.integers(0, big.size))]
    lens[top] += n - int(lens.sum())
    assert int(lens.sum()) == n and lens.min() >= 1
    raw = synth.raw_from_runs(torch.from_numpy(heads), torch.from_numpy(lens), seed, with_samples=True, n_docs=n_docs)
    assert raw.n == n
    sa_corners = [n - 1, 0, 1 << 24, 1 << 31, 1 << 32, 1 << 39, (1 << 32) - 1, (1 << 39) | (1 << 24) | 1, n - 2, (1 << 39) - 1]
    doc_corners = [d for d in (0, 255, 256, 32768, 65535) if d < n_docs]
    # a walk spends its time inside the long runs, so the runs its jumps land on are their neighbours: the corners go there
    # (samples_start / start_runs_doc of the run after a long one, samples_last / end_runs_doc of the run before)
    for arr, corners, step, shift in ((raw.ssa, sa_corners, 1, 0), (raw.esa, sa_corners, -1, 5), (raw.doc_start, doc_corners, 1, 1),
                                      (raw.doc_end, doc_corners, -1, 3)):
        at = big[::(7 if corners is sa_corners else 4)] + step
        at = at[(at != r // 2) & (at > 0) & (at < r - 1)]  # (not the last run: every read starts there)
        arr[torch.from_numpy(at)] = torch.tensor([corners[(i + shift) % len(corners)] for i in range(at.size)], dtype=torch.int64)
    # every read starts on the last run's sample and document id, and a matching read keeps them: wide ones
    if int(raw.esa[r - 1]) < (1 << 32):
        raw.esa[r - 1] += 1 << 39
    if n_docs > 256 and int(raw.doc_end[r - 1]) < 256:
        raw.doc_end[r - 1] += 256
    return raw, letters


def wide_reads(raw, letters, seed, nreads=600, length=60):
    """simulate_reads at positive fractions 0, 0.5 and 1 (`nreads` each), 3 % of the characters replaced by letters
    the index does not have -- one below 128, one above."""
    parts = [synth.simulate_reads(raw, nreads, length, seed=seed * 3 + i, positive_fraction=pf)[0].numpy()
             for i, pf in enumerate((0.0, 0.5, 1.0))]
    seqs = np.concatenate(parts).copy()
    rng = np.random.default_rng(seed + 77)
    absent = [[c for c in range(2, 128) if c not in letters][0], [c for c in range(255, 127, -1) if c not in letters][0]]
    hit = rng.random(seqs.size) < 0.03
    seqs[hit] = np.asarray(absent, dtype=np.uint8)[rng.integers(0, 2, size=int(hit.sum()))]
    offs = np.arange(3 * nreads + 1, dtype=np.int64) * length
    return seqs, offs


def wide_reach(raw, want_ms, want_docs):
    """What a test on a wide index must reach, asserted on its inputs and on the oracle's answers so that it cannot
    pass vacuously; returns the measured shares."""
    n = raw.n
    ptr = want_ms["pointers"].astype(np.uint64)
    wrapped = ptr >= (1 << 63)  # `sample--` below zero (the reference prints them as 20-digit numbers)
    got = dict(longest_run=int(raw.lens.max()), ptr_ge_2_32=float((ptr >= (1 << 32)).mean()),
               ptr_bits=int(ptr[~wrapped].max()).bit_length(), ptr_wrapped=int(wrapped.sum()),
               doc_ge_256=float((want_docs >= 256).mean()), doc_max=int(want_docs.max()))
    assert got["longest_run"] >= (1 << 39), got  # a length of 40 bits: offsets inside that run set bits 38 and 39
    assert got["ptr_ge_2_32"] >= 0.90 and got["ptr_bits"] == 40 and int(ptr[~wrapped].max()) < n, got
    assert got["doc_ge_256"] >= 0.90 and got["doc_max"] >= (1 << 15), got
    for arr in (raw.doc_start, raw.doc_end):
        assert set((0, 255, 256, 32768, 65535)) <= set(arr.tolist())
    for arr in (raw.ssa, raw.esa):
        vals = arr.numpy()
        assert (vals == n - 1).any() and (vals == 0).any()
        for bit in (24, 31, 32, 39):
            assert (vals == (1 << bit)).any()
    return got


def walk_offsets(orc, raw, seqs, offs, nreads=40):
    """The offsets inside their runs of the positions the reference's backward search visits on the first `nreads` reads
    (compute_ms_pml.cpp:238-286, followed with the oracle's primitives): what the walk's `off`, LFoff + off and the
    threshold comparison have to hold.  Vacuity measure only: no result is compared with it."""
    n = orc.n
    starts = (torch.cumsum(raw.lens, 0) - raw.lens).numpy()
    out = []
    for q in range(min(nreads, offs.size - 1)):
        pos = n - 1
        for c in seqs[offs[q]: offs[q + 1]][::-1].tolist():
            nc = orc.rank(n, c)
            if nc > 0 and not (pos < n and orc.at(pos) == c and c < 128):
                rnk = orc.rank(pos, c)
                thr, nxt = n + 1, pos
                if rnk < nc:
                    nxt = orc.select(rnk, c)
                    thr = orc.threshold(orc.run_of_position(nxt))
                if pos < thr and rnk > 0:
                    nxt = orc.select(rnk - 1, c)
                pos = nxt
            pos = orc.LF(pos, c)
            if pos < n:
                out.append(pos - int(starts[np.searchsorted(starts, pos, side="right") - 1]))
    return np.asarray(out, dtype=np.uint64)


# ---- the bin-max classifier over bin widths and thresholds (test_classify_cpu.py, test_gpu_classify.py) ----
CLASSIFY_LENGTHS = [0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 1000,
                    1023, 1024, 1025]
# w - 1, w, w + 1 (and 2 w - 1, 2 w, 2 w + 1, as a width or through the read lengths above) for the sizes the kernels count
# in: 8 values per 16-byte load, the 64-character flush word of k_walk_fast, the tiles of 256 / 512 values of
# k_classify_tiles; a read's length +- 1 (1000); 2^16 and 2^32 and their neighbours; one bin whatever the read (2^40, 2^63)
CLASSIFY_WIDTHS = [1, 2, 3, 7, 8, 9, 63, 64, 65, 128, 150, 255, 256, 257, 511, 512, 513, 999, 1000, 1001, 65535, 65536, 1 << 31,
                   (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 32) + 7, (1 << 32) + 64, 1 << 40, 1 << 63]


def classify_thresholds(lengths):
    """0, 1, the median and the maximum of `lengths`, max + 1, and the values around the widths an implementation may have
    narrowed the threshold to (16, 32 and 64 bits)."""
    v = np.sort(np.asarray(lengths, dtype=np.uint64))
    med, mx = int(v[v.size // 2]), int(v[-1])
    out = []
    for t in (0, 1, med, mx, mx + 1, 65535, 65536, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 64) - 1):
        if t not in out:
            out.append(t)
    return out, med, mx


def classify_bins(m, w):
    """The rule of compute_ms_pml.cpp:969-995 in plain integers: the bins [k w, (k + 1) w) of a read of m values, the last
    one taking the rest when fewer than w values would remain, and one bin at least for m > 0."""
    if m == 0:
        return []
    nb = max(1, m // w)
    return [(k * w, (k + 1) * w if k + 1 < nb else m) for k in range(nb)]


def classify_rule(lengths, offs, w, thr):
    """(above, below, sum_max) per read as lists of Python integers: a bin is above iff its maximum >= thr."""
    vals = [int(v) for v in lengths]
    out = []
    for q in range(len(offs) - 1):
        base, m = int(offs[q]), int(offs[q + 1]) - int(offs[q])
        mx = [max(vals[base + lo: base + hi]) for lo, hi in classify_bins(m, w)]
        above = sum(1 for v in mx if v >= thr)
        out.append((above, len(mx) - above, sum(mx)))
    return out


def classify_case(seed=5, n=6000, random_reads=30):
    """(raw, text, seqs, offs): an index with text, SA samples and documents over `n` characters, and reads of every length
    in CLASSIFY_LENGTHS twice -- once cut from the text with a few substitutions (long matches: large values), once random
    letters (values of a few units) -- plus `random_reads` reads of 1 .. 1200 characters, half of either kind, with runs of
    empty reads at the front, in the middle and at the end."""
    letters = list(b"ACGT")
    raw, text = real_case(seed, n, letters, ndocs=3)
    rng = np.random.default_rng(seed + 100)
    lens = [(m, kind) for m in CLASSIFY_LENGTHS for kind in (0, 1)]
    # (of the random lengths the longer half is cut from the text: most characters then carry large values, the median
    # lies among them, and a stretch of random letters inside such a read is a run of bins below it)
    extra = sorted(int(x) for x in rng.integers(1, 1201, size=random_reads))
    lens += [(m, 1 if q < random_reads // 2 else 0) for q, m in enumerate(extra)]
    order = rng.permutation(len(lens))
    lens = [lens[i] for i in order]
    half = len(lens) // 2
    lens = [(0, 0)] * 3 + lens[:half] + [(0, 0)] * 3 + lens[half:] + [(0, 0)] * 3
    reads = []
    for m, kind in lens:
        if kind == 0 and m:
            s = int(rng.integers(0, text.size - m))
            rd = text[s: s + m].copy()
            for _ in range(m // 150):  # a substitution every 150 characters or so: the values fall and rise inside a read
                rd[rng.integers(0, m)] = letters[rng.integers(0, 4)]
            if m >= 400:  # and a stretch of random letters, longer than two bins of 64
                at = int(rng.integers(0, m - 160))
                rd[at: at + 160] = np.asarray(letters, dtype=np.uint8)[rng.integers(0, 4, size=160)]
        else:
            rd = np.asarray(letters, dtype=np.uint8)[rng.integers(0, 4, size=m)]
        reads.append(rd.astype(np.uint8))
    offs = np.concatenate([[0], np.cumsum([r.size for r in reads])]).astype(np.int64)
    return raw, text, np.concatenate(reads), offs


def classify_conditions(oracle_mod, lengths, offs):
    """What a classifier test needs from its batch, asserted on the oracle's answers so that it cannot pass vacuously:
    at the median threshold and bins of 8 and of 64 some read has bins above and bins below at once; some read has more
    than one bin and a length that is no multiple of the width; nothing is below threshold 0, nothing above max + 1."""
    _, med, mx = classify_thresholds(lengths)
    m = np.diff(np.asarray(offs, dtype=np.int64))
    for w in (8, 64):
        _, a, b, _ = oracle_mod.classify(lengths, offs, w, med)
        assert ((a > 0) & (b > 0)).any(), (w, med)
        assert ((a + b > 1) & (m % w != 0)).any(), w
    _, a, b, _ = oracle_mod.classify(lengths, offs, 8, 0)
    assert a.any() and not b.any()
    _, a, b, _ = oracle_mod.classify(lengths, offs, 8, mx + 1)
    assert b.any() and not a.any()
    return med, mx
