"""Brute-force ground truth (first principles, no oracle / product code): Python for tiny texts, tests/brute_index.c
for the index of texts up to about 10^6 characters."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np


def naive_sa(t):
    """t: list of ints incl. terminator (unique smallest, last). Returns suffix array."""
    n = len(t)
    return sorted(range(n), key=lambda i: t[i:])


def naive_bwt(t):
    sa = naive_sa(t)
    n = len(t)
    return sa, [t[(s - 1) % n] for s in sa]


def naive_lcp(t, sa):
    n = len(t)
    lcp = [0] * n
    for i in range(1, n):
        a, b = sa[i - 1], sa[i]
        l = 0
        while a + l < n and b + l < n and t[a + l] == t[b + l]:
            l += 1
        lcp[i] = l
    return lcp


def runs_of(bwt):
    heads, lens = [], []
    for c in bwt:
        if heads and heads[-1] == c:
            lens[-1] += 1
        else:
            heads.append(c)
            lens.append(1)
    return heads, lens


def true_ms(text, read):
    """Matching statistics: ms[i] = longest prefix of read[i:] that occurs in text."""
    tb = bytes(text)
    rb = bytes(read)
    m = len(rb)
    out = []
    for i in range(m):
        l = 0
        while i + l < m and tb.find(rb[i : i + l + 1]) >= 0:
            l += 1
        out.append(l)
    return out


def rank_brute(bwt, p, c):
    return sum(1 for x in bwt[:p] if x == c)


def select_brute(bwt, i, c):
    cnt = 0
    for p, x in enumerate(bwt):
        if x == c:
            if cnt == i:
                return p
            cnt += 1
    raise IndexError


# ---------------------------------------------------------------------------------------------
# the index of a text (include/spumoni_build.h, synth.index_from_text) from first principles
INDEX_FIELDS = ("heads", "lens", "thr", "ssa", "esa", "doc_start", "doc_end")


def _brute_spec(text, doc_lengths):
    """The specification restated over naive_sa / naive_lcp: for texts of a few hundred characters."""
    t = list(text) + [0]
    n = len(t)
    sa = naive_sa(t)
    lcp = naive_lcp(t, sa)
    bwt = [t[(s - 1) % n] for s in sa]
    starts = [i for i in range(n) if i == 0 or bwt[i] != bwt[i - 1]]
    ends = [s - 1 for s in starts[1:]] + [n - 1]
    heads = [bwt[s] for s in starts]
    thr, last_end = [], {}
    for k, c in enumerate(heads):
        if c in last_end:
            lo, hi = last_end[c] + 1, starts[k]
            thr.append(min(range(lo, hi + 1), key=lambda i: (lcp[i], i)))
        else:
            thr.append(0)
        last_end[c] = ends[k]
    ssa = [(sa[s] - 1) % n for s in starts]
    esa = [(sa[e] - 1) % n for e in ends]
    cum = np.cumsum(doc_lengths)
    cum[-1] += 1
    ds = np.searchsorted(cum, ssa, side="right")
    de = np.searchsorted(cum, esa, side="right")
    return dict(heads=heads, lens=[e - s + 1 for s, e in zip(starts, ends)], thr=thr, ssa=ssa, esa=esa,
                doc_start=ds.tolist(), doc_end=de.tolist())


BRUTE_INDEX_C = os.path.join(os.path.dirname(os.path.abspath(__file__)), "brute_index.c")
_brute_index_lib = None  # (the ctypes library, the temporary directory that holds it)


def _index_lib():
    """tests/brute_index.c compiled with gcc into a temporary directory, once per process."""
    global _brute_index_lib
    if _brute_index_lib is None:
        d = tempfile.TemporaryDirectory(prefix="brute_index_")
        so = os.path.join(d.name, "libbrute_index.so")
        subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", so, BRUTE_INDEX_C], check=True)
        L = C.CDLL(so)
        vp = C.c_void_p
        L.brute_index.restype = C.c_int
        L.brute_index.argtypes = [vp, C.c_uint64, vp, C.c_uint32] + [vp] * 10
        _brute_index_lib = (L, d)
    return _brute_index_lib[0]


class BruteIndex:
    """What brute_index.c computed: n, r, sa and lcp (n entries each) and the seven fields (r entries each; the
    document ids are None without doc_lengths, samples and ids are None where `with_samples` was false)."""

    def __init__(self, text, doc_lengths=None, with_samples=True):
        text = np.ascontiguousarray(text, dtype=np.uint8)
        n = text.size + 1
        dl = None if doc_lengths is None else np.ascontiguousarray(np.asarray(list(doc_lengths), dtype=np.uint64))
        self.n = n
        self.sa, self.lcp = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
        heads = np.empty(n, dtype=np.uint8)
        six = [np.zeros(n, dtype=np.uint64) for _ in range(6)]
        r = C.c_uint64(0)

        def ptr(a):
            return None if a is None else a.ctypes.data

        rc = _index_lib().brute_index(ptr(text), text.size, ptr(dl), 0 if dl is None else dl.size, ptr(self.sa), ptr(self.lcp),
                                      C.addressof(r), ptr(heads), *[ptr(a) for a in six])
        if rc != 0:
            raise ValueError("brute_index refused the text (empty, a byte below 2, or document lengths that do not sum to it)")
        self.r = r = int(r.value)
        lens, thr, ssa, esa, ds, de = (a[:r].astype(np.int64) for a in six)
        self.heads, self.lens, self.thr = heads[:r].copy(), lens, thr
        self.ssa, self.esa = (ssa, esa) if with_samples else (None, None)
        self.doc_start, self.doc_end = (ds, de) if with_samples and dl is not None else (None, None)

    def mismatches(self, got):
        """Names of the fields in which `got` (a synth.RawIndex, or anything with these attributes as tensors or
        arrays) differs from this answer; ["n"] if the sizes differ."""
        if int(got.n) != self.n:
            return ["n"]
        bad = []
        for f in INDEX_FIELDS:
            a, b = getattr(got, f), getattr(self, f)
            if (a is None) != (b is None):
                bad.append(f)
            elif a is not None:
                a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
                if a.shape != b.shape or not np.array_equal(a.astype(np.int64), b.astype(np.int64)):
                    bad.append(f)
        return bad


# ---------------------------------------------------------------------------------------------
# matching statistics of a batch of reads from first principles (tests/brute_ms.c: binary search over `sa`)
BRUTE_MS_C = os.path.join(os.path.dirname(os.path.abspath(__file__)), "brute_ms.c")
_brute_ms_lib = None


def _ms_lib():
    """tests/brute_ms.c compiled with gcc into a temporary directory, once per process."""
    global _brute_ms_lib
    if _brute_ms_lib is None:
        d = tempfile.TemporaryDirectory(prefix="brute_ms_")
        so = os.path.join(d.name, "libbrute_ms.so")
        subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", so, BRUTE_MS_C], check=True)
        L = C.CDLL(so)
        vp = C.c_void_p
        L.brute_ms.restype = C.c_int
        L.brute_ms.argtypes = [vp, C.c_uint64, vp, vp, vp, C.c_uint64, vp]
        _brute_ms_lib = (L, d)
    return _brute_ms_lib[0]


def brute_ms(text, sa, seqs, offs):
    """The matching statistic of every position of every read (uint32, offs[-1] values): the longest prefix of
    read[i:] that occurs in `text`.  sa: the suffix array of text + terminator (BruteIndex.sa)."""
    text = np.ascontiguousarray(text, dtype=np.uint8)
    sa = np.ascontiguousarray(sa, dtype=np.uint32)
    seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    if sa.size != text.size + 1 or offs.size < 1 or int(offs[-1]) > seqs.size:
        raise ValueError("brute_ms: sa has n_text + 1 entries, offs ends inside seqs")
    tot = int(offs[-1])
    out = np.zeros(max(tot, 1), dtype=np.uint32)
    pad = np.concatenate([seqs, np.zeros(1, dtype=np.uint8)])  # (a valid address for an empty batch)
    rc = _ms_lib().brute_ms(text.ctypes.data, text.size, sa.ctypes.data, pad.ctypes.data, offs.ctypes.data, offs.size - 1,
                            out.ctypes.data)
    if rc != 0:
        raise ValueError("brute_ms refused its input (sa is no permutation, or offsets that fall)")
    return out[:tot]


# ---------------------------------------------------------------------------------------------
# minimizer digestion, written as a specification (slices and min(), no queue): what
# oracle/orc_digest.c and the HIP kernel must both produce.  See DESIGN.md 4.4 for the
# assumptions about bonsai this encodes.
LEX_XOR_MASK = 0xE37E28C4271B5A2D


def digest_spec(kind, k, w, seq: bytes, charhash):
    """kind 1: -m (promoted), kind 2: -a (DNA letters).  charhash: T[A], T[C], T[G], T[T]."""
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    wsz = max(1, w - k + 1)

    def rotl8(x, s):
        s %= 8
        return ((x << s) | (x >> (8 - s))) & 0xFF if s else x

    stream = []  # (score, element) of every k-mer made of ACGT only, in read order
    for i in range(k - 1, len(seq)):
        win = seq[i - k + 1 : i + 1]
        if any(c not in code for c in win):
            continue
        if kind == 2:
            km = 0
            for c in win:
                km = km * 4 + code[c]
            stream.append((km ^ LEX_XOR_MASK, km))
        else:
            h = 0
            for j, c in enumerate(win):
                h ^= rotl8(charhash[code[c]], k - 1 - j)
            stream.append((h, h))
    reports = [min(stream[t - wsz + 1 : t + 1])[1] for t in range(wsz - 1, len(stream))]
    out = bytearray()
    last = None
    for x in reports:
        if last is None or (last & 0xFF) != x:  # mseq_vec is a vector<uint8_t>
            last = x
            if kind == 2:
                out += bytes("ACGT"[(x >> (2 * (k - 1 - j))) & 3].encode()[0] for j in range(k))
            else:
                out.append(x if x > 2 else x + 3)
    return bytes(out)
