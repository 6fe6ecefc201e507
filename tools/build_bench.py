"""Index build times: the HIP builder (capi.build_raw, include/spumoni_build.h) against the torch prefix doubling
(synth.index_from_text) on the same device, alternating, on the texts of bench.py's two real-BWT legs; then a digested
pangenome-like text past 2^31 characters with the HIP builder alone, and the walk on its index at the declared table
density.  Per-phase times and peak device bytes of the HIP builder go to stderr (SPX_TIMING=1, set here).

    python tools/build_bench.py [--legs digest,ms,large] [--reps 2] [--large-n 2.4e9] [--large-sub 0.1]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["SPX_TIMING"] = "1"
os.environ.setdefault("SPX_FAT_SLOTS_PER_RUN", "6.8")  # the table density the declared C3 index gets (tools/real_ab.py)
from spumoni_amd import capi, synth  # noqa: E402

dev = torch.device("cuda:0")


def log(msg):
    print(msg, flush=True)
    print(msg, file=sys.stderr, flush=True)


def haplotypes(genome_bp, count=10):
    base = synth.random_genome(genome_bp, seed=1)
    return [base] + [synth.mutate(base, seed=sd) for sd in range(2, count + 1)]


def digest_text():
    """real_bwt_digest_walk: 10 haplotypes of a 20 Mbp genome + reverse complements, digested -m k=4 w=11"""
    dig = capi.digester(0)
    parts = []
    for g in haplotypes(20_000_000):
        for seq in (g, synth.revcomp(g)):
            d, _ = dig.digest_host(capi.SPX_DIGEST_PROMOTED, 4, 11, seq, np.array([0, seq.size], dtype=np.uint64))
            parts.append(d.copy())
    dig.close()
    return np.concatenate(parts), None


def ms_text():
    """real_bwt_ms_doc: the same 10 haplotypes un-digested (n = 4 * 10^8), one document each"""
    return synth.pangenome_text(haplotypes(20_000_000))


def hip(text, docs):
    torch.cuda.synchronize()
    t0 = time.time()
    raw = capi.build_raw(text, doc_lengths=docs, with_samples=docs is not None)
    return raw, time.time() - t0


def torch_build(text, docs):
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(0)
    torch.cuda.synchronize()
    t0 = time.time()
    raw = synth.index_from_text(torch.from_numpy(text).to(dev), doc_lengths=docs, with_samples=docs is not None).cpu()
    torch.cuda.synchronize()
    dt = time.time() - t0
    peak = torch.cuda.max_memory_allocated(0)
    torch.cuda.empty_cache()
    return raw, dt, peak


def compare(name, text, docs, reps):
    n = text.size + 1
    log(f"== {name}: n = {n}, documents = {0 if docs is None else len(docs)}, samples = {docs is not None}")
    ht, tt = [], []
    for rep in range(reps):
        a, dt = hip(text, docs)
        ht.append(dt)
        log(f"[{name}] rep {rep} HIP   {dt:8.2f} s  r = {a.r}")
        b, dt, peak = torch_build(text, docs)
        tt.append(dt)
        log(f"[{name}] rep {rep} torch {dt:8.2f} s  peak {peak / 1e9:.2f} GB ({peak / n:.1f} B/char)")
        same = a.n == b.n and all(
            (getattr(a, f) is None and getattr(b, f) is None) or torch.equal(getattr(a, f), getattr(b, f).to(getattr(a, f).dtype))
            for f in ("heads", "lens", "thr", "ssa", "esa", "doc_start", "doc_end"))
        log(f"[{name}] rep {rep} arrays identical: {same}")
        del a, b
    log(f"[{name}] median HIP {np.median(ht):.2f} s, torch {np.median(tt):.2f} s, speed-up {np.median(tt) / np.median(ht):.1f}x")


def large(n_target, sub):
    """A digested pangenome-like text: copies of a random 253-letter text (the promoted-minimizer alphabet), each with
    a fraction `sub` of its letters substituted, concatenated; HIP builder only (the torch builder does not fit)."""
    copies = 20
    L = int(n_target) // copies
    rng = np.random.default_rng(5)
    t0 = time.time()
    base = (3 + rng.integers(0, 253, size=L)).astype(np.uint8)
    parts = []
    for c in range(copies):
        p = base.copy()
        if c:
            pos = np.nonzero(rng.random(L) < sub)[0]
            p[pos] = (3 + rng.integers(0, 253, size=pos.size)).astype(np.uint8)
        parts.append(p)
    text = np.concatenate(parts)
    del parts
    log(f"== large: n = {text.size + 1} ({copies} copies of {L}, {sub:.2f} substituted), text made in {time.time() - t0:.1f} s")
    raw, dt = hip(text, None)
    log(f"[large] HIP {dt:.2f} s  n = {raw.n}  r = {raw.r}  n/r = {raw.n / raw.r:.2f}")
    raw = synth.RawIndex(heads=raw.heads, lens=raw.lens, thr=raw.thr, n=raw.n)
    t0 = time.time()
    ix = capi.Index.from_raw(raw, 0)
    desc = ix.describe()
    log(f"[large] index from the runs in {time.time() - t0:.1f} s, fat slots per run {desc.get('fat_slots_per_run')}")
    # reads: 64-letter substrings of the text with 2 % substitutions, half reversed (null model)
    nreads, ln = 4_000_000, 64
    start = rng.integers(0, text.size - ln, size=nreads)
    reads = text[start[:, None] + np.arange(ln)[None, :]]
    e = rng.random(reads.shape) < 0.02
    reads[e] = (3 + rng.integers(0, 253, size=int(e.sum()))).astype(np.uint8)
    null = rng.random(nreads) < 0.5
    reads[null] = reads[null, ::-1]
    d_seqs = capi.pad_seqs(torch.from_numpy(np.ascontiguousarray(reads.reshape(-1))).to(dev))
    offs = torch.arange(nreads + 1, dtype=torch.int64, device=dev) * ln
    d_len = torch.empty(nreads * ln, dtype=torch.int32, device=dev)
    d_cls = torch.empty((nreads, 2), dtype=torch.int64, device=dev)
    kms = []
    for _ in range(4):
        ix.query_device(capi.SPX_MODE_PML, d_seqs, offs, nreads * ln, d_lengths=d_len, d_class=d_cls, bin_width=50,
                        max_value_thr=5)
        torch.cuda.synchronize()
        kms.append(ix.last_stats()["kernel_ms"])
    st = ix.last_stats()
    km = float(np.median(kms[1:]))
    log(f"[large] walk (PML, {nreads} x {ln} letters): {km:.2f} ms, {st['steps'] / km / 1e6:.2f} G steps/s, "
        f"f_mis {st['jumps'] / st['steps']:.3f}, rows/step {st['row_loads'] / st['steps']:.3f}")
    ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="digest,ms,large")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--large-n", type=float, default=2.4e9)
    ap.add_argument("--large-sub", type=float, default=0.1)
    a = ap.parse_args()
    legs = a.legs.split(",")
    if "digest" in legs:
        t, d = digest_text()
        compare("real_bwt_digest_walk text", t, d, a.reps)
        del t
    if "ms" in legs:
        t, d = ms_text()
        compare("real_bwt_ms_doc text", t, d, a.reps)
        del t
    if "large" in legs:
        large(a.large_n, a.large_sub)


if __name__ == "__main__":
    main()
