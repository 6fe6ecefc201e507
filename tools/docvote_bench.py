"""Measures the document votes; the output is kept as profiles/docvote_bench.txt.

  1. the vote kernels against the walk that feeds them: same batch, same device, HIP-event times (spx_last_walk_stats /
     spv_last_votes_stats), median of --reps after a warm-up, and the votes' bytes per second beside a plain device copy
     of the same bytes;
  2. Index.assign_host against what a caller did before it existed: Index.digest_query_host(want_docs=True) +
     docvote.votes_reference, wall clock, median of --reps after a warm-up;
  3. `spumoni assign` against `spumoni run -P -d` on the same reads file on tmpfs, process start to process gone.

    python tools/docvote_bench.py [--runs R] [--reps N] [--skip-cli] [--label TEXT]
"""
import argparse
import os
import shutil
import socket
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spumoni_amd import capi, synth  # noqa: E402
from spumoni_amd.docvote import votes_reference  # noqa: E402

BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")


def med(xs):
    return statistics.median(xs)


def copy_ms(nbytes, reps):
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps + 1):
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return med(ts[1:])


def kernels_against_walk(ix, name, seqs, offs, bits, min_length, reps):
    total, nreads = seqs.numel(), offs.numel() - 1
    dt = torch.int16 if bits == 16 else torch.int32
    d_seqs = capi.pad_seqs(seqs)
    d_len = torch.empty(total + 16, dtype=dt, device="cuda")
    d_doc = torch.empty(total + 16, dtype=dt, device="cuda")
    out = torch.empty((nreads, 4), dtype=torch.int32, device="cuda")
    walk, vote = [], []
    for _ in range(reps + 1):
        ix.query_device(capi.SPX_MODE_PML, d_seqs, offs, total, d_lengths=d_len, d_docs=d_doc)
        ix.votes_device(d_len, d_doc, offs, min_length, d_out=out)
        torch.cuda.synchronize()
        walk.append(ix.last_stats()["kernel_ms"])
        st = ix.votes_stats()
        vote.append(st["kernel_ms"])
    w, v = med(walk[1:]), med(vote[1:])
    nbytes = 2 * total * (bits // 8) + nreads * 24  # lengths + ids read, an offset read and a record written per read
    c = copy_ms(nbytes, reps)
    print(f"{name}: {nreads} reads, {total} values, {bits}-bit, min_length {min_length}\n"
          f"    walk (k_walk_fast<PML, DOC>)  {w:9.3f} ms   (min {min(walk[1:]):.3f}, max {max(walk[1:]):.3f})\n"
          f"    vote kernels                  {v:9.3f} ms   (min {min(vote[1:]):.3f}, max {max(vote[1:]):.3f})   = {100 * v / w:.1f} % of the walk\n"
          f"    votes: {nbytes / 1e9:.3f} GB in {v:.3f} ms = {nbytes / v / 1e6:.0f} GB/s; a device copy of as many bytes: {c:.3f} ms = "
          f"{nbytes / c / 1e6:.0f} GB/s read (and as much written)\n"
          f"    reads by path: short {st['reads_short']}, medium {st['reads_medium']}, long {st['reads_long']} "
          f"({st['long_tiles']} tiles), empty {st['reads_empty']}; voting positions {st['voting_positions']}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    torch.cuda.set_device(0)
    print(f"docvote_bench: {a.label}\nhost {socket.gethostname()}, {torch.cuda.get_device_name(0)}, library {capi.version()}\n"
          f"index: synth.statistical_rlbwt(r={a.runs}, sigma=253, mean_run=6, zipf=1, SA samples, 10 documents)\n", flush=True)

    raw = synth.statistical_rlbwt(a.runs, 253, 6.0, seed=3, device="cuda:0", zipf=1.0, with_samples=True, n_docs=10)
    ix = capi.Index.from_raw(raw, 0)
    print("== 1. vote kernels against the walk that feeds them (HIP events, median of %d) ==" % a.reps, flush=True)
    for name, nreads, m in (("C3 shape", 10_000_000, 44), ("C4 shape", 5_000_000, 55)):
        seqs, offs = synth.simulate_reads(raw, nreads, m, seed=13, positive_fraction=0.5)
        kernels_against_walk(ix, name, seqs, offs, 16, 5, a.reps)
        del seqs, offs
    # heavy-tailed: Pareto lengths (median 26, some tens of thousands) and one read of 10^6 values; 32-bit arrays
    rng = np.random.default_rng(5)
    lens = np.minimum((rng.pareto(1.1, 1_000_000) * 30).astype(np.int64) + 1, 200_000)
    lens[rng.integers(0, lens.size)] = 1_000_000
    pool, pool_offs = synth.simulate_reads(raw, 20_000, 10_000, seed=14, positive_fraction=0.5)
    total = int(lens.sum())
    reps_needed = (total + pool.numel() - 1) // pool.numel()
    seqs = pool.repeat(reps_needed)[:total].contiguous()
    offs = torch.from_numpy(np.r_[0, np.cumsum(lens)].astype(np.int64)).cuda()
    kernels_against_walk(ix, "heavy-tailed mix with one read of 10^6 values", seqs, offs, 32, 5, a.reps)
    del seqs, offs, pool
    ix.close()
    del raw
    torch.cuda.empty_cache()

    print("\n== 2. host form: assign_host against digest_query_host + votes_reference (wall clock, median of %d) ==" % a.reps, flush=True)
    raw = synth.statistical_rlbwt(min(a.runs, 5_000_000), 253, 6.0, seed=4, device="cuda:0", zipf=1.0, with_samples=True, n_docs=10)
    ix = capi.Index.from_raw(raw, 0)
    rng = np.random.default_rng(6)
    nreads = 1_000_000
    seqs = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, nreads * 200)]
    offs = (np.arange(nreads + 1, dtype=np.uint64) * 200)
    kind, k, w = capi.SPX_DIGEST_PROMOTED, 4, 11
    new, old_q, old_v = [], [], []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        got = ix.assign_host(capi.SPX_MODE_PML, seqs, offs, 5, digest=(kind, k, w))
        new.append(time.perf_counter() - t0)
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        r = ix.digest_query_host(capi.SPX_MODE_PML, kind, k, w, seqs, offs, want_docs=True)
        t1 = time.perf_counter()
        want = votes_reference(r["lengths"], r["docs"], r["offsets"], 5)
        old_q.append(t1 - t0)
        old_v.append(time.perf_counter() - t1)
    same = all(np.array_equal(got[f], want[f]) for f in want.dtype.names)
    values = int(r["offsets"][-1])
    print(f"{nreads} x 200 bp, -m digestion (k=4, w=11) to {values} values; records equal: {same}\n"
          f"    assign_host                              {med(new[1:]):8.3f} s   (min {min(new[1:]):.3f}, max {max(new[1:]):.3f})\n"
          f"    digest_query_host (lengths + ids back)   {med(old_q[1:]):8.3f} s\n"
          f"    + votes_reference on the host            {med(old_v[1:]):8.3f} s   together {med(old_q[1:]) + med(old_v[1:]):.3f} s = "
          f"{(med(old_q[1:]) + med(old_v[1:])) / med(new[1:]):.1f} x assign_host", flush=True)
    assert same
    ix.close()

    if a.skip_cli:
        return
    print("\n== 3. CLI, process start to process gone, reads file and outputs on tmpfs ==", flush=True)
    from spumoni_amd.build_index import write_doc_array

    work = tempfile.mkdtemp(prefix="docvote_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        raw = synth.statistical_rlbwt(2_000_000, 4, 20.0, seed=8, device="cuda:0", letters=b"ACGT", with_samples=True, n_docs=10)
        rs, ro = synth.simulate_reads(raw, nreads, 150, seed=9, positive_fraction=0.5)
        raw = raw.cpu()
        prefix = os.path.join(work, "ref.fa")
        open(prefix, "w").write(">dummy\n")
        raw.write_raw_files(prefix)
        write_doc_array(prefix + ".doc", raw.doc_start.numpy(), raw.doc_end.numpy(), 10)
        rs = rs.cpu().numpy().reshape(nreads, 150)
        reads = os.path.join(work, "reads.fa")
        with open(reads, "wb") as f:
            for i in range(0, nreads, 10000):
                f.write(b"".join(b">read_%d\n%s\n" % (q, rs[q].tobytes()) for q in range(i, min(nreads, i + 10000))))
        del rs, ro
        torch.cuda.empty_cache()
        env = dict(os.environ, SPUMONI_GPUS="0")
        res = {}
        for name, cmd in (("run -P -d -n", [BIN, "run", "-r", prefix[:-3], "-p", reads, "-P", "-d", "-n"]),
                          ("assign -P -n", [BIN, "assign", "-r", prefix[:-3], "-p", reads, "-P", "-n"])):
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                p = subprocess.run(cmd, capture_output=True, env=env, timeout=600)
                ts.append(time.perf_counter() - t0)
                assert p.returncode == 0, p.stderr.decode()[-2000:]
            res[name] = ts
        out_run = os.path.getsize(reads + ".pseudo_lengths") + os.path.getsize(reads + ".doc_numbers")
        out_assign = os.path.getsize(reads + ".assignments") + os.path.getsize(reads + ".assignments.by_doc")
        print(f"{nreads} x 150 bp, index of 2*10^6 runs with 10 documents, no digestion\n"
              f"    spumoni run -P -d -n   {med(res['run -P -d -n']):7.3f} s  (runs: {', '.join('%.3f' % t for t in res['run -P -d -n'])}); writes {out_run / 1e6:.1f} MB\n"
              f"    spumoni assign -P -n   {med(res['assign -P -n']):7.3f} s  (runs: {', '.join('%.3f' % t for t in res['assign -P -n'])}); writes {out_assign / 1e6:.1f} MB",
              flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
