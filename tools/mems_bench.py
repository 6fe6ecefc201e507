"""Measures the matches; the output is kept as profiles/mems_bench.txt.

  1. the match kernels against the MS walk + k_ms_extend that feed them: same batch, same device, HIP-event times
     (events around the MS query; spm_last_mems_stats), median of --reps after a warm-up, and the kernels' bytes per
     second beside a plain device copy of as many bytes (all lengths, the pointers at reported starts, the records);
  2. Index.mems_host against what a caller did before it existed: Index.query_host (lengths + pointers back) +
     mems.mems_reference, wall clock, median of --reps after a warm-up;
  3. `spumoni mems` against `spumoni run -M` on the same reads file on tmpfs, process start to process gone.

The index is a real one (capi.build_raw over a repetitive DNA text), so that the MS lengths mean something.

    python tools/mems_bench.py [--text N] [--reps N] [--skip-cli] [--label TEXT]
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
from spumoni_amd import capi  # noqa: E402
from spumoni_amd.mems import mems_reference  # noqa: E402

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


def repetitive_text(rng, n):
    """Mutated copies of one random DNA sequence of n / 8 letters, back to back."""
    base = rng.integers(0, 4, n // 8)
    text = np.tile(base, 9)[:n]
    flip = rng.random(n) < 0.01
    text[flip] = rng.integers(0, 4, int(flip.sum()))
    return np.frombuffer(b"ACGT", dtype=np.uint8)[text]


def reads_from(text, lens, rng, f_mis=0.02):
    """Reads cut from the text at random places, one letter in 50 replaced; on the device."""
    t = torch.from_numpy(text).cuda()
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    total = int(offs[-1])
    start = torch.from_numpy(rng.integers(0, max(1, text.size - int(lens.max())), lens.size)).cuda()
    d_offs = torch.from_numpy(offs).cuda()
    read_of = torch.repeat_interleave(torch.arange(lens.size, device="cuda"), torch.from_numpy(lens).cuda())
    pos = torch.arange(total, device="cuda") - d_offs[read_of] + start[read_of]
    seqs = t[pos]
    g = torch.Generator(device="cuda").manual_seed(int(rng.integers(1 << 30)))
    flip = torch.rand(total, device="cuda", generator=g) < f_mis
    seqs[flip] = t[torch.randint(0, text.size, (int(flip.sum().item()),), device="cuda", generator=g)]
    return seqs.contiguous(), d_offs


def kernels_against_walk(ix, name, seqs, offs, bits, min_length, reps):
    total, nreads = seqs.numel(), offs.numel() - 1
    dt = torch.int16 if bits == 16 else torch.int32
    d_seqs = capi.pad_seqs(seqs)
    d_len = torch.empty(total + 16, dtype=dt, device="cuda")
    d_ptr = torch.empty(total + 16, dtype=torch.int64, device="cuda")
    mo = torch.empty(nreads + 1, dtype=torch.int64, device="cuda")
    ix.query_device(capi.SPX_MODE_MS, d_seqs, offs, total, d_lengths=d_len, d_pointers=d_ptr)
    ix.mems_device(d_len, d_ptr, offs, min_length, d_match_offsets=mo)  # (sizes the records)
    n = int(mo[-1].item())
    out = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    walk, mems = [], []
    for _ in range(reps + 1):
        e0.record()
        ix.query_device(capi.SPX_MODE_MS, d_seqs, offs, total, d_lengths=d_len, d_pointers=d_ptr)
        e1.record()
        ix.mems_device(d_len, d_ptr, offs, min_length, capacity=n, d_match_offsets=mo, d_out=out)
        torch.cuda.synchronize()
        walk.append(e0.elapsed_time(e1))
        st = ix.mems_stats()
        mems.append(st["kernel_ms"])
    w, v = med(walk[1:]), med(mems[1:])
    nbytes = total * (bits // 8) + n * (bits // 8 + 8 + 16) + (nreads + 1) * 16  # lengths; length, pointer and record per match; offsets in and out
    c = copy_ms(nbytes, reps)
    print(f"{name}: {nreads} reads, {total} values, {bits}-bit, min_length {min_length}: {st['matches']} matches "
          f"({100 * st['matches'] / max(total, 1):.2f} % of the values), longest {st['longest']}\n"
          f"    MS walk + k_ms_extend   {w:9.3f} ms   (min {min(walk[1:]):.3f}, max {max(walk[1:]):.3f})\n"
          f"    match kernels           {v:9.3f} ms   (min {min(mems[1:]):.3f}, max {max(mems[1:]):.3f})   = {100 * v / w:.1f} % of walk + extension\n"
          f"    matches: {nbytes / 1e9:.3f} GB in {v:.3f} ms = {nbytes / v / 1e6:.0f} GB/s; a device copy of as many bytes: {c:.3f} ms = "
          f"{nbytes / c / 1e6:.0f} GB/s read (and as much written): {v / c:.1f} x the copy", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text", type=int, default=8_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    torch.cuda.set_device(0)
    rng = np.random.default_rng(3)
    text = repetitive_text(rng, a.text)
    t0 = time.perf_counter()
    raw = capi.build_raw(text)
    ix = capi.Index.from_raw(raw, 0)
    print(f"mems_bench: {a.label}\nhost {socket.gethostname()}, {torch.cuda.get_device_name(0)}, library {capi.version()}\n"
          f"index: capi.build_raw over {a.text} DNA letters (mutated copies of one sequence of {a.text // 8}): n = {ix.n}, r = {ix.r}, "
          f"built in {time.perf_counter() - t0:.1f} s\n", flush=True)

    print("== 1. match kernels against the MS walk + extension that feed them (HIP events, median of %d) ==" % a.reps, flush=True)
    seqs, offs = reads_from(text, np.full(5_000_000, 55), rng)
    kernels_against_walk(ix, "c4_ms_doc's shape", seqs, offs, 16, 8, a.reps)
    kernels_against_walk(ix, "c4_ms_doc's shape", seqs, offs, 16, 25, a.reps)
    del seqs, offs
    # heavy-tailed: Pareto lengths (median 26, some tens of thousands) and one read of 10^6 values; 32-bit arrays
    lens = np.minimum((rng.pareto(1.1, 1_000_000) * 30).astype(np.int64) + 1, 200_000)
    lens[rng.integers(0, lens.size)] = 1_000_000
    seqs, offs = reads_from(text, lens, rng)
    kernels_against_walk(ix, "heavy-tailed mix with one read of 10^6 values", seqs, offs, 32, 25, a.reps)
    del seqs, offs
    torch.cuda.empty_cache()

    print("\n== 2. host form: mems_host against query_host + mems_reference (wall clock, median of %d) ==" % a.reps, flush=True)
    nreads = 1_000_000
    d_seqs, d_offs = reads_from(text, np.full(nreads, 200), rng)
    seqs, offs = d_seqs.cpu().numpy(), d_offs.cpu().numpy().astype(np.uint64)
    del d_seqs, d_offs
    new, old_q, old_r = [], [], []
    piece = 100_000  # reads per call: 20 M characters (spm_mems_begin takes up to 32 Mi)
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        got = [ix.mems_host(seqs[int(offs[q]):int(offs[q + piece])], offs[q:q + piece + 1] - offs[q], 25) for q in range(0, nreads, piece)]
        new.append(time.perf_counter() - t0)
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        r = ix.query_host(capi.SPX_MODE_MS, seqs, offs, bits=16)
        t1 = time.perf_counter()
        want = mems_reference(r["lengths"], r["pointers"], offs, 25)
        old_q.append(t1 - t0)
        old_r.append(time.perf_counter() - t1)
    rec = np.concatenate([g[1] for g in got])
    same = bool(np.array_equal(rec, want[1]) and np.array_equal(np.concatenate([np.diff(g[0].astype(np.int64)) for g in got]),
                                                                np.diff(want[0].astype(np.int64))))
    print(f"{nreads} x 200 bp, no digestion, min_length 25: {rec.size} matches; records equal: {same}\n"
          f"    mems_host ({nreads // piece} calls)                 {med(new[1:]):8.3f} s   (min {min(new[1:]):.3f}, max {max(new[1:]):.3f})\n"
          f"    query_host (lengths + pointers back)    {med(old_q[1:]):8.3f} s\n"
          f"    + mems_reference on the host            {med(old_r[1:]):8.3f} s   together {med(old_q[1:]) + med(old_r[1:]):.3f} s = "
          f"{(med(old_q[1:]) + med(old_r[1:])) / med(new[1:]):.1f} x mems_host", flush=True)
    assert same

    if a.skip_cli:
        return
    print("\n== 3. CLI, process start to process gone, reads file and outputs on tmpfs ==", flush=True)
    work = tempfile.mkdtemp(prefix="mems_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        prefix = os.path.join(work, "ref.fa")
        open(prefix, "w").write(">dummy\n")
        raw.write_raw_files(prefix)
        text.tofile(prefix + ".rawtext")
        rs = seqs.reshape(nreads, 200)
        reads = os.path.join(work, "reads.fa")
        with open(reads, "wb") as f:
            for i in range(0, nreads, 10000):
                f.write(b"".join(b">read_%d\n%s\n" % (q, rs[q].tobytes()) for q in range(i, min(nreads, i + 10000))))
        env = dict(os.environ, SPUMONI_GPUS="0", SPUMONI_TEXT=prefix + ".rawtext")
        res = {}
        for name, cmd in (("run -M -n", [BIN, "run", "-r", prefix[:-3], "-p", reads, "-M", "-n"]),
                          ("mems -n -L 25", [BIN, "mems", "-r", prefix[:-3], "-p", reads, "-n", "-L", "25"])):
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                p = subprocess.run(cmd, capture_output=True, env=env, timeout=600)
                ts.append(time.perf_counter() - t0)
                assert p.returncode == 0, p.stderr.decode()[-2000:]
            res[name] = ts
        out_run = os.path.getsize(reads + ".lengths") + os.path.getsize(reads + ".pointers")
        out_mems = os.path.getsize(reads + ".mems")
        print(f"{nreads} x 200 bp, the index above, no digestion\n"
              f"    spumoni run -M -n       {med(res['run -M -n']):7.3f} s  (runs: {', '.join('%.3f' % t for t in res['run -M -n'])}); writes {out_run / 1e6:.1f} MB\n"
              f"    spumoni mems -n -L 25   {med(res['mems -n -L 25']):7.3f} s  (runs: {', '.join('%.3f' % t for t in res['mems -n -L 25'])}); writes {out_mems / 1e6:.1f} MB",
              flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
