"""Measures the placements; the output is kept as profiles/place_bench.txt.

  1. the placement kernel against the MS walk + k_ms_extend that feed it: same batch, same device, HIP-event times, median
     of --reps after a warm-up, beside a plain device copy of the bytes the kernel must move (all lengths, the reads, 32
     bytes per read);
  2. Index.place_host against what a caller did before it existed: Index.mems_host + place.place_reference over the
     records, wall clock, with the records compared;
  3. `spumoni place` against `spumoni mems` on the same reads file on tmpfs, process start to process gone.

    python tools/place_bench.py [--text N] [--reps N] [--skip-cli] [--label TEXT]
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
from spumoni_amd.place import PLACEMENT_DTYPE, UNPLACED, place_reference  # noqa: E402
from tools.mems_bench import copy_ms, med, reads_from, repetitive_text  # noqa: E402

BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")


def kernel_against_walk(ix, name, seqs, offs, bits, min_seed, reps):
    total, nreads = seqs.numel(), offs.numel() - 1
    dt = torch.int16 if bits == 16 else torch.int32
    d_seqs = capi.pad_seqs(seqs)
    d_len = torch.empty(total + 16, dtype=dt, device="cuda")
    d_ptr = torch.empty(total + 16, dtype=torch.int64, device="cuda")
    out = torch.empty((nreads, 8), dtype=torch.int32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    walk, place = [], []
    for _ in range(reps + 1):
        e0.record()
        ix.query_device(capi.SPX_MODE_MS, d_seqs, offs, total, d_lengths=d_len, d_pointers=d_ptr)
        e1.record()
        ix.place_device(d_seqs, d_len, d_ptr, offs, min_seed, d_out=out, total_values=total)
        torch.cuda.synchronize()
        walk.append(e0.elapsed_time(e1))
        st = ix.place_stats()
        place.append(st["kernel_ms"])
    w, v = med(walk[1:]), med(place[1:])
    nbytes = total * (bits // 8) + total + nreads * (32 + 8)  # lengths, reads, a record and an offset per read (the text comes on top)
    c = copy_ms(nbytes, reps)
    rec = out.cpu().numpy().view(PLACEMENT_DTYPE).reshape(-1)
    ok = rec["ref_start"] != np.uint64(UNPLACED)
    span = rec["read_end"][ok].astype(np.int64) - rec["read_start"][ok]
    print(f"{name}: {nreads} reads, {total} values, {bits}-bit, min_seed {min_seed}, penalty 4, x-drop 16: {st['placed']} placed, "
          f"seeds {st['seed_values'] / max(st['placed'], 1):.1f}, extensions {st['extended_values'] / max(st['placed'], 1):.1f} and "
          f"identity {rec['matches'][ok].sum() / max(int(span.sum()), 1):.4f} on average\n"
          f"    MS walk + k_ms_extend   {w:9.3f} ms   (min {min(walk[1:]):.3f}, max {max(walk[1:]):.3f})\n"
          f"    k_place                 {v:9.3f} ms   (min {min(place[1:]):.3f}, max {max(place[1:]):.3f})   = {100 * v / w:.1f} % of walk + extension\n"
          f"    placements: {nbytes / 1e9:.3f} GB in {v:.3f} ms = {nbytes / v / 1e6:.0f} GB/s; a device copy of as many bytes: {c:.3f} ms = "
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
    print(f"place_bench: {a.label}\nhost {socket.gethostname()}, {torch.cuda.get_device_name(0)}, library {capi.version()}\n"
          f"index: capi.build_raw over {a.text} DNA letters (mutated copies of one sequence of {a.text // 8}): n = {ix.n}, r = {ix.r}, "
          f"built in {time.perf_counter() - t0:.1f} s\n", flush=True)

    print("== 1. the placement kernel against the MS walk + extension that feed it (HIP events, median of %d) ==" % a.reps, flush=True)
    seqs, offs = reads_from(text, np.full(5_000_000, 55), rng)
    kernel_against_walk(ix, "c4_ms_doc's shape", seqs, offs, 16, 20, a.reps)
    del seqs, offs
    for f_mis in (0.01, 0.05):
        seqs, offs = reads_from(text, np.full(1_000_000, 150), rng, f_mis=f_mis)
        kernel_against_walk(ix, f"150 bp, {100 * f_mis:.0f} % substitutions", seqs, offs, 16, 20, a.reps)
        del seqs, offs
    # heavy-tailed: Pareto lengths (median 26, some tens of thousands) and one read of 10^6 values; 32-bit arrays
    lens = np.minimum((rng.pareto(1.1, 1_000_000) * 30).astype(np.int64) + 1, 200_000)
    lens[rng.integers(0, lens.size)] = 1_000_000
    seqs, offs = reads_from(text, lens, rng)
    kernel_against_walk(ix, "heavy-tailed mix with one read of 10^6 values", seqs, offs, 32, 20, a.reps)
    del seqs, offs
    torch.cuda.empty_cache()

    print("\n== 2. host form: place_host against mems_host + place_reference (wall clock) ==", flush=True)
    nreads = 1_000_000
    d_seqs, d_offs = reads_from(text, np.full(nreads, 150), rng, f_mis=0.01)
    seqs, offs = d_seqs.cpu().numpy(), d_offs.cpu().numpy().astype(np.uint64)
    del d_seqs, d_offs
    new = []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        got, _ = ix.place_host(seqs, offs, 20)
        new.append(time.perf_counter() - t0)
    # before: the matches of every read come back, the host takes the longest per read as the seed and compares
    piece = 200_000  # reads per call: 30 M characters (spm_mems_begin takes up to 32 Mi)
    t0 = time.perf_counter()
    parts = [ix.mems_host(seqs[int(offs[q]):int(offs[q + piece])], offs[q:q + piece + 1] - offs[q], 20) for q in range(0, nreads, piece)]
    t1 = time.perf_counter()
    L, P = np.zeros(seqs.size, dtype=np.uint32), np.zeros(seqs.size, dtype=np.uint64)
    for q0, (mo, rec, _) in zip(range(0, nreads, piece), parts):
        at = np.repeat(offs[q0:q0 + piece], np.diff(mo.astype(np.int64))) + rec["read_pos"]
        L[at], P[at] = rec["length"], rec["ref_pos"]  # (every maximum of L is a match start: the seed is among the records)
    want = place_reference(seqs, L, P, offs, text, 20)
    t2 = time.perf_counter()
    same = bool(np.array_equal(got, want))
    print(f"{nreads} x 150 bp, 1 % substitutions, no digestion, min_seed 20; records equal: {same}\n"
          f"    place_host                              {med(new[1:]):8.3f} s   (min {min(new[1:]):.3f}, max {max(new[1:]):.3f})\n"
          f"    mems_host ({nreads // piece} calls, records back)       {t1 - t0:8.3f} s\n"
          f"    + place_reference on the host           {t2 - t1:8.3f} s   together {t2 - t0:.3f} s = {(t2 - t0) / med(new[1:]):.1f} x place_host",
          flush=True)
    assert same

    if a.skip_cli:
        return
    print("\n== 3. CLI, process start to process gone, reads file and outputs on tmpfs ==", flush=True)
    work = tempfile.mkdtemp(prefix="place_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        prefix = os.path.join(work, "ref.fa")
        open(prefix, "w").write(">dummy\n")
        raw.write_raw_files(prefix)
        text.tofile(prefix + ".rawtext")
        rs = seqs.reshape(nreads, 150)
        reads = os.path.join(work, "reads.fa")
        with open(reads, "wb") as f:
            for i in range(0, nreads, 10000):
                f.write(b"".join(b">read_%d\n%s\n" % (q, rs[q].tobytes()) for q in range(i, min(nreads, i + 10000))))
        env = dict(os.environ, SPUMONI_GPUS="0", SPUMONI_TEXT=prefix + ".rawtext")
        res = {}
        for name, cmd in (("mems", [BIN, "mems", "-r", prefix[:-3], "-p", reads, "-n", "-L", "20"]),
                          ("place", [BIN, "place", "-r", prefix[:-3], "-p", reads, "-n", "-L", "20"])):
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                p = subprocess.run(cmd, capture_output=True, env=env, timeout=600)
                ts.append(time.perf_counter() - t0)
                assert p.returncode == 0, p.stderr.decode()[-2000:]
            res[name] = ts
        print(f"{nreads} x 150 bp, the index above, no digestion\n"
              f"    spumoni mems -n -L 20    {med(res['mems']):7.3f} s  (runs: {', '.join('%.3f' % t for t in res['mems'])}); writes "
              f"{os.path.getsize(reads + '.mems') / 1e6:.1f} MB\n"
              f"    spumoni place -n -L 20   {med(res['place']):7.3f} s  (runs: {', '.join('%.3f' % t for t in res['place'])}); writes "
              f"{os.path.getsize(reads + '.placements') / 1e6:.1f} MB", flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
