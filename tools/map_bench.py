"""Measures the mappings; the output is kept as profiles/map_bench.txt.

  1. the map kernels and their two steps (locate and count with the scan, write: HIP events between them) beside the extend
     kernels on the same batch in the same loop -- the yardstick: the alignments the mappings are made of --: median of
     --reps after a warm-up, with the reads cut at a sequence border, the reads on the reverse strand, the entries in and
     out and the characters the cuts clipped.  The batches are tools/extend_bench.py's four, on an index of --seqs
     sequences with their reverse complements;
  2. Index.map_host against Index.extend_host, wall clock, with the middles compared;
  3. `spumoni map` against `spumoni extend` on the same reads file on tmpfs, process start to process gone.

    python tools/map_bench.py [--text N] [--seqs N] [--reps N] [--skip-cli] [--label TEXT]
"""
import argparse
import os
import shutil
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spumoni_amd import capi, synth  # noqa: E402
from spumoni_amd.map import write_seq_table  # noqa: E402
from tools.align_bench import feed  # noqa: E402
from tools.chain_bench import reads_with_indels  # noqa: E402
from tools.mems_bench import med, repetitive_text  # noqa: E402

BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
STEPS = ("locate + count + scan", "write")


def kernels_against_extend(ix, name, seqs, offs, bits, min_length, reps):
    total, nreads = seqs.numel(), offs.numel() - 1
    d_seqs, d_len, d_ptr, mo, n, rec = feed(ix, seqs, offs, bits, min_length)
    chains = torch.empty((nreads, 12), dtype=torch.int32, device="cuda")
    pred = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    out = torch.empty((nreads, 12), dtype=torch.int32, device="cuda")
    maps = torch.empty((nreads, 12), dtype=torch.int32, device="cuda")
    ooffs = torch.empty(nreads + 1, dtype=torch.int64, device="cuda")
    moffs = torch.empty(nreads + 1, dtype=torch.int64, device="cuda")
    op_cap = 2 * total + 2 * n + 3 * nreads
    ops = torch.empty(op_cap, dtype=torch.int32, device="cuda")
    mops = torch.empty(op_cap, dtype=torch.int32, device="cuda")
    ix.mems_device(d_len, d_ptr, offs, min_length, capacity=n, d_match_offsets=mo, d_out=rec)
    ix.chain_device(rec[:n], mo, d_out=chains, d_out_pred=pred)
    extend, mapping, steps = [], [], []
    for _ in range(reps + 1):
        ix.extend_device(d_seqs, offs, rec[:n], mo, chains, pred, gap_capacity=n, op_capacity=op_cap, d_out=out, d_out_op_offsets=ooffs,
                         d_out_ops=ops, want_ends=False)
        ix.map_device(out, ooffs, ops, offs, op_capacity=op_cap, in_entries=op_cap, d_out=maps, d_out_op_offsets=moffs, d_out_ops=mops)
        torch.cuda.synchronize()
        se, sm = ix.extend_stats(), ix.map_stats()
        extend.append(se["kernel_ms"])
        mapping.append(sm["kernel_ms"])
        steps.append(sm["step_ms"])
    assert sm["overflow"] == 0 and sm["error"] == 0 and se["overflow"] == 0 and se["error"] == 0, (sm, se)
    assert sm["mapped"] == se["aligned_reads"] and sm["entries_in"] == se["entries"]
    e, m = med(extend[1:]), med(mapping[1:])
    s = [med([x[i] for x in steps[1:]]) for i in range(2)]
    print(f"{name}: {nreads} reads, {total} values, min_length {min_length}, default parameters: {sm['mapped']} reads mapped, "
          f"{sm['cut_reads']} cut at a border, {sm['reverse_reads']} on the reverse strand, {sm['entries_in']} entries in "
          f"({sm['entries_in'] / max(sm['mapped'], 1):.1f} a read), {sm['entries_out']} out, {sm['cut_chars']} characters clipped by cuts\n"
          f"    extend kernels (the yardstick)  {e:9.3f} ms   (min {min(extend[1:]):.3f}, max {max(extend[1:]):.3f})\n"
          f"    map kernels                     {m:9.3f} ms   (min {min(mapping[1:]):.3f}, max {max(mapping[1:]):.3f})   = {m / max(e, 1e-6):.3f} x extend",
          flush=True)
    for label, t in zip(STEPS, s):
        print(f"        {label:28s}    {t:9.3f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text", type=int, default=8_000_000)
    ap.add_argument("--seqs", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    torch.cuda.set_device(0)
    rng = np.random.default_rng(3)
    # --seqs sequences cut from one repetitive text, each followed by its reverse complement: what `spumoni build -n` lays out
    per = a.text // (2 * a.seqs)
    genome = repetitive_text(rng, per * a.seqs)
    lengths = [per] * a.seqs
    text = np.concatenate([p for q in range(a.seqs) for p in (genome[q * per:(q + 1) * per], synth.revcomp(genome[q * per:(q + 1) * per]))])
    t0 = time.perf_counter()
    raw = capi.build_raw(text)
    ix = capi.Index.from_raw(raw, 0)
    ix.set_sequences(lengths, 2)
    print(f"map_bench: {a.label}\nhost {socket.gethostname()}, {torch.cuda.get_device_name(0)}, library {capi.version()}\n"
          f"index: capi.build_raw over {text.size} DNA letters: {a.seqs} sequences of {per} (mutated copies of one sequence of "
          f"{per * a.seqs // 8}, cut), each with its reverse complement: n = {ix.n}, r = {ix.r}, built in {time.perf_counter() - t0:.1f} s\n"
          f"mapping: a lane per read in both kernels (the only one built)\n", flush=True)

    print("== 1. the map kernels beside the extend kernels on the same batch (HIP events, median of %d) ==" % a.reps, flush=True)
    seqs, offs = reads_with_indels(text, np.full(1_000_000, 150), rng, 0.01)
    kernels_against_extend(ix, "150 bp, 1 % substitutions", seqs, offs, 16, 20, a.reps)
    del seqs, offs
    seqs, offs = reads_with_indels(text, np.full(1_000_000, 150), rng, 0.05, one_indel=True)
    kernels_against_extend(ix, "150 bp, 5 % substitutions and one indel per read", seqs, offs, 16, 20, a.reps)
    del seqs, offs
    seqs, offs = reads_with_indels(text, np.full(2000, 10_000), rng, 0.08, f_indel=0.02)
    kernels_against_extend(ix, "10 kbp, 10 % errors (8 % substitutions, 2 % indels)", seqs, offs, 16, 12, a.reps)
    kernels_against_extend(ix, "10 kbp, the same reads, min_length 16 (align_bench's fourth batch)", seqs, offs, 16, 16, a.reps)
    del seqs, offs
    torch.cuda.empty_cache()

    print("\n== 2. host form: map_host against extend_host (wall clock) ==", flush=True)
    nreads = 200_000  # 30 M characters: one piece
    d_seqs, d_offs = reads_with_indels(text, np.full(nreads, 150), rng, 0.05, one_indel=True)
    seqs, offs = d_seqs.cpu().numpy(), d_offs.cpu().numpy().astype(np.uint64)
    del d_seqs, d_offs
    new, old = [], []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        got = ix.map_host(seqs, offs, 20)
        new.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        want = ix.extend_host(seqs, offs, 20)
        old.append(time.perf_counter() - t0)
    same = bool(np.array_equal(got[3], want[0]))
    st = ix.map_stats()
    print(f"{nreads} x 150 bp, 5 % substitutions and one indel per read, no digestion, min_length 20; extend's records equal: {same}; "
          f"{got[2].size} entries against {want[2].size}, {st['cut_reads']} reads cut, {st['reverse_reads']} on the reverse strand\n"
          f"    map_host (begin + fetch)     {med(new[1:]):8.3f} s   (min {min(new[1:]):.3f}, max {max(new[1:]):.3f})\n"
          f"    extend_host (begin + fetch)  {med(old[1:]):8.3f} s   (min {min(old[1:]):.3f}, max {max(old[1:]):.3f})", flush=True)
    assert same

    if a.skip_cli:
        return
    print("\n== 3. CLI, process start to process gone, reads file and outputs on tmpfs ==", flush=True)
    work = tempfile.mkdtemp(prefix="map_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        prefix = os.path.join(work, "ref.fa")
        open(prefix, "w").write(">dummy\n")
        raw.write_raw_files(prefix)
        text.tofile(prefix + ".rawtext")
        write_seq_table(prefix + ".seqs", [b"sequence_%d" % q for q in range(a.seqs)], lengths, 2)
        rs = seqs.reshape(nreads, 150)
        reads = os.path.join(work, "reads.fa")
        with open(reads, "wb") as f:
            for i in range(0, nreads, 10000):
                f.write(b"".join(b">read_%d\n%s\n" % (q, rs[q].tobytes()) for q in range(i, min(nreads, i + 10000))))
        env = dict(os.environ, SPUMONI_GPUS="0", SPUMONI_TEXT=prefix + ".rawtext")
        res = {}
        for name in ("extend", "map"):
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                p = subprocess.run([BIN, name, "-r", prefix[:-3], "-p", reads, "-n", "-L", "20"], capture_output=True, env=env, timeout=600)
                ts.append(time.perf_counter() - t0)
                assert p.returncode == 0, p.stderr.decode()[-2000:]
            res[name] = ts
        print(f"{nreads} x 150 bp, the index above, no digestion\n"
              f"    spumoni extend -n -L 20   {med(res['extend']):7.3f} s  (runs: {', '.join('%.3f' % t for t in res['extend'])}); writes "
              f"{os.path.getsize(reads + '.extended') / 1e6:.1f} MB\n"
              f"    spumoni map -n -L 20      {med(res['map']):7.3f} s  (runs: {', '.join('%.3f' % t for t in res['map'])}); writes "
              f"{os.path.getsize(reads + '.paf') / 1e6:.1f} MB", flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
