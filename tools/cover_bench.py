"""Measures the coverage; the output is kept as profiles/cover_bench.txt.

  1. the cover kernels -- add, finish, runs, each between its own HIP events -- beside the map kernels on the same batch in
     the same loop -- the yardstick: the mappings the coverage is made of --: median of --reps after a warm-up, with the
     intervals and the atomic adds a read costs.  The batches are tools/map_bench.py's four.  The add step is measured three
     times: with the switch where it is (a read of more than 64 entries takes a wavefront), with a lane per read forced and
     with a wavefront per read forced;
  2. Index.cover_add_host + cover_summary against what a user does without it: Index.map_host, then a numpy accumulation
     of the fetched entries into a depth array and the per-sequence sums; wall clock;
  3. `spumoni cover` against `spumoni map` on the same reads file on tmpfs, process start to process gone, with the bytes
     each writes.

    python tools/cover_bench.py [--text N] [--seqs N] [--reps N] [--skip-cli] [--label TEXT]
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
from spumoni_amd.cover import seq_starts  # noqa: E402
from spumoni_amd.map import UNMAPPED, write_seq_table  # noqa: E402
from tools.align_bench import feed  # noqa: E402
from tools.chain_bench import reads_with_indels  # noqa: E402
from tools.mems_bench import med, repetitive_text  # noqa: E402

BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
STEPS = ("add", "finish (scan + summary)", "runs (count + scan + write)")
SWITCHES = (("the switch at 64 entries", 64), ("a lane per read forced", 1 << 30), ("a wavefront per read forced", 0))


def kernels_against_map(ix, name, seqs, offs, bits, min_length, reps, G, n_seqs):
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
    diff = torch.zeros(G + 1, dtype=torch.int32, device="cuda")
    mism = torch.zeros(G, dtype=torch.int32, device="cuda")
    counts = torch.zeros(2 * n_seqs, dtype=torch.int64, device="cuda")
    depth = torch.empty(G, dtype=torch.int32, device="cuda")
    summary = torch.empty((n_seqs, 6), dtype=torch.int64, device="cuda")
    run_cap = 2 * G
    runs = torch.empty((run_cap, 4), dtype=torch.int64, device="cuda")
    nruns = torch.empty(1, dtype=torch.int64, device="cuda")
    ix.mems_device(d_len, d_ptr, offs, min_length, capacity=n, d_match_offsets=mo, d_out=rec)
    ix.chain_device(rec[:n], mo, d_out=chains, d_out_pred=pred)
    ix.extend_device(d_seqs, offs, rec[:n], mo, chains, pred, gap_capacity=n, op_capacity=op_cap, d_out=out, d_out_op_offsets=ooffs,
                     d_out_ops=ops, want_ends=False)
    mapping, steps = [], []
    for _ in range(reps + 1):
        ix.map_device(out, ooffs, ops, offs, op_capacity=op_cap, in_entries=op_cap, d_out=maps, d_out_op_offsets=moffs, d_out_ops=mops)
        diff.zero_(), mism.zero_(), counts.zero_()
        ix.cover_add_device(maps, moffs, mops, diff, mism, counts, in_entries=op_cap)
        ix.cover_finish_device(diff, mism, counts, d_depth=depth, d_out=summary)
        ix.cover_runs_device(depth, mism, 1, run_cap, d_runs=runs, d_count=nruns)
        torch.cuda.synchronize()
        sm, sc = ix.map_stats(), ix.cover_stats()
        mapping.append(sm["kernel_ms"])
        steps.append(sc["step_ms"])
    assert sm["overflow"] == 0 and sm["error"] == 0 and sc["overflow"] == 0 and sc["error"] == 0 and sc["skipped"] == 0, (sm, sc)
    assert sc["added"] == sm["mapped"] and int(summary[:, 4].sum()) == sm["mapped"]
    m = med(mapping[1:])
    s = [med([x[i] for x in steps[1:]]) for i in range(3)]
    covered, bases = int(summary[:, 0].sum()), int(summary[:, 1].sum())
    print(f"{name}: {nreads} reads, {total} values, min_length {min_length}, default parameters: {sm['mapped']} reads mapped and added, "
          f"{sm['entries_out']} entries ({sm['entries_out'] / max(sm['mapped'], 1):.1f} a read), {sc['intervals']} intervals "
          f"({sc['intervals'] / max(sc['added'], 1):.2f} a read), {sc['atomics']} atomic adds ({sc['atomics'] / max(sc['added'], 1):.2f} a read); "
          f"{covered} of {G} bases covered, {bases} bases of depth, {sc['runs']} runs of depth >= 1\n"
          f"    map kernels (the yardstick)     {m:9.3f} ms   (min {min(mapping[1:]):.3f}, max {max(mapping[1:]):.3f})\n"
          f"    cover kernels                   {sum(s):9.3f} ms   = {sum(s) / max(m, 1e-6):.3f} x map", flush=True)
    for label, t in zip(STEPS, s):
        print(f"        {label:28s}    {t:9.3f} ms", flush=True)
    want = (diff.clone(), mism.clone(), counts.clone())
    try:
        for label, switch in SWITCHES:
            ix.set_option("cover_switch", switch)
            ts = []
            for _ in range(reps + 1):
                diff.zero_(), mism.zero_(), counts.zero_()
                ix.cover_add_device(maps, moffs, mops, diff, mism, counts, in_entries=op_cap)
                torch.cuda.synchronize()
                ts.append(ix.cover_stats()["step_ms"][0])
            assert all(torch.equal(a, b) for a, b in zip(want, (diff, mism, counts))), label
            print(f"        add, {label:28s} {med(ts[1:]):9.3f} ms   (min {min(ts[1:]):.3f}, max {max(ts[1:]):.3f})", flush=True)
    finally:
        ix.set_option("cover_switch", 64)


def numpy_coverage(maps, op_offsets, ops, lengths):
    """What a user does with map_host's output today: every '=' / 'X' entry as an interval into a difference array."""
    F = np.array(seq_starts(lengths), dtype=np.int64)
    mapped = np.flatnonzero(maps["seq"] != UNMAPPED)
    counts = np.diff(op_offsets.astype(np.int64))
    read_of = np.repeat(np.arange(maps.size), counts)
    op, n = (ops & 15).astype(np.int64), (ops >> 4).astype(np.int64)
    text = np.where(np.isin(op, (2, 3, 7, 8)), n, 0)  # D, N, =, X
    before = np.cumsum(text) - text
    first = before[np.minimum(op_offsets[:-1].astype(np.int64), max(ops.size - 1, 0))] if ops.size else np.zeros(maps.size, dtype=np.int64)
    pos = F[np.where(maps["seq"] == UNMAPPED, 0, maps["seq"]).astype(np.int64)][read_of] + maps["target_start"].astype(np.int64)[read_of] + \
        before - first[read_of]
    cov = np.isin(op, (7, 8))
    diff = np.zeros(F[-1] + 1, dtype=np.int64)
    np.add.at(diff, pos[cov], 1)
    np.add.at(diff, pos[cov] + n[cov], -1)
    depth = np.cumsum(diff)[:-1]
    covered = np.add.reduceat(depth > 0, F[:-1])
    bases = np.add.reduceat(depth, F[:-1])
    reads = np.bincount(maps["seq"][mapped].astype(np.int64), minlength=len(lengths))
    return covered, bases, reads


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
    per = a.text // (2 * a.seqs)
    genome = repetitive_text(rng, per * a.seqs)
    lengths = [per] * a.seqs
    G = per * a.seqs
    text = np.concatenate([p for q in range(a.seqs) for p in (genome[q * per:(q + 1) * per], synth.revcomp(genome[q * per:(q + 1) * per]))])
    t0 = time.perf_counter()
    raw = capi.build_raw(text)
    ix = capi.Index.from_raw(raw, 0)
    ix.set_sequences(lengths, 2)
    print(f"cover_bench: {a.label}\nhost {socket.gethostname()}, {torch.cuda.get_device_name(0)}, library {capi.version()}\n"
          f"index: capi.build_raw over {text.size} DNA letters: {a.seqs} sequences of {per} (mutated copies of one sequence of "
          f"{per * a.seqs // 8}, cut), each with its reverse complement: n = {ix.n}, r = {ix.r}, built in {time.perf_counter() - t0:.1f} s; "
          f"forward genome {G} bases: diff, mism and depth take {12 * G / 1e6:.1f} MB\n", flush=True)

    print("== 1. the cover kernels beside the map kernels on the same batch (HIP events, median of %d) ==" % a.reps, flush=True)
    seqs, offs = reads_with_indels(text, np.full(1_000_000, 150), rng, 0.01)
    kernels_against_map(ix, "150 bp, 1 % substitutions", seqs, offs, 16, 20, a.reps, G, a.seqs)
    del seqs, offs
    seqs, offs = reads_with_indels(text, np.full(1_000_000, 150), rng, 0.05, one_indel=True)
    kernels_against_map(ix, "150 bp, 5 % substitutions and one indel per read", seqs, offs, 16, 20, a.reps, G, a.seqs)
    del seqs, offs
    seqs, offs = reads_with_indels(text, np.full(2000, 10_000), rng, 0.08, f_indel=0.02)
    kernels_against_map(ix, "10 kbp, 10 % errors (8 % substitutions, 2 % indels)", seqs, offs, 16, 12, a.reps, G, a.seqs)
    kernels_against_map(ix, "10 kbp, the same reads, min_length 16", seqs, offs, 16, 16, a.reps, G, a.seqs)
    del seqs, offs
    torch.cuda.empty_cache()

    print("\n== 2. host form: cover_add_host + cover_summary against map_host + a numpy accumulation (wall clock) ==", flush=True)
    nreads = 200_000  # 30 M characters: one piece
    d_seqs, d_offs = reads_with_indels(text, np.full(nreads, 150), rng, 0.05, one_indel=True)
    seqs, offs = d_seqs.cpu().numpy(), d_offs.cpu().numpy().astype(np.uint64)
    del d_seqs, d_offs
    new, old, old_map = [], [], []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        ix.cover_reset()
        ix.cover_add_host(seqs, offs, 20)
        got = ix.cover_summary(a.seqs)
        new.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        maps, m_offs, m_ops, _ = ix.map_host(seqs, offs, 20)
        old_map.append(time.perf_counter() - t0)
        want = numpy_coverage(maps, m_offs, m_ops, lengths)
        old.append(time.perf_counter() - t0)
    same = bool(np.array_equal(got["covered"], want[0]) and np.array_equal(got["bases"], want[1]) and np.array_equal(got["reads"], want[2]))
    print(f"{nreads} x 150 bp, 5 % substitutions and one indel per read, no digestion, min_length 20; covered, bases and reads equal: {same}; "
          f"{got.nbytes} bytes come back against {maps.nbytes + m_offs.nbytes + m_ops.nbytes}\n"
          f"    cover_reset + cover_add_host + cover_summary  {med(new[1:]):8.3f} s   (min {min(new[1:]):.3f}, max {max(new[1:]):.3f})\n"
          f"    map_host + numpy accumulation                 {med(old[1:]):8.3f} s   (min {min(old[1:]):.3f}, max {max(old[1:]):.3f}); "
          f"map_host alone {med(old_map[1:]):.3f} s", flush=True)
    assert same

    if a.skip_cli:
        return
    print("\n== 3. CLI, process start to process gone, reads file and outputs on tmpfs ==", flush=True)
    work = tempfile.mkdtemp(prefix="cover_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
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
        for name, extra in (("map", []), ("cover", ["-b"])):
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                p = subprocess.run([BIN, name, "-r", prefix[:-3], "-p", reads, "-n", "-L", "20"] + extra, capture_output=True, env=env, timeout=600)
                ts.append(time.perf_counter() - t0)
                assert p.returncode == 0, p.stderr.decode()[-2000:]
            res[name] = ts
        print(f"{nreads} x 150 bp, the index above, no digestion\n"
              f"    spumoni map -n -L 20        {med(res['map']):7.3f} s  (runs: {', '.join('%.3f' % t for t in res['map'])}); writes "
              f"{os.path.getsize(reads + '.paf') / 1e6:.1f} MB\n"
              f"    spumoni cover -n -L 20 -b   {med(res['cover']):7.3f} s  (runs: {', '.join('%.3f' % t for t in res['cover'])}); writes "
              f"{os.path.getsize(reads + '.cover')} bytes and a bedgraph of {os.path.getsize(reads + '.bedgraph') / 1e6:.1f} MB", flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
