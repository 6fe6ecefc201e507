"""Measures the consensus; the output is kept as profiles/consensus_bench.txt.

  1. the consensus steps -- count, scans, write, each between HIP events of its own -- beside the calls step
     (spl_calls_device: count, scan and write of the call records) on the same arrays in the same loop -- the yardstick: a
     pass over the same tiles of the same genome --: median of --reps after a warm-up, with the body's bytes.  The batches
     are tools/call_bench.py's four;
  2. Index.call_reset + call_add_host + consensus against Index.call_reset + call_add_host + calls on the same reads, the
     bytes brought back; wall clock;
  3. `spumoni consensus` against `spumoni call` on the same reads file on tmpfs, process start to process gone.

    python tools/consensus_bench.py [--text N] [--seqs N] [--reps N] [--skip-cli] [--label TEXT]
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
STEPS = ("count", "scans", "write")


def kernels_against_calls(ix, name, seqs, offs, bits, min_length, reps, G, n_seqs):
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
    alt = torch.zeros(4 * G, dtype=torch.int32, device="cuda")
    other = torch.zeros(G, dtype=torch.int32, device="cuda")
    ins = torch.zeros(G, dtype=torch.int32, device="cuda")
    ddiff = torch.zeros(G + 1, dtype=torch.int32, device="cuda")
    dele = torch.empty(G, dtype=torch.int32, device="cuda")
    calls = torch.empty((G, 6), dtype=torch.int64, device="cuda")
    ncalls = torch.empty(1, dtype=torch.int64, device="cuda")
    body_cap = 2 * G + n_seqs
    records = torch.empty((n_seqs, 6), dtype=torch.int64, device="cuda")
    body = torch.empty(body_cap, dtype=torch.uint8, device="cuda")
    nbytes = torch.empty(1, dtype=torch.int64, device="cuda")
    ix.mems_device(d_len, d_ptr, offs, min_length, capacity=n, d_match_offsets=mo, d_out=rec)
    ix.chain_device(rec[:n], mo, d_out=chains, d_out_pred=pred)
    ix.extend_device(d_seqs, offs, rec[:n], mo, chains, pred, gap_capacity=n, op_capacity=op_cap, d_out=out, d_out_op_offsets=ooffs,
                     d_out_ops=ops, want_ends=False)
    ix.map_device(out, ooffs, ops, offs, op_capacity=op_cap, in_entries=op_cap, d_out=maps, d_out_op_offsets=moffs, d_out_ops=mops)
    ix.cover_add_device(maps, moffs, mops, diff, mism, counts, in_entries=op_cap)
    ix.cover_finish_device(diff, mism, counts, d_depth=depth, d_out=summary)
    ix.pileup_add_device(maps, moffs, mops, d_seqs, offs, alt, other, ins, ddiff, in_entries=op_cap, in_chars=total)
    ix.pileup_finish_device(ddiff, d_del=dele)
    yard, steps = [], []
    for _ in range(reps + 1):
        ix.calls_device(depth, mism, alt, other, ins, dele, 2, 2, 500, call_capacity=G, d_calls=calls, d_count=ncalls)
        ix.consensus_device(depth, alt, ins, dele, 2, 2, 500, body_capacity=body_cap, d_records=records, d_body=body, d_count=nbytes)
        torch.cuda.synchronize()
        sl, ss = ix.call_stats(), ix.consensus_stats()
        yard.append(sl["step_ms"][2])
        steps.append(ss["step_ms"])
    assert sl["overflow"] == 0 and ss["overflow"] == 0 and ss["bytes"] == int(nbytes.item()), (sl, ss)
    c = med(yard[1:])
    s = [med([x[i] for x in steps[1:]]) for i in range(3)]
    sums = [sum(x) for x in steps[1:]]
    print(f"{name}: {nreads} reads, {total} values, min_length {min_length}, default parameters: {ss['positions']} positions: {ss['kept']} kept, "
          f"{ss['substituted']} substituted ({sl['calls']} calls), {ss['deleted']} deleted, {ss['masked']} masked, {ss['ins_sites']} insertion "
          f"sites; the body is {ss['bytes']} bytes at 60 letters a line\n"
          f"    the calls step (the yardstick)     {c:9.3f} ms   (min {min(yard[1:]):.3f}, max {max(yard[1:]):.3f})\n"
          f"    consensus kernels                  {med(sums):9.3f} ms   (min {min(sums):.3f}, max {max(sums):.3f}) = "
          f"{med(sums) / max(c, 1e-6):.3f} x the calls step", flush=True)
    for label, t in zip(STEPS, s):
        print(f"        {label:28s}       {t:9.3f} ms", flush=True)


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
    print(f"consensus_bench: {a.label}\nhost {socket.gethostname()}, {torch.cuda.get_device_name(0)}, library {capi.version()}\n"
          f"index: capi.build_raw over {text.size} DNA letters: {a.seqs} sequences of {per} (mutated copies of one sequence of "
          f"{per * a.seqs // 8}, cut), each with its reverse complement: n = {ix.n}, r = {ix.r}, built in {time.perf_counter() - t0:.1f} s; "
          f"forward genome {G} bases: the consensus keeps {G / 1e6:.1f} MB of emitted bytes beside the pileup's {28 * G / 1e6:.1f} MB\n", flush=True)

    print("== 1. the consensus kernels beside the calls step on the same arrays (HIP events, median of %d) ==" % a.reps, flush=True)
    seqs, offs = reads_with_indels(text, np.full(1_000_000, 150), rng, 0.01)
    kernels_against_calls(ix, "150 bp, 1 % substitutions", seqs, offs, 16, 20, a.reps, G, a.seqs)
    del seqs, offs
    seqs, offs = reads_with_indels(text, np.full(1_000_000, 150), rng, 0.05, one_indel=True)
    kernels_against_calls(ix, "150 bp, 5 % substitutions and one indel per read", seqs, offs, 16, 20, a.reps, G, a.seqs)
    del seqs, offs
    seqs, offs = reads_with_indels(text, np.full(2000, 10_000), rng, 0.08, f_indel=0.02)
    kernels_against_calls(ix, "10 kbp, 10 % errors (8 % substitutions, 2 % indels)", seqs, offs, 16, 12, a.reps, G, a.seqs)
    kernels_against_calls(ix, "10 kbp, the same reads, min_length 16", seqs, offs, 16, 16, a.reps, G, a.seqs)
    del seqs, offs
    torch.cuda.empty_cache()

    print("\n== 2. host form: call_reset + call_add_host + consensus against call_reset + call_add_host + calls (wall clock) ==", flush=True)
    nreads = 200_000  # 30 M characters: one piece
    d_seqs, d_offs = reads_with_indels(text, np.full(nreads, 150), rng, 0.05, one_indel=True)
    seqs, offs = d_seqs.cpu().numpy(), d_offs.cpu().numpy().astype(np.uint64)
    del d_seqs, d_offs
    new, old = [], []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        ix.call_reset()
        ix.call_add_host(seqs, offs, 20)
        records, body = ix.consensus()
        new.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ix.call_reset()
        ix.call_add_host(seqs, offs, 20)
        got = ix.calls()
        old.append(time.perf_counter() - t0)
    print(f"{nreads} x 150 bp, 5 % substitutions and one indel per read, no digestion, min_length 20; the consensus brings back "
          f"{records.nbytes + body.nbytes} bytes ({int(records['substituted'].sum())} substituted, {int(records['deleted'].sum())} deleted, "
          f"{int(records['masked'].sum())} masked), the calls {got.nbytes} bytes ({got.size} calls)\n"
          f"    call_reset + call_add_host + consensus  {med(new[1:]):8.3f} s   (min {min(new[1:]):.3f}, max {max(new[1:]):.3f})\n"
          f"    call_reset + call_add_host + calls      {med(old[1:]):8.3f} s   (min {min(old[1:]):.3f}, max {max(old[1:]):.3f})", flush=True)

    if a.skip_cli:
        return
    print("\n== 3. CLI, process start to process gone, reads file and outputs on tmpfs ==", flush=True)
    work = tempfile.mkdtemp(prefix="consensus_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
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
        for name in ("call", "consensus"):
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                p = subprocess.run([BIN, name, "-r", prefix[:-3], "-p", reads, "-n", "-L", "20"], capture_output=True, env=env, timeout=600)
                ts.append(time.perf_counter() - t0)
                assert p.returncode == 0, p.stderr.decode()[-2000:]
            res[name] = ts
        print(f"{nreads} x 150 bp, the index above, no digestion\n"
              f"    spumoni call -n -L 20        {med(res['call']):7.3f} s  (runs: {', '.join('%.3f' % t for t in res['call'])}); writes a "
              f".vcf of {os.path.getsize(reads + '.vcf') / 1e6:.2f} MB\n"
              f"    spumoni consensus -n -L 20   {med(res['consensus']):7.3f} s  (runs: {', '.join('%.3f' % t for t in res['consensus'])}); "
              f"writes a .consensus.fa of {os.path.getsize(reads + '.consensus.fa') / 1e6:.2f} MB and a table of "
              f"{os.path.getsize(reads + '.consensus.tsv')} bytes", flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
