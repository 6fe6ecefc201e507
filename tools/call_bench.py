"""Measures the pileup and the calls; the output is kept as profiles/call_bench.txt.

  1. the call kernels -- add, finish, calls, each between its own HIP events -- beside the coverage's add on the same batch
     in the same loop -- the yardstick: one atomic per 'X' column in both --: median of --reps after a warm-up, with the
     atomic adds a read costs.  The batches are tools/cover_bench.py's four.  The add step is measured three times: with
     the switch where it is (a read of more than 64 entries takes a wavefront), with a lane per read forced and with a
     wavefront per read forced;
  2. Index.call_reset + call_add_host + calls against Index.cover_reset + cover_add_host + cover_summary on the same
     reads; wall clock.  The difference includes the second copy of the reads;
  3. `spumoni call` against `spumoni cover -b` on the same reads file on tmpfs, process start to process gone.

    python tools/call_bench.py [--text N] [--seqs N] [--reps N] [--skip-cli] [--label TEXT]
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
STEPS = ("add", "finish (scan)", "calls (count + scan + write)")
SWITCHES = (("the switch at 64 entries", 64), ("a lane per read forced", 1 << 30), ("a wavefront per read forced", 0))


def kernels_against_cover(ix, name, seqs, offs, bits, min_length, reps, G, n_seqs):
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
    call_cap = G
    calls = torch.empty((call_cap, 6), dtype=torch.int64, device="cuda")
    ncalls = torch.empty(1, dtype=torch.int64, device="cuda")
    ix.mems_device(d_len, d_ptr, offs, min_length, capacity=n, d_match_offsets=mo, d_out=rec)
    ix.chain_device(rec[:n], mo, d_out=chains, d_out_pred=pred)
    ix.extend_device(d_seqs, offs, rec[:n], mo, chains, pred, gap_capacity=n, op_capacity=op_cap, d_out=out, d_out_op_offsets=ooffs,
                     d_out_ops=ops, want_ends=False)
    ix.map_device(out, ooffs, ops, offs, op_capacity=op_cap, in_entries=op_cap, d_out=maps, d_out_op_offsets=moffs, d_out_ops=mops)
    cover_add, steps = [], []
    for _ in range(reps + 1):
        for t in (diff, mism, counts, alt, other, ins, ddiff):
            t.zero_()
        ix.cover_add_device(maps, moffs, mops, diff, mism, counts, in_entries=op_cap)
        ix.cover_finish_device(diff, mism, counts, d_depth=depth, d_out=summary)
        ix.pileup_add_device(maps, moffs, mops, d_seqs, offs, alt, other, ins, ddiff, in_entries=op_cap, in_chars=total)
        ix.pileup_finish_device(ddiff, d_del=dele)
        ix.calls_device(depth, mism, alt, other, ins, dele, 2, 2, 500, call_capacity=call_cap, d_calls=calls, d_count=ncalls)
        torch.cuda.synchronize()
        sc, sl = ix.cover_stats(), ix.call_stats()
        cover_add.append(sc["step_ms"][0])
        steps.append(sl["step_ms"])
    assert sc["error"] == 0 and sl["error"] == 0 and sl["overflow"] == 0 and sl["skipped"] == 0 and sl["added"] == sc["added"], (sc, sl)
    assert int(alt.sum()) + int(other.sum()) == sl["x_columns"] == int(mism.sum())
    c = med(cover_add[1:])
    s = [med([x[i] for x in steps[1:]]) for i in range(3)]
    print(f"{name}: {nreads} reads, {total} values, min_length {min_length}, default parameters: {sl['added']} reads mapped and added, "
          f"{sl['x_columns']} 'X' columns ({sl['other_columns']} of a byte outside ACGT), {sl['insertions']} 'I' and {sl['deletions']} 'D' entries, "
          f"{sl['atomics']} atomic adds ({sl['atomics'] / max(sl['added'], 1):.2f} a read) beside the coverage's {sc['atomics']} "
          f"({sc['atomics'] / max(sc['added'], 1):.2f} a read); {sl['calls']} calls at depth 2, 2 reads, 500 thousandths\n"
          f"    the coverage's add (the yardstick) {c:9.3f} ms   (min {min(cover_add[1:]):.3f}, max {max(cover_add[1:]):.3f})\n"
          f"    call kernels                       {sum(s):9.3f} ms; the add = {s[0] / max(c, 1e-6):.3f} x the coverage's add", flush=True)
    for label, t in zip(STEPS, s):
        print(f"        {label:28s}       {t:9.3f} ms", flush=True)
    want = tuple(t.clone() for t in (alt, other, ins, ddiff))
    try:
        for label, switch in SWITCHES:
            ix.set_option("call_switch", switch)
            ts = []
            for _ in range(reps + 1):
                for t in (alt, other, ins, ddiff):
                    t.zero_()
                ix.pileup_add_device(maps, moffs, mops, d_seqs, offs, alt, other, ins, ddiff, in_entries=op_cap, in_chars=total)
                torch.cuda.synchronize()
                ts.append(ix.call_stats()["step_ms"][0])
            assert all(torch.equal(a, b) for a, b in zip(want, (alt, other, ins, ddiff))), label
            print(f"        add, {label:28s}  {med(ts[1:]):9.3f} ms   (min {min(ts[1:]):.3f}, max {max(ts[1:]):.3f})", flush=True)
    finally:
        ix.set_option("call_switch", 64)


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
    print(f"call_bench: {a.label}\nhost {socket.gethostname()}, {torch.cuda.get_device_name(0)}, library {capi.version()}\n"
          f"index: capi.build_raw over {text.size} DNA letters: {a.seqs} sequences of {per} (mutated copies of one sequence of "
          f"{per * a.seqs // 8}, cut), each with its reverse complement: n = {ix.n}, r = {ix.r}, built in {time.perf_counter() - t0:.1f} s; "
          f"forward genome {G} bases: alt, other, ins, ddiff and del take {28 * G / 1e6:.1f} MB beside the coverage's {12 * G / 1e6:.1f} MB\n",
          flush=True)

    print("== 1. the call kernels beside the coverage's add on the same batch (HIP events, median of %d) ==" % a.reps, flush=True)
    seqs, offs = reads_with_indels(text, np.full(1_000_000, 150), rng, 0.01)
    kernels_against_cover(ix, "150 bp, 1 % substitutions", seqs, offs, 16, 20, a.reps, G, a.seqs)
    del seqs, offs
    seqs, offs = reads_with_indels(text, np.full(1_000_000, 150), rng, 0.05, one_indel=True)
    kernels_against_cover(ix, "150 bp, 5 % substitutions and one indel per read", seqs, offs, 16, 20, a.reps, G, a.seqs)
    del seqs, offs
    seqs, offs = reads_with_indels(text, np.full(2000, 10_000), rng, 0.08, f_indel=0.02)
    kernels_against_cover(ix, "10 kbp, 10 % errors (8 % substitutions, 2 % indels)", seqs, offs, 16, 12, a.reps, G, a.seqs)
    kernels_against_cover(ix, "10 kbp, the same reads, min_length 16", seqs, offs, 16, 16, a.reps, G, a.seqs)
    del seqs, offs
    torch.cuda.empty_cache()

    print("\n== 2. host form: call_reset + call_add_host + calls against cover_reset + cover_add_host + cover_summary (wall clock) ==", flush=True)
    nreads = 200_000  # 30 M characters: one piece
    d_seqs, d_offs = reads_with_indels(text, np.full(nreads, 150), rng, 0.05, one_indel=True)
    seqs, offs = d_seqs.cpu().numpy(), d_offs.cpu().numpy().astype(np.uint64)
    del d_seqs, d_offs
    new, old = [], []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        ix.call_reset()
        ix.call_add_host(seqs, offs, 20)
        got = ix.calls()
        new.append(time.perf_counter() - t0)
        mine = ix.cover_summary(a.seqs)
        t0 = time.perf_counter()
        ix.cover_reset()
        ix.cover_add_host(seqs, offs, 20)
        want = ix.cover_summary(a.seqs)
        old.append(time.perf_counter() - t0)
    same = mine.tobytes() == want.tobytes()
    print(f"{nreads} x 150 bp, 5 % substitutions and one indel per read, no digestion, min_length 20; {got.size} calls ({got.nbytes} bytes) come "
          f"back; the coverage is the same on both paths: {same}; the reads' second copy is {seqs.size / 1e6:.1f} MB\n"
          f"    call_reset + call_add_host + calls            {med(new[1:]):8.3f} s   (min {min(new[1:]):.3f}, max {max(new[1:]):.3f})\n"
          f"    cover_reset + cover_add_host + cover_summary  {med(old[1:]):8.3f} s   (min {min(old[1:]):.3f}, max {max(old[1:]):.3f})", flush=True)
    assert same

    if a.skip_cli:
        return
    print("\n== 3. CLI, process start to process gone, reads file and outputs on tmpfs ==", flush=True)
    work = tempfile.mkdtemp(prefix="call_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
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
        for name, extra in (("cover", ["-b"]), ("call", [])):
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                p = subprocess.run([BIN, name, "-r", prefix[:-3], "-p", reads, "-n", "-L", "20"] + extra, capture_output=True, env=env, timeout=600)
                ts.append(time.perf_counter() - t0)
                assert p.returncode == 0, p.stderr.decode()[-2000:]
            res[name] = ts
        print(f"{nreads} x 150 bp, the index above, no digestion\n"
              f"    spumoni cover -n -L 20 -b   {med(res['cover']):7.3f} s  (runs: {', '.join('%.3f' % t for t in res['cover'])}); writes "
              f"{os.path.getsize(reads + '.cover')} bytes and a bedgraph of {os.path.getsize(reads + '.bedgraph') / 1e6:.1f} MB\n"
              f"    spumoni call -n -L 20       {med(res['call']):7.3f} s  (runs: {', '.join('%.3f' % t for t in res['call'])}); writes a "
              f".vcf of {os.path.getsize(reads + '.vcf') / 1e6:.2f} MB", flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
