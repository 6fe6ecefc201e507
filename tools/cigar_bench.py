"""Measures the CIGARs; the output is kept as profiles/cigar_bench.txt.

  1. the cigar kernels, step by step (plan, the lane fills with their walk back, the wavefront fills with theirs, emit,
     reduce: HIP events between the steps, and the wavefronts' own clock for the share of the walk back), beside the align
     kernels on the same batch and device -- the yardstick: the same tables without their directions --: median of --reps
     after a warm-up.  The batches are tools/align_bench.py's four;
  2. the scratch the tracing takes at max_fill 512 and 4096: the wavefronts' trace buffers (by max_fill alone) and the path;
  3. Index.cigar_host against Index.align_host, wall clock, with the records compared;
  4. `spumoni cigar` against `spumoni align` on the same reads file on tmpfs, process start to process gone.

    python tools/cigar_bench.py [--text N] [--reps N] [--skip-cli] [--label TEXT]
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
from spumoni_amd import capi  # noqa: E402
from tools.align_bench import feed  # noqa: E402
from tools.chain_bench import reads_with_indels  # noqa: E402
from tools.mems_bench import med, repetitive_text  # noqa: E402

BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
STEPS = ("plan", "lane fills + walk back", "wavefront fills + walk back", "emit", "reduce")
TRACE_BUDGET, TRACE_GRID = 64 << 20, 4096  # spx_cigar.hip


def kernels_against_align(ix, name, seqs, offs, bits, min_length, reps):
    total, nreads = seqs.numel(), offs.numel() - 1
    d_seqs, d_len, d_ptr, mo, n, rec = feed(ix, seqs, offs, bits, min_length)
    chains = torch.empty((nreads, 12), dtype=torch.int32, device="cuda")
    pred = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    out = torch.empty((nreads, 12), dtype=torch.int32, device="cuda")
    out2 = torch.empty((nreads, 12), dtype=torch.int32, device="cuda")
    ooffs = torch.empty(nreads + 1, dtype=torch.int64, device="cuda")
    op_cap = 2 * total + 2 * n + nreads
    ops = torch.empty(op_cap, dtype=torch.int32, device="cuda")
    ix.mems_device(d_len, d_ptr, offs, min_length, capacity=n, d_match_offsets=mo, d_out=rec)
    ix.chain_device(rec[:n], mo, d_out=chains, d_out_pred=pred)
    align, fills, cigar, steps = [], [], [], []
    for _ in range(reps + 1):
        ix.align_device(d_seqs, offs, rec[:n], mo, chains, pred, gap_capacity=n, d_out=out)
        ix.cigar_device(d_seqs, offs, rec[:n], mo, chains, pred, gap_capacity=n, op_capacity=op_cap, d_out=out2, d_out_op_offsets=ooffs,
                        d_out_ops=ops)
        torch.cuda.synchronize()
        sa, st = ix.align_stats(), ix.cigar_stats()
        align.append(sa["kernel_ms"])
        fills.append(sa["step_ms"][2])
        cigar.append(st["kernel_ms"])
        steps.append(st["step_ms"])
    assert torch.equal(out, out2) and st["overflow"] == 0 and st["error"] == 0, st
    v, c = med(align[1:]), med(cigar[1:])
    s = [med([x[i] for x in steps[1:]]) for i in range(5)]
    ticks = st["wave_fill_ticks"] + st["wave_back_ticks"]
    print(f"{name}: {nreads} reads, {total} values, min_length {min_length}, default parameters: {st['aligned_reads']} reads aligned, "
          f"{st['gaps']} gaps, {st['cells']} cells, {st['entries']} entries ({st['entries'] / max(st['aligned_reads'], 1):.1f} per aligned read), "
          f"{st['path_words'] * 4} bytes of path; records equal to align's\n"
          f"    align kernels (the yardstick)   {v:9.3f} ms   (min {min(align[1:]):.3f}, max {max(align[1:]):.3f}; of it the fill {med(fills[1:]):.3f})\n"
          f"    cigar kernels                   {c:9.3f} ms   (min {min(cigar[1:]):.3f}, max {max(cigar[1:]):.3f})   = {c / max(v, 1e-6):.2f} x align", flush=True)
    for label, t in zip(STEPS, s):
        print(f"        {label:28s}    {t:9.3f} ms", flush=True)
    if ticks:
        print(f"    inside the wavefront step, by the wavefronts' own clock: {100 * st['wave_back_ticks'] / ticks:.1f} % walk back, the rest fill "
              f"(= {s[2] * st['wave_back_ticks'] / ticks:.3f} ms of the step's {s[2]:.3f})", flush=True)


def scratch_report(ix):
    print("\n== 2. scratch of the tracing ==", flush=True)
    for max_fill in (512, 4096):
        per_block = max_fill * ((max_fill + 15) // 16) * 4
        grid = max(1, min(TRACE_GRID, TRACE_BUDGET // per_block))
        print(f"max_fill {max_fill}: a wavefront's trace buffer {per_block} bytes, {grid} wavefronts at most -> {grid * per_block / 2**20:.1f} MiB "
              f"(the grid is also at most the gap capacity); LDS per wavefront {(max_fill + 1) * 4 + max_fill + 8192} bytes with the trace in LDS, "
              f"{(max_fill + 1) * 4 + max_fill} without; path scratch of the device form: min(gap_capacity * {(max_fill + 7) // 8}, 2^28) words, "
              f"of the host form: the words the gaps need (above: 'bytes of path')", flush=True)


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
    print(f"cigar_bench: {a.label}\nhost {socket.gethostname()}, {torch.cuda.get_device_name(0)}, library {capi.version()}\n"
          f"index: capi.build_raw over {a.text} DNA letters (mutated copies of one sequence of {a.text // 8}): n = {ix.n}, r = {ix.r}, "
          f"built in {time.perf_counter() - t0:.1f} s\n", flush=True)

    print("== 1. the cigar kernels step by step, beside the align kernels on the same batch (HIP events, median of %d) ==" % a.reps, flush=True)
    seqs, offs = reads_with_indels(text, np.full(1_000_000, 150), rng, 0.01)
    kernels_against_align(ix, "150 bp, 1 % substitutions", seqs, offs, 16, 20, a.reps)
    del seqs, offs
    seqs, offs = reads_with_indels(text, np.full(1_000_000, 150), rng, 0.05, one_indel=True)
    kernels_against_align(ix, "150 bp, 5 % substitutions and one indel per read", seqs, offs, 16, 20, a.reps)
    del seqs, offs
    seqs, offs = reads_with_indels(text, np.full(2000, 10_000), rng, 0.08, f_indel=0.02)
    kernels_against_align(ix, "10 kbp, 10 % errors (8 % substitutions, 2 % indels)", seqs, offs, 16, 12, a.reps)
    kernels_against_align(ix, "10 kbp, the same reads, min_length 16 (align_bench's fourth batch)", seqs, offs, 16, 16, a.reps)
    del seqs, offs
    torch.cuda.empty_cache()
    scratch_report(ix)

    print("\n== 3. host form: cigar_host against align_host (wall clock) ==", flush=True)
    nreads = 200_000  # 30 M characters: one piece
    d_seqs, d_offs = reads_with_indels(text, np.full(nreads, 150), rng, 0.05, one_indel=True)
    seqs, offs = d_seqs.cpu().numpy(), d_offs.cpu().numpy().astype(np.uint64)
    del d_seqs, d_offs
    new, old = [], []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        got = ix.cigar_host(seqs, offs, 20)
        new.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        want, _, _ = ix.align_host(seqs, offs, 20)
        old.append(time.perf_counter() - t0)
    same = bool(np.array_equal(got[0], want))
    print(f"{nreads} x 150 bp, 5 % substitutions and one indel per read, no digestion, min_length 20; records equal: {same}; {got[2].size} entries\n"
          f"    cigar_host (begin + fetch)   {med(new[1:]):8.3f} s   (min {min(new[1:]):.3f}, max {max(new[1:]):.3f})\n"
          f"    align_host                   {med(old[1:]):8.3f} s   (min {min(old[1:]):.3f}, max {max(old[1:]):.3f})", flush=True)
    assert same

    if a.skip_cli:
        return
    print("\n== 4. CLI, process start to process gone, reads file and outputs on tmpfs ==", flush=True)
    work = tempfile.mkdtemp(prefix="cigar_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
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
        for name in ("align", "cigar"):
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                p = subprocess.run([BIN, name, "-r", prefix[:-3], "-p", reads, "-n", "-L", "20"], capture_output=True, env=env, timeout=600)
                ts.append(time.perf_counter() - t0)
                assert p.returncode == 0, p.stderr.decode()[-2000:]
            res[name] = ts
        print(f"{nreads} x 150 bp, the index above, no digestion\n"
              f"    spumoni align -n -L 20   {med(res['align']):7.3f} s  (runs: {', '.join('%.3f' % t for t in res['align'])}); writes "
              f"{os.path.getsize(reads + '.alignments') / 1e6:.1f} MB\n"
              f"    spumoni cigar -n -L 20   {med(res['cigar']):7.3f} s  (runs: {', '.join('%.3f' % t for t in res['cigar'])}); writes "
              f"{os.path.getsize(reads + '.cigars') / 1e6:.1f} MB", flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
