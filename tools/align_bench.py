"""Measures the alignments; the output is kept as profiles/align_bench.txt.

  1. the align kernels, step by step (count and scan, walk, fill, reduce: HIP events between the steps), beside what feeds
     them -- the MS walk + k_ms_extend, the match kernels and k_chain -- on the same batch and device: median of --reps
     after a warm-up, and the table cells evaluated per second of the fill.  The batches are tools/chain_bench.py's three
     and a fourth: the 10 kbp reads with min_length raised until the median gap side is at least 16, so that the fill's
     table paths carry the load;
  2. Index.align_host against what a caller did before it existed: Index.mems_host + chain.chain_reference +
     align.align_reference on the host (and Index.chain_host alone beside it), wall clock, with the records compared;
  3. `spumoni align` against `spumoni chain` on the same reads file on tmpfs, process start to process gone.

    python tools/align_bench.py [--text N] [--reps N] [--skip-cli] [--label TEXT]
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
from spumoni_amd.align import ALIGN_DTYPE, GAP_DTYPE, UNFILLED, align_reference  # noqa: E402
from spumoni_amd.chain import chain_reference  # noqa: E402
from tools.chain_bench import reads_with_indels  # noqa: E402
from tools.mems_bench import med, repetitive_text  # noqa: E402

BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
STEPS = ("count + scan", "walk over pred", "fill", "reduce")


def feed(ix, seqs, offs, bits, min_length):
    """The MS arrays, the records, the chains and pred of a batch on the device."""
    total, nreads = seqs.numel(), offs.numel() - 1
    dt = torch.int16 if bits == 16 else torch.int32
    d_seqs = capi.pad_seqs(seqs)
    d_len = torch.empty(total + 16, dtype=dt, device="cuda")
    d_ptr = torch.empty(total + 16, dtype=torch.int64, device="cuda")
    mo = torch.empty(nreads + 1, dtype=torch.int64, device="cuda")
    ix.query_device(capi.SPX_MODE_MS, d_seqs, offs, total, d_lengths=d_len, d_pointers=d_ptr)
    ix.mems_device(d_len, d_ptr, offs, min_length, d_match_offsets=mo)  # (sizes the records)
    n = int(mo[-1].item())
    rec = torch.empty((max(n, 1), 4), dtype=torch.int32, device="cuda")
    return d_seqs, d_len, d_ptr, mo, n, rec


def kernels_against_feed(ix, name, seqs, offs, bits, min_length, reps, quiet=False):
    total, nreads = seqs.numel(), offs.numel() - 1
    d_seqs, d_len, d_ptr, mo, n, rec = feed(ix, seqs, offs, bits, min_length)
    chains = torch.empty((nreads, 12), dtype=torch.int32, device="cuda")
    pred = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    out = torch.empty((nreads, 12), dtype=torch.int32, device="cuda")
    goffs = torch.empty(nreads + 1, dtype=torch.int64, device="cuda")
    gaps = torch.empty((max(n, 1), 4), dtype=torch.int32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    walk, mems, chain, align, steps = [], [], [], [], []
    for _ in range(1 if quiet else reps + 1):
        e0.record()
        ix.query_device(capi.SPX_MODE_MS, d_seqs, offs, total, d_lengths=d_len, d_pointers=d_ptr)
        e1.record()
        ix.mems_device(d_len, d_ptr, offs, min_length, capacity=n, d_match_offsets=mo, d_out=rec)
        ix.chain_device(rec[:n], mo, d_out=chains, d_out_pred=pred)
        ix.align_device(d_seqs, offs, rec[:n], mo, chains, pred, gap_capacity=n, d_out=out, d_out_gap_offsets=goffs, d_out_gaps=gaps)
        torch.cuda.synchronize()
        walk.append(e0.elapsed_time(e1))
        mems.append(ix.mems_stats()["kernel_ms"])
        chain.append(ix.chain_stats()["kernel_ms"])
        st = ix.align_stats()
        align.append(st["kernel_ms"])
        steps.append(st["step_ms"])
    g = gaps[:int(goffs[-1].item())].cpu().numpy().view(GAP_DTYPE).reshape(-1)
    side = np.maximum(g["a"], g["b"]) if g.size else np.zeros(1)
    if quiet:
        return float(np.median(side))
    skip = 0 if len(walk) == 1 else 1
    w, m, c, v = med(walk[skip:]), med(mems[skip:]), med(chain[skip:]), med(align[skip:])
    s = [med([x[i] for x in steps[skip:]]) for i in range(4)]
    r = out.cpu().numpy().view(ALIGN_DTYPE).reshape(-1)
    ok = r["anchors"] > 0
    table = (g["a"] >= 1) & (g["b"] >= 1) & ~((g["a"] == 1) & (g["b"] == 1)) & (g["edits"] != UNFILLED)
    lane = table & (g["a"] <= 16) & (g["b"] <= 16)
    print(f"{name}: {nreads} reads, {total} values, {bits}-bit, min_length {min_length}, default parameters: {n} anchors, "
          f"{st['aligned_reads']} reads aligned, {st['gaps']} gaps ({st['gaps'] / max(st['aligned_reads'], 1):.1f} per aligned read; median side "
          f"{np.median(side):.0f}, largest {int(side.max())}), {st['filled_gaps']} filled, {int(table.sum())} through a table ({int(lane.sum())} a lane each, "
          f"{int((table & ~lane).sum())} a wavefront each), {st['cells']} cells; per aligned read {r['matches'][ok].mean():.1f} matches and "
          f"{r['edits'][ok].mean():.1f} edits\n"
          f"    MS walk + k_ms_extend   {w:9.3f} ms   (min {min(walk[skip:]):.3f}, max {max(walk[skip:]):.3f})\n"
          f"    match kernels           {m:9.3f} ms\n"
          f"    k_chain (with pred)     {c:9.3f} ms\n"
          f"    align kernels           {v:9.3f} ms   (min {min(align[skip:]):.3f}, max {max(align[skip:]):.3f})   = {100 * v / (w + m + c):.1f} % of what feeds them", flush=True)
    for label, t in zip(STEPS, s):
        print(f"        {label:16s}    {t:9.3f} ms", flush=True)
    if st["cells"]:
        print(f"    fill: {st['cells']} cells in {s[2]:.3f} ms = {st['cells'] / max(s[2], 1e-6) / 1e6:.2f} G cells/s (the step also visits every gap that needs no table)",
              flush=True)


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
    print(f"align_bench: {a.label}\nhost {socket.gethostname()}, {torch.cuda.get_device_name(0)}, library {capi.version()}\n"
          f"index: capi.build_raw over {a.text} DNA letters (mutated copies of one sequence of {a.text // 8}): n = {ix.n}, r = {ix.r}, "
          f"built in {time.perf_counter() - t0:.1f} s\n", flush=True)

    print("== 1. the align kernels step by step, beside the walk, match and chain kernels that feed them (HIP events, median of %d) ==" % a.reps,
          flush=True)
    seqs, offs = reads_with_indels(text, np.full(1_000_000, 150), rng, 0.01)
    kernels_against_feed(ix, "150 bp, 1 % substitutions", seqs, offs, 16, 20, a.reps)
    del seqs, offs
    seqs, offs = reads_with_indels(text, np.full(1_000_000, 150), rng, 0.05, one_indel=True)
    kernels_against_feed(ix, "150 bp, 5 % substitutions and one indel per read", seqs, offs, 16, 20, a.reps)
    del seqs, offs
    seqs, offs = reads_with_indels(text, np.full(2000, 10_000), rng, 0.08, f_indel=0.02)
    kernels_against_feed(ix, "10 kbp, 10 % errors (8 % substitutions, 2 % indels)", seqs, offs, 16, 12, a.reps)
    raised = None
    for min_length in (16, 20, 24, 28, 32, 40, 48, 64):
        side = kernels_against_feed(ix, "", seqs, offs, 16, min_length, 0, quiet=True)
        if side >= 16:
            raised = min_length
            break
    if raised is None:
        print("10 kbp: no min_length up to 64 gives a median gap side of 16 or more", flush=True)
    else:
        kernels_against_feed(ix, f"10 kbp, the same reads, min_length raised to {raised} (the first of 16, 20, ... with a median gap side >= 16)",
                             seqs, offs, 16, raised, a.reps)
    del seqs, offs
    torch.cuda.empty_cache()

    print("\n== 2. host form: align_host against mems_host + chain_reference + align_reference (wall clock) ==", flush=True)
    nreads = 200_000  # 30 M characters: one piece
    d_seqs, d_offs = reads_with_indels(text, np.full(nreads, 150), rng, 0.05, one_indel=True)
    seqs, offs = d_seqs.cpu().numpy(), d_offs.cpu().numpy().astype(np.uint64)
    del d_seqs, d_offs
    new, old = [], []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        got, _, _ = ix.align_host(seqs, offs, 20)
        new.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ix.chain_host(seqs, offs, 20)
        old.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    mo, rec, _ = ix.mems_host(seqs, offs, 20)
    t1 = time.perf_counter()
    chains, _, pred = chain_reference(mo, rec)
    t2 = time.perf_counter()
    want, _, _ = align_reference(seqs, offs, text, mo, rec, chains, pred)
    t3 = time.perf_counter()
    same = bool(np.array_equal(got, want))
    print(f"{nreads} x 150 bp, 5 % substitutions and one indel per read, no digestion, min_length 20; records equal: {same}\n"
          f"    align_host                              {med(new[1:]):8.3f} s   (min {min(new[1:]):.3f}, max {max(new[1:]):.3f})\n"
          f"    chain_host (no gaps filled)             {med(old[1:]):8.3f} s   (min {min(old[1:]):.3f}, max {max(old[1:]):.3f})\n"
          f"    mems_host (records back)                {t1 - t0:8.3f} s\n"
          f"    + chain_reference on the host           {t2 - t1:8.3f} s\n"
          f"    + align_reference on the host           {t3 - t2:8.3f} s   together {t3 - t0:.3f} s = {(t3 - t0) / med(new[1:]):.1f} x align_host",
          flush=True)
    assert same

    if a.skip_cli:
        return
    print("\n== 3. CLI, process start to process gone, reads file and outputs on tmpfs ==", flush=True)
    work = tempfile.mkdtemp(prefix="align_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
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
        for name, cmd in (("chain", [BIN, "chain", "-r", prefix[:-3], "-p", reads, "-n", "-L", "20"]),
                          ("align", [BIN, "align", "-r", prefix[:-3], "-p", reads, "-n", "-L", "20"])):
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                p = subprocess.run(cmd, capture_output=True, env=env, timeout=600)
                ts.append(time.perf_counter() - t0)
                assert p.returncode == 0, p.stderr.decode()[-2000:]
            res[name] = ts
        print(f"{nreads} x 150 bp, the index above, no digestion\n"
              f"    spumoni chain -n -L 20   {med(res['chain']):7.3f} s  (runs: {', '.join('%.3f' % t for t in res['chain'])}); writes "
              f"{os.path.getsize(reads + '.chains') / 1e6:.1f} MB\n"
              f"    spumoni align -n -L 20   {med(res['align']):7.3f} s  (runs: {', '.join('%.3f' % t for t in res['align'])}); writes "
              f"{os.path.getsize(reads + '.alignments') / 1e6:.1f} MB", flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
