"""Measures the extended CIGARs; the output is kept as profiles/extend_bench.txt.

  1. the extend kernels, step by step (plan with the ends' sizes, the lane fills, the wavefront fills, emit, reduce with the
     records' update, and the ends' own step: HIP events between the steps), beside the cigar kernels on the same batch in
     the same loop -- the yardstick: the same alignments without their ends --: median of --reps after a warm-up, with the
     ends looked at and extended, the band cells and the clipped characters.  The batches are tools/align_bench.py's four;
  2. the scratch the ends take: the trace (LDS, or a buffer per wavefront when the parameters let an end outgrow it) and
     the path;
  3. Index.extend_host against Index.cigar_host, wall clock, with the middles compared by their counts;
  4. `spumoni extend` against `spumoni cigar` on the same reads file on tmpfs, process start to process gone.

    python tools/extend_bench.py [--text N] [--reps N] [--skip-cli] [--label TEXT]
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
from spumoni_amd.extend import ExtendParams  # noqa: E402
from tools.align_bench import feed  # noqa: E402
from tools.chain_bench import reads_with_indels  # noqa: E402
from tools.mems_bench import med, repetitive_text  # noqa: E402

BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
STEPS = ("plan (with the ends' sizes)", "lane fills + walk back", "wavefront fills + walk back", "emit", "reduce + update", "ends")
TRACE_BUDGET, TRACE_GRID, TRACE_LDS_WORDS = 64 << 20, 16384, 2048  # spx_cigar_kernels.h: TRACE_BUDGET, ENDS_GRID, TRACE_LDS_WORDS


def kernels_against_cigar(ix, name, seqs, offs, bits, min_length, reps):
    total, nreads = seqs.numel(), offs.numel() - 1
    d_seqs, d_len, d_ptr, mo, n, rec = feed(ix, seqs, offs, bits, min_length)
    chains = torch.empty((nreads, 12), dtype=torch.int32, device="cuda")
    pred = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    out = torch.empty((nreads, 12), dtype=torch.int32, device="cuda")
    out2 = torch.empty((nreads, 12), dtype=torch.int32, device="cuda")
    ooffs = torch.empty(nreads + 1, dtype=torch.int64, device="cuda")
    ooffs2 = torch.empty(nreads + 1, dtype=torch.int64, device="cuda")
    op_cap = 2 * total + 2 * n + 3 * nreads
    ops = torch.empty(op_cap, dtype=torch.int32, device="cuda")
    ops2 = torch.empty(op_cap, dtype=torch.int32, device="cuda")
    ends = torch.empty((2 * nreads, 4), dtype=torch.int32, device="cuda")
    ix.mems_device(d_len, d_ptr, offs, min_length, capacity=n, d_match_offsets=mo, d_out=rec)
    ix.chain_device(rec[:n], mo, d_out=chains, d_out_pred=pred)
    cigar, csteps, extend, steps = [], [], [], []
    for _ in range(reps + 1):
        ix.cigar_device(d_seqs, offs, rec[:n], mo, chains, pred, gap_capacity=n, op_capacity=op_cap, d_out=out, d_out_op_offsets=ooffs,
                        d_out_ops=ops)
        ix.extend_device(d_seqs, offs, rec[:n], mo, chains, pred, gap_capacity=n, op_capacity=op_cap, d_out=out2, d_out_op_offsets=ooffs2,
                         d_out_ops=ops2, d_out_ends=ends)
        torch.cuda.synchronize()
        sc, st = ix.cigar_stats(), ix.extend_stats()
        cigar.append(sc["kernel_ms"])
        csteps.append(sc["step_ms"])
        extend.append(st["kernel_ms"])
        steps.append(st["step_ms"])
    assert st["overflow"] == 0 and st["error"] == 0 and sc["overflow"] == 0, (st, sc)
    assert torch.equal(out[:, 8:], out2[:, 8:]) and st["aligned_reads"] == sc["aligned_reads"] and st["cells"] == sc["cells"]
    v, c = med(cigar[1:]), med(extend[1:])
    s = [med([x[i] for x in steps[1:]]) for i in range(6)]
    cs = [med([x[i] for x in csteps[1:]]) for i in range(5)]
    lens = (offs[1:] - offs[:-1]).to(torch.int64)
    whole = int(((out2[:, 4] == 0) & (out2[:, 5].to(torch.int64) == lens)).sum())
    print(f"{name}: {nreads} reads, {total} values, min_length {min_length}, default parameters: {st['aligned_reads']} reads aligned, "
          f"{st['ends']} ends looked at, {st['extended_ends']} extended, {st['band_cells']} band cells, {st['clipped']} characters clipped, "
          f"{whole} reads aligned end to end, {st['entries']} entries against cigar's {sc['entries']}, {st['path_words'] * 4} bytes of path "
          f"against {sc['path_words'] * 4}\n"
          f"    cigar kernels (the yardstick)   {v:9.3f} ms   (min {min(cigar[1:]):.3f}, max {max(cigar[1:]):.3f}; emit {cs[3]:.3f})\n"
          f"    extend kernels                  {c:9.3f} ms   (min {min(extend[1:]):.3f}, max {max(extend[1:]):.3f})   = {c / max(v, 1e-6):.2f} x cigar",
          flush=True)
    for label, t in zip(STEPS, s):
        print(f"        {label:28s}    {t:9.3f} ms", flush=True)


def scratch_report():
    print("\n== 2. scratch of the ends ==", flush=True)
    for ep in (ExtendParams(), ExtendParams(4096, 16, 4, 6), ExtendParams(4096, 63, 4, 6)):
        words = (ep.max_extend + 15) // 16 * (2 * ep.band + 1)
        sizes = (4 * min(words, TRACE_LDS_WORDS), (ep.max_extend + 3) & ~3, (ep.max_extend + ep.band + 4) & ~3)
        where = "LDS always" if words <= TRACE_LDS_WORDS else \
            f"a buffer of {words * 4} bytes per wavefront above {TRACE_LDS_WORDS} words, {max(1, min(TRACE_GRID, TRACE_BUDGET // (words * 4)))} wavefronts at most"
        print(f"max_extend {ep.max_extend}, band {ep.band}: an end's trace is at most {words} words: {where}; LDS per wavefront {sum(sizes)} bytes "
              f"(trace {sizes[0]}, A {sizes[1]}, B {sizes[2]}); path scratch of the device form: + 2 * reads * {(2 * ep.max_extend + ep.band + 15) // 16} words, "
              f"of the host form: the words the ends need (above: 'bytes of path')", flush=True)


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
    print(f"extend_bench: {a.label}\nhost {socket.gethostname()}, {torch.cuda.get_device_name(0)}, library {capi.version()}\n"
          f"index: capi.build_raw over {a.text} DNA letters (mutated copies of one sequence of {a.text // 8}): n = {ix.n}, r = {ix.r}, "
          f"built in {time.perf_counter() - t0:.1f} s\n", flush=True)

    print("== 1. the extend kernels step by step, beside the cigar kernels on the same batch (HIP events, median of %d) ==" % a.reps, flush=True)
    seqs, offs = reads_with_indels(text, np.full(1_000_000, 150), rng, 0.01)
    kernels_against_cigar(ix, "150 bp, 1 % substitutions", seqs, offs, 16, 20, a.reps)
    del seqs, offs
    seqs, offs = reads_with_indels(text, np.full(1_000_000, 150), rng, 0.05, one_indel=True)
    kernels_against_cigar(ix, "150 bp, 5 % substitutions and one indel per read", seqs, offs, 16, 20, a.reps)
    del seqs, offs
    seqs, offs = reads_with_indels(text, np.full(2000, 10_000), rng, 0.08, f_indel=0.02)
    kernels_against_cigar(ix, "10 kbp, 10 % errors (8 % substitutions, 2 % indels)", seqs, offs, 16, 12, a.reps)
    kernels_against_cigar(ix, "10 kbp, the same reads, min_length 16 (align_bench's fourth batch)", seqs, offs, 16, 16, a.reps)
    del seqs, offs
    torch.cuda.empty_cache()
    scratch_report()

    print("\n== 3. host form: extend_host against cigar_host (wall clock) ==", flush=True)
    nreads = 200_000  # 30 M characters: one piece
    d_seqs, d_offs = reads_with_indels(text, np.full(nreads, 150), rng, 0.05, one_indel=True)
    seqs, offs = d_seqs.cpu().numpy(), d_offs.cpu().numpy().astype(np.uint64)
    del d_seqs, d_offs
    new, old = [], []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        got = ix.extend_host(seqs, offs, 20)
        new.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        want = ix.cigar_host(seqs, offs, 20)
        old.append(time.perf_counter() - t0)
    same = bool(np.array_equal(got[0]["anchors"], want[0]["anchors"]) and np.array_equal(got[3], want[3]))
    st = ix.extend_stats()
    print(f"{nreads} x 150 bp, 5 % substitutions and one indel per read, no digestion, min_length 20; chains and anchors equal: {same}; "
          f"{got[2].size} entries against {want[2].size}, {st['extended_ends']} of {st['ends']} ends extended, {st['clipped']} characters clipped\n"
          f"    extend_host (begin + fetch)  {med(new[1:]):8.3f} s   (min {min(new[1:]):.3f}, max {max(new[1:]):.3f})\n"
          f"    cigar_host (begin + fetch)   {med(old[1:]):8.3f} s   (min {min(old[1:]):.3f}, max {max(old[1:]):.3f})", flush=True)
    assert same

    if a.skip_cli:
        return
    print("\n== 4. CLI, process start to process gone, reads file and outputs on tmpfs ==", flush=True)
    work = tempfile.mkdtemp(prefix="extend_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
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
        for name in ("cigar", "extend"):
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                p = subprocess.run([BIN, name, "-r", prefix[:-3], "-p", reads, "-n", "-L", "20"], capture_output=True, env=env, timeout=600)
                ts.append(time.perf_counter() - t0)
                assert p.returncode == 0, p.stderr.decode()[-2000:]
            res[name] = ts
        print(f"{nreads} x 150 bp, the index above, no digestion\n"
              f"    spumoni cigar -n -L 20    {med(res['cigar']):7.3f} s  (runs: {', '.join('%.3f' % t for t in res['cigar'])}); writes "
              f"{os.path.getsize(reads + '.cigars') / 1e6:.1f} MB\n"
              f"    spumoni extend -n -L 20   {med(res['extend']):7.3f} s  (runs: {', '.join('%.3f' % t for t in res['extend'])}); writes "
              f"{os.path.getsize(reads + '.extended') / 1e6:.1f} MB", flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
