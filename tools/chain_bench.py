"""Measures the chains; the output is kept as profiles/chain_bench.txt.

  1. the chain kernel against what feeds it -- the MS walk + k_ms_extend and the match kernels -- on the same batch and
     device: HIP-event times, median of --reps after a warm-up, beside a plain device copy of the bytes the kernel must
     move (the records, an offset and 48 bytes per read);
  2. Index.chain_host against what a caller did before it existed: Index.mems_host + chain.chain_reference over the
     records, wall clock, with the records compared;
  3. `spumoni chain` against `spumoni mems` on the same reads file on tmpfs, process start to process gone.

    python tools/chain_bench.py [--text N] [--reps N] [--skip-cli] [--label TEXT]
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
from spumoni_amd.chain import CHAIN_DTYPE, chain_reference  # noqa: E402
from tools.mems_bench import copy_ms, med, repetitive_text  # noqa: E402

BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")


def reads_with_indels(text, lens, rng, f_sub, f_indel=0.0, one_indel=False):
    """Reads cut from the text at random places, on the device: a fraction f_sub of the letters replaced, and either one
    insertion or deletion of one letter per read (one_indel) or one at a fraction f_indel of the positions."""
    t = torch.from_numpy(text).cuda()
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    total, nreads = int(offs[-1]), lens.size
    g = torch.Generator(device="cuda").manual_seed(int(rng.integers(1 << 30)))
    start = torch.from_numpy(rng.integers(0, max(1, text.size - 2 * int(lens.max())), nreads)).cuda()
    d_offs = torch.from_numpy(offs).cuda()
    d_lens = torch.from_numpy(np.asarray(lens, dtype=np.int64)).cuda()
    read_of = torch.repeat_interleave(torch.arange(nreads, device="cuda"), d_lens)
    j = torch.arange(total, device="cuda") - d_offs[read_of]
    shift = torch.zeros(total, dtype=torch.int64, device="cuda")  # +1: a text letter is skipped here, -1: a letter is put in
    if one_indel:
        at = d_offs[:-1] + (torch.rand(nreads, device="cuda", generator=g) * (d_lens - 2).clamp(min=1)).long() + 1
        shift[at] = torch.randint(0, 2, (nreads,), device="cuda", generator=g) * 2 - 1
    elif f_indel:
        u = torch.rand(total, device="cuda", generator=g)
        shift[u < f_indel / 2] = 1
        shift[(u >= f_indel / 2) & (u < f_indel)] = -1
        shift[d_offs[:-1]] = 0
    run = torch.cumsum(shift, 0)
    run = run - (run - shift)[d_offs[:-1]][read_of]  # (the sum inside the read)
    seqs = t[(start[read_of] + j + run).clamp(0, text.size - 1)]
    flip = (torch.rand(total, device="cuda", generator=g) < f_sub) | (shift < 0)
    seqs[flip] = t[torch.randint(0, text.size, (int(flip.sum().item()),), device="cuda", generator=g)]
    return seqs.contiguous(), d_offs


def kernel_against_feed(ix, name, seqs, offs, bits, min_length, reps):
    total, nreads = seqs.numel(), offs.numel() - 1
    dt = torch.int16 if bits == 16 else torch.int32
    d_seqs = capi.pad_seqs(seqs)
    d_len = torch.empty(total + 16, dtype=dt, device="cuda")
    d_ptr = torch.empty(total + 16, dtype=torch.int64, device="cuda")
    mo = torch.empty(nreads + 1, dtype=torch.int64, device="cuda")
    ix.query_device(capi.SPX_MODE_MS, d_seqs, offs, total, d_lengths=d_len, d_pointers=d_ptr)
    ix.mems_device(d_len, d_ptr, offs, min_length, d_match_offsets=mo)  # (sizes the records)
    n = int(mo[-1].item())
    rec = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    out = torch.empty((nreads, 12), dtype=torch.int32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    walk, mems, chain = [], [], []
    for _ in range(reps + 1):
        e0.record()
        ix.query_device(capi.SPX_MODE_MS, d_seqs, offs, total, d_lengths=d_len, d_pointers=d_ptr)
        e1.record()
        ix.mems_device(d_len, d_ptr, offs, min_length, capacity=n, d_match_offsets=mo, d_out=rec)
        ix.chain_device(rec, mo, d_out=out)
        torch.cuda.synchronize()
        walk.append(e0.elapsed_time(e1))
        mems.append(ix.mems_stats()["kernel_ms"])
        st = ix.chain_stats()
        chain.append(st["kernel_ms"])
    w, m, v = med(walk[1:]), med(mems[1:]), med(chain[1:])
    nbytes = n * 16 + (nreads + 1) * 8 + nreads * 48
    c = copy_ms(nbytes, reps)
    r = out.cpu().numpy().view(CHAIN_DTYPE).reshape(-1)
    per = np.diff(mo.cpu().numpy())
    ok = r["anchors"] > 0
    cover = (r["read_end"][ok].astype(np.int64) - r["read_start"][ok]).sum() / max(total, 1)
    print(f"{name}: {nreads} reads, {total} values, {bits}-bit, min_length {min_length}, default parameters: {n} anchors "
          f"({n / max(nreads, 1):.1f} per read, at most {int(per.max(initial=0))}; {int((per > 16).sum())} reads on the wavefront path), "
          f"{st['candidates']} eligible pairs, {st['chained_reads']} reads chained with {st['chain_anchors'] / max(st['chained_reads'], 1):.1f} "
          f"anchors per chain, chains span {100 * cover:.1f} % of the values\n"
          f"    MS walk + k_ms_extend   {w:9.3f} ms   (min {min(walk[1:]):.3f}, max {max(walk[1:]):.3f})\n"
          f"    match kernels           {m:9.3f} ms   (min {min(mems[1:]):.3f}, max {max(mems[1:]):.3f})\n"
          f"    k_chain                 {v:9.3f} ms   (min {min(chain[1:]):.3f}, max {max(chain[1:]):.3f})   = {100 * v / (w + m):.1f} % of what feeds it, "
          f"{100 * v / w:.1f} % of walk + extension\n"
          f"    chains: {nbytes / 1e9:.3f} GB in {v:.3f} ms = {nbytes / v / 1e6:.0f} GB/s; a device copy of as many bytes: {c:.3f} ms = "
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
    print(f"chain_bench: {a.label}\nhost {socket.gethostname()}, {torch.cuda.get_device_name(0)}, library {capi.version()}\n"
          f"index: capi.build_raw over {a.text} DNA letters (mutated copies of one sequence of {a.text // 8}): n = {ix.n}, r = {ix.r}, "
          f"built in {time.perf_counter() - t0:.1f} s\n", flush=True)

    print("== 1. the chain kernel against the MS walk + extension and the match kernels that feed it (HIP events, median of %d) ==" % a.reps,
          flush=True)
    seqs, offs = reads_with_indels(text, np.full(1_000_000, 150), rng, 0.01)
    kernel_against_feed(ix, "150 bp, 1 % substitutions", seqs, offs, 16, 20, a.reps)
    del seqs, offs
    seqs, offs = reads_with_indels(text, np.full(1_000_000, 150), rng, 0.05, one_indel=True)
    kernel_against_feed(ix, "150 bp, 5 % substitutions and one indel per read", seqs, offs, 16, 20, a.reps)
    del seqs, offs
    seqs, offs = reads_with_indels(text, np.full(2000, 10_000), rng, 0.08, f_indel=0.02)
    kernel_against_feed(ix, "10 kbp, 10 % errors (8 % substitutions, 2 % indels)", seqs, offs, 16, 12, a.reps)
    del seqs, offs
    torch.cuda.empty_cache()

    print("\n== 2. host form: chain_host against mems_host + chain_reference (wall clock) ==", flush=True)
    nreads = 200_000  # 30 M characters: one piece
    d_seqs, d_offs = reads_with_indels(text, np.full(nreads, 150), rng, 0.05, one_indel=True)
    seqs, offs = d_seqs.cpu().numpy(), d_offs.cpu().numpy().astype(np.uint64)
    del d_seqs, d_offs
    new = []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        got, _ = ix.chain_host(seqs, offs, 20)
        new.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    mo, rec, _ = ix.mems_host(seqs, offs, 20)
    t1 = time.perf_counter()
    want, _, _ = chain_reference(mo, rec)
    t2 = time.perf_counter()
    same = bool(np.array_equal(got, want))
    print(f"{nreads} x 150 bp, 5 % substitutions and one indel per read, no digestion, min_length 20; records equal: {same}\n"
          f"    chain_host                              {med(new[1:]):8.3f} s   (min {min(new[1:]):.3f}, max {max(new[1:]):.3f})\n"
          f"    mems_host (records back)                {t1 - t0:8.3f} s\n"
          f"    + chain_reference on the host           {t2 - t1:8.3f} s   together {t2 - t0:.3f} s = {(t2 - t0) / med(new[1:]):.1f} x chain_host",
          flush=True)
    assert same

    if a.skip_cli:
        return
    print("\n== 3. CLI, process start to process gone, reads file and outputs on tmpfs ==", flush=True)
    work = tempfile.mkdtemp(prefix="chain_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
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
                          ("chain", [BIN, "chain", "-r", prefix[:-3], "-p", reads, "-n", "-L", "20"])):
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
              f"    spumoni chain -n -L 20   {med(res['chain']):7.3f} s  (runs: {', '.join('%.3f' % t for t in res['chain'])}); writes "
              f"{os.path.getsize(reads + '.chains') / 1e6:.1f} MB", flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
