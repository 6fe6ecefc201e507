"""`spumoni build` end to end against `python -m spumoni_amd.build_index` on the same FASTA input, with the SPX_TIMING
phases of the device text preparation ([spr]) and index builder ([spb]):
  hap-n / hap-m  the 10-haplotype x 20 Mbp input of the real-BWT legs (one file per haplotype, 80 columns), -n and -m;
  genome         a synthetic genome of --genome-bp bp in 24 sequences with runs of N as an assembly has them, -m
                 (build_index only with --python-genome: it takes minutes to prepare this input).

    python tools/build_cli_bench.py [--legs hap-n,hap-m,genome] [--genome-bp 3e9] [--python-genome] [--work DIR]
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spumoni_amd import synth  # noqa: E402

BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")


def write_fasta(path, seqs, width=80):
    with open(path, "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b">seq%d\n" % i)
            b = s.tobytes()
            body = b"\n".join(b[j: j + width] for j in range(0, len(b), width))
            f.write(body + b"\n")


def haplotype_files(d):
    base = synth.random_genome(20_000_000, seed=1)
    files = []
    for i, g in enumerate([base] + [synth.mutate(base, seed=sd) for sd in range(2, 11)]):
        p = os.path.join(d, f"hap{i}.fa")
        write_fasta(p, [g])
        files.append(p)
    lst = os.path.join(d, "haps.txt")
    with open(lst, "w") as f:
        f.write("".join(p + "\n" for p in files))
    return lst


def genome_file(d, total_bp):
    """24 sequences, sizes like an assembly's chromosomes, with N runs (telomeres, a centromere gap, scattered gaps)"""
    rng = np.random.default_rng(3)
    sizes = np.linspace(2.0, 0.4, 24)
    sizes = (sizes / sizes.sum() * total_bp).astype(np.int64)
    p = os.path.join(d, "genome.fa")
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(p, "wb") as f:
        for c, n in enumerate(sizes):
            s = acgt[rng.integers(0, 4, int(n), dtype=np.uint8)]
            s[:10_000] = ord("N")
            s[-10_000:] = ord("N")
            mid = int(n) // 2
            s[mid: mid + min(3_000_000, int(n) // 20)] = ord("N")
            for _ in range(20):
                a = int(rng.integers(0, int(n) - 60_000))
                s[a: a + int(rng.integers(100, 50_000))] = ord("N")
            f.write(b">chr%d\n" % (c + 1))
            b = s.tobytes()
            for j in range(0, len(b), 1 << 24):  # 60-column lines, written in blocks
                blk = b[j: j + (1 << 24)]
                f.write(b"\n".join(blk[k: k + 60] for k in range(0, len(blk), 60)) + b"\n")
    return p


def run(cmd, env=None):
    t0 = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT)
    dt = time.time() - t0
    if r.returncode != 0:
        print(r.stderr[-3000:], file=sys.stderr)
        raise SystemExit(f"failed: {' '.join(cmd)}")
    return dt, r.stderr


def leg(name, src_args, py_args, cli_flags, py_flags, work, python=True):
    env = dict(os.environ, SPX_TIMING="1")
    out_c, out_p = os.path.join(work, name, "cli"), os.path.join(work, name, "py")
    os.makedirs(out_c, exist_ok=True)
    os.makedirs(out_p, exist_ok=True)
    dt, err = run([BIN, "build"] + src_args + ["-o", os.path.join(out_c, "x"), "-P", "-M"] + cli_flags, env)
    print(f"{name}: spumoni build {' '.join(cli_flags)}: {dt:.2f} s end to end")
    for ln in err.splitlines():
        ln = re.sub(r"\x1b\[[0-9;]*m", "", ln)
        if ln.startswith("[spr]") or ln.startswith("[spb]") or "done." in ln:
            print("    " + ln)
    if python:
        dtp, _ = run([sys.executable, "-m", "spumoni_amd.build_index"] + py_args + ["-o", os.path.join(out_p, "x")]
                     + py_flags, env)
        ext = ".bin" if "-m" in cli_flags else ".fa"
        same = all(open(os.path.join(out_c, "x" + ext + e), "rb").read() == open(os.path.join(out_p, "x" + ext + e), "rb").read()
                   for e in ("", ".bwt.heads", ".bwt.len", ".thr_pos", ".ssa", ".esa", ".rawtext", ".fdi",
                             ".pmlnulldb", ".msnulldb"))
        print(f"{name}: python -m spumoni_amd.build_index {' '.join(py_flags)}: {dtp:.2f} s end to end "
              f"({dtp / dt:.1f}x); files identical: {same}")
    shutil.rmtree(os.path.join(work, name), ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="hap-n,hap-m,genome")
    ap.add_argument("--genome-bp", type=float, default=3e9)
    ap.add_argument("--python-genome", action="store_true")
    ap.add_argument("--work", default=None)
    a = ap.parse_args()
    legs = a.legs.split(",")
    work = a.work or tempfile.mkdtemp(prefix="build_cli_bench_")
    try:
        if "hap-n" in legs or "hap-m" in legs:
            lst = haplotype_files(work)
            if "hap-n" in legs:
                leg("hap-n", ["-i", lst], ["-l", lst], ["-n"], [], work)
            if "hap-m" in legs:
                leg("hap-m", ["-i", lst], ["-l", lst], ["-m"], ["-m"], work)
        if "genome" in legs:
            t0 = time.time()
            g = genome_file(work, int(a.genome_bp))
            print(f"genome: {os.path.getsize(g) / 1e9:.2f} GB FASTA written in {time.time() - t0:.1f} s")
            leg("genome", ["-r", g], ["-r", g], ["-m"], ["-m"], work, python=a.python_genome)
    finally:
        if not a.work:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
