#!/usr/bin/env python3
"""mix_penalty.py -- what the headline batch pays for holding reads of unequal cost in one launch.

The headline (bench.py `value`) walks 10^7 reads of which half are simulated-positive (~35 iterations of the walk's
loop each) and half random (~48), shuffled.  This tool times the SAME set of reads on the C3 index in four orders,
with HIP events, bench.py's settle and its time_steps protocol:

  (a) shuffled            one random permutation, as synth.simulate_reads leaves the headline's reads
  (b) unshuffled          all positive reads first, then all random ones: every lane of a strided deal gets the same
                          number of each, and a wavefront's lanes are of one class at any moment
  (c) groups of 64        whole groups of 64 consecutive reads of one class, the groups shuffled: wavefronts are pure
                          at any moment, but a wavefront's (and a lane's) total differs from its neighbours'
  (d) alternating         read i is positive iff i + i // nlanes is even (nlanes: the launch's lanes, --nlanes): under a
                          strided deal neighbouring lanes always differ in class (every wavefront is mixed) while every
                          lane alternates classes from round to round (equal totals)

(b) against (a) is the whole penalty; (c) and (d) split it into "unequal totals" (the tail of the launch) and "mixed
phases inside a wavefront" (divergence).  The additive figure -- half of an all-positive batch plus half of an
all-random one, timed in the same process -- is what the mix would cost if its parts did not disturb each other.

Prints a table and one JSON line; --out FILE also writes both there.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=1_000_000_000)
    ap.add_argument("--stand-in", action="store_true", help="r = 2^28 (quick runs)")
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=44)
    ap.add_argument("--nlanes", type=int, default=262144, help="lanes of the launch (order d)")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--settle", type=float, default=1.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.stand_in:
        a.runs = 1 << 28

    import torch

    import bench
    from spumoni_amd import capi, synth

    assert torch.cuda.is_available(), "mix_penalty.py needs an MI355X"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    sigma, L, n = 253, a.read_len, a.reads
    raw = synth.statistical_rlbwt(a.runs, sigma, 8.0, seed=3, device=dev, zipf=1.0)
    warm = 1
    while sigma ** warm < a.runs:
        warm += 1
    # the two classes, n reads each (bench.py's positive_100 / positive_0 legs), and the headline's own reads
    pos, _ = synth.simulate_reads(raw, n, L, seed=31, positive_fraction=1.0, f_mis=0.02, warmup=warm)
    rnd, _ = synth.simulate_reads(raw, n, L, seed=31, positive_fraction=0.0, f_mis=0.02, warmup=warm)
    head, offs = synth.simulate_reads(raw, n, L, seed=13, positive_fraction=0.5, f_mis=0.02, warmup=warm)
    pos, rnd = pos.view(n, L), rnd.view(n, L)
    torch.cuda.empty_cache()
    ix = capi.Index.from_raw(raw, 0)
    del raw
    torch.cuda.empty_cache()

    g = torch.Generator(device=dev)
    g.manual_seed(77)
    half = n // 2
    base_cls = torch.arange(n, device=dev) < half  # True: positive

    def batch_of(is_pos):
        """reads in the given class order: the k-th positive slot takes pos[k], the k-th random slot rnd[k]"""
        is_pos = is_pos.to(torch.bool)
        out = torch.empty((n, L), dtype=torch.uint8, device=dev)
        out[is_pos] = pos[: int(is_pos.sum())]
        out[~is_pos] = rnd[: int((~is_pos).sum())]
        return out.view(-1)

    i = torch.arange(n, device=dev)
    grp = torch.randperm((n + 63) // 64, generator=g, device=dev)
    orders = {
        "a_shuffled": base_cls[torch.randperm(n, generator=g, device=dev)],
        "b_unshuffled": base_cls,
        "c_groups_of_64": (grp[i // 64] < (half + 63) // 64),
        "d_alternating": ((i + i // a.nlanes) % 2 == 0),
    }
    batches = {"headline": head, "positive_100": pos.reshape(-1), "positive_0": rnd.reshape(-1)}
    npos = {"headline": None, "positive_100": n, "positive_0": 0}
    for name, cls in orders.items():
        batches[name] = batch_of(cls)
        npos[name] = int(cls.sum())

    total = n * L
    d_len = torch.empty(total + 8, dtype=torch.int16, device=dev)
    d_cls = torch.empty((n, 2), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    time.sleep(a.settle)
    res = {}
    for name, seqs in batches.items():
        d_seqs = capi.pad_seqs(seqs)
        ms = bench.time_steps(torch, lambda: ix.query_device(capi.SPX_MODE_PML, d_seqs, offs, total, d_lengths=d_len,
                                                             d_class=d_cls, bin_width=150, max_value_thr=5),
                              a.steps, a.warmup)
        st = ix.last_stats()
        res[name] = {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                     "positive_reads": npos[name], "row_loads_per_step": round(st["row_loads"] / max(1, st["steps"]), 3),
                     "dir_loads_per_step": round(st["dir_loads"] / max(1, st["steps"]), 3)}
        del d_seqs
    ix.close()
    add = 0.5 * (res["positive_100"]["ms_median"] + res["positive_0"]["ms_median"])
    lines = [f"mix_penalty: r={a.runs} reads={n} x {L}, nlanes={a.nlanes}, {a.steps} steps after {a.warmup} warm-up; ms per launch (HIP events)",
             f"{'order':<16} {'median':>8} {'min':>8} {'max':>8}  positive  rows/step dir/step"]
    for name, v in res.items():
        lines.append(f"{name:<16} {v['ms_median']:8.3f} {v['ms_min']:8.3f} {v['ms_max']:8.3f}  {str(v['positive_reads']):>8}  "
                     f"{v['row_loads_per_step']:.3f}     {v['dir_loads_per_step']:.3f}")
    lines.append(f"additive 0.5 * (positive_100 + positive_0) = {add:.3f} ms")
    aa, bb = res["a_shuffled"]["ms_median"], res["b_unshuffled"]["ms_median"]
    lines.append(f"whole penalty (a - b) = {aa - bb:+.3f} ms ({100 * (aa - bb) / bb:+.1f} %); "
                 f"unequal totals alone (c - b) = {res['c_groups_of_64']['ms_median'] - bb:+.3f} ms; "
                 f"mixed wavefronts alone (d - b) = {res['d_alternating']['ms_median'] - bb:+.3f} ms")
    text = "\n".join(lines) + "\n" + json.dumps({"additive_ms": round(add, 3), **res}) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
