"""The coverage's rule (spumoni_amd/cover.py) against an independent per-column restatement, its hand cases, its checks,
the runs and the summary; the header as C99 and the exports; `spumoni cover`'s usage and refusals.  No GPU."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from spumoni_amd import capi
from spumoni_amd.cigar import OP_D, OP_EQ, OP_I, OP_N, OP_X
from spumoni_amd.cover import (RUN_DTYPE, SEQ_COVER_DTYPE, cover_reference, depth_of, runs_reference, seq_starts,
                               summary_reference)
from spumoni_amd.extend import OP_S
from spumoni_amd.map import MAPPING_DTYPE, UNMAPPED
from tests.test_map_cpu import _golden_index, entries_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spumoni_amd", "bin", "spumoni")
HEADER = os.path.join(ROOT, "include", "spumoni_cover.h")
TEXT_OPS = (OP_EQ, OP_X, OP_D, OP_N)


@pytest.fixture(scope="module")
def built(built_all):
    return capi.lib()


def mapping(cigar, seq, start, strand=0):
    """(MAPPING_DTYPE record, entries) of a CIGAR given as text or as entries that stands at `start` of sequence `seq`."""
    entries = entries_of(cigar) if isinstance(cigar, str) else list(cigar)
    rec = np.zeros(1, dtype=MAPPING_DTYPE)[0]
    rec["seq"], rec["strand"], rec["target_start"] = seq, strand, start
    rec["target_end"] = start + sum(e >> 4 for e in entries if e & 15 in TEXT_OPS)
    return rec, entries


def mbatch(mappings):
    """(records, op_offsets, entries) of [(rec, entries) or None for an unmapped read]."""
    recs = np.zeros(len(mappings), dtype=MAPPING_DTYPE)
    ooffs, ents = [0], []
    for q, m in enumerate(mappings):
        if m is None:
            recs[q]["seq"] = UNMAPPED
        else:
            recs[q] = m[0]
            ents += m[1]
        ooffs.append(len(ents))
    return recs, np.array(ooffs, dtype=np.uint64), np.array(ents, dtype=np.uint32)


def restated(entries):
    """One list of (text position from the read's start, op) per column, and from it by counting: (depth, mism) over the
    read's span and the indel columns."""
    cols, t = [], 0
    for e in entries:
        for _ in range(e >> 4):
            if e & 15 != OP_S:
                cols.append((t, e & 15))
                t += e & 15 in TEXT_OPS
    depth, mism = [0] * t, [0] * t
    for at, op in cols:
        if op in (OP_EQ, OP_X):
            depth[at] += 1
        if op == OP_X:
            mism[at] += 1
    return depth, mism, sum(op in (OP_I, OP_D) for _, op in cols)


def pack(cols):
    return [len(list(g)) << 4 | op for op, g in itertools.groupby(cols)]


def _cigars():
    """Every CIGAR of up to 6 columns over = X I D N, run-length packed, each with one of the four clip shapes in turn."""
    out = []
    for k in range(1, 7):
        for i, cols in enumerate(itertools.product((OP_EQ, OP_X, OP_I, OP_D, OP_N), repeat=k)):
            lead, tail = ([], [2 << 4 | OP_S], [], [1 << 4 | OP_S])[i % 4], ([], [], [3 << 4 | OP_S], [1 << 4 | OP_S])[i % 4]
            ents = lead + pack(cols) + tail
            out.append((ents, restated(ents)))
    return out


def test_rule_against_the_restatement_over_every_cigar_up_to_6_columns():
    """Every CIGAR, at every place of every table of 1-3 sequences of lengths 1-4.  What a read adds relative to its
    sequence's start does not depend on the table: each (length, place, CIGAR) is held to the restatement read by read on
    the table of that one sequence, and every table takes all its reads in one batch against the sum of the restatements."""
    cigars = _cigars()
    assert len(cigars) == sum(5 ** k for k in range(1, 7))
    by_len = {t: [c for c in cigars if len(c[1][0]) == t] for t in range(7)}
    assert [len(by_len[t]) for t in range(7)] == [6, 84, 560, 2240, 5376, 7168, 4096]
    reads = 0
    for L in range(1, 5):
        for t in range(0, L + 1):
            for a in range(0, L - t + 1):
                for ents, (depth, mism, indels) in by_len[t]:
                    count = {}
                    d, m, c = cover_reference(*mbatch([mapping(ents, 0, a)]), [L], count=count)
                    want = np.zeros(L, dtype=np.uint32)
                    want[a:a + t] = depth
                    assert np.array_equal(depth_of(d), want), (L, a, ents)
                    want[a:a + t] = mism
                    assert np.array_equal(m, want) and c.tolist() == [[1, indels]] and count["added"] == 1 and count["error"] == 0
                    assert int(d.astype(np.uint64).sum()) % 2**32 == 0
                    reads += 1
        # a read that does not fit the sequence is skipped
        for ents, (depth, _, _) in by_len[L + 1][:50]:
            count = {}
            d, m, c = cover_reference(*mbatch([mapping(ents, 0, 0)]), [L], count=count)
            assert not d.any() and not m.any() and not c.any() and count == dict(reads=1, mapped=1, added=0, skipped=1, intervals=0,
                                                                              atomics=0, error=1)
    assert reads > 15_000
    tables = [T for n in (1, 2, 3) for T in itertools.product(range(1, 5), repeat=n)]
    assert len(tables) == 84
    ent = {t: (np.concatenate([np.array(c[0], dtype=np.uint32) for c in by_len[t]]), np.array([len(c[0]) for c in by_len[t]]),
               np.sum([c[1][0] for c in by_len[t]], axis=0, dtype=np.int64), np.sum([c[1][1] for c in by_len[t]], axis=0, dtype=np.int64),
               sum(c[1][2] for c in by_len[t])) for t in range(5)}
    total = 0
    for T in tables:
        F = seq_starts(T)
        w_depth, w_mism, w_counts = np.zeros(F[-1], dtype=np.int64), np.zeros(F[-1], dtype=np.int64), np.zeros((len(T), 2), dtype=np.int64)
        recs, ents, sizes = [], [], []
        for s, L in enumerate(T):
            for t in range(0, L + 1):
                for a in range(0, L - t + 1):
                    part = np.zeros(len(by_len[t]), dtype=MAPPING_DTYPE)
                    part["seq"], part["target_start"], part["target_end"] = s, a, a + t
                    recs.append(part)
                    ents.append(ent[t][0])
                    sizes.append(ent[t][1])
                    w_counts[s] += (len(by_len[t]), ent[t][4])
                    w_depth[F[s] + a:F[s] + a + t] += ent[t][2] if t else 0
                    w_mism[F[s] + a:F[s] + a + t] += ent[t][3] if t else 0
        recs = np.concatenate(recs)
        count = {}
        d, m, c = cover_reference(recs, np.r_[0, np.cumsum(np.concatenate(sizes))].astype(np.uint64), np.concatenate(ents), T, count=count)
        assert np.array_equal(depth_of(d), w_depth) and np.array_equal(m, w_mism) and np.array_equal(c, w_counts), T
        assert count["added"] == recs.size and count["error"] == 0
        total += recs.size
    assert total == 933_660


def _one(cigar, seq, start, lengths, **kw):
    count = {}
    d, m, c = cover_reference(*mbatch([mapping(cigar, seq, start, **kw)]), lengths, count=count)
    return depth_of(d).tolist(), m.tolist(), c.tolist(), count, d.tolist()


def test_the_hand_cases():
    # an interval that ends exactly at a sequence's end, and at G
    depth, mism, counts, count, diff = _one("3=", 0, 2, [5, 4])
    assert depth == [0, 0, 1, 1, 1, 0, 0, 0, 0] and diff == [0, 0, 1, 0, 0, 0xFFFFFFFF, 0, 0, 0, 0] and counts == [[1, 0], [0, 0]]
    depth, mism, counts, count, diff = _one("2S3=1S", 1, 1, [5, 4])
    assert depth == [0, 0, 0, 0, 0, 0, 1, 1, 1] and diff[-1] == 0xFFFFFFFF and diff[6] == 1 and counts == [[0, 0], [1, 0]]
    # 'D' / 'N' at both ends of an interval: not covered, and the interval between them is one
    depth, mism, counts, count, _ = _one("1D2=1X2N1=1I1=1D", 0, 1, [12])
    assert depth == [0, 0, 1, 1, 1, 0, 0, 1, 1, 0, 0, 0] and mism == [0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0] and counts == [[1, 3]]
    assert (count["intervals"], count["atomics"]) == (2, 5)
    # an all-'X' read
    depth, mism, counts, count, _ = _one("4X", 0, 0, [4])
    assert depth == [1, 1, 1, 1] and mism == [1, 1, 1, 1] and (count["intervals"], count["atomics"]) == (1, 6)
    # two reads on one base; a read on the last sequence's last base; the strand does not enter
    d, m, c = cover_reference(*mbatch([mapping("1=", 2, 2), mapping("1X", 2, 2, strand=1), None, mapping("1=", 0, 0)]), [1, 2, 3])
    assert depth_of(d).tolist() == [1, 0, 0, 0, 0, 2] and m.tolist() == [0, 0, 0, 0, 0, 1] and c.tolist() == [[1, 0], [0, 0], [2, 0]]
    a = cover_reference(*mbatch([mapping("2=1X", 1, 0, strand=0)]), [1, 3])
    b = cover_reference(*mbatch([mapping("2=1X", 1, 0, strand=1)]), [1, 3])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # an unmapped read and an empty batch add nothing
    count = {}
    d, m, c = cover_reference(*mbatch([None, None]), [3], count=count)
    assert not d.any() and not m.any() and not c.any() and count["reads"] == 2 and count["mapped"] == 0 and count["error"] == 0
    d, m, c = cover_reference(*mbatch([]), [3])
    assert d.shape == (4,) and m.shape == (3,) and c.shape == (1, 2)
    # a mapped read without entries covers nothing and counts as a read
    d, m, c = cover_reference(*mbatch([mapping("", 0, 2)]), [3])
    assert not d.any() and c.tolist() == [[1, 0]]


def test_adds_accumulate_in_any_order():
    rng = np.random.default_rng(1)
    lengths = [7, 1, 12]
    maps = []
    for _ in range(60):
        s = int(rng.integers(0, 3))
        t = int(rng.integers(1, lengths[s] + 1))
        maps.append(mapping(pack([int(v) for v in rng.choice([OP_EQ, OP_X, OP_D], t)]), s, int(rng.integers(0, lengths[s] - t + 1))))
    whole = cover_reference(*mbatch(maps), lengths)
    first = cover_reference(*mbatch(maps[:25]), lengths)
    kept = [a.copy() for a in first]
    both = cover_reference(*mbatch(maps[25:]), lengths, into=first)
    assert all(np.array_equal(a, b) for a, b in zip(first, kept))  # `into` is left as it is
    other = cover_reference(*mbatch(maps[:25]), lengths, into=cover_reference(*mbatch(maps[25:][::-1]), lengths))
    for a, b, c in zip(whole, both, other):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes() == c.tobytes()
    assert whole[0].dtype == np.uint32 and whole[1].dtype == np.uint32 and whole[2].dtype == np.uint64


def spoiled(kind):
    """(a batch of three good reads and a bad one behind them, the same batch with the bad one unmapped, in_entries)."""
    good = [mapping("3=1X", 0, 1), mapping("2=2D1=", 1, 0), mapping("1X", 1, 4)]
    rec, ents = mapping("2=1I2=", 1, 0)
    if kind == "seq_beyond_the_table":
        rec["seq"] = 2
    elif kind == "end_beyond_the_sequence":
        rec["target_start"], rec["target_end"] = 2, 6
    elif kind == "start_behind_end":
        rec["target_start"], rec["target_end"] = 3, 2
    elif kind == "unknown_operation":
        ents[1] = 1 << 4 | 5
    elif kind == "clip_between_entries":
        ents = entries_of("2=1S2=")
    elif kind == "sum_too_short":
        rec["target_end"] = 5
    elif kind == "sum_too_long":
        rec["target_end"] = 3
    elif kind not in ("offsets_decrease", "offsets_beyond_in_entries"):
        raise ValueError(kind)
    args = list(mbatch(good + [(rec, ents)]))
    clean = list(mbatch(good + [None]))
    in_entries = args[2].size
    if kind == "offsets_decrease":
        args[1][4] = args[1][3] - 1
    if kind == "offsets_beyond_in_entries":
        in_entries -= 1
    return args, clean, in_entries


BAD = ["seq_beyond_the_table", "end_beyond_the_sequence", "start_behind_end", "unknown_operation", "clip_between_entries",
       "sum_too_short", "sum_too_long", "offsets_decrease", "offsets_beyond_in_entries"]
BAD_LENGTHS = [6, 5]


@pytest.mark.parametrize("kind", BAD)
def test_each_check_failing_alone_skips_the_read_and_changes_nothing(kind):
    args, clean, in_entries = spoiled(kind)
    count, count_clean = {}, {}
    got = cover_reference(*args, BAD_LENGTHS, count=count, in_entries=in_entries)
    want = cover_reference(*clean, BAD_LENGTHS, count=count_clean)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), kind
    assert (count["error"], count["skipped"], count["added"], count["mapped"]) == (1, 1, 3, 4)
    assert (count_clean["error"], count_clean["skipped"], count_clean["added"], count_clean["mapped"]) == (0, 0, 3, 3)
    # the good version of the same read does add: the check is what skipped it
    fine = cover_reference(*mbatch([mapping("3=1X", 0, 1), mapping("2=2D1=", 1, 0), mapping("1X", 1, 4), mapping("2=1I2=", 1, 0)]), BAD_LENGTHS)
    assert fine[0].tobytes() != want[0].tobytes() and fine[2].tolist() == [[1, 0], [3, 3]]


def test_runs_partition_staircase_and_borders():
    lengths = [4, 3, 5]
    depth = np.array([0, 2, 2, 0, 1, 1, 1, 1, 1, 3, 0, 0], dtype=np.uint32)
    mism = np.array([0, 1, 2, 0, 0, 1, 0, 1, 0, 3, 0, 0], dtype=np.uint32)
    runs = runs_reference(depth, mism, lengths, 0)
    assert runs.dtype == RUN_DTYPE
    assert [tuple(r)[:5] for r in runs.tolist()] == [(0, 1, 0, 0, 0), (1, 3, 0, 2, 3), (3, 4, 0, 0, 0), (0, 3, 1, 1, 1), (0, 2, 2, 1, 1),
                                                      (2, 3, 2, 3, 3), (3, 5, 2, 0, 0)]
    # no run across the border between sequences 1 and 2 although the depth is 1 on both sides
    assert [tuple(r)[:4] for r in runs_reference(depth, mism, lengths, 1).tolist()] == [(1, 3, 0, 2), (0, 3, 1, 1), (0, 2, 2, 1), (2, 3, 2, 3)]
    assert [tuple(r)[:4] for r in runs_reference(depth, mism, lengths, 2).tolist()] == [(1, 3, 0, 2), (2, 3, 2, 3)]
    assert runs_reference(depth, mism, lengths, 4).size == 0
    # the partition at min_depth 0: every sequence from 0 to its length without a hole, and the sums are kept
    rng = np.random.default_rng(2)
    lengths = [int(v) for v in rng.integers(1, 40, 30)]
    G = sum(lengths)
    depth = rng.integers(0, 3, G).astype(np.uint32)
    mism = np.minimum(depth, rng.integers(0, 3, G)).astype(np.uint32)
    runs = runs_reference(depth, mism, lengths, 0)
    for s, L in enumerate(lengths):
        mine = runs[runs["seq"] == s]
        assert mine["start"][0] == 0 and mine["end"][-1] == L and np.array_equal(mine["start"][1:], mine["end"][:-1])
        assert (mine["start"] < mine["end"]).all()
    assert int(((runs["end"] - runs["start"]) * runs["depth"]).sum()) == int(depth.sum()) and int(runs["mismatches"].sum()) == int(mism.sum())
    assert np.array_equal(runs, np.sort(runs, order=["seq", "start"]))
    kept = runs_reference(depth, mism, lengths, 1)
    assert np.array_equal(kept, runs[runs["depth"] >= 1])
    # a staircase where every base differs: as many runs as bases
    stairs = np.arange(1, 21, dtype=np.uint32)
    runs = runs_reference(stairs, np.zeros(20, dtype=np.uint32), [20], 1)
    assert runs.size == 20 and (runs["end"] - runs["start"] == 1).all() and np.array_equal(runs["depth"], stairs)


def test_summary_equals_sums_over_the_arrays():
    rng = np.random.default_rng(3)
    lengths = [9, 1, 30, 4]
    F = seq_starts(lengths)
    maps = []
    for _ in range(80):
        s = int(rng.integers(0, 4))
        t = int(rng.integers(1, lengths[s] + 1))
        cols = [int(v) for v in rng.choice([OP_EQ, OP_EQ, OP_X, OP_D, OP_N, OP_I], t + 2)]
        t = sum(c in TEXT_OPS for c in cols)
        if t <= lengths[s]:
            maps.append(mapping(pack(cols), s, int(rng.integers(0, lengths[s] - t + 1))))
    diff, mism, counts = cover_reference(*mbatch(maps), lengths)
    out = summary_reference(diff, mism, counts, lengths)
    assert out.dtype == SEQ_COVER_DTYPE and out.size == 4
    depth = depth_of(diff)
    for s in range(4):
        d, m = depth[F[s]:F[s + 1]], mism[F[s]:F[s + 1]]
        assert out[s].tolist() == (int((d > 0).sum()), int(d.sum()), int(m.sum()), int(counts[s, 1]), int(counts[s, 0]), int(d.max()), 0)
    assert int(out["reads"].sum()) == len(maps) and (out["covered"] <= np.array(lengths)).all() and (mism <= depth).all()
    with pytest.raises(ValueError, match="length 0"):
        seq_starts([3, 0])


# ---- header and exports ------------------------------------------------------------------------------------------------
def _declared():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return code, sorted(set(re.findall(r"\b(spd_[a-z_0-9]+)\s*\(", code)))


def test_cover_header_is_plain_c(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include "spumoni_cover.h"\nint main(void) { spd_seq_cover c; spd_run r; spd_cover_stats s; (void)c; (void)r; (void)s; '
                   'return sizeof(spd_seq_cover) == 48 && sizeof(spd_run) == 32 && sizeof(spd_cover_stats) == 80 && '
                   'sizeof(spn_mapping) == 48 && SPN_UNMAPPED == 0xFFFFFFFFu ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "c"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "c")]).returncode == 0
    code, _ = _declared()
    assert "hipStream_t" not in code and "std::" not in code and "#include <hip" not in code and "spx_" not in code.replace("spx_index", "")
    assert re.findall(r'#include\s+[<"]([^>"]+)', code) == ["stdint.h", "spumoni_map.h"]


def test_cover_header_symbols_exported(built):
    _, names = _declared()
    assert names == sorted(capi.COVER_EXPORTS) and len(names) == 10
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(spd_[a-z_0-9]+)\b", out))) == names
    for other in (capi.EXPORTS, capi.DOCVOTE_EXPORTS, capi.MEMS_EXPORTS, capi.PLACE_EXPORTS, capi.CHAIN_EXPORTS, capi.ALIGN_EXPORTS,
                  capi.CIGAR_EXPORTS, capi.EXTEND_EXPORTS, capi.REFTEXT_EXPORTS, capi.MAP_EXPORTS):
        assert not set(capi.COVER_EXPORTS) & set(other)
    assert capi.C.sizeof(capi.SpdCoverStats) == 80 and SEQ_COVER_DTYPE.itemsize == 48 and RUN_DTYPE.itemsize == 32
    assert list(SEQ_COVER_DTYPE.names) == ["covered", "bases", "mismatches", "indels", "reads", "max_depth", "reserved"]
    assert list(RUN_DTYPE.names) == ["start", "end", "seq", "depth", "mismatches", "reserved"]
    assert [f[0] for f in capi.SpdCoverStats._fields_] == ["reads", "mapped", "added", "skipped", "intervals", "atomics", "runs", "error",
                                                           "overflow", "kernel_ms", "step_ms"]
    for method in ("cover_add_device", "cover_finish_device", "cover_runs_device", "cover_reset", "cover_add_host", "cover_summary",
                   "cover_runs", "cover_depth", "cover_stats"):
        assert callable(getattr(capi.Index, method))


def test_cover_calls_without_an_index_fail_loudly(built):
    L = capi._spd()
    n = capi.C.c_uint64(0)
    assert L.spd_cover_reset(None) == -1 and b"index must be non-null" in L.spx_last_error()
    assert L.spd_cover_add_batch(None, 0, 0, 0, None, None, 0, 1, 0, None, None, None, None) == -1
    assert b"index must be non-null" in L.spx_last_error()
    assert L.spd_cover_add_device(None, None, None, None, 0, 0, None, None, None, None) == -1
    assert L.spd_cover_finish_device(None, None, None, None, None, None, None) == -1
    assert L.spd_cover_runs_device(None, None, None, 0, 0, None, None, None) == -1
    assert L.spd_cover_summary(None, None, 0) == -1 and L.spd_cover_runs_begin(None, 1, capi.C.byref(n)) == -1
    assert L.spd_cover_runs_fetch(None, None) == -1 and L.spd_cover_depth(None, 0, 0, None, None) == -1
    assert L.spd_last_cover_stats(None, None) == -1


# ---- the command -----------------------------------------------------------------------------------------------------------
def _cover(args, cwd, env=None):
    return subprocess.run([BIN, "cover"] + args, cwd=cwd, capture_output=True, text=True, env=env, timeout=120)


def test_cover_usage_without_arguments(built, tmp_path):
    r = _cover([], str(tmp_path))
    assert r.returncode == 1
    assert "spumoni cover - " in r.stderr
    for opt in ("-h, --help", "-r, --ref", "-p, --pattern", "-n, --no-digest", "-m, --minimizer-alphabet", "-a, --dna-minimizer",
                "-d, --doc-array", "-b, --bedgraph", "-D, --min-depth", "-L -S -G -B -H", "-F -E -O -N -I"):
        assert opt in r.stderr, opt
    for word in ("<pattern>.cover", "<pattern>.bedgraph", "breadth", "mean depth", ".fa.seqs", "spumoni build -n -s", "not\ncovered"):
        assert word in r.stderr, word
    top = subprocess.run([BIN], capture_output=True, text=True)
    assert top.returncode == 1 and "\tcover\t" in top.stderr and "\tmap\t" in top.stderr
    assert _cover(["-h"], str(tmp_path)).returncode == 1


@pytest.mark.parametrize("args,table,message", [
    (["-p", "reads.fa", "-n"], None, "Both a reference file (-r) and pattern file (-p) must be provided."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-P"], None, "-P cannot be used with `spumoni cover`"),
    (["-r", "ref", "-p", "reads.fa", "-m"], None, "-m / -a cannot be used with `spumoni cover`"),
    (["-r", "ref", "-p", "reads.fa", "-a"], None, "-m / -a cannot be used with `spumoni cover`"),
    (["-r", "ref", "-p", "reads.fa", "-n", "-m"], None, "-m / -a cannot be used with `spumoni cover`"),
    (["-r", "ref", "-p", "reads.fa"], None, "`spumoni cover` needs -n"),
    (["-r", "nosuch", "-p", "reads.fa", "-n"], None, "The following path is not valid: nosuch.fa"),
    (["-r", "ref", "-p", "missing.fa", "-n"], None, "The following path is not valid: missing.fa"),
    (["-r", "ref", "-p", "reads.fa", "-n", "-L", "0"], None, "the minimum match length (-L) must be at least 1."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-E", "4097"], None, "the largest extended end (-E) must be between 1 and 4096."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-b", "-D", "-1"], None, "the smallest depth (-D) must be between 0 and 4294967295."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-D", "4294967296"], None, "the smallest depth (-D) must be between 0 and 4294967295."),
    (["-r", "ref", "-p", "reads.fa", "-n", "-b"], None, "the index has no sequence table (ref.fa.seqs): build it with -s"),
    (["-r", "ref", "-p", "reads.fa", "-n"], b"a\t5\t0\n", "ref.fa.seqs: line 1 is not name<TAB>length<TAB>text_start<TAB>strands"),
    (["-r", "ref", "-p", "reads.fa", "-n"], b"a\t5\t0\t2\nb\t4\t10\t1\n", "ref.fa.seqs: line 2: strands, length or text_start"),
    (["-r", "ref", "-p", "reads.fa", "-n"], b"\n", "ref.fa.seqs: no sequences"),
])
def test_cover_refusals_leave_no_file(built, tmp_path, args, table, message):
    _golden_index(tmp_path, table)
    before = sorted(os.listdir(tmp_path))
    r = _cover(args, str(tmp_path))
    assert r.returncode == 1
    assert message in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_cover_missing_entry_point_on_the_fake_device(built, fake_device, tmp_path):
    _golden_index(tmp_path)
    before = sorted(os.listdir(tmp_path))
    env = dict(os.environ, LD_LIBRARY_PATH=fake_device + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = _cover(["-r", "ref", "-p", "reads.fa", "-n", "-L", "4", "-b"], str(tmp_path), env=env)
    assert r.returncode == 1
    assert "has no spd_cover_add_batch" in r.stderr and "`spumoni cover`" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_a_failing_cover_run_writes_nothing(built, tmp_path):
    """Without a device the command stops at its entry points; with one, at a table that does not add up to the text, and
    then at a read that is empty: either way neither file."""
    _golden_index(tmp_path)
    before = sorted(os.listdir(tmp_path))
    if built.spx_device_count() > 0:
        n = os.path.getsize(tmp_path / "ref.fa.rawtext")
        (tmp_path / "ref.fa.seqs").write_bytes(b"whole\t%d\t0\t1\n" % (n - 1))
        r = _cover(["-r", "ref", "-p", "reads.fa", "-n", "-b"], str(tmp_path))
        assert r.returncode == 1 and f"ref.fa.seqs: the sequences add up to {n - 1} characters, the text has {n}" in r.stderr, r.stderr
        assert sorted(os.listdir(tmp_path)) == before
        (tmp_path / "ref.fa.seqs").write_bytes(b"whole\t%d\t0\t1\n" % n)
        # (a FASTA file of the test's own: the golden reads are FASTQ records under this name)
        text = (tmp_path / "ref.fa.rawtext").read_bytes()
        (tmp_path / "reads.fa").write_bytes(b">good\n" + text[:40] + b"\n>bad_one\n>after\n" + text[5:45] + b"\n")
    r = _cover(["-r", "ref", "-p", "reads.fa", "-n", "-d", "-b"], str(tmp_path))
    assert r.returncode == 1
    if built.spx_device_count() > 0:
        assert "bad_one was empty" in r.stderr, r.stderr
    else:
        assert "no usable gfx950 device" in r.stderr and "no CPU fallback" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before
