// spx_cover.hip -- the coverage (include/spumoni_cover.h): per-base depth and mismatch counts along every
// sequence's forward strand and a summary per sequence, accumulated over any number of batches of spx_map.hip's mappings,
// and the product's C-ABI.  The kernels read mappings, entries and the piece starts of the sequence table (sequence s
// begins at F[s] = P[s * strands] / strands of the forward genome and has P[s * strands + 1] - P[s * strands] bases).
//
//   add      k_cover_add_lane, a lane per read of up to `sw` entries (64): one pass checks the read, a second walks it.  A
//            stretch of '=' and 'X' between two 'D' / 'N' is one +1 and one -1 in diff, an 'X' column one add in mism.  A
//            read of more entries is put on a list, and k_cover_add_wave gives each of them a wavefront: 64 entries a
//            step, their text positions by a wave-wide prefix sum, and the interval borders by two ballots -- a '=' / 'X'
//            entry opens an interval when the last entry before it that is not 'I' or 'S' was a 'D' / 'N' (or none), a
//            'D' / 'N' closes one when that entry was a '=' / 'X'.  reads[s] and indels[s] are summed per block in a table
//            of 256 slots of LDS (slot s & 255; a sequence that finds its slot taken goes to memory at once) and leave the
//            block as one pair of atomics per sequence.
//   finish   hipcub's inclusive sum over diff gives depth.  k_cover_summary: a block per tile of 4096 positions, a thread
//            per 16 of them.  A thread finds its first sequence by a search in P and walks on across the borders; the part
//            of a sequence that lies in one thread goes to the summary at once, the part that spans threads is summed in
//            the LDS slot of its first thread: one set of atomics per (tile, sequence).
//   runs     count -> exclusive sum -> write over the same tiles, as in spx_mems.hip.  A position starts a run when it is
//            a sequence's first or its depth differs from its predecessor's; the thread that holds a run's start writes
//            start, seq and depth, the one that holds its last position writes end, and every thread the run passes
//            through adds its mism to the record (zero sums are not added: an uncovered stretch costs nothing).
//
// The sequence table, the tiles, the head of a mapping with its checks and the host code that works on the index's
// GenomeAcc are spx_genome_kernels.h's, shared by the coverage and the pileup.
//
// Control flow: every shuffle and ballot of k_cover_add_wave stands in a loop whose trip count is the same for the whole
// wavefront (the list's length, the read's entries in steps of 64) or behind them; the other kernels shuffle and
// synchronise only outside their loops.
#include <vector>

#include "../../include/spumoni_cover.h"
#include "spx_genome_kernels.h"

namespace spx {
namespace {

constexpr uint32_t EMPTY = 0xffffffffu;

struct AddCounters {  // device; zeroed in front of every launch
    unsigned long long reads, mapped, added, skipped, intervals, atomics;
    unsigned long long nlong;  // reads on the list of k_cover_add_wave
    unsigned long long error;  // bit 0: a read failed the checks
};
constexpr int ADD_WORDS = sizeof(AddCounters) / 8;
struct RunCounters {
    unsigned long long runs;
    unsigned long long error;  // bit 1: the runs did not fit run_capacity
};
constexpr int RUN_WORDS = sizeof(RunCounters) / 8;
struct FinCounters {
    unsigned long long tiles, error;
};
constexpr int FIN_WORDS = sizeof(FinCounters) / 8;

struct AddArgs {
    Table t;
    const uint4* map;       // 3 per read: spn_mapping
    const uint64_t* ioffs;  // nreads + 1
    const uint32_t* iops;
    uint64_t in_entries, nreads;
    uint32_t* diff;  // G + 1
    uint32_t* mism;  // G
    unsigned long long* counts;  // 2 per sequence: reads, indels
    uint64_t* longs;             // nreads: the reads of more than sw entries
    uint64_t sw;
    AddCounters* c;
};
struct FinArgs {
    Table t;
    const uint32_t* depth;
    const uint32_t* mism;
    const unsigned long long* counts;
    spd_seq_cover* out;
};
struct RunArgs {
    Table t;
    const uint32_t* depth;
    const uint32_t* mism;
    uint32_t min_depth;
    uint64_t cap, ntiles;
    spd_run* rec;
    uint64_t* tcnt;   // ntiles + 1: runs that start in a tile, then a 0
    uint64_t* toffs;  // ntiles + 1
    uint64_t* count;
    RunCounters* c;
};

// the two halves of in_text
__device__ inline bool covers(uint32_t op) { return op == OP_EQ || op == OP_X; }
__device__ inline bool skips(uint32_t op) { return op == OP_D || op == OP_N; }

// A block's sums of reads[s] and indels[s]
struct Tally {
    uint32_t key[256];
    unsigned long long reads[256], indels[256];
};
__device__ inline void tally_init(Tally& t) {
    t.key[threadIdx.x] = EMPTY;
    t.reads[threadIdx.x] = t.indels[threadIdx.x] = 0;
    __syncthreads();
}
__device__ inline void tally_add(Tally& t, unsigned long long* counts, uint32_t s, unsigned long long indels) {
    const uint32_t slot = s & 255u;
    const uint32_t old = atomicCAS(&t.key[slot], EMPTY, s);
    if (old == EMPTY || old == s) {
        atomicAdd(&t.reads[slot], 1ull);
        if (indels) atomicAdd(&t.indels[slot], indels);
    } else {
        atomicAdd(&counts[2 * (uint64_t)s], 1ull);
        if (indels) atomicAdd(&counts[2 * (uint64_t)s + 1], indels);
    }
}
__device__ inline void tally_flush(Tally& t, unsigned long long* counts) {
    __syncthreads();
    const uint32_t s = t.key[threadIdx.x];
    if (s == EMPTY) return;
    atomicAdd(&counts[2 * (uint64_t)s], t.reads[threadIdx.x]);
    if (t.indels[threadIdx.x]) atomicAdd(&counts[2 * (uint64_t)s + 1], t.indels[threadIdx.x]);
}

// A lane per read, a block over a stride of reads.
__global__ __launch_bounds__(256) void k_cover_add_lane(AddArgs a) {
    __shared__ Tally tally;
    __shared__ unsigned long long part[20];
    tally_init(tally);
    unsigned long long mapped = 0, added = 0, skipped = 0, intervals = 0, columns = 0;
    for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < a.nreads; q += (uint64_t)gridDim.x * 256) {
        MapHead h;
        const int st = map_head<false>(a, q, h);
        if (st == 0) continue;
        mapped += 1;
        if (st == 2) {
            skipped += 1;
            continue;
        }
        if (h.ne > a.sw) {  // (the wavefront's kernel counts it as added or skipped)
            a.longs[atomicAdd(&a.c->nlong, 1ull)] = q;
            continue;
        }
        const uint32_t* src = a.iops + h.i0;
        const uint32_t ne = (uint32_t)h.ne;
        // pass 1: the checks
        bool ok = true, seen = false, tail = false;
        uint64_t tsum = 0, indels = 0;
        for (uint32_t e = 0; e < ne && ok; ++e) {
            const uint32_t v = src[e], op = v & 15u;
            const uint64_t n = v >> 4;
            if (!is_op(op)) {
                ok = false;
            } else if (op == OP_S) {
                tail = seen;
            } else {
                ok = !tail;
                seen = true;
                if (covers(op) || skips(op)) tsum += n;
                if (op == OP_I || op == OP_D) indels += n;
            }
        }
        if (!ok || tsum != h.span) {
            skipped += 1;
            continue;
        }
        // pass 2: every position below stays under F[s] + target_end <= G
        uint64_t pos = h.pos;
        bool open = false;
        for (uint32_t e = 0; e < ne; ++e) {
            const uint32_t v = src[e], op = v & 15u;
            const uint64_t n = v >> 4;
            if (covers(op)) {
                if (!open) {
                    atomicAdd(a.diff + pos, 1u);
                    intervals += 1;
                    open = true;
                }
                if (op == OP_X) {
                    for (uint64_t k = 0; k < n; ++k) atomicAdd(a.mism + pos + k, 1u);
                    columns += n;
                }
                pos += n;
            } else if (skips(op)) {
                if (open) {
                    atomicAdd(a.diff + pos, 0xffffffffu);
                    open = false;
                }
                pos += n;
            }
        }
        if (open) atomicAdd(a.diff + pos, 0xffffffffu);
        added += 1;
        tally_add(tally, a.counts, h.s, indels);
    }
    tally_flush(tally, a.counts);
    if (skipped) atomicOr(&a.c->error, 1ull);
    unsigned long long v[5] = {mapped, added, skipped, intervals, columns + 2 * intervals};
    block_counts<5>(part, &a.c->mapped, v);
    if (blockIdx.x == 0 && threadIdx.x == 0) a.c->reads = a.nreads;
}

// A wavefront per read of the list, a grid over a stride of the list.
__global__ __launch_bounds__(256) void k_cover_add_wave(AddArgs a) {
    __shared__ Tally tally;
    __shared__ unsigned long long part[20];
    const uint64_t nlong = a.c->nlong;
    if ((uint64_t)blockIdx.x * 4 >= nlong) return;  // (the whole block: a batch of short reads has no list)
    tally_init(tally);
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1;
    unsigned long long added = 0, skipped = 0, intervals = 0, columns = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < nlong; i += (uint64_t)gridDim.x * 4) {
        MapHead h;
        if (map_head<false>(a, a.longs[i], h) != 1) continue;  // (the lane's kernel listed it because it is 1; the same for every lane)
        const uint32_t* src = a.iops + h.i0;
        // pass 1: each lane over its entries, the sums behind the loop.  No 'S' between two others: the entries that
        // are not 'S' are as many as lie between the first and the last of them
        bool bad = false;
        unsigned long long tsum = 0, indels = 0, others = 0, first = ~0ull, last = 0;
        for (uint64_t e = lane; e < h.ne; e += 64) {
            const uint32_t v = src[e], op = v & 15u;
            const unsigned long long n = v >> 4;
            if (!is_op(op)) {
                bad = true;
            } else if (op != OP_S) {
                others += 1;
                first = e < first ? e : first;
                last = e;
                if (covers(op) || skips(op)) tsum += n;
                if (op == OP_I || op == OP_D) indels += n;
            }
        }
        bad = __ballot(bad) != 0;
        tsum = wave_sum(tsum);
        indels = wave_sum(indels);
        others = wave_sum(others);
        first = wave_min(first);
        last = wave_max(last);
        if (bad || tsum != h.span || (others && last - first + 1 != others)) {
            skipped += lane == 0;
            continue;
        }
        // pass 2
        uint64_t carry = h.pos;
        bool open = false;  // the last entry so far that is not 'I' or 'S' was a '=' or an 'X'
        for (uint64_t base = 0; base < h.ne; base += 64) {
            const uint64_t e = base + lane;
            const uint32_t v = e < h.ne ? src[e] : OP_S, op = v & 15u;
            const unsigned long long n = v >> 4;
            const bool cov = covers(op), gap = skips(op);
            unsigned long long incl = cov || gap ? n : 0;
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned long long up = __shfl_up(incl, d);
                if ((int)lane >= d) incl += up;
            }
            const uint64_t pos = carry + incl - (cov || gap ? n : 0);
            const unsigned long long cov_mask = __ballot(cov), any_mask = cov_mask | __ballot(gap);
            const unsigned long long before = any_mask & below;
            const bool was = before ? (cov_mask >> (63 - __clzll((long long)before))) & 1 : open;
            if (cov && !was) {
                atomicAdd(a.diff + pos, 1u);
                intervals += 1;
            }
            if (gap && was) atomicAdd(a.diff + pos, 0xffffffffu);
            if (op == OP_X) {
                for (uint64_t k = 0; k < n; ++k) atomicAdd(a.mism + pos + k, 1u);
                columns += n;
            }
            carry += __shfl(incl, 63);
            if (any_mask) open = (cov_mask >> (63 - __clzll((long long)any_mask))) & 1;
        }
        if (lane == 0) {
            if (open) atomicAdd(a.diff + carry, 0xffffffffu);
            added += 1;
            tally_add(tally, a.counts, h.s, indels);
        }
    }
    tally_flush(tally, a.counts);
    if (skipped) atomicOr(&a.c->error, 1ull);
    unsigned long long v[4] = {added, skipped, intervals, columns + 2 * intervals};
    block_counts<4>(part, &a.c->added, v);
}

__global__ __launch_bounds__(256) void k_cover_summary_init(FinArgs a) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= a.t.n_seqs) return;
    spd_seq_cover o;
    o.covered = o.bases = o.mismatches = 0;
    o.indels = a.counts[2 * s + 1];
    o.reads = a.counts[2 * s];
    o.max_depth = o.reserved = 0;
    a.out[s] = o;
}

struct Part {
    uint32_t covered, max_depth;
    unsigned long long bases, mism;
};
__device__ inline void part_to_summary(spd_seq_cover* o, uint32_t covered, unsigned long long bases, unsigned long long mism,
                                       uint32_t max_depth) {
    if (covered) atomicAdd((unsigned long long*)&o->covered, (unsigned long long)covered);
    if (bases) atomicAdd((unsigned long long*)&o->bases, bases);
    if (mism) atomicAdd((unsigned long long*)&o->mismatches, mism);
    if (max_depth) atomicMax(&o->max_depth, max_depth);
}

__global__ __launch_bounds__(256) void k_cover_summary(FinArgs a) {
    __shared__ uint32_t l_seq[256], l_cov[256], l_max[256];
    __shared__ unsigned long long l_bases[256], l_mism[256];
    l_seq[threadIdx.x] = EMPTY;
    l_cov[threadIdx.x] = l_max[threadIdx.x] = 0;
    l_bases[threadIdx.x] = l_mism[threadIdx.x] = 0;
    __syncthreads();
    const Tile x = tile_of(a.t.G);
    const uint64_t t0 = x.t0, t1 = x.t1, p0 = x.p0, p1 = x.p1;
    if (p0 < t1) {
        uint64_t s = seq_of(a.t, p0), lo = seq_start(a.t, s), hi = seq_start(a.t, s + 1);
        Part acc{0, 0, 0, 0};
        // the part [from, to) of sequence s in this tile: in this thread alone, or summed in its first thread's slot
        auto flush = [&](uint64_t to) {
            const uint64_t from = lo > t0 ? lo : t0;
            const uint32_t first = (uint32_t)((from - t0) / PER_THREAD), last = (uint32_t)((to - 1 - t0) / PER_THREAD);
            if (first == last) {
                part_to_summary(a.out + s, acc.covered, acc.bases, acc.mism, acc.max_depth);
            } else {
                l_seq[first] = (uint32_t)s;
                if (acc.covered) atomicAdd(&l_cov[first], acc.covered);
                if (acc.bases) atomicAdd(&l_bases[first], acc.bases);
                if (acc.mism) atomicAdd(&l_mism[first], acc.mism);
                if (acc.max_depth) atomicMax(&l_max[first], acc.max_depth);
            }
            acc = Part{0, 0, 0, 0};
        };
        for (uint64_t p = p0; p < p1; ++p) {
            if (p == hi) {
                flush(hi);
                s += 1;
                lo = hi;
                hi = seq_start(a.t, s + 1);
            }
            const uint32_t d = a.depth[p];
            acc.covered += d != 0;
            acc.bases += d;
            acc.mism += a.mism[p];
            acc.max_depth = d > acc.max_depth ? d : acc.max_depth;
        }
        flush(hi < t1 ? hi : t1);
    }
    __syncthreads();
    if (l_seq[threadIdx.x] != EMPTY)
        part_to_summary(a.out + l_seq[threadIdx.x], l_cov[threadIdx.x], l_bases[threadIdx.x], l_mism[threadIdx.x], l_max[threadIdx.x]);
}

// the runs of depth >= min_depth that start in [p0, p1)
__device__ inline uint32_t count_starts(const RunArgs& a, uint64_t p0, uint64_t p1) {
    if (p0 >= p1) return 0;
    uint64_t s = seq_of(a.t, p0), lo = seq_start(a.t, s), hi = seq_start(a.t, s + 1);
    uint32_t prev = p0 ? a.depth[p0 - 1] : 0, n = 0;
    for (uint64_t p = p0; p < p1; ++p) {
        if (p == hi) {
            s += 1;
            lo = hi;
            hi = seq_start(a.t, s + 1);
        }
        const uint32_t d = a.depth[p];
        n += (p == lo || d != prev) && d >= a.min_depth;
        prev = d;
    }
    return n;
}

__global__ __launch_bounds__(256) void k_cover_runs_count(RunArgs a) {
    using Reduce = hipcub::BlockReduce<uint32_t, 256>;
    __shared__ typename Reduce::TempStorage tmp;
    const Tile x = tile_of(a.t.G);
    const uint32_t n = Reduce(tmp).Sum(count_starts(a, x.p0, x.p1));
    if (threadIdx.x == 0) {
        a.tcnt[blockIdx.x] = n;
        if (blockIdx.x == 0) a.tcnt[a.ntiles] = 0;
    }
}

// The count, the overflow, and the words of the records that several threads add to.
__global__ __launch_bounds__(256) void k_cover_runs_zero(RunArgs a) {
    const uint64_t total = a.toffs[a.ntiles], n = total < a.cap ? total : a.cap;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        a.rec[i].mismatches = 0;
        a.rec[i].reserved = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *a.count = total;
        a.c->runs = total;
        if (total > a.cap) atomicOr(&a.c->error, 2ull);
    }
}

__global__ __launch_bounds__(256) void k_cover_runs_write(RunArgs a) {
    using Scan = hipcub::BlockScan<uint32_t, 256>;
    __shared__ typename Scan::TempStorage tmp;
    const Tile x = tile_of(a.t.G);
    const uint64_t p0 = x.p0, p1 = x.p1;
    uint32_t before = 0;
    Scan(tmp).ExclusiveSum(count_starts(a, p0, p1), before);
    if (p0 >= p1) return;
    uint64_t next = a.toffs[blockIdx.x] + before;  // the record of the next run that starts here
    uint64_t s = seq_of(a.t, p0), lo = seq_start(a.t, s), hi = seq_start(a.t, s + 1);
    uint32_t prev = p0 ? a.depth[p0 - 1] : 0;
    // the run in force at p0, when p0 does not start one, has depth[p0] and began in this sequence: when it is kept its
    // record is the last one before `next`
    bool kept = false, ended = true;
    uint64_t cur = 0;
    uint32_t sum = 0;
    for (uint64_t p = p0; p < p1; ++p) {
        if (p == hi) {
            s += 1;
            lo = hi;
            hi = seq_start(a.t, s + 1);
        }
        const uint32_t d = a.depth[p];
        const bool start = p == lo || d != prev;
        if (start || p == p0) {
            kept = d >= a.min_depth;
            if (start) {
                if (kept) {
                    cur = next++;
                    if (cur < a.cap) {
                        a.rec[cur].start = p - lo;
                        a.rec[cur].seq = (uint32_t)s;
                        a.rec[cur].depth = d;
                    }
                }
            } else {
                cur = next - 1;  // (kept: a run of this depth started before p0, so next >= 1)
            }
            sum = 0;
        }
        sum += a.mism[p];
        ended = p + 1 == hi || a.depth[p + 1] != d;  // (p + 1 < hi <= G)
        if (ended && kept && cur < a.cap) {
            a.rec[cur].end = p + 1 - lo;
            if (sum) atomicAdd(&a.rec[cur].mismatches, sum);
        }
        prev = d;
    }
    if (!ended && kept && cur < a.cap && sum) atomicAdd(&a.rec[cur].mismatches, sum);
}

constexpr GenomeKind KIND = {"spd_cover_reset", "the coverage", "about 12 per base", "spd_cover_runs_begin", "spd_cover_runs_fetch", "out_runs",
                             {ADD_WORDS, FIN_WORDS, RUN_WORDS}, 6, sizeof(spd_run)};

int cover_add_enqueue(spx_index* ix, AddArgs& a, hipStream_t st) { return add_enqueue(ix, ix->cover, KIND, a, st, k_cover_add_lane, k_cover_add_wave); }

int cover_finish_enqueue(spx_index* ix, FinArgs& a, const uint32_t* d_diff, uint32_t* d_depth, hipStream_t st) {
    a.depth = d_depth;
    return finish_enqueue(ix, ix->cover, KIND, d_diff, d_depth, st, [&](const Table& t) -> int {
        a.t = t;
        k_cover_summary_init<<<(unsigned)((t.n_seqs + 255) / 256), 256, 0, st>>>(a);
        SPX_HIP(hipGetLastError());
        k_cover_summary<<<(unsigned)tiles_of(t.G), 256, 0, st>>>(a);
        SPX_HIP(hipGetLastError());
        return SPX_OK;
    });
}

int runs_enqueue(spx_index* ix, RunArgs& a, hipStream_t st, bool count, bool write) {
    return tiles_enqueue(
        ix, ix->cover, KIND, a, st, count, write, [&] { k_cover_runs_count<<<(unsigned)a.ntiles, 256, 0, st>>>(a); },
        [&]() -> int {
            k_cover_runs_zero<<<(unsigned)std::min<uint64_t>(a.cap / 256 + 1, 1024), 256, 0, st>>>(a);
            SPX_HIP(hipGetLastError());
            k_cover_runs_write<<<(unsigned)a.ntiles, 256, 0, st>>>(a);
            SPX_HIP(hipGetLastError());
            return SPX_OK;
        });
}

int add_error_code(const spx_index* ix) {
    if (ix->cover.step[GenomeAcc::ADD].error & 1) {
        set_error("a read's mapping failed the coverage's checks (a sequence outside the table, a span outside the sequence, entries "
                  "whose text lengths disagree with it, an unknown operation, an 'S' between two other entries, or offsets outside "
                  "the entries): such a read adds nothing");
        return SPX_E_FORMAT;
    }
    return SPX_OK;
}

template <typename T>
T* array_of(spx_index* ix, int slot) {
    return (T*)ix->cover.scr[slot].p;
}

}  // namespace

void release_cover(spx_index* ix) { release_acc(ix->cover); }
int clone_cover(spx_index* src, spx_index* ix) { return src->cover.G ? spd_cover_reset(ix) : SPX_OK; }
void cover_table_changed(spx_index* ix) { acc_table_changed(ix->cover); }
int cover_need_arrays(spx_index* ix, const char* who) { return need_arrays(ix, ix->cover, KIND, who); }

// depth and the summary from the handle's arrays, when something was added since they were made.  The caller holds host_mu.
int cover_finish_host(spx_index* ix) {
    return finish_host(ix, ix->cover, KIND, [&](hipStream_t st) {
        FinArgs a{};
        a.mism = array_of<const uint32_t>(ix, spx_index::D_MISM);
        a.counts = array_of<const unsigned long long>(ix, spx_index::D_COUNTS);
        a.out = array_of<spd_seq_cover>(ix, spx_index::D_OUT);
        return cover_finish_enqueue(ix, a, array_of<const uint32_t>(ix, spx_index::D_DIFF), array_of<uint32_t>(ix, spx_index::D_DEPTH), st);
    });
}

// What spd_cover_add_batch does behind its first check, for it and for spl_call_add_batch (spx_call.hip): `who` names the
// caller in the messages; `also` (may be empty) is called under host_mu with the coverage's add enqueued and enqueues its
// own work on the same records and entries, in front of the one wait.
int cover_add_batch_with(spx_index* ix, const char* who, int digest_kind, uint32_t k, uint32_t w, const uint8_t* seqs, const uint64_t* offsets,
                         uint64_t nreads, uint64_t min_length, int want_docs, const spc_params* chain_params, const spa_params* align_params,
                         const spe_params* extend_params, spn_mapping* out_mappings, const std::function<int(const CoverBatch&)>& also) {
    int rc;
    {
        std::lock_guard<std::mutex> hg(ix->host_mu);
        if ((rc = cover_need_arrays(ix, who)) != SPX_OK) return rc;
    }
    // the pipeline up to the mappings is spn_map_begin itself: its checks, its waits, its results on the device
    std::vector<spn_mapping> own;
    if (!out_mappings && nreads) {
        own.resize(nreads);
        out_mappings = own.data();
    }
    uint64_t n_in = 0;
    if ((rc = spn_map_begin(ix, digest_kind, k, w, seqs, offsets, nreads, min_length, want_docs, chain_params, align_params, extend_params,
                            out_mappings, nullptr, &n_in)) != SPX_OK)
        return rc;
    std::lock_guard<std::mutex> hg(ix->host_mu);
    SPX_HIP(hipSetDevice(ix->device));
    // (another host thread on this handle between the two locks would have taken the entries, or the arrays)
    if ((rc = ready_take(ix->map_ready, nreads, n_in, who, "the mappings")) != SPX_OK) return rc;
    if ((rc = cover_need_arrays(ix, who)) != SPX_OK) return rc;
    if (nreads == 0) return SPX_OK;
    uint64_t mapped = 0;
    for (uint64_t q = 0; q < nreads; ++q) mapped += out_mappings[q].seq != SPN_UNMAPPED;
    if (mapped >= (1ull << 32) - ix->cover_mapped) {
        set_error("%s: %llu mapped reads were added since spd_cover_reset and this batch has %llu: 2^32 or more could "
                  "wrap a depth; nothing was added",
                  who, (unsigned long long)ix->cover_mapped, (unsigned long long)mapped);
        return SPX_E_ARG;
    }
    hipStream_t st = nullptr;
    if ((rc = ctx_stream_of(ix, &st)) != SPX_OK) return rc;
    AddArgs a{};
    const spn_mapping* d_maps = (const spn_mapping*)ix->map_scr[spx_index::N_OUT].p;
    a.map = (const uint4*)d_maps;
    a.ioffs = (const uint64_t*)ix->map_scr[spx_index::N_OOFFS].p;
    a.iops = (const uint32_t*)ix->map_scr[spx_index::N_OPS].p;
    a.in_entries = n_in;
    a.nreads = nreads;
    a.diff = array_of<uint32_t>(ix, spx_index::D_DIFF);
    a.mism = array_of<uint32_t>(ix, spx_index::D_MISM);
    a.counts = array_of<unsigned long long>(ix, spx_index::D_COUNTS);
    ix->cover.dirty = true;
    ix->cover.ready = false;
    if ((rc = cover_add_enqueue(ix, a, st)) != SPX_OK) return rc;
    if (also && (rc = also(CoverBatch{d_maps, a.ioffs, a.iops, n_in, nreads, st})) != SPX_OK) return rc;
    if ((rc = ctx_wait(ix, st)) != SPX_OK) return rc;
    if ((rc = step_collect(ix, ix->cover, KIND, GenomeAcc::ADD)) != SPX_OK) return rc;
    ix->cover_mapped += mapped;
    return add_error_code(ix);
}

}  // namespace spx

using namespace spx;

extern "C" {

int spd_cover_add_device(spx_index* ix, const spn_mapping* d_mappings, const uint64_t* d_op_offsets, const uint32_t* d_ops,
                         uint64_t in_entries, uint64_t nreads, uint32_t* d_diff, uint32_t* d_mism, uint64_t* d_seq_counts, void* stream) {
    int rc;
    if ((rc = need_table(ix, "spd_cover_add_device")) != SPX_OK) return rc;
    if (!d_diff || !d_mism || !d_seq_counts || (in_entries && !d_ops) || (nreads && (!d_mappings || !d_op_offsets))) {
        set_error("d_mappings, d_op_offsets, d_ops, d_diff, d_mism and d_seq_counts must be non-null");
        return SPX_E_ARG;
    }
    if (((uintptr_t)d_mappings & 15) != 0 || (((uintptr_t)d_op_offsets | (uintptr_t)d_seq_counts) & 7) != 0 ||
        (((uintptr_t)d_ops | (uintptr_t)d_diff | (uintptr_t)d_mism) & 3) != 0) {
        set_error("d_mappings must be 16-byte aligned (records are read as 16-byte vectors), the 64-bit arrays 8-byte, d_ops, d_diff "
                  "and d_mism 4-byte aligned");
        return SPX_E_ARG;
    }
    add_reset(ix, ix->cover);
    AddArgs a{};
    a.map = (const uint4*)d_mappings;
    a.ioffs = d_op_offsets;
    a.iops = d_ops;
    a.in_entries = in_entries;
    a.nreads = nreads;
    a.diff = d_diff;
    a.mism = d_mism;
    a.counts = (unsigned long long*)d_seq_counts;
    return cover_add_enqueue(ix, a, (hipStream_t)stream);
}

int spd_cover_finish_device(spx_index* ix, const uint32_t* d_diff, const uint32_t* d_mism, const uint64_t* d_seq_counts, uint32_t* d_depth,
                            spd_seq_cover* d_out, void* stream) {
    int rc;
    if ((rc = need_table(ix, "spd_cover_finish_device")) != SPX_OK) return rc;
    if (!d_diff || !d_mism || !d_seq_counts || !d_depth || !d_out) {
        set_error("d_diff, d_mism, d_seq_counts, d_depth and d_out must be non-null");
        return SPX_E_ARG;
    }
    if ((((uintptr_t)d_seq_counts | (uintptr_t)d_out) & 7) != 0 || (((uintptr_t)d_diff | (uintptr_t)d_mism | (uintptr_t)d_depth) & 3) != 0) {
        set_error("d_seq_counts and d_out must be 8-byte aligned, d_diff, d_mism and d_depth 4-byte aligned");
        return SPX_E_ARG;
    }
    FinArgs a{};
    a.mism = d_mism;
    a.counts = (const unsigned long long*)d_seq_counts;
    a.out = d_out;
    return cover_finish_enqueue(ix, a, d_diff, d_depth, (hipStream_t)stream);
}

int spd_cover_runs_device(spx_index* ix, const uint32_t* d_depth, const uint32_t* d_mism, uint32_t min_depth, uint64_t run_capacity,
                          spd_run* d_runs, uint64_t* d_count, void* stream) {
    int rc;
    if ((rc = need_table(ix, "spd_cover_runs_device")) != SPX_OK) return rc;
    if (!d_depth || !d_mism || !d_count || (run_capacity && !d_runs)) {
        set_error("d_depth, d_mism, d_runs and d_count must be non-null");
        return SPX_E_ARG;
    }
    if ((((uintptr_t)d_runs | (uintptr_t)d_count) & 7) != 0 || (((uintptr_t)d_depth | (uintptr_t)d_mism) & 3) != 0) {
        set_error("d_runs and d_count must be 8-byte aligned, d_depth and d_mism 4-byte aligned");
        return SPX_E_ARG;
    }
    RunArgs a{};
    a.depth = d_depth;
    a.mism = d_mism;
    a.min_depth = min_depth;
    a.cap = run_capacity;
    a.rec = d_runs;
    a.count = d_count;
    return runs_enqueue(ix, a, (hipStream_t)stream, true, true);
}

int spd_cover_reset(spx_index* ix) {
    int rc;
    if ((rc = need_table(ix, "spd_cover_reset")) != SPX_OK) return rc;
    std::lock_guard<std::mutex> hg(ix->host_mu);
    SPX_HIP(hipSetDevice(ix->device));
    const Table t = table_of(ix);
    if ((rc = reset_arrays(ix, ix->cover, KIND, t.G,
                           {{spx_index::D_DIFF, (size_t)(t.G + 1) * 4, true},
                            {spx_index::D_MISM, (size_t)t.G * 4, true},
                            {spx_index::D_DEPTH, (size_t)t.G * 4, false},
                            {spx_index::D_COUNTS, (size_t)t.n_seqs * 16, true},
                            {spx_index::D_OUT, (size_t)t.n_seqs * sizeof(spd_seq_cover), false}})) != SPX_OK)
        return rc;
    ix->cover_mapped = 0;
    return SPX_OK;
}

int spd_cover_add_batch(spx_index* ix, int digest_kind, uint32_t k, uint32_t w, const uint8_t* seqs, const uint64_t* offsets, uint64_t nreads,
                        uint64_t min_length, int want_docs, const spc_params* chain_params, const spa_params* align_params,
                        const spe_params* extend_params, spn_mapping* out_mappings) {
    int rc;
    if ((rc = need_table(ix, "spd_cover_add_batch")) != SPX_OK) return rc;
    return cover_add_batch_with(ix, "spd_cover_add_batch", digest_kind, k, w, seqs, offsets, nreads, min_length, want_docs, chain_params,
                                align_params, extend_params, out_mappings, nullptr);
}

int spd_cover_summary(spx_index* ix, spd_seq_cover* out, uint64_t n_seqs) {
    if (!ix || !out) {
        set_error("index and out must be non-null");
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> hg(ix->host_mu);
    int rc;
    if ((rc = cover_need_arrays(ix, "spd_cover_summary")) != SPX_OK) return rc;
    if (n_seqs != ix->map_seq_lengths.size()) {
        set_error("spd_cover_summary: n_seqs is %llu, the sequence table has %llu", (unsigned long long)n_seqs,
                  (unsigned long long)ix->map_seq_lengths.size());
        return SPX_E_ARG;
    }
    SPX_HIP(hipSetDevice(ix->device));
    if ((rc = cover_finish_host(ix)) != SPX_OK) return rc;
    SPX_HIP(hipMemcpy(out, ix->cover.scr[spx_index::D_OUT].p, n_seqs * sizeof(spd_seq_cover), hipMemcpyDeviceToHost));
    return SPX_OK;
}

int spd_cover_runs_begin(spx_index* ix, uint32_t min_depth, uint64_t* n_runs) {
    if (!ix || !n_runs) {
        set_error("index and n_runs must be non-null");
        return SPX_E_ARG;
    }
    *n_runs = 0;
    std::lock_guard<std::mutex> hg(ix->host_mu);
    int rc;
    if ((rc = cover_need_arrays(ix, "spd_cover_runs_begin")) != SPX_OK) return rc;
    RunArgs a{};
    a.depth = array_of<const uint32_t>(ix, spx_index::D_DEPTH);
    a.mism = array_of<const uint32_t>(ix, spx_index::D_MISM);
    a.min_depth = min_depth;
    return records_begin(ix, ix->cover, KIND, a, n_runs, [&] { return cover_finish_host(ix); },
                         [&](RunArgs& r, hipStream_t st, bool count, bool write) { return runs_enqueue(ix, r, st, count, write); });
}

int spd_cover_runs_fetch(spx_index* ix, spd_run* out_runs) { return records_fetch(ix, &spx_index::cover, KIND, out_runs); }

int spd_cover_depth(spx_index* ix, uint64_t first, uint64_t count, uint32_t* out_depth, uint32_t* out_mism) {
    if (!ix) {
        set_error("index must be non-null");
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> hg(ix->host_mu);
    int rc;
    if ((rc = cover_need_arrays(ix, "spd_cover_depth")) != SPX_OK) return rc;
    if ((rc = check_range(ix->cover, "spd_cover_depth", first, count)) != SPX_OK) return rc;
    SPX_HIP(hipSetDevice(ix->device));
    if ((rc = cover_finish_host(ix)) != SPX_OK) return rc;
    if (!count) return SPX_OK;
    if (out_depth) SPX_HIP(hipMemcpy(out_depth, array_of<const uint32_t>(ix, spx_index::D_DEPTH) + first, count * 4, hipMemcpyDeviceToHost));
    if (out_mism) SPX_HIP(hipMemcpy(out_mism, array_of<const uint32_t>(ix, spx_index::D_MISM) + first, count * 4, hipMemcpyDeviceToHost));
    return SPX_OK;
}

int spd_last_cover_stats(spx_index* ix, spd_cover_stats* out) {
    if (!ix || !out) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    if (!have_any(ix->cover)) {
        set_error("no coverage has been computed on this index yet");
        return SPX_E_ARG;
    }
    const int rc = collect_all(ix, ix->cover, KIND);
    if (rc != SPX_OK) return rc;
    const GenomeAcc& ga = ix->cover;
    out->reads = ga.acc[0];
    out->mapped = ga.acc[1];
    out->added = ga.acc[2];
    out->skipped = ga.acc[3];
    out->intervals = ga.acc[4];
    out->atomics = ga.acc[5];
    out->runs = ga.n_out;
    out->error = (uint32_t)(ga.step[GenomeAcc::ADD].error & 1);
    out->overflow = (uint32_t)((ga.step[GenomeAcc::OUT].error >> 1) & 1);
    for (int i = 0; i < 3; ++i) out->step_ms[i] = ga.step_ms[i];
    out->kernel_ms = out->step_ms[0] + out->step_ms[1] + out->step_ms[2];
    return add_error_code(ix);
}

}  // extern "C"
