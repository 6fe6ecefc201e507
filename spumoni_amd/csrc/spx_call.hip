// spx_call.hip -- the pileup and the calls (include/spumoni_call.h): per base of every sequence's forward
// strand the letters of the reads' 'X' columns, the insertions that start there and the reads that delete it, accumulated
// beside the coverage of spx_cover.hip over any number of batches of spx_map.hip's mappings; the single-nucleotide calls
// these counts support; and the product's C-ABI.  The kernels read mappings, entries, the reads' bytes, the piece starts
// of the sequence table and the text (the forward piece of sequence s starts at P[s * strands]).
//
//   add      k_call_add_lane, a lane per read of up to `sw` entries (64): one pass checks the read, a second walks it with
//            a text position and a read position.  An 'X' column is one add in alt (codes 0 .. 3 of the oriented read) or
//            in other, an 'I' entry one add in ins, a 'D' entry a +1 and a -1 in ddiff.  A read of more entries is put on
//            a list, and k_call_add_wave gives each of them a wavefront: 64 entries a step, both positions of every lane
//            by wave-wide inclusive sums plus carries, the checks as sums reduced behind the first loop.  An 'X' entry of
//            more than 16 columns is spread over the wavefront, one entry after the other by a ballot.  The statistics
//            leave a block as one set of atomics.
//   finish   hipcub's inclusive sum over ddiff gives del.
//   calls    count -> exclusive sum -> write over tiles of 4096 positions, a thread per 16 consecutive ones.  A thread
//            finds its first sequence by a search in P and walks on across the borders; a position whose depth passes
//            min_depth costs one 16-byte load of alt and one byte of text.
//
// The sequence table, the tiles, the head of a mapping with its checks and the host code that works on the index's
// GenomeAcc are spx_genome_kernels.h's, shared by the coverage and the pileup.
//
// Control flow: every shuffle and ballot of k_call_add_wave stands in a loop whose trip count is the same for the whole
// wavefront (the list's length, the read's entries in steps of 64, the long 'X' entries of a step by their ballot) or
// behind them; the other kernels shuffle and synchronise only outside their loops.
#include <vector>

#include "../../include/spumoni_call.h"
#include "spx_genome_kernels.h"

namespace spx {
namespace {

constexpr uint32_t SPREAD = 16;  // an 'X' entry of more columns is spread over the wavefront

struct AddCounters {  // device; zeroed in front of every launch
    unsigned long long reads, mapped, added, skipped, xcols, others, ins, dels;
    unsigned long long nlong;  // reads on the list of k_call_add_wave
    unsigned long long error;  // bit 0: a read failed the checks
};
constexpr int ADD_WORDS = sizeof(AddCounters) / 8;
struct FinCounters {
    unsigned long long words, error;
};
constexpr int FIN_WORDS = sizeof(FinCounters) / 8;
struct CallCounters {
    unsigned long long calls;
    unsigned long long error;  // bit 1: the calls did not fit call_capacity
};
constexpr int CALL_WORDS = sizeof(CallCounters) / 8;

struct AddArgs {
    Table t;
    const uint4* map;       // 3 per read: spn_mapping
    const uint64_t* ioffs;  // nreads + 1
    const uint32_t* iops;
    uint64_t in_entries, nreads;
    const uint8_t* reads;
    const uint64_t* roffs;  // nreads + 1
    uint64_t in_chars;
    uint32_t* alt;    // 4 * G
    uint32_t* other;  // G
    uint32_t* ins;    // G
    uint32_t* ddiff;  // G + 1
    uint64_t* longs;  // nreads: the reads of more than sw entries
    uint64_t sw;
    AddCounters* c;
};
struct CallArgs {
    Table t;
    const uint8_t* text;
    const uint32_t* depth;
    const uint4* alt;
    const uint32_t* other;
    const uint32_t* ins;
    const uint32_t* del;
    uint32_t min_depth, min_alt, min_permille;
    uint64_t cap, ntiles;
    uint4* rec;       // 3 per record: spl_call
    uint64_t* tcnt;   // ntiles + 1: calls in a tile, then a 0
    uint64_t* toffs;  // ntiles + 1
    uint64_t* count;
    CallCounters* c;
};

// 0 .. 3 for A/a, C/c, G/g, T/t, 4 for every other byte
__device__ inline uint32_t code_of(uint8_t b) {
    const uint32_t u = b & 0xdfu;  // (only 'a' .. 'z' land on 'A' .. 'Z')
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 4u;
}

// One 'X' column of a checked read: g < F[s] + target_end <= G, j < len.  1 when the column's code is 4.
__device__ inline unsigned long long add_column(const AddArgs& a, const MapHead& h, uint64_t g, uint64_t j) {
    uint32_t c = code_of(a.reads[h.r0 + (h.rev ? h.len - 1 - j : j)]);
    if (c == 4) {
        atomicAdd(a.other + g, 1u);
        return 1;
    }
    if (h.rev) c = 3 - c;
    atomicAdd(a.alt + 4 * g + c, 1u);
    return 0;
}

// A lane per read, a block over a stride of reads.
__global__ __launch_bounds__(256) void k_call_add_lane(AddArgs a) {
    __shared__ unsigned long long part[4 * 7];
    unsigned long long mapped = 0, added = 0, skipped = 0, xcols = 0, others = 0, nins = 0, ndel = 0;
    for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < a.nreads; q += (uint64_t)gridDim.x * 256) {
        MapHead h;
        const int st = map_head<true>(a, q, h);
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
        // pass 1: the checks.  pend: an 'I' with no text column behind it so far
        bool ok = true, seen = false, tail = false, pend = false;
        uint64_t tsum = 0, rsum = 0;
        for (uint32_t e = 0; e < ne && ok; ++e) {
            const uint32_t v = src[e], op = v & 15u;
            const uint64_t n = v >> 4;
            if (!is_op(op)) {
                ok = false;
            } else if (op == OP_S) {
                tail = seen;
                rsum += n;
            } else {
                ok = !tail;
                seen = true;
                if (in_text(op)) {
                    tsum += n;
                    if (n) pend = false;
                } else {
                    pend = true;
                }
                if (in_read(op)) rsum += n;
            }
        }
        if (!ok || pend || tsum != h.span || rsum != h.len) {
            skipped += 1;
            continue;
        }
        // pass 2: every text position below stays under F[s] + target_end <= G, every read position under len
        uint64_t pos = h.pos, j = 0;
        for (uint32_t e = 0; e < ne; ++e) {
            const uint32_t v = src[e], op = v & 15u;
            const uint64_t n = v >> 4;
            if (op == OP_X) {
                for (uint64_t k = 0; k < n; ++k) others += add_column(a, h, pos + k, j + k);
                xcols += n;
            } else if (op == OP_I) {
                atomicAdd(a.ins + pos, 1u);
                nins += 1;
            } else if (op == OP_D) {
                atomicAdd(a.ddiff + pos, 1u);
                atomicAdd(a.ddiff + pos + n, 0xffffffffu);
                ndel += 1;
            }
            if (in_text(op)) pos += n;
            if (in_read(op)) j += n;
        }
        added += 1;
    }
    if (skipped) atomicOr(&a.c->error, 1ull);
    unsigned long long v[7] = {mapped, added, skipped, xcols, others, nins, ndel};
    block_counts<7>(part, &a.c->mapped, v);
    if (blockIdx.x == 0 && threadIdx.x == 0) a.c->reads = a.nreads;
}

// A wavefront per read of the list, a grid over a stride of the list.
__global__ __launch_bounds__(256) void k_call_add_wave(AddArgs a) {
    __shared__ unsigned long long part[4 * 6];
    const uint64_t nlong = a.c->nlong;
    if ((uint64_t)blockIdx.x * 4 >= nlong) return;  // (the whole block: a batch of short reads has no list)
    const uint32_t lane = threadIdx.x & 63;
    unsigned long long added = 0, skipped = 0, xcols = 0, others = 0, nins = 0, ndel = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < nlong; i += (uint64_t)gridDim.x * 4) {
        MapHead h;
        if (map_head<true>(a, a.longs[i], h) != 1) continue;  // (the lane's kernel listed it because it is 1; the same for every lane)
        const uint32_t* src = a.iops + h.i0;
        // pass 1: each lane over its entries, the sums behind the loop.  No 'S' between two others: the entries that are
        // not 'S' are as many as lie between the first and the last of them.  No 'I' behind the last text column: the
        // last 'I' (index + 1, 0: none) stands in front of the last text-consuming entry of a length above 0
        bool bad = false;
        unsigned long long tsum = 0, rsum = 0, inner = 0, first = ~0ull, last = 0, last_i = 0, last_t = 0;
        for (uint64_t e = lane; e < h.ne; e += 64) {
            const uint32_t v = src[e], op = v & 15u;
            const unsigned long long n = v >> 4;
            if (!is_op(op)) {
                bad = true;
            } else {
                if (op != OP_S) {
                    inner += 1;
                    first = e < first ? e : first;
                    last = e;
                }
                if (in_text(op)) {
                    tsum += n;
                    if (n) last_t = e + 1;
                }
                if (in_read(op)) rsum += n;
                if (op == OP_I) last_i = e + 1;
            }
        }
        bad = __ballot(bad) != 0;
        tsum = wave_sum(tsum);
        rsum = wave_sum(rsum);
        inner = wave_sum(inner);
        first = wave_min(first);
        last = wave_max(last);
        last_i = wave_max(last_i);
        last_t = wave_max(last_t);
        if (bad || tsum != h.span || rsum != h.len || last_i > last_t || (inner && last - first + 1 != inner)) {
            skipped += lane == 0;
            continue;
        }
        // pass 2
        uint64_t cpos = h.pos, cj = 0;
        for (uint64_t base = 0; base < h.ne; base += 64) {
            const uint64_t e = base + lane;
            const uint32_t v = e < h.ne ? src[e] : OP_S, op = v & 15u;  // (an 'S' of no columns moves nothing)
            const unsigned long long n = v >> 4;
            const unsigned long long tn = in_text(op) ? n : 0, rn = in_read(op) ? n : 0;
            unsigned long long it = tn, ir = rn;
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned long long ut = __shfl_up(it, d), ur = __shfl_up(ir, d);
                if ((int)lane >= d) {
                    it += ut;
                    ir += ur;
                }
            }
            const uint64_t pos = cpos + it - tn, j = cj + ir - rn;
            const bool spread = op == OP_X && n > SPREAD;
            if (op == OP_X) {
                if (!spread)
                    for (uint64_t k = 0; k < n; ++k) others += add_column(a, h, pos + k, j + k);
                xcols += n;
            } else if (op == OP_I) {
                atomicAdd(a.ins + pos, 1u);
                nins += 1;
            } else if (op == OP_D) {
                atomicAdd(a.ddiff + pos, 1u);
                atomicAdd(a.ddiff + pos + n, 0xffffffffu);
                ndel += 1;
            }
            // the long 'X' entries of this step, one after the other, their columns dealt to the lanes
            for (unsigned long long m = __ballot(spread); m; m &= m - 1) {
                const int from = __ffsll((long long)m) - 1;
                const uint64_t bpos = __shfl(pos, from), bj = __shfl(j, from);
                const unsigned long long bn = __shfl(n, from);
                for (uint64_t k = lane; k < bn; k += 64) others += add_column(a, h, bpos + k, bj + k);
            }
            cpos += __shfl(it, 63);
            cj += __shfl(ir, 63);
        }
        added += lane == 0;
    }
    if (skipped) atomicOr(&a.c->error, 1ull);
    unsigned long long v[6] = {added, skipped, xcols, others, nins, ndel};
    block_counts<6>(part, &a.c->added, v);
}

// The calls among the positions [p0, p1) of the forward genome, in order: emit(position in the sequence, sequence, depth,
// alt, reference byte, allele) for each.
template <typename Emit>
__device__ inline uint32_t scan_calls(const CallArgs& a, uint64_t p0, uint64_t p1, Emit&& emit) {
    if (p0 >= p1) return 0;
    uint64_t s = seq_of(a.t, p0), lo = seq_start(a.t, s), hi = seq_start(a.t, s + 1);
    uint32_t found = 0;
    for (uint64_t p = p0; p < p1; ++p) {
        if (p == hi) {
            s += 1;
            lo = hi;
            hi = seq_start(a.t, s + 1);
        }
        const uint32_t d = a.depth[p];
        if (d < a.min_depth) continue;
        const uint4 al = a.alt[p];
        const uint8_t ref = a.text[a.t.P[s * a.t.strands] + (p - lo)];
        const uint32_t rc = code_of(ref), cnt[4] = {al.x, al.y, al.z, al.w};
        uint32_t best = rc == 0 ? 1u : 0u;  // the lowest candidate
#pragma unroll
        for (uint32_t c = 1; c < 4; ++c)
            if (c != rc && c > best && cnt[c] > cnt[best]) best = c;
        if (cnt[best] >= a.min_alt && (unsigned long long)cnt[best] * 1000ull >= (unsigned long long)a.min_permille * d) {
            emit(p - lo, (uint32_t)s, d, al, ref, best, p);
            found += 1;
        }
    }
    return found;
}

__global__ __launch_bounds__(256) void k_call_count(CallArgs a) {
    using Reduce = hipcub::BlockReduce<uint32_t, 256>;
    __shared__ typename Reduce::TempStorage tmp;
    const Tile x = tile_of(a.t.G);
    const uint32_t mine = scan_calls(a, x.p0, x.p1, [](uint64_t, uint32_t, uint32_t, const uint4&, uint8_t, uint32_t, uint64_t) {});
    const uint32_t n = Reduce(tmp).Sum(mine);
    if (threadIdx.x == 0) {
        a.tcnt[blockIdx.x] = n;
        if (blockIdx.x == 0) a.tcnt[a.ntiles] = 0;
    }
}

__global__ __launch_bounds__(256) void k_call_write(CallArgs a) {
    using Scan = hipcub::BlockScan<uint32_t, 256>;
    __shared__ typename Scan::TempStorage tmp;
    const Tile x = tile_of(a.t.G);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t total = a.toffs[a.ntiles];
        *a.count = total;
        a.c->calls = total;
        if (total > a.cap) atomicOr(&a.c->error, 2ull);
    }
    const uint32_t mine = scan_calls(a, x.p0, x.p1, [](uint64_t, uint32_t, uint32_t, const uint4&, uint8_t, uint32_t, uint64_t) {});
    uint32_t before = 0;
    Scan(tmp).ExclusiveSum(mine, before);
    if (!mine) return;
    uint64_t next = a.toffs[blockIdx.x] + before;
    scan_calls(a, x.p0, x.p1, [&](uint64_t at, uint32_t s, uint32_t d, const uint4& al, uint8_t ref, uint32_t allele, uint64_t p) {
        const uint64_t r = next++;
        if (r >= a.cap) return;
        a.rec[3 * r] = make_uint4((uint32_t)at, (uint32_t)(at >> 32), s, d);
        a.rec[3 * r + 1] = al;
        a.rec[3 * r + 2] = make_uint4(a.other[p], a.del[p], a.ins[p], (uint32_t)ref | (allele << 8));
    });
}

constexpr GenomeKind KIND = {"spl_call_reset", "the pileup", "about 28 per base beside the coverage's 12", "spl_calls_begin", "spl_calls_fetch",
                             "out_calls", {ADD_WORDS, FIN_WORDS, CALL_WORDS}, 8, sizeof(spl_call)};

int check_params(uint32_t min_depth, uint32_t min_alt, uint32_t min_permille) {
    if (min_depth < 1 || min_alt < 1 || min_permille > 1000) {
        set_error("min_depth and min_alt must be at least 1 and min_permille between 0 and 1000 (they are %u, %u, %u)", min_depth, min_alt,
                  min_permille);
        return SPX_E_ARG;
    }
    return SPX_OK;
}

int call_add_enqueue(spx_index* ix, AddArgs& a, hipStream_t st) { return add_enqueue(ix, ix->call, KIND, a, st, k_call_add_lane, k_call_add_wave); }

// hipcub's inclusive sum over ddiff gives del
int call_finish_enqueue(spx_index* ix, const uint32_t* d_ddiff, uint32_t* d_del, hipStream_t st) {
    return finish_enqueue(ix, ix->call, KIND, d_ddiff, d_del, st, [](const Table&) { return SPX_OK; });
}

int calls_enqueue(spx_index* ix, CallArgs& a, hipStream_t st, bool count, bool write) {
    // (the callables run under ix->mu, which guards ix->text as it guards the table)
    return tiles_enqueue(
        ix, ix->call, KIND, a, st, count, write,
        [&] {
            a.text = ix->text;
            k_call_count<<<(unsigned)a.ntiles, 256, 0, st>>>(a);
        },
        [&]() -> int {
            a.text = ix->text;
            k_call_write<<<(unsigned)a.ntiles, 256, 0, st>>>(a);
            SPX_HIP(hipGetLastError());
            return SPX_OK;
        });
}

int add_error_code(const spx_index* ix) {
    if (ix->call.step[GenomeAcc::ADD].error & 1) {
        set_error("a read failed the pileup's checks (the coverage's checks on its mapping, entries whose read lengths disagree with "
                  "the read's, an 'I' behind the last text column, or read offsets outside the reads): such a read adds nothing");
        return SPX_E_FORMAT;
    }
    return SPX_OK;
}

// The host forms' arrays of both products are there and belong to the table in force.  The caller holds host_mu.
int call_need_arrays(spx_index* ix, const char* who) {
    const int rc = need_arrays(ix, ix->call, KIND, who);
    return rc != SPX_OK ? rc : cover_need_arrays(ix, who);
}

template <typename T>
T* array_of(spx_index* ix, int slot) {
    return (T*)ix->call.scr[slot].p;
}

// del from the handle's ddiff, when something was added since it was made.  The caller holds host_mu.
int call_finish_host(spx_index* ix) {
    return finish_host(ix, ix->call, KIND, [&](hipStream_t st) {
        return call_finish_enqueue(ix, array_of<const uint32_t>(ix, spx_index::PL_DDIFF), array_of<uint32_t>(ix, spx_index::PL_DEL), st);
    });
}

// Waits for the copy of a batch's reads when the call that issued it ends, however it ends: the copy reads the caller's
// memory and the call's own offsets.
struct CopyGuard {
    hipStream_t s = nullptr;
    ~CopyGuard() {
        if (s) (void)hipStreamSynchronize(s);
    }
};

}  // namespace

void release_call(spx_index* ix) {
    release_acc(ix->call);
    if (ix->call_copy_ev) (void)hipEventDestroy(ix->call_copy_ev);
    if (ix->call_copy_s) (void)hipStreamDestroy(ix->call_copy_s);
}
int clone_call(spx_index* src, spx_index* ix) { return src->call.G ? spl_call_reset(ix) : SPX_OK; }
void call_table_changed(spx_index* ix) { acc_table_changed(ix->call); }
int call_arrays_ready(spx_index* ix, const char* who) { return call_need_arrays(ix, who); }
int call_finish_arrays(spx_index* ix) { return call_finish_host(ix); }

}  // namespace spx

using namespace spx;

extern "C" {

int spl_pileup_add_device(spx_index* ix, const spn_mapping* d_mappings, const uint64_t* d_op_offsets, const uint32_t* d_ops,
                          uint64_t in_entries, const uint8_t* d_reads, const uint64_t* d_read_offsets, uint64_t in_chars, uint64_t nreads,
                          uint32_t* d_alt, uint32_t* d_other, uint32_t* d_ins, uint32_t* d_ddiff, void* stream) {
    int rc;
    if ((rc = need_table(ix, "spl_pileup_add_device")) != SPX_OK) return rc;
    if (!d_alt || !d_other || !d_ins || !d_ddiff || (in_entries && !d_ops) || (in_chars && !d_reads) ||
        (nreads && (!d_mappings || !d_op_offsets || !d_read_offsets))) {
        set_error("d_mappings, d_op_offsets, d_ops, d_reads, d_read_offsets, d_alt, d_other, d_ins and d_ddiff must be non-null");
        return SPX_E_ARG;
    }
    if ((((uintptr_t)d_mappings | (uintptr_t)d_alt) & 15) != 0 || (((uintptr_t)d_op_offsets | (uintptr_t)d_read_offsets) & 7) != 0 ||
        (((uintptr_t)d_ops | (uintptr_t)d_other | (uintptr_t)d_ins | (uintptr_t)d_ddiff) & 3) != 0) {
        set_error("d_mappings and d_alt must be 16-byte aligned (records and the four counts of a base are 16-byte vectors), the offsets "
                  "8-byte, d_ops, d_other, d_ins and d_ddiff 4-byte aligned");
        return SPX_E_ARG;
    }
    add_reset(ix, ix->call);
    AddArgs a{};
    a.map = (const uint4*)d_mappings;
    a.ioffs = d_op_offsets;
    a.iops = d_ops;
    a.in_entries = in_entries;
    a.nreads = nreads;
    a.reads = d_reads;
    a.roffs = d_read_offsets;
    a.in_chars = in_chars;
    a.alt = d_alt;
    a.other = d_other;
    a.ins = d_ins;
    a.ddiff = d_ddiff;
    return call_add_enqueue(ix, a, (hipStream_t)stream);
}

int spl_pileup_finish_device(spx_index* ix, const uint32_t* d_ddiff, uint32_t* d_del, void* stream) {
    int rc;
    if ((rc = need_table(ix, "spl_pileup_finish_device")) != SPX_OK) return rc;
    if (!d_ddiff || !d_del) {
        set_error("d_ddiff and d_del must be non-null");
        return SPX_E_ARG;
    }
    if ((((uintptr_t)d_ddiff | (uintptr_t)d_del) & 3) != 0) {
        set_error("d_ddiff and d_del must be 4-byte aligned");
        return SPX_E_ARG;
    }
    return call_finish_enqueue(ix, d_ddiff, d_del, (hipStream_t)stream);
}

int spl_calls_device(spx_index* ix, const uint32_t* d_depth, const uint32_t* d_mism, const uint32_t* d_alt, const uint32_t* d_other,
                     const uint32_t* d_ins, const uint32_t* d_del, uint32_t min_depth, uint32_t min_alt, uint32_t min_permille,
                     uint64_t call_capacity, spl_call* d_calls, uint64_t* d_count, void* stream) {
    int rc;
    if ((rc = need_table(ix, "spl_calls_device")) != SPX_OK) return rc;
    if (!d_depth || !d_mism || !d_alt || !d_other || !d_ins || !d_del || !d_count || (call_capacity && !d_calls)) {
        set_error("d_depth, d_mism, d_alt, d_other, d_ins, d_del, d_calls and d_count must be non-null");
        return SPX_E_ARG;
    }
    if ((((uintptr_t)d_alt | (uintptr_t)d_calls) & 15) != 0 || ((uintptr_t)d_count & 7) != 0 ||
        (((uintptr_t)d_depth | (uintptr_t)d_mism | (uintptr_t)d_other | (uintptr_t)d_ins | (uintptr_t)d_del) & 3) != 0) {
        set_error("d_alt and d_calls must be 16-byte aligned, d_count 8-byte, d_depth, d_mism, d_other, d_ins and d_del 4-byte aligned");
        return SPX_E_ARG;
    }
    if ((rc = check_params(min_depth, min_alt, min_permille)) != SPX_OK) return rc;
    CallArgs a{};
    a.depth = d_depth;
    a.alt = (const uint4*)d_alt;
    a.other = d_other;
    a.ins = d_ins;
    a.del = d_del;
    a.min_depth = min_depth;
    a.min_alt = min_alt;
    a.min_permille = min_permille;
    a.cap = call_capacity;
    a.rec = (uint4*)d_calls;
    a.count = d_count;
    return calls_enqueue(ix, a, (hipStream_t)stream, true, true);
}

int spl_call_reset(spx_index* ix) {
    int rc;
    if ((rc = need_table(ix, "spl_call_reset")) != SPX_OK) return rc;
    if ((rc = spd_cover_reset(ix)) != SPX_OK) return rc;
    std::lock_guard<std::mutex> hg(ix->host_mu);
    SPX_HIP(hipSetDevice(ix->device));
    const size_t G = table_of(ix).G;
    return reset_arrays(ix, ix->call, KIND, G,
                        {{spx_index::PL_ALT, G * 16, true},
                         {spx_index::PL_OTHER, G * 4, true},
                         {spx_index::PL_INS, G * 4, true},
                         {spx_index::PL_DDIFF, (G + 1) * 4, true},
                         {spx_index::PL_DEL, G * 4, false}});
}

int spl_call_add_batch(spx_index* ix, int digest_kind, uint32_t k, uint32_t w, const uint8_t* seqs, const uint64_t* offsets, uint64_t nreads,
                       uint64_t min_length, int want_docs, const spc_params* chain_params, const spa_params* align_params,
                       const spe_params* extend_params, spn_mapping* out_mappings) {
    int rc;
    if ((rc = need_table(ix, "spl_call_add_batch")) != SPX_OK) return rc;
    // the reads' bytes once more, for the pileup alone: the staged walk does not promise them behind spn_map_begin.  Rebased
    // offsets and the copy go out on the product's own stream in front of spn_map_begin, which checks the same offsets
    std::vector<uint64_t> rel;
    uint64_t chars = 0;
    bool copied = false;
    CopyGuard guard;
    void *d_reads = nullptr, *d_roffs = nullptr;
    {
        std::lock_guard<std::mutex> hg(ix->host_mu);
        if ((rc = call_need_arrays(ix, "spl_call_add_batch")) != SPX_OK) return rc;
        bool sorted = seqs && offsets && nreads;
        for (uint64_t q = 0; sorted && q < nreads; ++q) sorted = offsets[q] <= offsets[q + 1];
        if (sorted) {
            chars = offsets[nreads] - offsets[0];
            rel.resize(nreads + 1);
            for (uint64_t q = 0; q <= nreads; ++q) rel[q] = offsets[q] - offsets[0];
            std::lock_guard<std::mutex> g(ix->mu);
            SPX_HIP(hipSetDevice(ix->device));
            if ((rc = ix->call.scr[spx_index::PL_READS].reserve(chars + 16, &d_reads)) != SPX_OK) return rc;
            if ((rc = ix->call.scr[spx_index::PL_ROFFS].reserve((nreads + 1) * 8, &d_roffs)) != SPX_OK) return rc;
            if (!ix->call_copy_s) SPX_HIP(hipStreamCreateWithFlags(&ix->call_copy_s, hipStreamNonBlocking));
            if (!ix->call_copy_ev) SPX_HIP(hipEventCreateWithFlags(&ix->call_copy_ev, hipEventDisableTiming));
            guard.s = ix->call_copy_s;
            SPX_HIP(hipMemcpyAsync(d_roffs, rel.data(), (nreads + 1) * 8, hipMemcpyHostToDevice, ix->call_copy_s));
            if (chars) SPX_HIP(hipMemcpyAsync(d_reads, seqs + offsets[0], chars, hipMemcpyHostToDevice, ix->call_copy_s));
            SPX_HIP(hipEventRecord(ix->call_copy_ev, ix->call_copy_s));
            copied = true;
        }
    }
    rc = cover_add_batch_with(ix, "spl_call_add_batch", digest_kind, k, w, seqs, offsets, nreads, min_length, want_docs, chain_params,
                              align_params, extend_params, out_mappings, [&](const CoverBatch& b) -> int {
                                  int rc2;
                                  if ((rc2 = call_need_arrays(ix, "spl_call_add_batch")) != SPX_OK) return rc2;
                                  if (!copied) {
                                      set_error("spl_call_add_batch: the reads' offsets decrease");
                                      return SPX_E_ARG;
                                  }
                                  SPX_HIP(hipStreamWaitEvent(b.stream, ix->call_copy_ev, 0));
                                  AddArgs a{};
                                  a.map = (const uint4*)b.d_mappings;
                                  a.ioffs = b.d_op_offsets;
                                  a.iops = b.d_ops;
                                  a.in_entries = b.in_entries;
                                  a.nreads = b.nreads;
                                  a.reads = (const uint8_t*)d_reads;
                                  a.roffs = (const uint64_t*)d_roffs;
                                  a.in_chars = chars;
                                  a.alt = array_of<uint32_t>(ix, spx_index::PL_ALT);
                                  a.other = array_of<uint32_t>(ix, spx_index::PL_OTHER);
                                  a.ins = array_of<uint32_t>(ix, spx_index::PL_INS);
                                  a.ddiff = array_of<uint32_t>(ix, spx_index::PL_DDIFF);
                                  ix->call.dirty = true;
                                  ix->call.ready = false;
                                  return call_add_enqueue(ix, a, b.stream);
                              });
    std::lock_guard<std::mutex> hg(ix->host_mu);
    if (ix->call.step[GenomeAcc::ADD].pending) {  // (enqueued: the coverage's wait may or may not have come behind it)
        const int rc2 = step_collect(ix, ix->call, KIND, GenomeAcc::ADD);
        if (rc == SPX_OK) rc = rc2;
    }
    return rc != SPX_OK ? rc : add_error_code(ix);
}

int spl_calls_begin(spx_index* ix, uint32_t min_depth, uint32_t min_alt, uint32_t min_permille, uint64_t* n_calls) {
    if (!ix || !n_calls) {
        set_error("index and n_calls must be non-null");
        return SPX_E_ARG;
    }
    *n_calls = 0;
    std::lock_guard<std::mutex> hg(ix->host_mu);
    int rc;
    if ((rc = call_need_arrays(ix, "spl_calls_begin")) != SPX_OK) return rc;
    if ((rc = check_params(min_depth, min_alt, min_permille)) != SPX_OK) return rc;
    CallArgs a{};
    a.depth = (const uint32_t*)ix->cover.scr[spx_index::D_DEPTH].p;
    a.alt = array_of<const uint4>(ix, spx_index::PL_ALT);
    a.other = array_of<const uint32_t>(ix, spx_index::PL_OTHER);
    a.ins = array_of<const uint32_t>(ix, spx_index::PL_INS);
    a.del = array_of<const uint32_t>(ix, spx_index::PL_DEL);
    a.min_depth = min_depth;
    a.min_alt = min_alt;
    a.min_permille = min_permille;
    return records_begin(
        ix, ix->call, KIND, a, n_calls,
        [&] {
            const int rc2 = cover_finish_host(ix);
            return rc2 != SPX_OK ? rc2 : call_finish_host(ix);
        },
        [&](CallArgs& c, hipStream_t st, bool count, bool write) { return calls_enqueue(ix, c, st, count, write); });
}

int spl_calls_fetch(spx_index* ix, spl_call* out_calls) { return records_fetch(ix, &spx_index::call, KIND, out_calls); }

int spl_pileup_counts(spx_index* ix, uint64_t first, uint64_t count, uint32_t* out_alt, uint32_t* out_other, uint32_t* out_ins,
                      uint32_t* out_del) {
    if (!ix) {
        set_error("index must be non-null");
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> hg(ix->host_mu);
    int rc;
    if ((rc = call_need_arrays(ix, "spl_pileup_counts")) != SPX_OK) return rc;
    if ((rc = check_range(ix->call, "spl_pileup_counts", first, count)) != SPX_OK) return rc;
    SPX_HIP(hipSetDevice(ix->device));
    if ((rc = call_finish_host(ix)) != SPX_OK) return rc;
    if (!count) return SPX_OK;
    uint32_t* const out[4] = {out_alt, out_other, out_ins, out_del};
    const int slot[4] = {spx_index::PL_ALT, spx_index::PL_OTHER, spx_index::PL_INS, spx_index::PL_DEL};
    for (int i = 0; i < 4; ++i) {
        const uint64_t per = i == 0 ? 4 : 1;
        if (out[i]) SPX_HIP(hipMemcpy(out[i], array_of<const uint32_t>(ix, slot[i]) + first * per, count * per * 4, hipMemcpyDeviceToHost));
    }
    return SPX_OK;
}

int spl_last_call_stats(spx_index* ix, spl_call_stats* out) {
    if (!ix || !out) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    if (!have_any(ix->call)) {
        set_error("no pileup has been computed on this index yet");
        return SPX_E_ARG;
    }
    const int rc = collect_all(ix, ix->call, KIND);
    if (rc != SPX_OK) return rc;
    const GenomeAcc& ga = ix->call;
    std::memset(out, 0, sizeof *out);
    out->reads = ga.acc[0];
    out->mapped = ga.acc[1];
    out->added = ga.acc[2];
    out->skipped = ga.acc[3];
    out->x_columns = ga.acc[4];
    out->other_columns = ga.acc[5];
    out->insertions = ga.acc[6];
    out->deletions = ga.acc[7];
    out->atomics = out->x_columns + out->insertions + 2 * out->deletions;
    out->calls = ga.n_out;
    out->error = (uint32_t)(ga.step[GenomeAcc::ADD].error & 1);
    out->overflow = (uint32_t)((ga.step[GenomeAcc::OUT].error >> 1) & 1);
    for (int i = 0; i < 3; ++i) out->step_ms[i] = ga.step_ms[i];
    return add_error_code(ix);
}

}  // extern "C"
