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
// Control flow: every shuffle and ballot of k_call_add_wave stands in a loop whose trip count is the same for the whole
// wavefront (the list's length, the read's entries in steps of 64, the long 'X' entries of a step by their ballot) or
// behind them; the other kernels shuffle and synchronise only outside their loops.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/spumoni_call.h"
#include "spx_internal.h"

namespace spx {
namespace {

constexpr uint32_t OP_I = SPG_OP_I, OP_D = SPG_OP_D, OP_N = SPG_OP_N, OP_S = SPE_OP_S, OP_EQ = SPG_OP_EQ, OP_X = SPG_OP_X;
constexpr int PER_THREAD = 16, TILE = 256 * PER_THREAD;  // positions of a calls tile
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

struct Table {
    const uint64_t* P;  // n_seqs * strands + 1
    uint64_t n_seqs;
    uint32_t strands;
    uint64_t G;
};
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
    uint4* calls;     // 3 per record: spl_call
    uint64_t* tcnt;   // ntiles + 1: calls in a tile, then a 0
    uint64_t* toffs;  // ntiles + 1
    uint64_t* count;
    CallCounters* c;
};

__device__ inline unsigned long long wave_sum(unsigned long long v) {
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    return v;
}
__device__ inline unsigned long long wave_min(unsigned long long v) {
    for (int s = 32; s > 0; s >>= 1) {
        const unsigned long long o = __shfl_xor(v, s);
        v = o < v ? o : v;
    }
    return v;
}
__device__ inline unsigned long long wave_max(unsigned long long v) {
    for (int s = 32; s > 0; s >>= 1) {
        const unsigned long long o = __shfl_xor(v, s);
        v = o > v ? o : v;
    }
    return v;
}
__device__ inline bool in_text(uint32_t op) { return op == OP_EQ || op == OP_X || op == OP_D || op == OP_N; }
__device__ inline bool in_read(uint32_t op) { return op == OP_EQ || op == OP_X || op == OP_I || op == OP_S; }
__device__ inline bool is_op(uint32_t op) { return in_text(op) || op == OP_I || op == OP_S; }
__device__ inline uint64_t seq_start(const Table& t, uint64_t s) { return t.P[s * t.strands] / t.strands; }  // s <= n_seqs
// the sequence that holds position x < G of the forward genome
__device__ inline uint64_t seq_of(const Table& t, uint64_t x) {
    uint64_t lo = 0, hi = t.n_seqs;  // F[lo] <= x < F[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (seq_start(t, mid) <= x)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}
// 0 .. 3 for A/a, C/c, G/g, T/t, 4 for every other byte
__device__ inline uint32_t code_of(uint8_t b) {
    const uint32_t u = b & 0xdfu;  // (only 'a' .. 'z' land on 'A' .. 'Z')
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 4u;
}

struct ReadHead {
    uint32_t s;
    bool rev;
    uint64_t pos, span, i0, ne, r0, len;  // pos: F[s] + target_start; span: target_end - target_start
};
// 0: unmapped, 1: the record and the offsets pass, 2: they do not
__device__ inline int read_head(const AddArgs& a, uint64_t q, ReadHead& h) {
    const uint4 w1 = a.map[3 * q + 1];
    if (w1.x == SPN_UNMAPPED) return 0;
    const uint4 w0 = a.map[3 * q];
    const uint64_t ts = (uint64_t)w0.x | ((uint64_t)w0.y << 32), te = (uint64_t)w0.z | ((uint64_t)w0.w << 32);
    const uint64_t i0 = a.ioffs[q], i1 = a.ioffs[q + 1], r0 = a.roffs[q], r1 = a.roffs[q + 1];
    if (w1.x >= a.t.n_seqs || i1 < i0 || i1 > a.in_entries || r1 < r0 || r1 > a.in_chars || ts > te) return 2;
    const uint64_t p0 = a.t.P[(uint64_t)w1.x * a.t.strands], p1 = a.t.P[(uint64_t)w1.x * a.t.strands + 1];
    if (te > p1 - p0) return 2;
    h.s = w1.x;
    h.rev = w1.y != 0;
    h.pos = p0 / a.t.strands + ts;
    h.span = te - ts;
    h.i0 = i0;
    h.ne = i1 - i0;
    h.r0 = r0;
    h.len = r1 - r0;
    return 1;
}

// One 'X' column of a checked read: g < F[s] + target_end <= G, j < len.  1 when the column's code is 4.
__device__ inline unsigned long long add_column(const AddArgs& a, const ReadHead& h, uint64_t g, uint64_t j) {
    uint32_t c = code_of(a.reads[h.r0 + (h.rev ? h.len - 1 - j : j)]);
    if (c == 4) {
        atomicAdd(a.other + g, 1u);
        return 1;
    }
    if (h.rev) c = 3 - c;
    atomicAdd(a.alt + 4 * g + c, 1u);
    return 0;
}

// N sums leave a block of four wavefronts as one set of atomics
template <int N>
__device__ inline void block_counts(unsigned long long* part, unsigned long long* to, unsigned long long (&v)[N]) {
    const uint32_t wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const unsigned long long s = wave_sum(v[i]);
        if ((threadIdx.x & 63) == 0) part[wv * N + i] = s;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const unsigned long long s = part[threadIdx.x] + part[N + threadIdx.x] + part[2 * N + threadIdx.x] + part[3 * N + threadIdx.x];
        if (s) atomicAdd(to + threadIdx.x, s);
    }
}

// A lane per read, a block over a stride of reads.
__global__ __launch_bounds__(256) void k_call_add_lane(AddArgs a) {
    __shared__ unsigned long long part[4 * 7];
    unsigned long long mapped = 0, added = 0, skipped = 0, xcols = 0, others = 0, nins = 0, ndel = 0;
    for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < a.nreads; q += (uint64_t)gridDim.x * 256) {
        ReadHead h;
        const int st = read_head(a, q, h);
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
        ReadHead h;
        if (read_head(a, a.longs[i], h) != 1) continue;  // (the lane's kernel listed it because it is 1; the same for every lane)
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
    const uint64_t t0 = (uint64_t)blockIdx.x * TILE, t1 = t0 + TILE < a.t.G ? t0 + TILE : a.t.G;
    const uint64_t p0 = t0 + (uint64_t)threadIdx.x * PER_THREAD, p1 = p0 + PER_THREAD < t1 ? p0 + PER_THREAD : t1;
    const uint32_t mine = scan_calls(a, p0, p1, [](uint64_t, uint32_t, uint32_t, const uint4&, uint8_t, uint32_t, uint64_t) {});
    const uint32_t n = Reduce(tmp).Sum(mine);
    if (threadIdx.x == 0) {
        a.tcnt[blockIdx.x] = n;
        if (blockIdx.x == 0) a.tcnt[a.ntiles] = 0;
    }
}

__global__ __launch_bounds__(256) void k_call_write(CallArgs a) {
    using Scan = hipcub::BlockScan<uint32_t, 256>;
    __shared__ typename Scan::TempStorage tmp;
    const uint64_t t0 = (uint64_t)blockIdx.x * TILE, t1 = t0 + TILE < a.t.G ? t0 + TILE : a.t.G;
    const uint64_t p0 = t0 + (uint64_t)threadIdx.x * PER_THREAD, p1 = p0 + PER_THREAD < t1 ? p0 + PER_THREAD : t1;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t total = a.toffs[a.ntiles];
        *a.count = total;
        a.c->calls = total;
        if (total > a.cap) atomicOr(&a.c->error, 2ull);
    }
    const uint32_t mine = scan_calls(a, p0, p1, [](uint64_t, uint32_t, uint32_t, const uint4&, uint8_t, uint32_t, uint64_t) {});
    uint32_t before = 0;
    Scan(tmp).ExclusiveSum(mine, before);
    if (!mine) return;
    uint64_t next = a.toffs[blockIdx.x] + before;
    scan_calls(a, p0, p1, [&](uint64_t at, uint32_t s, uint32_t d, const uint4& al, uint8_t ref, uint32_t allele, uint64_t p) {
        const uint64_t r = next++;
        if (r >= a.cap) return;
        a.calls[3 * r] = make_uint4((uint32_t)at, (uint32_t)(at >> 32), s, d);
        a.calls[3 * r + 1] = al;
        a.calls[3 * r + 2] = make_uint4(a.other[p], a.del[p], a.ins[p], (uint32_t)ref | (allele << 8));
    });
}

int need_table(const spx_index* ix, const char* who) {
    if (!ix) {
        set_error("index must be non-null");
        return SPX_E_ARG;
    }
    if (!ix->map_P) {
        set_error("%s needs the sequence table: the index has none (spn_set_sequences; spumoni build -s writes it)", who);
        return SPX_E_ARG;
    }
    return SPX_OK;
}
Table table_of(const spx_index* ix) {
    return Table{ix->map_P, ix->map_seq_lengths.size(), ix->map_strands, ix->n_text / ix->map_strands};
}
uint64_t tiles_of(uint64_t G) { return (G + TILE - 1) / TILE; }

int check_params(uint32_t min_depth, uint32_t min_alt, uint32_t min_permille) {
    if (min_depth < 1 || min_alt < 1 || min_permille > 1000) {
        set_error("min_depth and min_alt must be at least 1 and min_permille between 0 and 1000 (they are %u, %u, %u)", min_depth, min_alt,
                  min_permille);
        return SPX_E_ARG;
    }
    return SPX_OK;
}

void add_reset(spx_index* ix) {
    product_reset(ix, ix->call_add);
    std::lock_guard<std::mutex> g(ix->mu);
    std::memset(ix->call_acc, 0, sizeof ix->call_acc);
}

// The list of one call and both kernels on st, between the step's two events.  Takes ix->mu.
int add_enqueue(spx_index* ix, AddArgs& a, hipStream_t st) {
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    a.t = table_of(ix);
    a.sw = (uint64_t)ix->call_switch;
    void* p = nullptr;
    int rc;
    if ((rc = ix->call_scr[spx_index::PL_LONG].reserve(a.nreads * 8 + 8, &p)) != SPX_OK) return rc;
    a.longs = (uint64_t*)p;
    return product_enqueue(ix->call_add, ADD_WORDS, st, [&](void* counters) -> int {
        a.c = (AddCounters*)counters;
        if (!a.nreads) return SPX_OK;
        const unsigned grid = (unsigned)std::min<uint64_t>((a.nreads + 255) / 256, 1024);
        k_call_add_lane<<<grid, 256, 0, st>>>(a);
        SPX_HIP(hipGetLastError());
        k_call_add_wave<<<(unsigned)std::min<uint64_t>((a.nreads + 3) / 4, 2048), 256, 0, st>>>(a);
        SPX_HIP(hipGetLastError());
        return SPX_OK;
    });
}

int finish_enqueue(spx_index* ix, const uint32_t* d_ddiff, uint32_t* d_del, hipStream_t st) {
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    const uint64_t G = table_of(ix).G;
    size_t cub_bytes = 0;
    SPX_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, cub_bytes, d_ddiff, d_del, G, (hipStream_t) nullptr));
    void* cub = nullptr;
    int rc;
    if ((rc = ix->call_scr[spx_index::PL_CUB].reserve(cub_bytes + 16, &cub)) != SPX_OK) return rc;
    return product_enqueue(ix->call_fin, FIN_WORDS, st, [&](void*) -> int {
        SPX_HIP(hipcub::DeviceScan::InclusiveSum(cub, cub_bytes, d_ddiff, d_del, G, st));
        return SPX_OK;
    });
}

// count without write: the tiles' counts and their scan only; write without count: the second half of the host form,
// which sizes its records from the count before it writes them
int calls_enqueue(spx_index* ix, CallArgs& a, hipStream_t st, bool count, bool write) {
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    a.t = table_of(ix);
    a.text = ix->text;
    a.ntiles = tiles_of(a.t.G);
    void* p = nullptr;
    int rc;
    if ((rc = ix->call_scr[spx_index::PL_TCNT].reserve((a.ntiles + 1) * 8, &p)) != SPX_OK) return rc;
    a.tcnt = (uint64_t*)p;
    if ((rc = ix->call_scr[spx_index::PL_TOFFS].reserve((a.ntiles + 1) * 8, &p)) != SPX_OK) return rc;
    a.toffs = (uint64_t*)p;
    size_t cub_bytes = 0;
    SPX_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, a.tcnt, a.toffs, a.ntiles + 1, (hipStream_t) nullptr));
    void* cub = nullptr;
    if ((rc = ix->call_scr[spx_index::PL_CUB2].reserve(cub_bytes + 16, &cub)) != SPX_OK) return rc;
    auto launch = [&](void* counters) -> int {
        a.c = (CallCounters*)counters;
        if (count) {
            k_call_count<<<(unsigned)a.ntiles, 256, 0, st>>>(a);
            SPX_HIP(hipGetLastError());
            SPX_HIP(hipcub::DeviceScan::ExclusiveSum(cub, cub_bytes, a.tcnt, a.toffs, a.ntiles + 1, st));
        }
        if (write) {
            k_call_write<<<(unsigned)a.ntiles, 256, 0, st>>>(a);
            SPX_HIP(hipGetLastError());
        }
        return SPX_OK;
    };
    if (count) return product_enqueue(ix->call_calls, CALL_WORDS, st, launch);
    // the second half of the host form: the same counters, the step's end moved behind the write
    if ((rc = launch(ix->call_calls.counters.p)) != SPX_OK) return rc;
    SPX_HIP(hipEventRecord(ix->call_calls.ev1, st));
    return SPX_OK;
}

// Waits for what a step enqueued last and takes its counters and its time.  Takes ix->mu.
int step_collect(spx_index* ix, spx_index::Product& p, int words, int step) {
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    SPX_HIP(hipEventSynchronize(p.ev1));
    unsigned long long c[ADD_WORDS] = {};
    SPX_HIP(hipMemcpy(c, p.counters.p, (size_t)words * 8, hipMemcpyDeviceToHost));
    SPX_HIP(hipEventElapsedTime(&ix->call_step_ms[step], p.ev0, p.ev1));
    if (step == 0)
        for (int i = 0; i < 8; ++i) ix->call_acc[i] += c[i];
    if (step == 2) ix->call_ncalls = c[0];
    p.error = step == 2 ? c[words - 1] : p.error | c[words - 1];
    p.pending = false;
    return SPX_OK;
}

int collect_all(spx_index* ix) {
    int rc;
    if (ix->call_add.pending && (rc = step_collect(ix, ix->call_add, ADD_WORDS, 0)) != SPX_OK) return rc;
    if (ix->call_fin.pending && (rc = step_collect(ix, ix->call_fin, FIN_WORDS, 1)) != SPX_OK) return rc;
    if (ix->call_calls.pending && (rc = step_collect(ix, ix->call_calls, CALL_WORDS, 2)) != SPX_OK) return rc;
    return SPX_OK;
}

int add_error_code(const spx_index* ix) {
    if (ix->call_add.error & 1) {
        set_error("a read failed the pileup's checks (the coverage's checks on its mapping, entries whose read lengths disagree with "
                  "the read's, an 'I' behind the last text column, or read offsets outside the reads): such a read adds nothing");
        return SPX_E_FORMAT;
    }
    return SPX_OK;
}

// The host forms' arrays are there and belong to the table in force.  The caller holds host_mu.
int need_arrays(spx_index* ix, const char* who) {
    int rc;
    if ((rc = need_table(ix, who)) != SPX_OK) return rc;
    if (ix->call_dropped) {
        set_error("%s: spn_set_sequences replaced the sequence table after spl_call_reset and dropped the pileup: reset again", who);
        return SPX_E_ARG;
    }
    if (!ix->call_G) {
        set_error("%s without a successful spl_call_reset before it", who);
        return SPX_E_ARG;
    }
    return cover_need_arrays(ix, who);
}

// del from the handle's ddiff, when something was added since it was made.  The caller holds host_mu.
int finish_host(spx_index* ix) {
    if (!ix->call_dirty) return SPX_OK;
    hipStream_t st = nullptr;
    int rc;
    if ((rc = ctx_stream_of(ix, &st)) != SPX_OK) return rc;
    if ((rc = finish_enqueue(ix, (const uint32_t*)ix->call_scr[spx_index::PL_DDIFF].p, (uint32_t*)ix->call_scr[spx_index::PL_DEL].p, st)) != SPX_OK)
        return rc;
    if ((rc = ctx_wait(ix, st)) != SPX_OK) return rc;
    if ((rc = step_collect(ix, ix->call_fin, FIN_WORDS, 1)) != SPX_OK) return rc;
    ix->call_dirty = false;
    return SPX_OK;
}

// exactly `bytes`: the arrays of a genome are not given the scratch buffers' head-room
int exact(spx_index::Scratch& sc, size_t bytes) {
    if (sc.cap >= bytes) return SPX_OK;
    if (sc.p) (void)hipFree(sc.p);
    sc.p = nullptr;
    sc.cap = 0;
    SPX_HIP(hipMalloc(&sc.p, bytes));
    sc.cap = bytes;
    return SPX_OK;
}

constexpr int ARRAYS[5] = {spx_index::PL_ALT, spx_index::PL_OTHER, spx_index::PL_INS, spx_index::PL_DDIFF, spx_index::PL_DEL};

void drop_arrays(spx_index* ix) {
    for (int i : {spx_index::PL_ALT, spx_index::PL_OTHER, spx_index::PL_INS, spx_index::PL_DDIFF, spx_index::PL_DEL, spx_index::PL_CALLS}) {
        spx_index::Scratch& sc = ix->call_scr[i];
        if (sc.p) (void)hipFree(sc.p);
        sc.p = nullptr;
        sc.cap = 0;
    }
    ix->call_G = 0;
    ix->call_ready = false;
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
    for (auto& sc : ix->call_scr)
        if (sc.p) (void)hipFree(sc.p);
    product_release(ix->call_add);
    product_release(ix->call_fin);
    product_release(ix->call_calls);
    if (ix->call_copy_ev) (void)hipEventDestroy(ix->call_copy_ev);
    if (ix->call_copy_s) (void)hipStreamDestroy(ix->call_copy_s);
}

int clone_call(spx_index* src, spx_index* ix) { return src->call_G ? spl_call_reset(ix) : SPX_OK; }

void call_table_changed(spx_index* ix) {
    // (a kernel of an earlier call may still read the old table or the arrays)
    for (spx_index::Product* p : {&ix->call_add, &ix->call_fin, &ix->call_calls})
        if (p->have && p->ev1) (void)hipEventSynchronize(p->ev1);  // (a reset sets `have` for the stats and creates no event)
    if (!ix->call_G) return;
    drop_arrays(ix);
    ix->call_dropped = true;
}

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
    add_reset(ix);
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
    return add_enqueue(ix, a, (hipStream_t)stream);
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
    return finish_enqueue(ix, d_ddiff, d_del, (hipStream_t)stream);
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
    a.calls = (uint4*)d_calls;
    a.count = d_count;
    return calls_enqueue(ix, a, (hipStream_t)stream, true, true);
}

int spl_call_reset(spx_index* ix) {
    int rc;
    if ((rc = need_table(ix, "spl_call_reset")) != SPX_OK) return rc;
    if ((rc = spd_cover_reset(ix)) != SPX_OK) return rc;
    std::lock_guard<std::mutex> hg(ix->host_mu);
    SPX_HIP(hipSetDevice(ix->device));
    const Table t = table_of(ix);
    const size_t bytes[5] = {(size_t)t.G * 16, (size_t)t.G * 4, (size_t)t.G * 4, (size_t)(t.G + 1) * 4, (size_t)t.G * 4};
    size_t need = 0;
    for (int i = 0; i < 5; ++i)
        if (ix->call_scr[ARRAYS[i]].cap < bytes[i]) need += bytes[i];
    size_t free_b = 0, total_b = 0;
    SPX_HIP(hipMemGetInfo(&free_b, &total_b));
    {
        std::lock_guard<std::mutex> g(ix->mu);
        if (need > free_b) {
            set_error("spl_call_reset: the pileup of %llu bases needs %llu more bytes of device memory (about 28 per base beside the "
                      "coverage's 12), %llu are free",
                      (unsigned long long)t.G, (unsigned long long)need, (unsigned long long)free_b);
            return SPX_E_UNSUPPORTED;
        }
        for (int i = 0; i < 5; ++i)
            if ((rc = exact(ix->call_scr[ARRAYS[i]], bytes[i])) != SPX_OK) {
                drop_arrays(ix);
                return rc;
            }
    }
    hipStream_t st = nullptr;
    if ((rc = ctx_stream_of(ix, &st)) != SPX_OK) return rc;
    for (int i = 0; i < 4; ++i) SPX_HIP(hipMemsetAsync(ix->call_scr[ARRAYS[i]].p, 0, bytes[i], st));
    if ((rc = ctx_wait(ix, st)) != SPX_OK) return rc;
    add_reset(ix);
    ix->call_G = t.G;
    ix->call_dropped = false;
    ix->call_dirty = true;
    ix->call_ready = false;
    ix->call_add.have = true;  // (the stats of no adds are zeros)
    return SPX_OK;
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
        if ((rc = need_arrays(ix, "spl_call_add_batch")) != SPX_OK) return rc;
        bool sorted = seqs && offsets && nreads;
        for (uint64_t q = 0; sorted && q < nreads; ++q) sorted = offsets[q] <= offsets[q + 1];
        if (sorted) {
            chars = offsets[nreads] - offsets[0];
            rel.resize(nreads + 1);
            for (uint64_t q = 0; q <= nreads; ++q) rel[q] = offsets[q] - offsets[0];
            std::lock_guard<std::mutex> g(ix->mu);
            SPX_HIP(hipSetDevice(ix->device));
            if ((rc = ix->call_scr[spx_index::PL_READS].reserve(chars + 16, &d_reads)) != SPX_OK) return rc;
            if ((rc = ix->call_scr[spx_index::PL_ROFFS].reserve((nreads + 1) * 8, &d_roffs)) != SPX_OK) return rc;
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
                                  if ((rc2 = need_arrays(ix, "spl_call_add_batch")) != SPX_OK) return rc2;
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
                                  a.alt = (uint32_t*)ix->call_scr[spx_index::PL_ALT].p;
                                  a.other = (uint32_t*)ix->call_scr[spx_index::PL_OTHER].p;
                                  a.ins = (uint32_t*)ix->call_scr[spx_index::PL_INS].p;
                                  a.ddiff = (uint32_t*)ix->call_scr[spx_index::PL_DDIFF].p;
                                  ix->call_dirty = true;
                                  ix->call_ready = false;
                                  return add_enqueue(ix, a, b.stream);
                              });
    std::lock_guard<std::mutex> hg(ix->host_mu);
    if (ix->call_add.pending) {  // (enqueued: the coverage's wait may or may not have come behind it)
        const int rc2 = step_collect(ix, ix->call_add, ADD_WORDS, 0);
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
    if ((rc = need_arrays(ix, "spl_calls_begin")) != SPX_OK) return rc;
    if ((rc = check_params(min_depth, min_alt, min_permille)) != SPX_OK) return rc;
    SPX_HIP(hipSetDevice(ix->device));
    ix->call_ready = false;
    if ((rc = cover_finish_host(ix)) != SPX_OK) return rc;
    if ((rc = finish_host(ix)) != SPX_OK) return rc;
    hipStream_t st = nullptr;
    if ((rc = ctx_stream_of(ix, &st)) != SPX_OK) return rc;
    void* d_n = nullptr;
    if ((rc = ix->call_scr[spx_index::PL_NCALLS].reserve(8, &d_n)) != SPX_OK) return rc;
    CallArgs a{};
    a.depth = (const uint32_t*)ix->cover_scr[spx_index::D_DEPTH].p;
    a.alt = (const uint4*)ix->call_scr[spx_index::PL_ALT].p;
    a.other = (const uint32_t*)ix->call_scr[spx_index::PL_OTHER].p;
    a.ins = (const uint32_t*)ix->call_scr[spx_index::PL_INS].p;
    a.del = (const uint32_t*)ix->call_scr[spx_index::PL_DEL].p;
    a.min_depth = min_depth;
    a.min_alt = min_alt;
    a.min_permille = min_permille;
    a.count = (uint64_t*)d_n;
    // count, the one wait of the calls' own, the records at their exact size, write
    if ((rc = calls_enqueue(ix, a, st, true, false)) != SPX_OK) return rc;
    if ((rc = ctx_wait(ix, st)) != SPX_OK) return rc;
    uint64_t total = 0;
    SPX_HIP(hipMemcpy(&total, a.toffs + a.ntiles, 8, hipMemcpyDeviceToHost));
    void* d_calls = nullptr;
    if ((rc = ix->call_scr[spx_index::PL_CALLS].reserve(total * sizeof(spl_call) + 48, &d_calls)) != SPX_OK) return rc;
    a.calls = (uint4*)d_calls;
    a.cap = total;
    if ((rc = calls_enqueue(ix, a, st, false, true)) != SPX_OK) return rc;
    if ((rc = ctx_wait(ix, st)) != SPX_OK) return rc;
    if ((rc = step_collect(ix, ix->call_calls, CALL_WORDS, 2)) != SPX_OK) return rc;
    ix->call_ready = true;
    ix->call_ready_n = total;
    *n_calls = total;
    return SPX_OK;
}

int spl_calls_fetch(spx_index* ix, spl_call* out_calls) {
    if (!ix) {
        set_error("index must be non-null");
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> hg(ix->host_mu);
    if (!ix->call_ready) {
        set_error("spl_calls_fetch without a successful spl_calls_begin before it");
        return SPX_E_ARG;
    }
    if (ix->call_ready_n && !out_calls) {
        set_error("out_calls must be non-null");
        return SPX_E_ARG;
    }
    ix->call_ready = false;
    if (!ix->call_ready_n) return SPX_OK;
    SPX_HIP(hipSetDevice(ix->device));
    SPX_HIP(hipMemcpy(out_calls, ix->call_scr[spx_index::PL_CALLS].p, ix->call_ready_n * sizeof(spl_call), hipMemcpyDeviceToHost));
    return SPX_OK;
}

int spl_pileup_counts(spx_index* ix, uint64_t first, uint64_t count, uint32_t* out_alt, uint32_t* out_other, uint32_t* out_ins,
                      uint32_t* out_del) {
    if (!ix) {
        set_error("index must be non-null");
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> hg(ix->host_mu);
    int rc;
    if ((rc = need_arrays(ix, "spl_pileup_counts")) != SPX_OK) return rc;
    if (first > ix->call_G || count > ix->call_G - first) {
        set_error("spl_pileup_counts: [%llu, %llu + %llu) does not lie in the forward genome of %llu bases", (unsigned long long)first,
                  (unsigned long long)first, (unsigned long long)count, (unsigned long long)ix->call_G);
        return SPX_E_ARG;
    }
    SPX_HIP(hipSetDevice(ix->device));
    if ((rc = finish_host(ix)) != SPX_OK) return rc;
    if (!count) return SPX_OK;
    uint32_t* const out[4] = {out_alt, out_other, out_ins, out_del};
    const int slot[4] = {spx_index::PL_ALT, spx_index::PL_OTHER, spx_index::PL_INS, spx_index::PL_DEL};
    for (int i = 0; i < 4; ++i) {
        const uint64_t per = i == 0 ? 4 : 1;
        if (out[i])
            SPX_HIP(hipMemcpy(out[i], (const uint32_t*)ix->call_scr[slot[i]].p + first * per, count * per * 4, hipMemcpyDeviceToHost));
    }
    return SPX_OK;
}

int spl_last_call_stats(spx_index* ix, spl_call_stats* out) {
    if (!ix || !out) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    if (!ix->call_add.have && !ix->call_fin.have && !ix->call_calls.have) {
        set_error("no pileup has been computed on this index yet");
        return SPX_E_ARG;
    }
    const int rc = collect_all(ix);
    if (rc != SPX_OK) return rc;
    std::memset(out, 0, sizeof *out);
    out->reads = ix->call_acc[0];
    out->mapped = ix->call_acc[1];
    out->added = ix->call_acc[2];
    out->skipped = ix->call_acc[3];
    out->x_columns = ix->call_acc[4];
    out->other_columns = ix->call_acc[5];
    out->insertions = ix->call_acc[6];
    out->deletions = ix->call_acc[7];
    out->atomics = out->x_columns + out->insertions + 2 * out->deletions;
    out->calls = ix->call_ncalls;
    out->error = (uint32_t)(ix->call_add.error & 1);
    out->overflow = (uint32_t)((ix->call_calls.error >> 1) & 1);
    for (int i = 0; i < 3; ++i) out->step_ms[i] = ix->call_step_ms[i];
    return add_error_code(ix);
}

}  // extern "C"
