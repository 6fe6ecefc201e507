// spx_docvote.hip -- the document votes (include/spumoni_docvote.h): per read, which document most of
// its voting positions name, how many named it, and how many named the runner-up.
//
// Input are the per-position lengths and document ids a query left in device memory; a position votes when its length
// is at least min_length.  There may be 10^7 reads in a batch and 65536 documents, so nothing here is sized by the
// number of documents: every path counts the DISTINCT ids of what it looks at in an open-addressing table (id, count)
// whose size follows the number of values.  Counts are exact whatever lane or workgroup counted what, and the winner
// is the maximum of (count, ~id) -- the smallest id among equals -- so the records do not depend on any order.
//
//   k_votes_short   every read passes through it, 16 lanes per read (four reads per wavefront): lane j loads the j-th
//                   aligned 16-byte vector of the read's lengths and of its ids.  A read of <= 64 values that 16 vectors
//                   cover is counted there, in a 128-slot table of the group's own in LDS; a read without values gets
//                   its record; the others are put on the medium or the long list (the binning: on the device, in the
//                   same pass).
//   k_votes_medium  a workgroup per read of <= MEDIUM_MAX values, table of >= 2 m slots (<= 32 KiB) in LDS.
//   k_long_*        a read beyond that is cut into tiles of MEDIUM_MAX values, a workgroup per tile: the tile is counted
//                   in LDS as above, its distinct (id, count) pairs are added to a table of 2 m slots of the read's own
//                   in device scratch, and the tiles then scan that table for the maximum and, the winner known, for
//                   the runner-up (atomicMax on a word per read).  Work O(m) expected, spread over m / MEDIUM_MAX
//                   workgroups.
// The lists' fill is only known on the device: the kernels behind k_votes_short are launched with fixed grids and loop
// over what the counters say.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/spumoni_docvote.h"
#include "spx_internal.h"

namespace spx {
namespace {

constexpr uint32_t EMPTY = 0xFFFFFFFFu;
constexpr uint32_t MEDIUM_MAX = 2048;           // values a workgroup counts in LDS: 4096 slots of 8 bytes
constexpr uint32_t MEDIUM_SLOTS = 2 * MEDIUM_MAX;
constexpr uint32_t SHORT_MAX = 64, SHORT_SLOTS = 128, GROUP = 16;
constexpr uint64_t BAD_ENTRY = ~0ull;

struct VoteCounters {  // device; zeroed in front of every launch
    unsigned long long reads_short, reads_medium, reads_long, reads_empty, voting, tiles;
    unsigned long long n_medium, n_long, n_tiles, table_used;  // fill of the lists; values the long reads' tables are for
    unsigned long long error;  // bit 0: a read of 2^32 values or more; bit 1: the batch holds more than total_values said
};
constexpr int VOTE_WORDS = sizeof(VoteCounters) / 8;  // (the first six are what spv_votes_stats reports, the last the error)
struct LongAcc {  // 32 B per long read
    unsigned long long top;  // max of (count << 32 | ~id)
    unsigned int voters, second;
    unsigned long long table;  // first value slot pair of the read's table
    unsigned long long pad_;
};
struct VoteArgs {
    const uint4* L;
    const uint4* D;
    const uint64_t* offs;
    uint64_t nreads, min_length;
    uint4* out;
    VoteCounters* c;
    uint64_t* medium_list;
    uint64_t medium_cap;
    uint64_t* long_list;
    uint64_t long_cap;
    uint64_t* tile_list;  // long-list index << 24 | tile
    uint64_t tile_cap;
    LongAcc* acc;
    uint4* table;  // two (id, count) slots per uint4
    uint64_t table_cap;  // in values: 2 slots each
};

__device__ inline uint64_t min64(uint64_t x, uint64_t y) { return x < y ? x : y; }
__device__ inline uint32_t hash_id(uint32_t id) { return id * 2654435761u; }
__device__ inline unsigned long long pack_top(uint32_t count, uint32_t id) {
    return count ? ((unsigned long long)count << 32) | (uint32_t)(~id) : 0ull;
}
__device__ inline uint4 record_of(unsigned long long top, uint32_t voters, uint32_t second) {
    const uint32_t votes = (uint32_t)(top >> 32);
    return make_uint4(voters, votes ? ~(uint32_t)top : SPV_NO_DOC, votes, second);
}

// the voting values of one aligned 16-byte vector, restricted to positions [lo, hi): f(id) for each
template <int BITS, typename F>
__device__ inline void vector_votes(const VoteArgs& a, uint64_t c, uint64_t lo, uint64_t hi, F&& f) {
    constexpr int V = BITS == 16 ? 8 : 4;
    const uint4 l = a.L[c], d = a.D[c];
    const uint32_t lw[4] = {l.x, l.y, l.z, l.w}, dw[4] = {d.x, d.y, d.z, d.w};
    const uint64_t i0 = c * V;
#pragma unroll
    for (int t = 0; t < V; ++t) {
        const uint32_t lv = BITS == 16 ? (lw[t >> 1] >> ((t & 1) * 16)) & 0xffffu : lw[t];
        const uint32_t dv = BITS == 16 ? (dw[t >> 1] >> ((t & 1) * 16)) & 0xffffu : dw[t];
        const uint64_t i = i0 + t;
        if (i >= lo && i < hi && (uint64_t)lv >= a.min_length) f(dv);
    }
}

// open addressing, linear probing; `shift` = 32 - log2(slots).  The tables are never more than half full.
__device__ inline void lds_add(uint32_t* keys, uint32_t* cnts, uint32_t mask, int shift, uint32_t id, uint32_t n) {
    uint32_t h = hash_id(id) >> shift;
    for (;;) {
        const uint32_t prev = atomicCAS(&keys[h], EMPTY, id);
        if (prev == EMPTY || prev == id) {
            atomicAdd(&cnts[h], n);
            return;
        }
        h = (h + 1) & mask;
    }
}

__device__ inline unsigned long long wave_max64(unsigned long long v, int width) {
    for (int s = width >> 1; s > 0; s >>= 1) {
        const unsigned long long o = __shfl_xor(v, s, width);
        v = o > v ? o : v;
    }
    return v;
}
__device__ inline uint32_t wave_max32(uint32_t v, int width) {
    for (int s = width >> 1; s > 0; s >>= 1) v = max(v, (uint32_t)__shfl_xor(v, s, width));
    return v;
}
__device__ inline unsigned long long wave_sum64(unsigned long long v, int width) {
    for (int s = width >> 1; s > 0; s >>= 1) v += __shfl_xor(v, s, width);
    return v;
}
// over the 256 threads of a block; red: 4 words of LDS.  Every thread gets the result.
template <bool SUM>
__device__ inline unsigned long long block_reduce64(unsigned long long v, unsigned long long* red) {
    v = SUM ? wave_sum64(v, 64) : wave_max64(v, 64);
    __syncthreads();  // (red may still be read from the reduction before)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const unsigned long long a = red[0], b = red[1], c = red[2], d = red[3];
    return SUM ? a + b + c + d : max(max(a, b), max(c, d));
}
// one atomic per wavefront
__device__ inline void wave_count(unsigned long long* dst, unsigned long long v) {
    v = wave_sum64(v, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}

// ---- short reads, empty reads, and the binning of the rest ------------------------------------------------------------
template <int BITS>
__global__ __launch_bounds__(256) void k_votes_short(VoteArgs a) {
    constexpr int V = BITS == 16 ? 8 : 4;
    __shared__ uint32_t s_keys[256 / GROUP][SHORT_SLOTS];
    __shared__ uint32_t s_cnts[256 / GROUP][SHORT_SLOTS];
    const uint32_t gl = threadIdx.x & (GROUP - 1), grp = threadIdx.x / GROUP;
    uint32_t* keys = s_keys[grp];
    uint32_t* cnts = s_cnts[grp];
    constexpr int SHIFT = 32 - 7;  // SHORT_SLOTS = 128
    unsigned long long n_short = 0, n_empty = 0, n_voting = 0;
    // (the trip count depends on the block alone: the barriers below are reached by every thread)
    for (uint64_t first = (uint64_t)blockIdx.x * (256 / GROUP); first < a.nreads; first += (uint64_t)gridDim.x * (256 / GROUP)) {
        const uint64_t q = first + grp;
        const bool active = q < a.nreads;
        const uint64_t o = active ? a.offs[q] : 0, e = active ? a.offs[q + 1] : 0;
        const uint64_t m = e - o;
        const bool sane = active && e >= o && m < (1ull << 32);
        const uint64_t c0 = o / V, c1 = m ? (e - 1) / V : c0;
        const bool is_short = sane && m >= 1 && m <= SHORT_MAX && c1 - c0 < GROUP;
        if (active && !is_short && gl == 0) {
            if (!sane) {
                atomicOr(&a.c->error, 1ull);
                a.out[q] = record_of(0, 0, 0);
            } else if (m == 0) {
                a.out[q] = record_of(0, 0, 0);
                n_empty++;
            } else if (m <= MEDIUM_MAX) {
                const unsigned long long at = atomicAdd(&a.c->n_medium, 1ull);
                if (at < a.medium_cap)
                    a.medium_list[at] = q;
                else
                    atomicOr(&a.c->error, 2ull);
            } else {
                const uint64_t nt = (m + MEDIUM_MAX - 1) / MEDIUM_MAX;
                const unsigned long long li = atomicAdd(&a.c->n_long, 1ull);
                const unsigned long long tb = atomicAdd(&a.c->n_tiles, (unsigned long long)nt);
                const unsigned long long tab = atomicAdd(&a.c->table_used, (unsigned long long)m);
                const bool ok = li < a.long_cap && tb + nt <= a.tile_cap && tab + m <= a.table_cap;
                if (!ok) atomicOr(&a.c->error, 2ull);
                if (li < a.long_cap) {
                    a.long_list[li] = ok ? q : BAD_ENTRY;
                    LongAcc z;
                    z.top = 0;
                    z.voters = z.second = 0;
                    z.table = tab;
                    z.pad_ = 0;
                    a.acc[li] = z;
                }
                for (uint64_t t = 0; t < nt && tb + t < a.tile_cap; ++t) a.tile_list[tb + t] = ok ? (li << 24) | t : BAD_ENTRY;
            }
        }
        for (uint32_t s = gl; s < SHORT_SLOTS; s += GROUP) {
            keys[s] = EMPTY;
            cnts[s] = 0;
        }
        __syncthreads();
        uint32_t mine = 0;
        if (is_short && c0 + gl <= c1)
            vector_votes<BITS>(a, c0 + gl, o, e, [&](uint32_t id) {
                lds_add(keys, cnts, SHORT_SLOTS - 1, SHIFT, id, 1);
                ++mine;
            });
        __syncthreads();
        unsigned long long best = 0;
        for (uint32_t s = gl; s < SHORT_SLOTS; s += GROUP) best = max(best, pack_top(cnts[s], keys[s]));
        best = wave_max64(best, GROUP);
        const uint32_t top_id = ~(uint32_t)best;
        uint32_t second = 0;
        for (uint32_t s = gl; s < SHORT_SLOTS; s += GROUP)
            if (keys[s] != top_id) second = max(second, cnts[s]);
        second = wave_max32(second, GROUP);
        const uint32_t voters = (uint32_t)wave_sum64(mine, GROUP);
        if (is_short && gl == 0) {
            a.out[q] = record_of(best, voters, second);
            n_short++;
            n_voting += voters;
        }
        __syncthreads();  // (the tables are cleared again at the top)
    }
    wave_count(&a.c->reads_short, n_short);
    wave_count(&a.c->reads_empty, n_empty);
    wave_count(&a.c->voting, n_voting);
}

// A workgroup counts the voting values of positions [lo, hi) (at most MEDIUM_MAX) in its LDS table of 1 << lg slots.
template <int BITS>
__device__ inline void block_tally(const VoteArgs& a, uint64_t lo, uint64_t hi, uint32_t* keys, uint32_t* cnts, int lg) {
    constexpr int V = BITS == 16 ? 8 : 4;
    const uint32_t slots = 1u << lg;
    __syncthreads();  // (the table may still be read for the read before)
    for (uint32_t s = threadIdx.x; s < slots; s += 256) {
        keys[s] = EMPTY;
        cnts[s] = 0;
    }
    __syncthreads();
    for (uint64_t c = lo / V + threadIdx.x, c1 = (hi - 1) / V; c <= c1; c += 256)
        vector_votes<BITS>(a, c, lo, hi, [&](uint32_t id) { lds_add(keys, cnts, slots - 1, 32 - lg, id, 1); });
    __syncthreads();
}
__device__ inline int table_log2(uint64_t m) {  // smallest table of >= 256 slots that m values fill to half at most
    int lg = 8;
    while ((1ull << lg) < 2 * m) ++lg;
    return lg;
}

template <int BITS>
__global__ __launch_bounds__(256) void k_votes_medium(VoteArgs a) {
    __shared__ uint32_t s_keys[MEDIUM_SLOTS];
    __shared__ uint32_t s_cnts[MEDIUM_SLOTS];
    __shared__ unsigned long long s_red[4];
    const uint64_t n = min64((uint64_t)a.c->n_medium, a.medium_cap);
    unsigned long long n_reads = 0, n_voting = 0;
    for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint64_t q = a.medium_list[i];
        const uint64_t o = a.offs[q], e = a.offs[q + 1];
        const int lg = table_log2(e - o);
        block_tally<BITS>(a, o, e, s_keys, s_cnts, lg);
        unsigned long long best = 0, sum = 0;
        for (uint32_t s = threadIdx.x; s < (1u << lg); s += 256) {
            best = max(best, pack_top(s_cnts[s], s_keys[s]));
            sum += s_cnts[s];
        }
        best = block_reduce64<false>(best, s_red);
        sum = block_reduce64<true>(sum, s_red);
        const uint32_t top_id = ~(uint32_t)best;
        unsigned long long second = 0;
        for (uint32_t s = threadIdx.x; s < (1u << lg); s += 256)
            if (s_keys[s] != top_id) second = max(second, (unsigned long long)s_cnts[s]);
        second = block_reduce64<false>(second, s_red);
        if (threadIdx.x == 0) {
            a.out[q] = record_of(best, (uint32_t)sum, (uint32_t)second);
            n_reads++;
            n_voting += sum;
        }
    }
    if (threadIdx.x == 0 && n_reads) {
        atomicAdd(&a.c->reads_medium, n_reads);
        atomicAdd(&a.c->voting, n_voting);
    }
}

// ---- long reads: a workgroup per tile of MEDIUM_MAX values ----------------------------------------------------------
struct Tile {
    bool ok;
    uint64_t li, lo, hi;     // long-list index; the tile's positions
    uint64_t share;          // first uint4 of the tile's share of the read's table (one uint4 = 2 slots per value)
    uint64_t table, slots;   // the read's table: first slot, number of slots (2 per value, < 2^32)
};
__device__ inline Tile tile_of(const VoteArgs& a, uint64_t entry) {
    Tile t{};
    if (entry == BAD_ENTRY) return t;
    t.li = entry >> 24;
    const uint64_t k = entry & 0xFFFFFFull;
    const uint64_t q = a.long_list[t.li];
    const uint64_t o = a.offs[q], e = a.offs[q + 1];
    t.lo = o + k * MEDIUM_MAX;
    t.hi = min64(e, t.lo + MEDIUM_MAX);
    const uint64_t tab = a.acc[t.li].table;
    t.share = tab + k * MEDIUM_MAX;
    t.table = 2 * tab;
    t.slots = min64(2 * (e - o), 0xFFFFFFFFull);
    t.ok = true;
    return t;
}
__global__ __launch_bounds__(256) void k_long_clear(VoteArgs a) {
    const uint64_t n = min64((uint64_t)a.c->n_tiles, a.tile_cap);
    for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const Tile t = tile_of(a, a.tile_list[i]);
        if (!t.ok) continue;
        for (uint64_t v = threadIdx.x; v < t.hi - t.lo; v += 256) a.table[t.share + v] = make_uint4(EMPTY, 0, EMPTY, 0);
    }
}
template <int BITS>
__global__ __launch_bounds__(256) void k_long_tally(VoteArgs a) {
    __shared__ uint32_t s_keys[MEDIUM_SLOTS];
    __shared__ uint32_t s_cnts[MEDIUM_SLOTS];
    const uint64_t n = min64((uint64_t)a.c->n_tiles, a.tile_cap);
    uint32_t* g = reinterpret_cast<uint32_t*>(a.table);
    for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const Tile t = tile_of(a, a.tile_list[i]);
        if (!t.ok) continue;  // (the same for every thread of the block)
        block_tally<BITS>(a, t.lo, t.hi, s_keys, s_cnts, 12);
        for (uint32_t s = threadIdx.x; s < MEDIUM_SLOTS; s += 256) {
            const uint32_t cnt = s_cnts[s], id = s_keys[s];
            if (!cnt) continue;
            uint64_t h = ((uint64_t)hash_id(id) * t.slots) >> 32;
            for (;;) {
                uint32_t* slot = g + 2 * (t.table + h);
                const uint32_t prev = atomicCAS(slot, EMPTY, id);
                if (prev == EMPTY || prev == id) {
                    atomicAdd(slot + 1, cnt);
                    break;
                }
                h = h + 1 == t.slots ? 0 : h + 1;
            }
        }
    }
}
// pass 0: the maximum and the voters; pass 1 (the winner known): the runner-up
template <int PASS>
__global__ __launch_bounds__(256) void k_long_scan(VoteArgs a) {
    __shared__ unsigned long long s_red[4];
    const uint64_t n = min64((uint64_t)a.c->n_tiles, a.tile_cap);
    for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const Tile t = tile_of(a, a.tile_list[i]);
        if (!t.ok) continue;
        const uint32_t top_id = PASS ? ~(uint32_t)a.acc[t.li].top : 0;
        unsigned long long best = 0, sum = 0;
        for (uint64_t v = threadIdx.x; v < t.hi - t.lo; v += 256) {
            const uint4 s = a.table[t.share + v];
            if (PASS == 0) {
                best = max(best, max(pack_top(s.y, s.x), pack_top(s.w, s.z)));
                sum += s.y + s.w;
            } else {
                if (s.x != top_id) best = max(best, (unsigned long long)s.y);
                if (s.z != top_id) best = max(best, (unsigned long long)s.w);
            }
        }
        best = block_reduce64<false>(best, s_red);
        if (PASS == 0) sum = block_reduce64<true>(sum, s_red);
        if (threadIdx.x == 0) {
            if (PASS == 0) {
                if (best) atomicMax(&a.acc[t.li].top, best);
                if (sum) atomicAdd(&a.acc[t.li].voters, (unsigned int)sum);
            } else if (best) {
                atomicMax(&a.acc[t.li].second, (unsigned int)best);
            }
        }
    }
}
__global__ __launch_bounds__(256) void k_long_write(VoteArgs a) {
    const uint64_t n = min64((uint64_t)a.c->n_long, a.long_cap);
    unsigned long long n_reads = 0, n_voting = 0;
    for (uint64_t li = (uint64_t)blockIdx.x * 256 + threadIdx.x; li < n; li += (uint64_t)gridDim.x * 256) {
        const uint64_t q = a.long_list[li];
        if (q == BAD_ENTRY) continue;
        const LongAcc r = a.acc[li];
        a.out[q] = record_of(r.top, r.voters, r.second);
        n_reads++;
        n_voting += r.voters;
    }
    wave_count(&a.c->reads_long, n_reads);
    wave_count(&a.c->voting, n_voting);
    if (blockIdx.x == 0 && threadIdx.x == 0) a.c->tiles = min64((uint64_t)a.c->n_tiles, a.tile_cap);
}

// Enqueues the vote kernels on st.  long_values: an upper bound of the values in reads longer than MEDIUM_MAX (it sizes
// their tables: 16 bytes per value).  Takes ix->mu.
int votes_enqueue(spx_index* ix, const void* d_lengths, const void* d_docs, int value_bits, const uint64_t* d_offsets,
                  uint64_t nreads, uint64_t total_values, uint64_t long_values, uint64_t min_length, spv_vote* d_out,
                  hipStream_t st) {
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    VoteArgs a{};
    a.L = (const uint4*)d_lengths;
    a.D = (const uint4*)d_docs;
    a.offs = d_offsets;
    a.nreads = nreads;
    a.min_length = min_length;
    a.out = (uint4*)d_out;
    // a medium read has more than 61 values, a long one more than MEDIUM_MAX, and is cut into at most 2 m / MEDIUM_MAX tiles
    a.medium_cap = total_values / 32 + 1;
    a.long_cap = total_values > MEDIUM_MAX ? total_values / MEDIUM_MAX + 1 : 0;
    a.tile_cap = 2 * a.long_cap;
    a.table_cap = a.long_cap ? std::min(long_values, total_values) : 0;
    void* p = nullptr;
    int rc;
    if ((rc = ix->vote_scr[spx_index::V_MEDIUM].reserve(a.medium_cap * 8, &p)) != SPX_OK) return rc;
    a.medium_list = (uint64_t*)p;
    if ((rc = ix->vote_scr[spx_index::V_LONG].reserve(a.long_cap * 8, &p)) != SPX_OK) return rc;
    a.long_list = (uint64_t*)p;
    if ((rc = ix->vote_scr[spx_index::V_TILES].reserve(a.tile_cap * 8, &p)) != SPX_OK) return rc;
    a.tile_list = (uint64_t*)p;
    if ((rc = ix->vote_scr[spx_index::V_ACC].reserve(a.long_cap * sizeof(LongAcc), &p)) != SPX_OK) return rc;
    a.acc = (LongAcc*)p;
    if ((rc = ix->vote_scr[spx_index::V_TABLE].reserve(a.table_cap * 16, &p)) != SPX_OK) return rc;
    a.table = (uint4*)p;
    return product_enqueue(ix->votes, VOTE_WORDS, st, [&](void* counters) -> int {
        a.c = (VoteCounters*)counters;
        if (!nreads) return SPX_OK;
        const unsigned short_grid = (unsigned)std::min<uint64_t>((nreads + 15) / 16, 2048);
        const unsigned medium_grid = (unsigned)std::min<uint64_t>(a.medium_cap, 1280);
        if (value_bits == 16) {
            k_votes_short<16><<<short_grid, 256, 0, st>>>(a);
            k_votes_medium<16><<<medium_grid, 256, 0, st>>>(a);
        } else {
            k_votes_short<32><<<short_grid, 256, 0, st>>>(a);
            k_votes_medium<32><<<medium_grid, 256, 0, st>>>(a);
        }
        if (a.long_cap) {
            const unsigned tile_grid = (unsigned)std::min<uint64_t>(a.tile_cap, 1024);
            k_long_clear<<<tile_grid, 256, 0, st>>>(a);
            if (value_bits == 16)
                k_long_tally<16><<<tile_grid, 256, 0, st>>>(a);
            else
                k_long_tally<32><<<tile_grid, 256, 0, st>>>(a);
            k_long_scan<0><<<tile_grid, 256, 0, st>>>(a);
            k_long_scan<1><<<tile_grid, 256, 0, st>>>(a);
            k_long_write<<<(unsigned)std::min<uint64_t>((a.long_cap + 255) / 256, 64), 256, 0, st>>>(a);
        }
        SPX_HIP(hipGetLastError());
        return SPX_OK;
    });
}
int vote_error_code(const spx_index* ix) {
    if (ix->votes.error & 1) {
        set_error("a read has 2^32 values or more (or its offsets decrease): the votes take reads below that");
        return SPX_E_FORMAT;
    }
    if (ix->votes.error & 2) {
        set_error("the batch holds more values than total_values said: the records are undefined");
        return SPX_E_FORMAT;
    }
    return SPX_OK;
}

int check_index(const spx_index* ix) {
    if (!ix) {
        set_error("index must be non-null");
        return SPX_E_ARG;
    }
    if (!ix->has_docs) {
        set_error("the index has no document array: there are no document ids to vote with");
        return SPX_E_ARG;
    }
    return SPX_OK;
}

}  // namespace

void release_votes(spx_index* ix) { release(ix->vote_scr, spx_index::V_COUNT, &ix->votes); }

}  // namespace spx

using namespace spx;

extern "C" {

int spv_votes_device(spx_index* ix, const void* d_lengths, const void* d_docs, int value_bits, const uint64_t* d_offsets,
                     uint64_t nreads, uint64_t total_values, uint64_t min_length, spv_vote* d_out, void* stream) {
    int rc = check_index(ix);
    if (rc != SPX_OK) return rc;
    if (value_bits != 16 && value_bits != 32) {
        set_error("value_bits must be 16 or 32 (the width of d_lengths and d_docs)");
        return SPX_E_ARG;
    }
    if (nreads && (!d_lengths || !d_docs || !d_offsets || !d_out)) {
        set_error("d_lengths, d_docs, d_offsets and d_out must be non-null");
        return SPX_E_ARG;
    }
    if ((((uintptr_t)d_lengths | (uintptr_t)d_docs | (uintptr_t)d_out) & 15) != 0 || ((uintptr_t)d_offsets & 7) != 0) {
        set_error("d_lengths, d_docs and d_out must be 16-byte aligned (the values are read as 16-byte vectors)");
        return SPX_E_ARG;
    }
    product_reset(ix, ix->votes);
    return votes_enqueue(ix, d_lengths, d_docs, value_bits, d_offsets, nreads, total_values, total_values, min_length, d_out,
                         (hipStream_t)stream);
}

int spv_last_votes_stats(spx_index* ix, spv_votes_stats* out) {
    if (!ix || !out) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    if (!ix->votes.have) {
        set_error("no votes have been computed on this index yet");
        return SPX_E_ARG;
    }
    if (ix->votes.pending) {
        const int rc = product_collect(ix, ix->votes, VOTE_WORDS, 6);
        if (rc != SPX_OK) return rc;
    }
    out->reads_short = ix->votes.acc[0];
    out->reads_medium = ix->votes.acc[1];
    out->reads_long = ix->votes.acc[2];
    out->reads_empty = ix->votes.acc[3];
    out->voting_positions = ix->votes.acc[4];
    out->long_tiles = ix->votes.acc[5];
    out->kernel_ms = ix->votes.ms;
    return vote_error_code(ix);
}

// The staged walk (spx_stage.hip) with the vote kernels behind every piece's walk.
int spv_assign_batch(spx_index* ix, int mode, int digest_kind, uint32_t k, uint32_t w, const uint8_t* seqs,
                     const uint64_t* offsets, uint64_t nreads, uint64_t min_length, spv_vote* out, uint64_t* out_values) {
    if (spx_device_count() <= 0) {
        set_error("no HIP device visible: the document votes run on the GPU and have no CPU fallback");
        return SPX_E_NODEVICE;
    }
    int rc = check_index(ix);
    if (rc != SPX_OK) return rc;
    if (mode != SPX_MODE_PML && mode != SPX_MODE_MS) {
        set_error("mode must be SPX_MODE_PML or SPX_MODE_MS");
        return SPX_E_ARG;
    }
    if ((rc = check_digest_kind(digest_kind)) != SPX_OK) return rc;
    if (mode == SPX_MODE_MS && (!ix->has_samples || !ix->text)) {
        set_error("MS mode needs an index built with SA samples and the text (spx_index_set_text / spx_index_rebuild_text): "
                  "the votes go by the MS lengths");
        return SPX_E_ARG;
    }
    if (nreads && (!seqs || !offsets || !out)) {
        set_error("seqs, offsets and out must be non-null");
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> hg(ix->host_mu);
    SPX_HIP(hipSetDevice(ix->device));
    product_reset(ix, ix->votes);
    if (nreads == 0) return SPX_OK;
    StageJob job;
    job.mode = mode;
    job.digest_kind = digest_kind;
    job.k = k;
    job.w = w;
    job.seqs = seqs;
    job.offsets = offsets;
    job.nreads = nreads;
    job.out_values = out_values;
    job.want_docs = true;
    StagePlan plan;
    if ((rc = stage_streams(ix, job.streams)) != SPX_OK) return rc;
    if ((rc = stage_plan(ix, job, &plan)) != SPX_OK) return rc;
    void* d_out[2] = {};
    for (int b = 0; b < plan.sets; ++b)
        if ((rc = ix->vote_scr[spx_index::V_OUT0 + b].reserve((plan.worst_reads + 1) * sizeof(spv_vote), &d_out[b])) != SPX_OK) return rc;
    job.wait = [](hipStream_t st) -> int {
        SPX_HIP(hipStreamSynchronize(st));
        return SPX_OK;
    };
    job.enqueue = [&](const StageView& v) -> int {
        // what the piece's long reads hold (a digestion only shortens them): the size of their tables
        uint64_t piece_long_values = 0;
        for (uint64_t q = v.q0; q < v.q0 + v.nreads; ++q)
            if (offsets[q + 1] - offsets[q] > MEDIUM_MAX) piece_long_values += offsets[q + 1] - offsets[q];
        const int r = votes_enqueue(ix, v.lengths, v.docs, v.value_bits, v.offs, v.nreads, v.total_values, piece_long_values, min_length,
                                    (spv_vote*)d_out[v.set], v.stream);
        if (r != SPX_OK) return r;
        SPX_HIP(hipMemcpyAsync(out + v.q0, d_out[v.set], v.nreads * sizeof(spv_vote), hipMemcpyDeviceToHost, v.stream));
        return SPX_OK;
    };
    job.collect = [&](const StageView&) -> int {
        const int r = product_collect(ix, ix->votes, VOTE_WORDS, 6);
        return r != SPX_OK ? r : vote_error_code(ix);
    };
    QuietOnError quiet(nullptr, true);  // (two streams: a failed call waits for the device)
    return quiet.done(stage_run(ix, job, plan));
}

}  // extern "C"
