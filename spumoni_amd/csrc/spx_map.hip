// spx_map.hip -- the mappings (include/spumoni_map.h): the extended alignments of spx_extend.hip in the
// coordinates of the sequence they lie on, and the product's C-ABI with the sequence table.  The kernels read records,
// entries, read offsets and the piece starts; they read neither the text nor the reads.  The number of entries changes,
// so the shape is count -> exclusive sum -> write, as in spx_mems.hip and the emit of spx_cigar_kernels.h.
//
//   locate and count   a lane per read.  The record's spans and the offsets are checked, then one pass over the entries
//            checks every operation and every sum and, with a running text position, finds the home piece: the piece of
//            ref_start by a binary search in P, the next ones as the position crosses their ends (the neighbour by one
//            comparison, a far one -- behind a long 'D' or 'N' -- by another search).  Pieces are visited in text order,
//            so the state is the current piece, its '=' count and the best piece so far.  A second pass finds where the
//            kept part begins and ends -- entry, offset within it, text and read position -- and, from running sums taken
//            at both places, matches, edits and block.  The record is written complete; the plan (first and last kept
//            entry, what is kept of each) goes to a 16-byte record of scratch, and the read's entries are counted by the
//            same code that writes them.
//   write    a lane per read: clip, kept operations with the two border entries cut, clip, through the merging push of the
//            emit in spx_cigar_kernels.h; on a reverse piece entry k of c goes to place c - 1 - k.  A read whose entries
//            end beyond op_capacity is rewritten as unmapped.  The counts of spn_map_stats are taken here, so that such a
//            read counts in none.
//
// Control flow: the only shuffles and the only barrier are the sums at the end of k_map_write, outside every loop.  No
// scratch memory; 192 bytes of LDS for a block's sums in k_map_write, none in k_map_count.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/spumoni_map.h"
#include "spx_internal.h"

namespace spx {
namespace {

constexpr uint32_t OP_I = SPG_OP_I, OP_D = SPG_OP_D, OP_N = SPG_OP_N, OP_S = SPE_OP_S, OP_EQ = SPG_OP_EQ, OP_X = SPG_OP_X;

struct MapCounters {  // device; zeroed in front of every launch
    unsigned long long reads, mapped, cut, reverse, entries_in, entries_out, cut_chars;  // (k_map_write adds to the six by index)
    unsigned long long error;  // bit 0: a read failed the checks, bit 1: a read's entries did not fit
};
constexpr int MAP_WORDS = sizeof(MapCounters) / 8;

struct MapArgs {
    const uint4* rec;       // 3 per read: spa_alignment
    const uint64_t* ioffs;  // nreads + 1
    const uint32_t* iops;
    uint64_t in_entries;
    const uint64_t* roffs;  // nreads + 1
    uint64_t nreads;
    const uint64_t* P;      // np + 1
    uint64_t np;
    uint32_t strands;
    uint4* out;             // 3 per read: spn_mapping
    uint4* plan;            // per read: first kept entry, last kept entry (both from ioffs[q]), kept of the first, of the last
    uint64_t* ocnt;         // nreads + 1: entries per read, then a 0
    uint64_t* ooffs;        // nreads + 1
    uint32_t* ops;
    uint64_t op_cap;
    MapCounters* c;
};

__device__ inline void write_unmapped(const MapArgs& a, uint64_t q) {
    a.out[3 * q] = make_uint4(0, 0, 0, 0);
    a.out[3 * q + 1] = make_uint4(SPN_UNMAPPED, 0, 0, 0);
    a.out[3 * q + 2] = make_uint4(0, 0, 0, 0);
}
__device__ inline bool reads_read(uint32_t op) { return op == OP_EQ || op == OP_X || op == OP_I; }
__device__ inline bool reads_text(uint32_t op) { return op == OP_EQ || op == OP_X || op == OP_D || op == OP_N; }
__device__ inline bool is_op(uint32_t op) { return reads_read(op) || op == OP_D || op == OP_N || op == OP_S; }
// the piece that holds t < P[np]
__device__ inline uint64_t piece_of(const uint64_t* P, uint64_t np, uint64_t t) {
    uint64_t lo = 0, hi = np;  // P[lo] <= t < P[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (P[mid] <= t)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// A mapped read's entries: counted, or (WRITE) written to dst, entry k of `total` at k, on a reverse piece at
// total - 1 - k.  src: the read's own entries; plan: k_map_count's.
template <bool WRITE>
__device__ inline uint64_t emit_mapping(const uint32_t* src, const uint4& plan, uint64_t left, uint64_t right, bool rev, uint32_t* dst,
                                        uint64_t total) {
    uint32_t op = OP_S;
    uint64_t len = left, n = 0;
    auto put = [&](uint32_t v) {
        if (WRITE) dst[rev ? total - 1 - n : n] = v;
        ++n;
    };
    auto flush = [&]() {
        if (!len) return;
        for (; len > SPG_MAX_LENGTH; len -= SPG_MAX_LENGTH) put(SPG_MAX_LENGTH << 4 | op);
        put((uint32_t)len << 4 | op);
    };
    auto push = [&](uint32_t o, uint64_t l) {
        if (!l) return;
        if (o == op) {
            len += l;
        } else {
            flush();
            op = o;
            len = l;
        }
    };
    for (uint32_t e = plan.x; e <= plan.y; ++e) {  // (plan.y is below the read's entry count)
        const uint32_t v = src[e];
        push(v & 15u, e == plan.x ? plan.z : e == plan.y ? plan.w : v >> 4);
    }
    push(OP_S, right);
    flush();
    return n;
}

__global__ __launch_bounds__(256) void k_map_count(MapArgs a) {
    const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (q > a.nreads) return;
    a.ocnt[q] = 0;
    if (q == a.nreads) return;
    write_unmapped(a, q);
    const uint4 w0 = a.rec[3 * q];
    if (w0.x == 0xffffffffu && w0.y == 0xffffffffu) return;  // unaligned: unmapped
    const uint4 w1 = a.rec[3 * q + 1];
    const uint64_t n_text = a.P[a.np];
    const uint64_t r0 = a.roffs[q], r1 = a.roffs[q + 1], i0 = a.ioffs[q], i1 = a.ioffs[q + 1];
    const uint64_t ts = (uint64_t)w0.x | ((uint64_t)w0.y << 32), te = (uint64_t)w0.z | ((uint64_t)w0.w << 32);
    const uint64_t rs = w1.x, re = w1.y;
    bool ok = r1 >= r0 && r1 - r0 <= 0xffffffffull && i1 >= i0 && i1 <= a.in_entries && i1 - i0 <= 0xffffffffull;
    const uint64_t len = r1 - r0;
    ok = ok && rs <= re && re <= len && ts <= te && te <= n_text;
    if (!ok) {
        atomicOr(&a.c->error, 1ull);
        return;
    }
    const uint32_t ne = (uint32_t)(i1 - i0);
    const uint32_t* src = a.iops + i0;
    // pass 1: the checks, and the home piece
    uint64_t lead = 0, tail = 0, rsum = 0, tsum = 0, eq = 0, t = ts;
    uint64_t p = 0, pend = 0, cur = 0, best = 0, home = 0;  // pend: P[p + 1]; 0: no piece yet
    bool seen = false;
    for (uint32_t e = 0; e < ne && ok; ++e) {
        const uint32_t v = src[e], op = v & 15u;
        uint64_t n = v >> 4;
        if (!is_op(op)) {
            ok = false;
        } else if (op == OP_S) {
            if (seen)
                tail += n;
            else
                lead += n;
        } else {
            ok = tail == 0;
            seen = true;
            if (reads_read(op)) rsum += n;
            if (reads_text(op)) {
                tsum += n;
                if (tsum > te - ts) {  // (every t below stays under te <= n_text)
                    ok = false;
                } else if (op != OP_EQ) {
                    t += n;
                } else {
                    eq += n;
                    while (n) {
                        if (t >= pend) {
                            if (cur > best) {
                                best = cur;
                                home = p;
                            }
                            cur = 0;
                            p = pend && p + 2 <= a.np && t < a.P[p + 2] ? p + 1 : piece_of(a.P, a.np, t);
                            pend = a.P[p + 1];
                        }
                        const uint64_t take = n < pend - t ? n : pend - t;
                        cur += take;
                        t += take;
                        n -= take;
                    }
                }
            }
        }
    }
    if (cur > best) {
        best = cur;
        home = p;
    }
    ok = ok && lead == rs && rsum == re - rs && tail == len - re && tsum == te - ts && eq != 0;
    if (!ok) {
        atomicOr(&a.c->error, 1ull);
        return;
    }
    // pass 2: where the kept part begins and ends.  m, d and b: '=', X + I + D and the columns but 'N' so far; c: columns
    const uint64_t h0 = a.P[home], h1 = a.P[home + 1];
    uint64_t r = rs, m = 0, d = 0, b = 0, c = 0;
    uint64_t t_first = 0, r_first = 0, m_first = 0, d_first = 0, b_first = 0, c_first = 0;
    uint64_t t_end = 0, r_end = 0, m_end = 0, d_end = 0, b_end = 0, c_end = 0;
    uint32_t e0 = 0, e1 = 0, n_e0 = 0, off0 = 0, off1 = 0;
    bool first = true;
    t = ts;
    for (uint32_t e = 0; e < ne; ++e) {
        const uint32_t v = src[e], op = v & 15u;
        const uint64_t n = v >> 4;
        if (op == OP_S) continue;
        if (op == OP_EQ) {
            const uint64_t lo = t > h0 ? t : h0, hi = t + n < h1 ? t + n : h1;
            if (lo < hi) {
                if (first) {
                    first = false;
                    e0 = e;
                    n_e0 = (uint32_t)n;
                    off0 = (uint32_t)(lo - t);
                    t_first = lo;
                    r_first = r + off0;
                    m_first = m + off0;
                    d_first = d;
                    b_first = b + off0;
                    c_first = c + off0;
                }
                e1 = e;
                off1 = (uint32_t)(hi - t);
                t_end = hi;
                r_end = r + off1;
                m_end = m + off1;
                d_end = d;
                b_end = b + off1;
                c_end = c + off1;
            }
            m += n;
        } else if (op != OP_N) {
            d += n;
        }
        if (op != OP_N) b += n;
        c += n;
        if (reads_read(op)) r += n;
        if (reads_text(op)) t += n;
    }
    // (best >= 1: the home piece holds an '=' column, so first is false here)
    const uint32_t strand = (uint32_t)(home % a.strands);
    uint64_t start = t_first - h0, end = t_end - h0;
    if (strand) {
        const uint64_t s = start;
        start = (h1 - h0) - end;
        end = (h1 - h0) - s;
    }
    const uint64_t left = r_first, right = len - r_end;
    const uint4 plan = make_uint4(e0, e1, e0 == e1 ? (uint32_t)(t_end - t_first) : n_e0 - off0, off1);
    a.plan[q] = plan;
    a.out[3 * q] = make_uint4((uint32_t)start, (uint32_t)(start >> 32), (uint32_t)end, (uint32_t)(end >> 32));
    a.out[3 * q + 1] = make_uint4((uint32_t)(home / a.strands), strand, (uint32_t)left, (uint32_t)r_end);
    a.out[3 * q + 2] = make_uint4((uint32_t)(m_end - m_first), (uint32_t)(d_end - d_first), (uint32_t)(b_end - b_first),
                                  (c_first ? SPN_CUT_LEFT : 0u) | (c_end < c ? SPN_CUT_RIGHT : 0u));
    a.ocnt[q] = emit_mapping<false>(src, plan, left, right, false, nullptr, 0);
}

// A lane per read, a block over a stride of reads: the six sums leave a block as one set of atomics (one set per wavefront
// took 0.79 ms on 10^6 reads of 3.5 entries each, this takes 0.06: DESIGN.md 4.16).
__global__ __launch_bounds__(256) void k_map_write(MapArgs a) {
    __shared__ unsigned long long part[4][6];
    unsigned long long mapped = 0, cut = 0, reverse = 0, ein = 0, eout = 0, chars = 0;
    for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < a.nreads; q += (uint64_t)gridDim.x * 256) {
        const uint4 o1 = a.out[3 * q + 1];
        if (o1.x == SPN_UNMAPPED) continue;
        const uint64_t b0 = a.ooffs[q], b1 = a.ooffs[q + 1];
        if (b1 > a.op_cap) {
            atomicOr(&a.c->error, 2ull);
            write_unmapped(a, q);
            continue;
        }
        // (k_map_count has checked this read's offsets and spans)
        const uint64_t i0 = a.ioffs[q], len = a.roffs[q + 1] - a.roffs[q];
        const uint4 w1 = a.rec[3 * q + 1];
        eout += emit_mapping<true>(a.iops + i0, a.plan[q], o1.z, len - o1.w, o1.y != 0, a.ops + b0, b1 - b0);
        mapped += 1;
        cut += a.out[3 * q + 2].w != 0;
        reverse += o1.y;
        ein += a.ioffs[q + 1] - i0;
        chars += (unsigned long long)(o1.z - w1.x) + (w1.y - o1.w);
    }
    mapped = wave_sum(mapped);
    cut = wave_sum(cut);
    reverse = wave_sum(reverse);
    ein = wave_sum(ein);
    eout = wave_sum(eout);
    chars = wave_sum(chars);
    const uint32_t wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wv][0] = mapped;
        part[wv][1] = cut;
        part[wv][2] = reverse;
        part[wv][3] = ein;
        part[wv][4] = eout;
        part[wv][5] = chars;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const unsigned long long v = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (v) atomicAdd(&a.c->mapped + threadIdx.x, v);  // mapped, cut, reverse, entries_in, entries_out, cut_chars: in this order
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.c->reads = a.nreads;
}

// The scratch of one call and both kernels on st, between the product's two events, with a mark where the second step
// begins (none for a batch without reads: its step times are zeros).  Takes ix->mu.
int map_enqueue(spx_index* ix, MapArgs& a, hipStream_t st) {
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    a.P = ix->map_P;
    a.np = ix->map_pieces;
    a.strands = ix->map_strands;
    void* p = nullptr;
    int rc;
    if ((rc = ix->map_scr[spx_index::N_PLAN].reserve(a.nreads * 16 + 16, &p)) != SPX_OK) return rc;
    a.plan = (uint4*)p;
    if ((rc = ix->map_scr[spx_index::N_OCNT].reserve((a.nreads + 1) * 8, &p)) != SPX_OK) return rc;
    a.ocnt = (uint64_t*)p;
    size_t cub_bytes = 0;
    SPX_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, a.ocnt, a.ooffs, a.nreads + 1, (hipStream_t) nullptr));
    void* cub = nullptr;
    if ((rc = ix->map_scr[spx_index::N_CUB].reserve(cub_bytes + 16, &cub)) != SPX_OK) return rc;
    return product_enqueue(ix->map, MAP_WORDS, st, [&](void* counters) -> int {
        a.c = (MapCounters*)counters;
        if (!a.nreads) {
            SPX_HIP(hipMemsetAsync(a.ooffs, 0, 8, st));
            return SPX_OK;
        }
        const unsigned grid = (unsigned)((a.nreads + 1 + 255) / 256);
        k_map_count<<<grid, 256, 0, st>>>(a);
        SPX_HIP(hipGetLastError());
        SPX_HIP(hipcub::DeviceScan::ExclusiveSum(cub, cub_bytes, a.ocnt, a.ooffs, a.nreads + 1, st));
        if ((rc = product_mark(ix->map, 1, st)) != SPX_OK) return rc;
        k_map_write<<<std::min(grid, 1024u), 256, 0, st>>>(a);
        SPX_HIP(hipGetLastError());
        return SPX_OK;
    }, a.nreads ? 0 : -1);
}

int map_error_code(const spx_index* ix) {
    if (ix->map.error & 1) {
        set_error("a read's extended alignment failed the mapping's checks (spans outside the read or the text, entries whose sums "
                  "disagree with them, an unknown operation, no '=', or offsets outside the entries): such a read is left unmapped");
        return SPX_E_FORMAT;
    }
    return SPX_OK;
}

}  // namespace

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

void release_map(spx_index* ix) {
    if (ix->map_P) (void)hipFree(ix->map_P);
    release(ix->map_scr, spx_index::N_COUNT, &ix->map);
}

int clone_map(spx_index* src, spx_index* ix) {
    if (!src->map_P) return SPX_OK;
    int rc = spn_set_sequences(ix, src->map_seq_lengths.data(), src->map_seq_lengths.size(), src->map_strands);
    if (rc != SPX_OK || (rc = clone_cover(src, ix)) != SPX_OK) return rc;
    return clone_call(src, ix);
}

}  // namespace spx

using namespace spx;

extern "C" {

int spn_set_sequences(spx_index* ix, const uint64_t* seq_lengths, uint64_t n_seqs, uint32_t strands) {
    if (!ix || !seq_lengths || n_seqs == 0) {
        set_error("index and seq_lengths must be non-null and n_seqs at least 1");
        return SPX_E_ARG;
    }
    if (strands < 1 || strands > 2) {
        set_error("strands must be 1 or 2");
        return SPX_E_ARG;
    }
    if (!ix->text) {
        set_error("the sequence table needs the text (spx_index_set_text / spx_index_rebuild_text): its total is checked against it");
        return SPX_E_ARG;
    }
    std::vector<uint64_t> P;
    P.reserve(n_seqs * strands + 1);
    P.push_back(0);
    for (uint64_t s = 0; s < n_seqs; ++s) {
        const uint64_t n = seq_lengths[s];
        if (n == 0) {
            set_error("sequence %llu of the table has length 0", (unsigned long long)s);
            return SPX_E_ARG;
        }
        for (uint32_t k = 0; k < strands; ++k) {
            if (n > ix->n_text - P.back()) {
                set_error("the sequences add up to more than the text's %llu characters", (unsigned long long)ix->n_text);
                return SPX_E_ARG;
            }
            P.push_back(P.back() + n);
        }
    }
    if (P.back() != ix->n_text) {
        set_error("the sequences add up to %llu characters, the text has %llu", (unsigned long long)P.back(),
                  (unsigned long long)ix->n_text);
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> hg(ix->host_mu);
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    uint64_t* d = nullptr;
    SPX_HIP(hipMalloc((void**)&d, P.size() * 8));
    const hipError_t e = hipMemcpy(d, P.data(), P.size() * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        SPX_HIP(e);
    }
    if (ix->map_P) {
        // (a kernel of an earlier call may still read the old table)
        if (ix->map.have) (void)hipEventSynchronize(ix->map.ev1);
        (void)hipFree(ix->map_P);
    }
    ix->map_P = d;
    ix->map_pieces = P.size() - 1;
    ix->map_strands = strands;
    ix->map_seq_lengths.assign(seq_lengths, seq_lengths + n_seqs);
    ix->map_ready.ok = false;
    cover_table_changed(ix);
    call_table_changed(ix);
    consensus_table_changed(ix);
    return SPX_OK;
}

int spn_map_device(spx_index* ix, const spa_alignment* d_alignments, const uint64_t* d_op_offsets, const uint32_t* d_ops,
                   uint64_t in_entries, const uint64_t* d_read_offsets, uint64_t nreads, uint64_t op_capacity, spn_mapping* d_out,
                   uint64_t* d_out_op_offsets, uint32_t* d_out_ops, void* stream) {
    int rc;
    if ((rc = need_table(ix, "spn_map_device")) != SPX_OK) return rc;
    if (!d_out_op_offsets || (op_capacity && !d_out_ops) || (in_entries && !d_ops) ||
        (nreads && (!d_alignments || !d_op_offsets || !d_read_offsets || !d_out))) {
        set_error("d_alignments, d_op_offsets, d_ops, d_read_offsets, d_out, d_out_op_offsets and d_out_ops must be non-null");
        return SPX_E_ARG;
    }
    if (op_capacity > 0xffffffffull) {
        set_error("op_capacity must be at most 2^32 - 1");
        return SPX_E_ARG;
    }
    if ((((uintptr_t)d_alignments | (uintptr_t)d_out) & 15) != 0 ||
        (((uintptr_t)d_op_offsets | (uintptr_t)d_read_offsets | (uintptr_t)d_out_op_offsets) & 7) != 0 ||
        (((uintptr_t)d_ops | (uintptr_t)d_out_ops) & 3) != 0) {
        set_error("d_alignments and d_out must be 16-byte aligned (records are read and written as 16-byte vectors), the 64-bit "
                  "arrays 8-byte, d_ops and d_out_ops 4-byte aligned");
        return SPX_E_ARG;
    }
    product_reset(ix, ix->map);
    MapArgs a{};
    a.rec = (const uint4*)d_alignments;
    a.ioffs = d_op_offsets;
    a.iops = d_ops;
    a.in_entries = in_entries;
    a.roffs = d_read_offsets;
    a.nreads = nreads;
    a.out = (uint4*)d_out;
    a.ooffs = d_out_op_offsets;
    a.ops = d_out_ops;
    a.op_cap = op_capacity;
    return map_enqueue(ix, a, (hipStream_t)stream);
}

int spn_last_map_stats(spx_index* ix, spn_map_stats* out) {
    if (!ix || !out) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    if (!ix->map.have) {
        set_error("no mappings have been computed on this index yet");
        return SPX_E_ARG;
    }
    const spx_index::Product& p = ix->map;
    if (p.pending) {
        const int rc = product_collect(ix, ix->map, MAP_WORDS, MAP_WORDS - 1);
        if (rc != SPX_OK) return rc;
    }
    out->reads = p.acc[0];
    out->mapped = p.acc[1];
    out->cut_reads = p.acc[2];
    out->reverse_reads = p.acc[3];
    out->entries_in = p.acc[4];
    out->entries_out = p.acc[5];
    out->cut_chars = p.acc[6];
    out->error = (uint32_t)(p.error & 1);
    out->overflow = (uint32_t)((p.error >> 1) & 1);
    out->kernel_ms = p.ms;
    out->step_ms[0] = p.step_ms[0];
    out->step_ms[1] = p.step_ms[1];
    out->reserved = 0;
    return map_error_code(ix);
}

int spn_map_begin(spx_index* ix, int digest_kind, uint32_t k, uint32_t w, const uint8_t* seqs, const uint64_t* offsets, uint64_t nreads,
                  uint64_t min_length, int want_docs, const spc_params* chain_params, const spa_params* align_params,
                  const spe_params* extend_params, spn_mapping* out_mappings, spa_alignment* out_alignments, uint64_t* n_entries) {
    int rc;
    if ((rc = need_table(ix, "spn_map_begin")) != SPX_OK) return rc;
    if (!n_entries || (nreads && !out_mappings)) {
        set_error("out_mappings and n_entries must be non-null");
        return SPX_E_ARG;
    }
    *n_entries = 0;
    // the pipeline up to the extended CIGARs is spe_extend_begin itself: its checks, its waits, its results on the device
    std::vector<spa_alignment> own;
    if (!out_alignments && nreads) {
        own.resize(nreads);
        out_alignments = own.data();
    }
    std::vector<uint64_t> roffs(nreads + 1, 0);
    uint64_t n_in = 0;
    if ((rc = spe_extend_begin(ix, digest_kind, k, w, seqs, offsets, nreads, min_length, want_docs, chain_params, align_params,
                               extend_params, out_alignments, nullptr, roffs.data() + 1, nullptr, &n_in)) != SPX_OK)
        return rc;
    std::lock_guard<std::mutex> hg(ix->host_mu);
    SPX_HIP(hipSetDevice(ix->device));
    if ((rc = ready_take(ix->extend_ready, nreads, n_in, "spn_map_begin", "the extended CIGARs")) != SPX_OK) return rc;
    product_reset(ix, ix->map);
    ix->map_ready.ok = false;
    if (nreads == 0) {
        ix->map.have = true;  // (the stats of an empty batch are zeros)
        ready_publish(ix->map_ready, 0, 0);
        return SPX_OK;
    }
    // the reads' lengths in the characters the walk saw are the values spe_extend_begin reports
    for (uint64_t q = 0; q < nreads; ++q) roffs[q + 1] += roffs[q];
    // a cut can split an entry in two on either side and makes no other new entry: the clips only take in what stood there
    const uint64_t cap = std::min<uint64_t>(n_in + 2 * nreads, 0xffffffffull);
    void *d_roffs = nullptr, *d_out = nullptr, *d_ooffs = nullptr, *d_ops = nullptr;
    if ((rc = ix->map_scr[spx_index::N_ROFFS].reserve((nreads + 1) * 8, &d_roffs)) != SPX_OK) return rc;
    if ((rc = ix->map_scr[spx_index::N_OUT].reserve(nreads * sizeof(spn_mapping), &d_out)) != SPX_OK) return rc;
    if ((rc = ix->map_scr[spx_index::N_OOFFS].reserve((nreads + 1) * 8, &d_ooffs)) != SPX_OK) return rc;
    if ((rc = ix->map_scr[spx_index::N_OPS].reserve(cap * 4 + 16, &d_ops)) != SPX_OK) return rc;
    hipStream_t st = nullptr;
    if ((rc = ctx_stream_of(ix, &st)) != SPX_OK) return rc;
    QuietOnError quiet(st);
    SPX_HIP(hipMemcpyAsync(d_roffs, roffs.data(), (nreads + 1) * 8, hipMemcpyHostToDevice, st));
    MapArgs a{};
    a.rec = (const uint4*)ix->extend_scr[spx_index::TB_OUT].p;
    a.ioffs = (const uint64_t*)ix->extend_scr[spx_index::TB_OOFFS].p;
    a.iops = (const uint32_t*)ix->extend_scr[spx_index::TB_OPS].p;
    a.in_entries = n_in;
    a.roffs = (const uint64_t*)d_roffs;
    a.nreads = nreads;
    a.out = (uint4*)d_out;
    a.ooffs = (uint64_t*)d_ooffs;
    a.ops = (uint32_t*)d_ops;
    a.op_cap = cap;
    if ((rc = map_enqueue(ix, a, st)) != SPX_OK) return rc;
    SPX_HIP(hipMemcpyAsync(out_mappings, d_out, nreads * sizeof(spn_mapping), hipMemcpyDeviceToHost, st));
    // the one wait of the mapping's own: for the records and the entry count
    if ((rc = ctx_wait(ix, st)) != SPX_OK) return rc;
    if ((rc = product_collect(ix, ix->map, MAP_WORDS, MAP_WORDS - 1)) != SPX_OK) return rc;
    if ((rc = map_error_code(ix)) != SPX_OK) return rc;
    if (ix->map.error & 2) {
        set_error("internal: the bound of the mapping's entries did not hold");
        return SPX_E_FORMAT;
    }
    *n_entries = ix->map.acc[5];
    ready_publish(ix->map_ready, *n_entries, nreads);
    return quiet.done(SPX_OK);
}

int spn_map_fetch(spx_index* ix, uint64_t* out_op_offsets, uint32_t* out_ops) {
    if (!ix) {
        set_error("index must be non-null");
        return SPX_E_ARG;
    }
    return ready_fetch(ix, ix->map_ready, ix->map_scr[spx_index::N_OOFFS], ix->map_scr[spx_index::N_OPS], "spn_map_fetch", "spn_map_begin",
                       out_op_offsets, out_ops);
}

}  // extern "C"
