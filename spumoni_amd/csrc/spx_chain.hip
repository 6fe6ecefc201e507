// spx_chain.hip -- the chains (include/spumoni_chain.h): per read, the best collinear chain of its match
// records (spx_mems.hip) under a windowed dynamic programme, as one 48-byte record, and on request the programme's whole
// table (f and pred of every anchor).
//
// One kernel, k_chain.  The recurrence is serial in the anchor i and parallel over its at most 64 predecessors:
//   the ring     a group of G lanes keeps the last G anchors of its read in registers: lane j mod G holds x, y, l, D and
//                f of anchor j, and with them what the chain that ends in j looks like (first anchor, anchors, gap), so
//                that nothing walks back over pred;
//   a block      G records at a time come in as whole 16-byte vectors, a lane each; anchor i's fields are broadcast from
//                the lane that loaded it, every lane evaluates the candidate of the anchor it holds (lanes below i mod G
//                hold this block's anchors, the others the block's before), and one group maximum of
//                candidate << 32 | j gives f[i] and pred[i]: the largest j among equal candidates.  A candidate that
//                does not beat l_i enters as 0, so the anchor alone wins a tie;
//   the record   the smallest i with the largest f is kept on the way; its chain's first anchor is read once at the end.
// Mapping: a group of 16 lanes per read, four reads per wavefront (reads of one to six anchors are the common case), and
// a read of more than 16 anchors gets the whole wavefront -- a ring of 64 = the largest lookback -- right after.  A
// wavefront has four reads, or at most 1 / 16384 of a batch above 65536: a read of 10^5 anchors (10^5 serial steps) holds
// up the few reads behind it in its own wavefront, and the others take the batch.  (A claim counter per four reads was
// tried first: 250 000 atomics on one word cost 3.6 ms for 10^6 reads, more than the chaining.)  No LDS, no scratch but
// the counters, no atomics but the statistics; a read's record depends on that read alone: the same input gives the
// same bytes.
//
// Control flow: every loop that holds a shuffle or a ballot has a trip count that depends on the wavefront alone (a
// ballot over "some group is not done"); groups that are done take part with nothing to do.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/spumoni_chain.h"
#include "spx_internal.h"

namespace spx {
namespace {

constexpr uint32_t SHORT_MAX = 16;  // a read of more anchors than this gets the whole wavefront

struct ChainCounters {  // device; zeroed in front of every launch
    unsigned long long reads, anchors, chained_reads, chain_anchors, candidates;
    unsigned long long error;  // bit 0: a read of 2^32 anchors or more, or decreasing offsets
};
constexpr int CHAIN_WORDS = sizeof(ChainCounters) / 8;  // (the first five are what spc_chain_stats reports, the last the error)
struct ChainArgs {
    const uint4* M;
    const uint32_t* D;
    const uint64_t* offs;
    uint64_t nreads;
    uint64_t chunk_reads;  // reads a wavefront takes at a time, a multiple of four
    uint32_t lookback;
    int64_t max_dist, max_gap, gap_penalty;
    uint4* out;  // three per read
    uint32_t *out_score, *out_pred;
    ChainCounters* c;
};

template <int G>
__device__ inline unsigned long long group_maxu(unsigned long long v) {
    for (int s = G >> 1; s > 0; s >>= 1) {
        const unsigned long long o = __shfl_xor(v, s, G);
        v = o > v ? o : v;
    }
    return v;
}

struct Chained {  // the same in every lane of the group
    uint4 w0, w1, w2;
    uint32_t anchors;
};
__device__ inline Chained unchained() {
    Chained r;
    r.w0 = make_uint4(0xffffffffu, 0xffffffffu, 0, 0);
    r.w1 = make_uint4(0, 0, 0, 0);
    r.w2 = make_uint4(0, 0, 0, SPC_NO_DOC);
    r.anchors = 0;
    return r;
}

// The chain of one read by a group of G lanes, every lane of the wavefront inside (on: this group has a read with
// anchors, h of them from record o on; G == 16: h <= 16).  gl: the lane within its group.  Writes the read's part of the
// table and counts the eligible pairs.  Widths: under the input contract dx, dy, ex and ey are exact in 64 bits; d is
// only used where dx and dy lie in [1, 2^31), gap_penalty * d stays below 2^47 and a candidate below 2^32.  Outside the
// contract the arithmetic wraps (it is done unsigned), and whatever comes out indexes nothing: every index below is made
// of lane and block numbers.
template <int G>
__device__ inline Chained chain_read(const ChainArgs& a, uint64_t o, uint64_t h, bool on, uint32_t gl, unsigned long long& n_cand) {
    uint32_t rx = 0, rl = 0, rf = 0, rD = 0, rfirst = 0, rcnt = 0, rgap = 0, rpred = SPC_NO_PRED;  // the ring: anchor j in lane j mod G
    uint64_t ry = 0;
    long long best_f = -1;  // the best end so far and its chain
    uint32_t b_last = 0, b_first = 0, b_cnt = 0, b_gap = 0, b_xe = 0, b_doc = 0;
    uint64_t b_ye = 0;
    for (uint64_t b0 = 0; __ballot(on && b0 < h); b0 += G) {
        const uint64_t k = b0 + gl;  // the lane's anchor of this block
        const bool have = on && k < h;
        uint4 m = make_uint4(0, 0, 0, 0);
        uint32_t nD = 0;
        if (have) {
            m = a.M[o + k];
            if (a.D) nD = a.D[o + k];
        }
        const uint32_t nx = m.z, nl = m.w;
        const uint64_t ny = (uint64_t)m.x | ((uint64_t)m.y << 32);
        const uint32_t cnt = (on && b0 < h) ? (uint32_t)(h - b0 < G ? h - b0 : G) : 0u;
        for (uint32_t t = 0; __ballot(t < cnt); ++t) {
            const bool act = t < cnt;
            const uint32_t xi = __shfl(nx, t, G), li = __shfl(nl, t, G), Di = __shfl(nD, t, G);
            const uint64_t yi = __shfl((unsigned long long)ny, t, G);
            // the lane's candidate: the anchor its ring entry holds, `dist` in front of i
            const bool cur = gl < t;
            const uint32_t dist = cur ? t - gl : t + G - gl;
            const int64_t dx = (int64_t)xi - (int64_t)rx, dy = (int64_t)(yi - ry);
            const uint64_t ll = (uint64_t)li - (uint64_t)rl;
            const int64_t ex = (int64_t)((uint64_t)dx + ll), ey = (int64_t)((uint64_t)dy + ll);
            const int64_t diff = (int64_t)((uint64_t)dx - (uint64_t)dy);
            const uint64_t d = diff < 0 ? 0 - (uint64_t)diff : (uint64_t)diff;
            const bool eligible = act && (cur || b0 != 0) && dist <= a.lookback && dx >= 1 && dy >= 1 && ex >= 1 && ey >= 1 &&
                                  dx <= a.max_dist && dy <= a.max_dist && d <= (uint64_t)a.max_gap && rD == Di;
            n_cand += eligible ? 1 : 0;
            int64_t gain = (int64_t)li;
            gain = ex < gain ? ex : gain;
            gain = ey < gain ? ey : gain;
            const int64_t c = (int64_t)((uint64_t)rf + (uint64_t)gain - (uint64_t)a.gap_penalty * d);
            const uint32_t i_rel = (uint32_t)(b0 + t);
            unsigned long long key = (eligible && c > (int64_t)li) ? ((unsigned long long)c << 32) | (uint32_t)(i_rel - dist) : 0ull;
            key = group_maxu<G>(key);
            const uint32_t src = (uint32_t)key & (G - 1);  // the lane that holds the winner
            const uint32_t p_first = __shfl(rfirst, src, G), p_cnt = __shfl(rcnt, src, G), p_gap = __shfl(rgap, src, G);
            const uint32_t p_d = __shfl((uint32_t)d, src, G);
            const bool alone = key == 0;
            const uint32_t f = alone ? li : (uint32_t)(key >> 32), pred = alone ? SPC_NO_PRED : (uint32_t)key;
            const uint32_t first = alone ? i_rel : p_first, n = alone ? 1u : p_cnt + 1;
            const uint64_t gsum = (uint64_t)p_gap + p_d;
            const uint32_t gap = alone ? 0u : (gsum > 0xffffffffull ? 0xffffffffu : (uint32_t)gsum);
            if (act && gl == t) {
                rx = nx;
                ry = ny;
                rl = nl;
                rD = nD;
                rf = f;
                rfirst = first;
                rcnt = n;
                rgap = gap;
                rpred = pred;
            }
            if (act && (long long)f > best_f) {
                best_f = f;
                b_last = i_rel;
                b_first = first;
                b_cnt = n;
                b_gap = gap;
                b_xe = xi + li;
                b_ye = yi + li;
                b_doc = Di;
            }
        }
        if (have) {  // the lane's ring entry is anchor k now
            if (a.out_score) a.out_score[o + k] = rf;
            if (a.out_pred) a.out_pred[o + k] = rpred;
        }
    }
    if (!on || best_f < 0) return unchained();
    const uint4 m = a.M[o + b_first];  // (b_first < h: it is some anchor's index)
    Chained r;
    r.w0 = make_uint4(m.x, m.y, (uint32_t)b_ye, (uint32_t)(b_ye >> 32));
    r.w1 = make_uint4(m.z, b_xe, (uint32_t)best_f, b_cnt);
    r.w2 = make_uint4(b_first, b_last, b_gap, a.D ? b_doc : SPC_NO_DOC);
    r.anchors = b_cnt;
    return r;
}

__global__ __launch_bounds__(256) void k_chain(ChainArgs a) {
    constexpr uint32_t G = 16, PER_WAVE = 64 / G;
    const uint32_t lane = threadIdx.x & 63, gl = lane & (G - 1), grp = lane / G;
    const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    unsigned long long n_cand = 0, n_chained = 0, n_in_chains = 0;
    if (wave == 0 && lane == 0) {
        const uint64_t lo = a.offs[0], hi = a.offs[a.nreads];
        a.c->reads = a.nreads;
        a.c->anchors = hi < lo ? 0 : hi - lo;
    }
    // a wavefront's reads are one chunk, and the grid covers the batch (chain_enqueue).  (The trip count depends on the
    // wavefront alone: q0 is the same in all of its lanes)
    {
        const uint64_t c0 = wave * a.chunk_reads < a.nreads ? wave * a.chunk_reads : a.nreads;
        const uint64_t c1 = c0 + a.chunk_reads < a.nreads ? c0 + a.chunk_reads : a.nreads;
        for (uint64_t q0 = c0; q0 < c1; q0 += PER_WAVE) {
            const uint64_t q = q0 + grp;
            const bool active = q < a.nreads;
            const uint64_t o = active ? a.offs[q] : 0, e = active ? a.offs[q + 1] : 0;
            const bool sane = active && e >= o && e - o < (1ull << 32);
            if (active && gl == 0 && !sane) atomicOr(&a.c->error, 1ull);
            const uint64_t h = sane ? e - o : 0;
            const bool is_long = h > SHORT_MAX;
            const Chained r = chain_read<G>(a, o, h, h != 0 && !is_long, gl, n_cand);
            if (active && !is_long && gl == 0) {
                a.out[3 * q] = r.w0;
                a.out[3 * q + 1] = r.w1;
                a.out[3 * q + 2] = r.w2;
                n_chained += r.anchors != 0;
                n_in_chains += r.anchors;
            }
            unsigned long long long_mask = __ballot(is_long && gl == 0);
            while (long_mask) {
                const int src = __ffsll(long_mask) - 1;
                long_mask &= long_mask - 1;
                const uint64_t lo = __shfl((unsigned long long)o, src), lh = __shfl((unsigned long long)h, src);
                const Chained w = chain_read<64>(a, lo, lh, true, lane, n_cand);
                if (lane == 0) {
                    const uint64_t lq = q0 + (uint32_t)src / G;
                    a.out[3 * lq] = w.w0;
                    a.out[3 * lq + 1] = w.w1;
                    a.out[3 * lq + 2] = w.w2;
                    n_chained += w.anchors != 0;
                    n_in_chains += w.anchors;
                }
            }
        }
    }
    n_cand = wave_sum(n_cand);
    n_chained = wave_sum(n_chained);
    n_in_chains = wave_sum(n_in_chains);
    if (lane == 0 && (n_cand | n_chained)) {
        atomicAdd(&a.c->candidates, n_cand);
        atomicAdd(&a.c->chained_reads, n_chained);
        atomicAdd(&a.c->chain_anchors, n_in_chains);
    }
}

// The chain kernel on st, between the index's two events.  Takes ix->mu.
int chain_enqueue(spx_index* ix, ChainArgs& a, hipStream_t st) {
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    return product_enqueue(ix->chain, CHAIN_WORDS, st, [&](void* counters) -> int {
        a.c = (ChainCounters*)counters;
        if (!a.nreads) return SPX_OK;
        // four reads per wavefront while the grid may grow, more beyond that: the grid always covers the batch
        constexpr uint64_t MAX_BLOCKS = 4096;
        a.chunk_reads = 4 * std::max<uint64_t>(1, (a.nreads + MAX_BLOCKS * 16 - 1) / (MAX_BLOCKS * 16));
        const unsigned grid = (unsigned)std::min<uint64_t>((a.nreads + 15) / 16, MAX_BLOCKS);
        k_chain<<<grid, 256, 0, st>>>(a);
        SPX_HIP(hipGetLastError());
        return SPX_OK;
    });
}
int chain_error_code(const spx_index* ix) {
    if (ix->chain.error & 1) {
        set_error("a read has 2^32 anchors or more (or its match offsets decrease): such a read is left without a chain");
        return SPX_E_FORMAT;
    }
    return SPX_OK;
}

void set_params(ChainArgs& a, const spc_params& p) {
    a.lookback = p.lookback;
    a.max_dist = p.max_dist;
    a.max_gap = p.max_gap;
    a.gap_penalty = p.gap_penalty;
}

}  // namespace

int chain_check_params(const spx_index* ix, const spc_params* p) {
    if (!ix) {
        set_error("index must be non-null");
        return SPX_E_ARG;
    }
    if (!p) {
        set_error("params must be non-null");
        return SPX_E_ARG;
    }
    if (p->lookback < 1 || p->lookback > 64) {
        set_error("lookback must be 1 .. 64");
        return SPX_E_ARG;
    }
    if (p->max_dist < 1 || p->max_dist > 0x7fffffffu) {
        set_error("max_dist must be 1 .. 2^31 - 1");
        return SPX_E_ARG;
    }
    if (p->max_gap > 0x7fffffffu) {
        set_error("max_gap must be 0 .. 2^31 - 1");
        return SPX_E_ARG;
    }
    if (p->gap_penalty > 65535u) {
        set_error("gap_penalty must be 0 .. 65535");
        return SPX_E_ARG;
    }
    return SPX_OK;
}
void release_chain(spx_index* ix) { release(ix->chain_scr, spx_index::H_COUNT, &ix->chain); }

}  // namespace spx

using namespace spx;

extern "C" {

int spc_chain_device(spx_index* ix, const spm_match* d_matches, const uint32_t* d_match_docs, const uint64_t* d_match_offsets,
                     uint64_t nreads, const spc_params* params, spc_chain* d_out, uint32_t* d_out_score, uint32_t* d_out_pred,
                     void* stream) {
    int rc = chain_check_params(ix, params);
    if (rc != SPX_OK) return rc;
    if (nreads && (!d_matches || !d_match_offsets || !d_out)) {
        set_error("d_matches, d_match_offsets and d_out must be non-null");
        return SPX_E_ARG;
    }
    if ((((uintptr_t)d_matches | (uintptr_t)d_out) & 15) != 0 || ((uintptr_t)d_match_offsets & 7) != 0 ||
        (((uintptr_t)d_match_docs | (uintptr_t)d_out_score | (uintptr_t)d_out_pred) & 3) != 0) {
        set_error("d_matches and d_out must be 16-byte aligned (records are read and written as 16-byte vectors), "
                  "d_match_offsets 8-byte and the 32-bit arrays 4-byte aligned");
        return SPX_E_ARG;
    }
    product_reset(ix, ix->chain);
    ChainArgs a{};
    a.M = (const uint4*)d_matches;
    a.D = d_match_docs;
    a.offs = d_match_offsets;
    a.nreads = nreads;
    set_params(a, *params);
    a.out = (uint4*)d_out;
    a.out_score = d_out_score;
    a.out_pred = d_out_pred;
    return chain_enqueue(ix, a, (hipStream_t)stream);
}

int spc_last_chain_stats(spx_index* ix, spc_chain_stats* out) {
    if (!ix || !out) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    if (!ix->chain.have) {
        set_error("no chains have been computed on this index yet");
        return SPX_E_ARG;
    }
    if (ix->chain.pending) {
        const int rc = product_collect(ix, ix->chain, CHAIN_WORDS, 5);
        if (rc != SPX_OK) return rc;
    }
    out->reads = ix->chain.acc[0];
    out->anchors = ix->chain.acc[1];
    out->chained_reads = ix->chain.acc[2];
    out->chain_anchors = ix->chain.acc[3];
    out->candidates = ix->chain.acc[4];
    out->kernel_ms = ix->chain.ms;
    return chain_error_code(ix);
}

// spm_mems_begin's steps (mems_begin_staged: the staged walk in MS mode with exactly one piece, the count, the host wait,
// the records at their exact size) with the chain kernel behind k_mems_write on the same stream.
int spc_chain_batch(spx_index* ix, int digest_kind, uint32_t k, uint32_t w, const uint8_t* seqs, const uint64_t* offsets,
                    uint64_t nreads, uint64_t min_length, int want_docs, const spc_params* params, spc_chain* out_chains,
                    uint64_t* out_values) {
    if (spx_device_count() <= 0) {
        set_error("no HIP device visible: the chains are computed on the GPU and there is no CPU fallback");
        return SPX_E_NODEVICE;
    }
    int rc = chain_check_params(ix, params);
    if (rc != SPX_OK) return rc;
    if ((rc = check_batch(ix, "the chains", BATCH_MIN_LENGTH | BATCH_TEXT | BATCH_ONE_PIECE, min_length, digest_kind, want_docs,
                          nreads && (!seqs || !offsets || !out_chains) ? "seqs, offsets and out_chains must be non-null" : nullptr, offsets,
                          nreads)) != SPX_OK)
        return rc;
    std::lock_guard<std::mutex> hg(ix->host_mu);
    SPX_HIP(hipSetDevice(ix->device));
    product_reset(ix, ix->chain);
    if (nreads == 0) {
        ix->chain.have = true;  // (the stats of an empty batch are zeros)
        return SPX_OK;
    }
    void* d_out = nullptr;
    if ((rc = ix->chain_scr[spx_index::H_OUT].reserve(nreads * sizeof(spc_chain), &d_out)) != SPX_OK) return rc;
    std::vector<uint64_t> match_offsets(nreads + 1);
    uint64_t n = 0;
    rc = mems_begin_staged(ix, digest_kind, k, w, seqs, offsets, nreads, min_length, want_docs, match_offsets.data(), out_values, &n,
                           false, [&](const MemsOnDevice& m) -> int {
                               ChainArgs a{};
                               a.M = (const uint4*)m.records;
                               a.D = m.docs;
                               a.offs = m.match_offsets;
                               a.nreads = m.nreads;
                               set_params(a, *params);
                               a.out = (uint4*)d_out;
                               const int r = chain_enqueue(ix, a, m.stream);
                               if (r != SPX_OK) return r;
                               SPX_HIP(hipMemcpyAsync(out_chains, d_out, m.nreads * sizeof(spc_chain), hipMemcpyDeviceToHost, m.stream));
                               return SPX_OK;
                           });
    if (rc != SPX_OK) return rc;
    if ((rc = product_collect(ix, ix->chain, CHAIN_WORDS, 5)) != SPX_OK) return rc;
    return chain_error_code(ix);
}

}  // extern "C"
