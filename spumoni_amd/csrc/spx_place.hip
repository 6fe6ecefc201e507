// spx_place.hip -- the placements (include/spumoni_place.h): per read, the seed = the largest MS length
// (the smallest position among equals), extended to both sides on its diagonal without gaps under an x-drop rule, as one
// 32-byte record.
//
// One kernel, k_place, two steps per read with nothing returning to the host between the walk and the records:
//   the argmax   the lanes of a group take the aligned 16-byte vectors of lengths the walk stored, 8 or 4 values each,
//                and the group keeps the maximum of length << 32 | ~position, as the votes do: the largest length, the
//                smallest position among equals;
//   the x-drop   a lane takes 16 characters of read and text (two 16-byte loads at whatever alignment they have) as
//                one equality mask and reduces it to four integers: total, largest prefix, smallest prefix, and the
//                worst drop below a running maximum that starts at 0.  These compose: with the running maximum g above
//                a segment's start, its worst drop is max(g - smallest prefix, drop_0).  The group scans the totals and
//                the running maxima and ballots for the first lane whose drop exceeds x_drop; only that lane walks its
//                16 characters for the exact k.  A side that has stopped loads nothing more.
// Mapping: a group of 16 lanes per read, four reads per wavefront (k_votes_short's mapping: a read of 44 .. 250 values
// is 6 .. 32 vectors of 16-bit lengths and at most 16 segments per side), and a read of more than LONG_MIN values is
// taken by the whole wavefront right after: a read of 10^6 values keeps one wavefront busy for 2000 rounds while every
// other wavefront goes on.  No LDS, no scratch but the counters, no atomics but the statistics; a read's record depends
// on that read alone: the same input gives the same bytes.
//
// Control flow: every loop that holds a shuffle or a ballot has a trip count that depends on the wavefront alone (a
// ballot over "some group is not done"); groups that are done take part with nothing to do.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/spumoni_place.h"
#include "spx_internal.h"

namespace spx {
namespace {

constexpr uint32_t LONG_MIN_VALUES = 2048;  // a read of more values than this gets the whole wavefront
constexpr int SEG = 16;                     // characters per lane and round

struct PlaceCounters {  // device; zeroed in front of every launch
    unsigned long long values, placed, seed_values, extended_values;
    unsigned long long error;  // bit 0: a read of 2^32 values or more, or decreasing offsets; bit 1: more values than total_values said
};
constexpr int PLACE_WORDS = sizeof(PlaceCounters) / 8;  // (the first four are what spp_place_stats reports, the last the error)
struct PlaceArgs {
    const uint8_t* R;
    const uint4* L;
    const uint64_t* P;
    const void* D;
    const uint64_t* offs;
    const uint8_t* T;
    uint64_t n_text;
    uint64_t nreads, total_values, min_seed;
    int32_t penalty;  // 0 .. 65535
    int64_t x_drop;   // 0 .. 2^31 - 1
    uint4* out;       // two per read
    PlaceCounters* c;
};

template <int BITS>
__device__ inline uint32_t value_at(const void* p, uint64_t i) {
    return BITS == 16 ? (uint32_t)((const uint16_t*)p)[i] : ((const uint32_t*)p)[i];
}
__device__ __forceinline__ uint4 load16_unaligned(const uint8_t* p) {
    uint4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}
// bit t: byte t of x is zero
__device__ inline uint32_t zero_bytes(uint32_t x) {
    uint32_t m = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) m |= ((x >> (8 * t)) & 0xffu) == 0 ? 1u << t : 0u;
    return m;
}
// the bits of a wavefront-wide ballot that belong to the lane's group, lane 0 of the group in bit 0
template <int G>
__device__ inline unsigned long long group_ballot(bool p, uint32_t lane) {
    const unsigned long long b = __ballot(p);
    return G == 64 ? b : (b >> (lane & ~(uint32_t)(G - 1))) & ((1ull << (G & 63)) - 1);
}
template <int G>
__device__ inline long long group_max(long long v) {
    for (int s = G >> 1; s > 0; s >>= 1) {
        const long long o = __shfl_xor(v, s, G);
        v = o > v ? o : v;
    }
    return v;
}
template <int G>
__device__ inline unsigned long long group_maxu(unsigned long long v) {
    for (int s = G >> 1; s > 0; s >>= 1) {
        const unsigned long long o = __shfl_xor(v, s, G);
        v = o > v ? o : v;
    }
    return v;
}

struct Side {
    uint32_t len, equal;  // steps of the extension, equal characters inside
};

// One x-drop extension by a group of G lanes, every lane of the wavefront inside (on: this group has one to do).  Step k
// (1 .. K) compares R[r0 + k - 1] with T[t0 + k - 1], LEFT: R[r0 - k] with T[t0 - k]; the caller has made sure that all
// of them exist.  Widths: a character scores +1 or -penalty >= -65535, so the sums of a segment (16 characters) and of
// a round (G segments) stay inside +-2^26 and are 32-bit; everything carried from round to round (K < 2^32 characters:
// above -2^48) is 64-bit.
template <int G, bool LEFT>
__device__ inline Side extend(const uint8_t* R, const uint8_t* T, uint64_t r0, uint64_t t0, uint64_t K, bool on, int32_t pen,
                              int64_t x_drop, uint32_t gl, uint32_t lane) {
    uint64_t base = 0;          // steps the rounds before this one took
    long long s_carry = 0;      // s at base
    long long bestv = 0;        // the running maximum of s up to base: s_bestk
    uint64_t bestk = 0, bestm = 0, m_carry = 0;  // ... where it was first reached, equal characters below it / below base
    bool done = !on || K == 0;
    while (__ballot(!done)) {
        const uint64_t j0 = base + (uint64_t)gl * SEG;  // the lane's steps: j0 + 1 .. j0 + nv
        const uint32_t nv = (!done && j0 < K) ? (uint32_t)(K - j0 < SEG ? K - j0 : SEG) : 0u;
        uint32_t eq = 0;  // bit t: step j0 + t + 1 compares equal
        if (nv == SEG) {
            const uint4 a = load16_unaligned(LEFT ? R + (r0 - j0 - SEG) : R + (r0 + j0));
            const uint4 b = load16_unaligned(LEFT ? T + (t0 - j0 - SEG) : T + (t0 + j0));
            eq = zero_bytes(a.x ^ b.x) | zero_bytes(a.y ^ b.y) << 4 | zero_bytes(a.z ^ b.z) << 8 | zero_bytes(a.w ^ b.w) << 12;
            if (LEFT) eq = __brev(eq) >> 16;  // (the nearest character is the last byte)
        } else {
            for (uint32_t t = 0; t < nv; ++t) {
                const uint8_t a = LEFT ? R[r0 - j0 - t - 1] : R[r0 + j0 + t];
                const uint8_t b = LEFT ? T[t0 - j0 - t - 1] : T[t0 + j0 + t];
                eq |= a == b ? 1u << t : 0u;
            }
        }
        // the segment alone: prefix sums p_1 .. p_nv above p_0 = 0
        int32_t p = 0, maxp = 0, minp = 0, drop0 = 0;
        uint32_t argp = 0;  // the smallest u with p_u = maxp
#pragma unroll
        for (int t = 0; t < SEG; ++t)
            if ((uint32_t)t < nv) {
                p += (eq >> t) & 1u ? 1 : -pen;
                if (p > maxp) {
                    maxp = p;
                    argp = t + 1;
                }
                minp = (t == 0 || p < minp) ? p : minp;
                drop0 = max(drop0, maxp - p);
            }
        // the round: where every segment starts (s, equal characters) and the running maximum above its start
        int32_t s_incl = p, m_incl = (int32_t)__popc(eq);
#pragma unroll
        for (int d = 1; d < G; d <<= 1) {
            const int32_t so = __shfl_up(s_incl, d, G), mo = __shfl_up(m_incl, d, G);
            if (gl >= (uint32_t)d) {
                s_incl += so;
                m_incl += mo;
            }
        }
        const long long s0 = s_carry + (s_incl - p);  // s at the segment's start
        long long cand = s0 + maxp;                   // the largest s inside the segment (or at its start)
        long long g_incl = cand;
#pragma unroll
        for (int d = 1; d < G; d <<= 1) {
            const long long go = __shfl_up(g_incl, d, G);
            if (gl >= (uint32_t)d && go > g_incl) g_incl = go;
        }
        long long g0 = __shfl_up(g_incl, 1, G);  // the largest s of the segments before, and of the rounds before
        g0 = (gl == 0 || g0 < bestv) ? bestv : g0;
        const long long worst = max(g0 - (s0 + minp), (long long)drop0);
        const bool stops = nv > 0 && worst > x_drop;
        const unsigned long long stop_mask = group_ballot<G>(stops, lane);
        const uint32_t first = stop_mask ? (uint32_t)__ffsll(stop_mask) - 1 : (uint32_t)G;  // the lane the extension stops in
        if (__ballot(stops)) {
            // the exact step, and the segment's largest prefix below it (lane `first` alone is listened to)
            long long s = s0, g = g0;
            int32_t q = 0, qmax = 0;
            uint32_t qarg = 0;
            bool hit = false;
#pragma unroll
            for (int t = 0; t < SEG; ++t)
                if ((uint32_t)t < nv && !hit) {
                    const int32_t d = (eq >> t) & 1u ? 1 : -pen;
                    s += d;
                    q += d;
                    if (s > g) g = s;
                    if (g - s > x_drop) {
                        hit = true;
                    } else if (q > qmax) {
                        qmax = q;
                        qarg = t + 1;
                    }
                }
            if (gl == first) {  // (s at the stopping step is below the maximum: the prefixes before it are all there is)
                cand = s0 + qmax;
                argp = qarg;
            }
        }
        // the largest s of this round, in the first lane that has it; a larger one than before moves the best
        const bool eligible = nv > 0 && gl <= first;
        const long long rmax = group_max<G>(eligible ? cand : (long long)INT64_MIN);
        const unsigned long long win_mask = group_ballot<G>(eligible && cand == rmax, lane);
        const uint32_t winner = win_mask ? (uint32_t)__ffsll(win_mask) - 1 : 0u;
        const uint32_t w_arg = __shfl(argp, winner, G);
        const uint32_t w_equal = __shfl((uint32_t)(m_incl - (int32_t)__popc(eq)) + (uint32_t)__popc(eq & ((1u << argp) - 1u)), winner, G);
        const int32_t round_s = __shfl(s_incl, G - 1, G), round_m = __shfl(m_incl, G - 1, G);
        if (!done) {
            if (win_mask && rmax > bestv) {
                bestv = rmax;
                bestk = base + (uint64_t)winner * SEG + w_arg;
                bestm = m_carry + w_equal;
            }
            s_carry += round_s;
            m_carry += (uint64_t)(uint32_t)round_m;
            base += (uint64_t)G * SEG;
            done = stop_mask != 0 || base >= K;
        }
    }
    Side r;
    r.len = (uint32_t)bestk;
    r.equal = (uint32_t)bestm;
    return r;
}

struct Placed {
    uint4 w0, w1;
    uint32_t placed, seed_len, extended;
};
__device__ inline Placed unplaced() {
    Placed r;
    r.w0 = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);
    r.w1 = make_uint4(0u, 0u, 0u, SPP_NO_DOC);
    r.placed = r.seed_len = r.extended = 0;
    return r;
}

// The record of the read at [o, e) (0 < e - o < 2^32 where on) by the group of G lanes the lane belongs to; every lane of
// the wavefront is inside.  Every lane of the group returns the record.
template <int BITS, int G>
__device__ inline Placed place_read(const PlaceArgs& a, uint64_t o, uint64_t e, bool on, uint32_t gl, uint32_t lane) {
    constexpr int V = BITS == 16 ? 8 : 4;
    const uint64_t m = on ? e - o : 0;
    // the seed
    const uint64_t c1 = on ? (e - 1) / V : 0;
    uint64_t c = o / V + gl;
    unsigned long long best = 0;
    while (__ballot(on && c <= c1)) {
        if (on && c <= c1) {
            const uint4 l = a.L[c];
            const uint32_t lw[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
            for (int t = 0; t < V; ++t) {
                const uint32_t v = BITS == 16 ? (lw[t >> 1] >> ((t & 1) * 16)) & 0xffffu : lw[t];
                const uint64_t i = c * V + t;
                // (a position below 2^32 - 1: ~position is never 0, and a key is never 0)
                const unsigned long long key = ((unsigned long long)v << 32) | (uint32_t)~(uint32_t)(i - o);
                if (i >= o && i < e && key > best) best = key;
            }
        }
        c += G;
    }
    best = group_maxu<G>(best);
    const uint64_t seed_pos = (uint32_t)~(uint32_t)best, seed_len = best >> 32;
    const bool placed = on && best != 0 && seed_len >= a.min_seed;
    const uint64_t ptr = placed ? a.P[o + seed_pos] : 0;
    const uint32_t doc = (placed && a.D) ? value_at<BITS>(a.D, o + seed_pos) : SPP_NO_DOC;
    // the extensions: K steps each, all of them inside the read and the text
    const uint64_t er = seed_pos + seed_len, te = ptr + seed_len;  // (te modulo 2^64)
    uint64_t kr = (placed && er < m) ? m - er : 0;
    const uint64_t room = te < a.n_text ? a.n_text - te : 0;
    kr = kr < room ? kr : room;
    const uint64_t kl = (placed && ptr <= a.n_text) ? (seed_pos < ptr ? seed_pos : ptr) : 0;
    const Side right = extend<G, false>(a.R, a.T, o + er, te, kr, placed, a.penalty, a.x_drop, gl, lane);
    const Side left = extend<G, true>(a.R, a.T, o + seed_pos, ptr, kl, placed, a.penalty, a.x_drop, gl, lane);
    if (!placed) return unplaced();
    Placed r;
    const uint64_t ref_start = ptr - left.len;
    r.w0 = make_uint4((uint32_t)ref_start, (uint32_t)(ref_start >> 32), (uint32_t)seed_pos - left.len, (uint32_t)(er + right.len));
    r.w1 = make_uint4((uint32_t)seed_len + left.equal + right.equal, (uint32_t)seed_pos, (uint32_t)seed_len, doc);
    r.placed = 1;
    r.seed_len = (uint32_t)seed_len;
    r.extended = left.len + right.len;
    return r;
}

template <int BITS>
__global__ __launch_bounds__(256) void k_place(PlaceArgs a) {
    constexpr uint32_t G = 16, PER_WAVE = 64 / G;
    const uint32_t lane = threadIdx.x & 63, gl = lane & (G - 1), grp = lane / G;
    const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (uint64_t)gridDim.x * 4;
    const uint64_t batch_lo = a.offs[0], batch_hi = batch_lo + a.total_values;
    unsigned long long n_placed = 0, n_seed = 0, n_ext = 0;
    if (wave == 0 && lane == 0) {
        const uint64_t end = a.offs[a.nreads];
        a.c->values = end < batch_lo ? 0 : end - batch_lo;
        if (end > batch_hi || batch_hi < batch_lo) atomicOr(&a.c->error, 2ull);
    }
    // (the trip count depends on the wavefront alone: the shuffles and ballots below are reached by all of its lanes)
    for (uint64_t q0 = wave * PER_WAVE; q0 < a.nreads; q0 += nwaves * PER_WAVE) {
        const uint64_t q = q0 + grp;
        const bool active = q < a.nreads;
        const uint64_t o = active ? a.offs[q] : 0, e = active ? a.offs[q + 1] : 0;
        const bool ordered = active && e >= o && o >= batch_lo && e - o < (1ull << 32);
        const bool sane = ordered && e <= batch_hi && batch_hi >= batch_lo;  // (a read behind what total_values said is not looked at)
        if (active && gl == 0 && !sane) atomicOr(&a.c->error, ordered ? 2ull : 1ull);
        const bool is_long = sane && e - o > LONG_MIN_VALUES;
        const Placed r = place_read<BITS, G>(a, o, e, sane && e > o && !is_long, gl, lane);
        if (active && !is_long && gl == 0) {
            a.out[2 * q] = r.w0;
            a.out[2 * q + 1] = r.w1;
            n_placed += r.placed;
            n_seed += r.seed_len;
            n_ext += r.extended;
        }
        unsigned long long long_mask = __ballot(is_long && gl == 0);
        while (long_mask) {
            const int src = __ffsll(long_mask) - 1;
            long_mask &= long_mask - 1;
            const uint64_t lo = __shfl(o, src), le = __shfl(e, src);
            const Placed w = place_read<BITS, 64>(a, lo, le, true, lane, lane);
            if (lane == 0) {
                const uint64_t lq = q0 + (uint32_t)src / G;
                a.out[2 * lq] = w.w0;
                a.out[2 * lq + 1] = w.w1;
                n_placed += w.placed;
                n_seed += w.seed_len;
                n_ext += w.extended;
            }
        }
    }
    n_placed = wave_sum(n_placed);
    n_seed = wave_sum(n_seed);
    n_ext = wave_sum(n_ext);
    if (lane == 0 && n_placed) {
        atomicAdd(&a.c->placed, n_placed);
        atomicAdd(&a.c->seed_values, n_seed);
        atomicAdd(&a.c->extended_values, n_ext);
    }
}

// The placement kernel on st, between the index's two events.  Takes ix->mu.
int place_enqueue(spx_index* ix, PlaceArgs& a, int value_bits, hipStream_t st) {
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    a.T = ix->text;
    a.n_text = ix->n_text;
    return product_enqueue(ix->place, PLACE_WORDS, st, [&](void* counters) -> int {
        a.c = (PlaceCounters*)counters;
        if (!a.nreads) return SPX_OK;
        const unsigned grid = (unsigned)std::min<uint64_t>((a.nreads + 15) / 16, 8192);
        if (value_bits == 16)
            k_place<16><<<grid, 256, 0, st>>>(a);
        else
            k_place<32><<<grid, 256, 0, st>>>(a);
        SPX_HIP(hipGetLastError());
        return SPX_OK;
    });
}
int place_error_code(const spx_index* ix) {
    if (ix->place.error & 1) {
        set_error("a read has 2^32 values or more (or its offsets decrease): the placements take reads below that");
        return SPX_E_FORMAT;
    }
    if (ix->place.error & 2) {
        set_error("the batch holds more values than total_values said: the reads behind it are not placed");
        return SPX_E_FORMAT;
    }
    return SPX_OK;
}

int check_params(const spx_index* ix, uint64_t min_seed, uint32_t mismatch_penalty, uint64_t x_drop) {
    if (!ix) {
        set_error("index must be non-null");
        return SPX_E_ARG;
    }
    if (min_seed == 0) {
        set_error("min_seed must be at least 1: a position of length 0 matches nothing");
        return SPX_E_ARG;
    }
    if (mismatch_penalty > 65535u) {
        set_error("mismatch_penalty must be 0 .. 65535");
        return SPX_E_ARG;
    }
    if (x_drop > 0x7fffffffull) {
        set_error("x_drop must be 0 .. 2^31 - 1");
        return SPX_E_ARG;
    }
    return SPX_OK;
}

}  // namespace

void release_place(spx_index* ix) { release(ix->place_scr, 2, &ix->place); }

}  // namespace spx

using namespace spx;

extern "C" {

int spp_place_device(spx_index* ix, const uint8_t* d_seqs, const void* d_lengths, int value_bits, const uint64_t* d_pointers,
                     const void* d_docs, const uint64_t* d_offsets, uint64_t nreads, uint64_t total_values, uint64_t min_seed,
                     uint32_t mismatch_penalty, uint64_t x_drop, spp_placement* d_out, void* stream) {
    int rc = check_params(ix, min_seed, mismatch_penalty, x_drop);
    if (rc != SPX_OK) return rc;
    if (value_bits != 16 && value_bits != 32) {
        set_error("value_bits must be 16 or 32 (the width of d_lengths and d_docs)");
        return SPX_E_ARG;
    }
    if (!ix->text) {
        set_error("the placements compare the reads with the text, and the index holds none (spx_index_set_text / "
                  "spx_index_rebuild_text)");
        return SPX_E_ARG;
    }
    if (nreads && (!d_seqs || !d_lengths || !d_pointers || !d_offsets || !d_out)) {
        set_error("d_seqs, d_lengths, d_pointers, d_offsets and d_out must be non-null");
        return SPX_E_ARG;
    }
    if ((((uintptr_t)d_lengths | (uintptr_t)d_out) & 15) != 0 || (((uintptr_t)d_offsets | (uintptr_t)d_pointers) & 7) != 0 ||
        ((uintptr_t)d_docs & (value_bits == 16 ? 1 : 3)) != 0) {
        set_error("d_lengths and d_out must be 16-byte aligned (the lengths are read as 16-byte vectors), the 64-bit arrays "
                  "8-byte and d_docs to its values");
        return SPX_E_ARG;
    }
    product_reset(ix, ix->place);
    PlaceArgs a{};
    a.R = d_seqs;
    a.L = (const uint4*)d_lengths;
    a.P = d_pointers;
    a.D = d_docs;
    a.offs = d_offsets;
    a.nreads = nreads;
    a.total_values = total_values;
    a.min_seed = min_seed;
    a.penalty = (int32_t)mismatch_penalty;
    a.x_drop = (int64_t)x_drop;
    a.out = (uint4*)d_out;
    return place_enqueue(ix, a, value_bits, (hipStream_t)stream);
}

int spp_last_place_stats(spx_index* ix, spp_place_stats* out) {
    if (!ix || !out) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    if (!ix->place.have) {
        set_error("no placements have been computed on this index yet");
        return SPX_E_ARG;
    }
    if (ix->place.pending) {
        const int rc = product_collect(ix, ix->place, PLACE_WORDS, 4);
        if (rc != SPX_OK) return rc;
    }
    out->values = ix->place.acc[0];
    out->placed = ix->place.acc[1];
    out->seed_values = ix->place.acc[2];
    out->extended_values = ix->place.acc[3];
    out->kernel_ms = ix->place.ms;
    return place_error_code(ix);
}

// The staged walk (spx_stage.hip) with the placement kernel behind every piece's walk.  The kernel reads the digested
// reads at the offsets of the concatenation: the one product that sets reads_characters.
int spp_place_batch(spx_index* ix, int digest_kind, uint32_t k, uint32_t w, const uint8_t* seqs, const uint64_t* offsets,
                    uint64_t nreads, uint64_t min_seed, uint32_t mismatch_penalty, uint64_t x_drop, int want_docs,
                    spp_placement* out, uint64_t* out_values) {
    if (spx_device_count() <= 0) {
        set_error("no HIP device visible: the placements are computed on the GPU and there is no CPU fallback");
        return SPX_E_NODEVICE;
    }
    int rc = check_params(ix, min_seed, mismatch_penalty, x_drop);
    if (rc != SPX_OK) return rc;
    if ((rc = check_batch(ix, "the placements", BATCH_TEXT, 0, digest_kind, want_docs,
                          nreads && (!seqs || !offsets || !out) ? "seqs, offsets and out must be non-null" : nullptr, offsets, nreads)) != SPX_OK)
        return rc;
    std::lock_guard<std::mutex> hg(ix->host_mu);
    SPX_HIP(hipSetDevice(ix->device));
    product_reset(ix, ix->place);
    if (nreads == 0) {
        ix->place.have = true;  // (the stats of an empty batch are zeros)
        return SPX_OK;
    }
    StageJob job;
    job.digest_kind = digest_kind;
    job.k = k;
    job.w = w;
    job.seqs = seqs;
    job.offsets = offsets;
    job.nreads = nreads;
    job.out_values = out_values;
    job.want_docs = want_docs != 0;
    job.reads_characters = true;
    StagePlan plan;
    if ((rc = stage_streams(ix, job.streams)) != SPX_OK) return rc;
    if ((rc = stage_plan(ix, job, &plan)) != SPX_OK) return rc;
    void* d_out[2] = {};
    for (int b = 0; b < plan.sets; ++b)
        if ((rc = ix->place_scr[b].reserve((plan.worst_reads + 1) * sizeof(spp_placement), &d_out[b])) != SPX_OK) return rc;
    job.wait = [](hipStream_t st) -> int {
        SPX_HIP(hipStreamSynchronize(st));
        return SPX_OK;
    };
    job.enqueue = [&](const StageView& v) -> int {
        PlaceArgs a{};
        a.R = v.reads;
        a.L = (const uint4*)v.lengths;
        a.P = v.pointers;
        a.D = v.docs;
        a.offs = v.offs;
        a.nreads = v.nreads;
        a.total_values = v.total_values;
        a.min_seed = min_seed;
        a.penalty = (int32_t)mismatch_penalty;
        a.x_drop = (int64_t)x_drop;
        a.out = (uint4*)d_out[v.set];
        const int r = place_enqueue(ix, a, v.value_bits, v.stream);
        if (r != SPX_OK) return r;
        SPX_HIP(hipMemcpyAsync(out + v.q0, d_out[v.set], v.nreads * sizeof(spp_placement), hipMemcpyDeviceToHost, v.stream));
        return SPX_OK;
    };
    job.collect = [&](const StageView&) -> int {
        const int r = product_collect(ix, ix->place, PLACE_WORDS, 4);
        return r != SPX_OK ? r : place_error_code(ix);
    };
    QuietOnError quiet(nullptr, true);  // (two streams: a failed call waits for the device)
    return quiet.done(stage_run(ix, job, plan));
}

}  // extern "C"
