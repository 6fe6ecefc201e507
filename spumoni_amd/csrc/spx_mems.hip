// spx_mems.hip -- the matches (include/spumoni_mems.h): per read, the positions where a new exact match
// starts (L[i] >= L[i - 1], or the read's first position) and is at least min_length long, as 16-byte records in read
// order with a CSR array of where each read's records start.
//
// A streaming pass over the values, count -> scan -> write; no kernel is shaped by the reads, so one read of 10^6 values
// among short ones is spread like everything else.  Positions are counted in 64-value WORDS of the concatenated arrays,
// aligned at multiples of 64 (word 0 holds d_offsets[0]):
//   k_mems_mark     a lane per aligned 16-byte vector of lengths (8 or 4 values): the predecessor of a vector's first
//                   value comes from the lane before; the lanes of a word OR their bits together and one stores the word.
//                   The bit of position i says L[i] >= min_length and L[i] >= L[i - 1], whatever read i - 1 belongs to;
//   k_mems_force    a lane per read: the bit of a read's first position is set when its length alone says so (atomicOr:
//                   the word does not depend on who comes first);
//   hipcub scan     exclusive sums of the words' popcounts: the rank of every word's first record;
//   k_mems_offsets  a lane per read: match_offsets[q] = rank of d_offsets[q] = prefix + a masked popcount;
//   k_mems_write    a lane per word: one binary search in d_offsets for the read of the word's first set bit, then along
//                   the bits and the reads; pointer, id and length are loaded at set bits only and the record leaves as
//                   one 16-byte store at its rank -- below out_capacity.  The longest length goes through atomicMax.
// Every record's place is its rank: the same input gives the same bytes.
#include <algorithm>
#include <cstring>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "../../include/spumoni_mems.h"
#include "spx_internal.h"

namespace spx {
namespace {

struct MemCounters {  // device; zeroed in front of every count
    unsigned long long values, matches, longest;
    unsigned long long error;  // bit 0: a read of 2^32 values or more, or decreasing offsets; bit 1: more values than total_values said
};
// (longest is a maximum, not a sum: every call resets before it enqueues and collects once, so product_collect's adding is
// assigning)
constexpr int MEM_WORDS = sizeof(MemCounters) / 8;
struct MemArgs {
    const uint4* L;
    const uint64_t* P;
    const void* D;
    const uint64_t* offs;
    uint64_t nreads, min_length;
    uint64_t* bits;    // nwords + 1 words (the last one stays 0)
    uint64_t* prefix;  // nwords + 1 sums
    uint64_t nwords;
    uint64_t* moffs;
    uint4* out;
    uint64_t cap;
    uint32_t* out_docs;
    MemCounters* c;
};
// the positions the call looks at: [base, end), end held to what the scratch was sized for; a0: first position of word 0
struct Span {
    uint64_t base, end, a0, true_end;
};
__device__ inline Span span_of(const MemArgs& a) {
    Span s;
    s.base = a.offs[0];
    s.true_end = a.offs[a.nreads] < s.base ? s.base : a.offs[a.nreads];
    s.a0 = s.base & ~63ull;
    const uint64_t lim = s.a0 + a.nwords * 64;
    s.end = s.true_end < lim ? s.true_end : lim;
    return s;
}
template <int BITS>
__device__ inline uint32_t value_at(const void* p, uint64_t i) {
    return BITS == 16 ? (uint32_t)((const uint16_t*)p)[i] : ((const uint32_t*)p)[i];
}

template <int BITS>
__global__ __launch_bounds__(256) void k_mems_mark(MemArgs a) {
    constexpr int V = BITS == 16 ? 8 : 4, LPW = 64 / V;  // values per vector, lanes per word
    const Span s = span_of(a);
    const uint64_t total = (a.nwords + 1) * LPW;
    const uint32_t lane = threadIdx.x & 63;
    // (the trip count depends on the wavefront alone: the shuffles below are reached by all of its lanes)
    for (uint64_t g0 = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); g0 < total; g0 += (uint64_t)gridDim.x * 256) {
        const uint64_t g = g0 + lane;
        const uint64_t p0 = s.a0 + g * V;
        const bool live = g < total && p0 < s.end && p0 + V > s.base;
        uint4 l = make_uint4(0, 0, 0, 0);
        if (live) l = a.L[p0 / V];
        const uint32_t lw[4] = {l.x, l.y, l.z, l.w};
        uint32_t v[V];
#pragma unroll
        for (int t = 0; t < V; ++t) v[t] = BITS == 16 ? (lw[t >> 1] >> ((t & 1) * 16)) & 0xffffu : lw[t];
        uint32_t prev = __shfl_up(v[V - 1], 1);
        if (lane == 0 && live && p0 > s.base) prev = value_at<BITS>(a.L, p0 - 1);
        uint32_t m = 0;
#pragma unroll
        for (int t = 0; t < V; ++t) {
            const uint64_t i = p0 + t;
            // (i == base starts a read: k_mems_force sets its bit, whatever lies in front of the batch)
            if (live && i > s.base && i < s.end && (uint64_t)v[t] >= a.min_length && v[t] >= prev) m |= 1u << t;
            prev = v[t];
        }
        unsigned long long word = (unsigned long long)m << (V * (lane % LPW));
#pragma unroll
        for (int d = 1; d < LPW; d <<= 1) word |= __shfl_xor(word, d);
        if (lane % LPW == 0 && g < total) a.bits[g / LPW] = word;
    }
}

template <int BITS>
__global__ __launch_bounds__(256) void k_mems_force(MemArgs a) {
    const Span s = span_of(a);
    for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < a.nreads; q += (uint64_t)gridDim.x * 256) {
        const uint64_t o = a.offs[q], e = a.offs[q + 1];
        if (e < o || e - o >= (1ull << 32)) {
            atomicOr(&a.c->error, 1ull);
            continue;
        }
        if (e == o || o < s.base || o >= s.end) continue;
        if ((uint64_t)value_at<BITS>(a.L, o) >= a.min_length)
            atomicOr((unsigned long long*)&a.bits[(o - s.a0) >> 6], 1ull << ((o - s.a0) & 63));
    }
}

struct Popcount {
    __host__ __device__ uint64_t operator()(const uint64_t& w) const {
#if defined(__HIP_DEVICE_COMPILE__)
        return (uint64_t)__popcll(w);
#else
        return (uint64_t)__builtin_popcountll(w);
#endif
    }
};
using PopcountIter = hipcub::TransformInputIterator<uint64_t, Popcount, const uint64_t*>;

__global__ __launch_bounds__(256) void k_mems_offsets(MemArgs a) {
    const Span s = span_of(a);
    for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q <= a.nreads; q += (uint64_t)gridDim.x * 256) {
        uint64_t pos = a.offs[q];
        pos = pos < s.base ? s.base : (pos > s.end ? s.end : pos);
        const uint64_t r = pos - s.a0, w = r >> 6;  // w <= nwords
        const uint64_t rank = a.prefix[w] + (uint64_t)__popcll(a.bits[w] & ((1ull << (r & 63)) - 1));
        a.moffs[q] = rank;
        if (q == a.nreads) {
            a.c->matches = rank;
            a.c->values = s.true_end - s.base;
            if (s.true_end > s.end) atomicOr(&a.c->error, 2ull);
        }
    }
}

template <int BITS, bool DOCS>
__global__ __launch_bounds__(256) void k_mems_write(MemArgs a) {
    const Span s = span_of(a);
    uint32_t longest = 0;
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < a.nwords; w += (uint64_t)gridDim.x * 256) {
        unsigned long long word = a.bits[w];
        if (!word) continue;
        uint64_t rank = a.prefix[w];
        const uint64_t p0 = s.a0 + w * 64;
        // the read of the first set position: the last one that starts at or before it (offs[0] = base does)
        const uint64_t first = p0 + (uint64_t)__ffsll(word) - 1;
        uint64_t lo = 0, hi = a.nreads;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (a.offs[mid] <= first)
                lo = mid + 1;
            else
                hi = mid;
        }
        uint64_t q = lo ? lo - 1 : 0;
        uint64_t qo = a.offs[q], qe = a.offs[q + 1];
        while (word) {
            const uint64_t i = p0 + (uint64_t)__ffsll(word) - 1;
            word &= word - 1;
            while (i >= qe && q + 1 < a.nreads) {  // (empty reads are passed here)
                ++q;
                qo = qe;
                qe = a.offs[q + 1];
            }
            const uint32_t len = value_at<BITS>(a.L, i);
            longest = max(longest, len);
            if (rank < a.cap) {
                const uint64_t p = a.P[i];
                a.out[rank] = make_uint4((uint32_t)p, (uint32_t)(p >> 32), (uint32_t)(i - qo), len);
                if (DOCS) a.out_docs[rank] = value_at<BITS>(a.D, i);
            }
            ++rank;
        }
    }
    for (int d = 32; d > 0; d >>= 1) longest = max(longest, (uint32_t)__shfl_xor(longest, d));
    if ((threadIdx.x & 63) == 0 && longest) atomicMax(&a.c->longest, (unsigned long long)longest);
}

uint64_t words_for(uint64_t total_values) { return total_values / 64 + 2; }  // (base need not be a multiple of 64)

// mark, force, scan and offsets on st: d_match_offsets complete, the bitmap and the ranks left in the scratch.  Opens the
// product: the count is its step 0, and what follows belongs to no step (in the host form, a wait).  Takes ix->mu.
int mems_enqueue_count(spx_index* ix, MemArgs& a, int value_bits, uint64_t total_values, hipStream_t st) {
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    int rc;
    a.nwords = words_for(total_values);
    if (a.nwords + 1 >= (1ull << 31)) {
        set_error("total_values is too large for one call (2^37 values)");
        return SPX_E_ARG;
    }
    const int items = (int)(a.nwords + 1);
    size_t cub_bytes = 0;
    SPX_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, PopcountIter(nullptr, Popcount()), (uint64_t*)nullptr, items, st));
    void* p = nullptr;
    if ((rc = ix->mems_scr[spx_index::M_BITS].reserve((a.nwords + 1) * 8, &p)) != SPX_OK) return rc;
    a.bits = (uint64_t*)p;
    if ((rc = ix->mems_scr[spx_index::M_PREFIX].reserve((a.nwords + 1) * 8, &p)) != SPX_OK) return rc;
    a.prefix = (uint64_t*)p;
    void* cub = nullptr;
    if ((rc = ix->mems_scr[spx_index::M_CUB].reserve(cub_bytes + 256, &cub)) != SPX_OK) return rc;
    if ((rc = product_open(ix->mems, MEM_WORDS, st, 0, &p)) != SPX_OK) return rc;
    a.c = (MemCounters*)p;
    const uint64_t lanes = (a.nwords + 1) * (value_bits == 16 ? 8 : 16);
    const unsigned mark_grid = (unsigned)std::min<uint64_t>((lanes + 255) / 256, 4096);
    const unsigned read_grid = (unsigned)std::min<uint64_t>((a.nreads + 256) / 256, 2048);
    if (value_bits == 16) {
        k_mems_mark<16><<<mark_grid, 256, 0, st>>>(a);
        k_mems_force<16><<<read_grid, 256, 0, st>>>(a);
    } else {
        k_mems_mark<32><<<mark_grid, 256, 0, st>>>(a);
        k_mems_force<32><<<read_grid, 256, 0, st>>>(a);
    }
    SPX_HIP(hipGetLastError());
    SPX_HIP(hipcub::DeviceScan::ExclusiveSum(cub, cub_bytes, PopcountIter(a.bits, Popcount()), a.prefix, items, st));
    k_mems_offsets<<<read_grid, 256, 0, st>>>(a);
    SPX_HIP(hipGetLastError());
    return product_mark(ix->mems, -1, st);
}

// the records of rank < a.cap, behind mems_enqueue_count on the same stream: step 1, and the product is closed.  Takes ix->mu.
int mems_enqueue_write(spx_index* ix, const MemArgs& a, int value_bits, hipStream_t st) {
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    int rc;
    if ((rc = product_mark(ix->mems, 1, st)) != SPX_OK) return rc;
    const unsigned grid = (unsigned)std::min<uint64_t>((a.nwords + 255) / 256, 4096);
    const bool docs = a.D != nullptr;
    if (value_bits == 16) {
        if (docs)
            k_mems_write<16, true><<<grid, 256, 0, st>>>(a);
        else
            k_mems_write<16, false><<<grid, 256, 0, st>>>(a);
    } else {
        if (docs)
            k_mems_write<32, true><<<grid, 256, 0, st>>>(a);
        else
            k_mems_write<32, false><<<grid, 256, 0, st>>>(a);
    }
    SPX_HIP(hipGetLastError());
    ix->mems_capacity = a.cap;
    return product_close(ix->mems, st);
}

void mems_reset(spx_index* ix) {
    product_reset(ix, ix->mems);
    std::lock_guard<std::mutex> g(ix->mu);
    ix->mems_capacity = 0;
    ix->mems_ready.ok = false;
}
int mems_error_code(const spx_index* ix) {
    if (ix->mems.error & 1) {
        set_error("a read has 2^32 values or more (or its offsets decrease): the matches take reads below that");
        return SPX_E_FORMAT;
    }
    if (ix->mems.error & 2) {
        set_error("the batch holds more values than total_values said: the output is undefined");
        return SPX_E_FORMAT;
    }
    return SPX_OK;
}

}  // namespace

void release_mems(spx_index* ix) { release(ix->mems_scr, spx_index::M_COUNT, &ix->mems); }

}  // namespace spx

using namespace spx;

extern "C" {

int spm_mems_device(spx_index* ix, const void* d_lengths, int value_bits, const uint64_t* d_pointers, const void* d_docs,
                    const uint64_t* d_offsets, uint64_t nreads, uint64_t total_values, uint64_t min_length,
                    uint64_t* d_match_offsets, spm_match* d_out, uint64_t out_capacity, uint32_t* d_out_docs, void* stream) {
    if (!ix) {
        set_error("index must be non-null");
        return SPX_E_ARG;
    }
    if (value_bits != 16 && value_bits != 32) {
        set_error("value_bits must be 16 or 32 (the width of d_lengths and d_docs)");
        return SPX_E_ARG;
    }
    if (min_length == 0) {
        set_error("min_length must be at least 1: a position of length 0 matches nothing");
        return SPX_E_ARG;
    }
    if (!d_match_offsets || (nreads && (!d_lengths || !d_pointers || !d_offsets))) {
        set_error("d_lengths, d_pointers, d_offsets and d_match_offsets must be non-null");
        return SPX_E_ARG;
    }
    if (out_capacity && (!d_out || (d_docs && !d_out_docs))) {
        set_error("d_out (and, with d_docs, d_out_docs) must be non-null unless out_capacity is 0");
        return SPX_E_ARG;
    }
    if ((((uintptr_t)d_lengths | (uintptr_t)d_docs | (uintptr_t)d_out) & 15) != 0 ||
        (((uintptr_t)d_offsets | (uintptr_t)d_pointers | (uintptr_t)d_match_offsets) & 7) != 0 || ((uintptr_t)d_out_docs & 3) != 0) {
        set_error("d_lengths, d_docs and d_out must be 16-byte aligned (the lengths are read as 16-byte vectors), the 64-bit "
                  "arrays 8-byte and d_out_docs 4-byte aligned");
        return SPX_E_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    mems_reset(ix);
    if (nreads == 0) {
        SPX_HIP(hipSetDevice(ix->device));
        SPX_HIP(hipMemsetAsync(d_match_offsets, 0, 8, st));
        return SPX_OK;
    }
    MemArgs a{};
    a.L = (const uint4*)d_lengths;
    a.P = d_pointers;
    a.D = d_docs;
    a.offs = d_offsets;
    a.nreads = nreads;
    a.min_length = min_length;
    a.moffs = d_match_offsets;
    a.out = (uint4*)d_out;
    a.cap = out_capacity;
    a.out_docs = d_out_docs;
    int rc;
    if ((rc = mems_enqueue_count(ix, a, value_bits, total_values, st)) != SPX_OK) return rc;
    return mems_enqueue_write(ix, a, value_bits, st);
}

int spm_last_mems_stats(spx_index* ix, spm_mems_stats* out) {
    if (!ix || !out) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    const spx_index::Product& p = ix->mems;
    if (p.pending) {
        const int rc = product_collect(ix, ix->mems, MEM_WORDS, MEM_WORDS - 1);
        if (rc != SPX_OK) return rc;
    }
    out->values = p.acc[0];
    out->matches = p.acc[1];
    out->written = std::min(p.acc[1], ix->mems_capacity);
    out->longest = p.acc[2];
    out->kernel_ms = p.step_ms[0] + p.step_ms[1];  // (count and write: not what lies between them)
    return mems_error_code(ix);
}

int spm_mems_begin(spx_index* ix, int digest_kind, uint32_t k, uint32_t w, const uint8_t* seqs, const uint64_t* offsets,
                   uint64_t nreads, uint64_t min_length, int want_docs, uint64_t* match_offsets, uint64_t* out_values,
                   uint64_t* n_matches) {
    if (spx_device_count() <= 0) {
        set_error("no HIP device visible: the matches are found on the GPU and there is no CPU fallback");
        return SPX_E_NODEVICE;
    }
    if (!ix || !match_offsets || !n_matches) {
        set_error("index, match_offsets and n_matches must be non-null");
        return SPX_E_ARG;
    }
    const int rc = check_batch(ix, "the matches", BATCH_MIN_LENGTH | BATCH_TEXT, min_length, digest_kind, want_docs,
                               nreads && (!seqs || !offsets) ? "seqs and offsets must be non-null" : nullptr, offsets, nreads);
    if (rc != SPX_OK) return rc;
    std::lock_guard<std::mutex> hg(ix->host_mu);
    SPX_HIP(hipSetDevice(ix->device));
    mems_reset(ix);
    *n_matches = 0;
    match_offsets[0] = 0;
    if (nreads == 0) {
        ready_publish(ix->mems_ready, 0, 0);
        ix->mems_ready_docs = want_docs != 0;
        return SPX_OK;
    }
    return mems_begin_staged(ix, digest_kind, k, w, seqs, offsets, nreads, min_length, want_docs, match_offsets, out_values,
                             n_matches, false, {});
}

}  // extern "C"

namespace spx {

int mems_begin_staged(spx_index* ix, int digest_kind, uint32_t k, uint32_t w, const uint8_t* seqs, const uint64_t* offsets,
                      uint64_t nreads, uint64_t min_length, int want_docs, uint64_t* match_offsets, uint64_t* out_values,
                      uint64_t* n_matches, bool reads_characters, const std::function<int(const MemsOnDevice&)>& then) {
    mems_reset(ix);
    *n_matches = 0;
    match_offsets[0] = 0;
    // the staged walk (spx_stage.hip) with exactly one piece, on the handle's stream: the count kernels behind the walk,
    // and -- the host has waited and knows the number of records -- the write kernels
    StageJob job;
    job.digest_kind = digest_kind;
    job.k = k;
    job.w = w;
    job.seqs = seqs;
    job.offsets = offsets;
    job.nreads = nreads;
    job.out_values = out_values;
    job.want_docs = want_docs != 0;
    job.one_piece = true;
    job.reads_characters = reads_characters;
    int rc;
    if ((rc = ctx_stream_of(ix, &job.streams[0])) != SPX_OK) return rc;
    hipStream_t st = job.streams[0];
    StagePlan plan;
    if ((rc = stage_plan(ix, job, &plan)) != SPX_OK) return rc;
    void* d_moffs = nullptr;
    if ((rc = ix->mems_scr[spx_index::M_MOFFS].reserve((nreads + 1) * 8, &d_moffs)) != SPX_OK) return rc;
    MemArgs a{};
    uint64_t n = 0;
    job.wait = [&](hipStream_t s) -> int { return ctx_wait(ix, s); };
    job.enqueue = [&](const StageView& v) -> int {
        a.L = (const uint4*)v.lengths;
        a.P = v.pointers;
        a.D = v.docs;
        a.offs = v.offs;
        a.nreads = nreads;
        a.min_length = min_length;
        a.moffs = (uint64_t*)d_moffs;
        const int r = mems_enqueue_count(ix, a, v.value_bits, v.total_values, st);
        if (r != SPX_OK) return r;
        SPX_HIP(hipMemcpyAsync(match_offsets, d_moffs, (nreads + 1) * 8, hipMemcpyDeviceToHost, st));
        return SPX_OK;
    };
    job.collect = [&](const StageView& v) -> int {
        // the records, at their exact size
        n = match_offsets[nreads];
        void *d_out = nullptr, *d_out_docs = nullptr;
        int r;
        if ((r = ix->mems_scr[spx_index::M_OUT].reserve(n * sizeof(spm_match) + 16, &d_out)) != SPX_OK) return r;
        if (want_docs && (r = ix->mems_scr[spx_index::M_OUT_DOCS].reserve(n * 4 + 16, &d_out_docs)) != SPX_OK) return r;
        a.out = (uint4*)d_out;
        a.out_docs = (uint32_t*)d_out_docs;
        a.cap = n;
        if ((r = mems_enqueue_write(ix, a, v.value_bits, st)) != SPX_OK) return r;
        if (then && (r = then(MemsOnDevice{v.reads, v.offs, (const uint64_t*)d_moffs, d_out, (const uint32_t*)d_out_docs, nreads, n, st})) != SPX_OK)
            return r;
        if ((r = product_collect(ix, ix->mems, MEM_WORDS, MEM_WORDS - 1)) != SPX_OK) return r;
        if (then && (r = ctx_wait(ix, st)) != SPX_OK) return r;
        return mems_error_code(ix);
    };
    QuietOnError quiet(st);  // (a failed call leaves nothing reading seqs / offsets or writing the outputs)
    if ((rc = stage_run(ix, job, plan)) != SPX_OK) return rc;
    *n_matches = n;
    if (!then) {  // (with `then` the records are its caller's: nothing waits for spm_mems_fetch)
        ready_publish(ix->mems_ready, n, nreads);
        ix->mems_ready_docs = want_docs != 0;
    }
    return quiet.done(SPX_OK);
}

}  // namespace spx

extern "C" {

int spm_mems_fetch(spx_index* ix, spm_match* out, uint32_t* out_docs) {
    if (!ix) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> hg(ix->host_mu);
    if (!ix->mems_ready.ok) {
        set_error("spm_mems_fetch without a successful spm_mems_begin");
        return SPX_E_ARG;
    }
    const uint64_t n = ix->mems_ready.n;
    if (n && (!out || (ix->mems_ready_docs && !out_docs))) {
        set_error("out (and, when ids were asked for, out_docs) must be non-null");
        return SPX_E_ARG;
    }
    SPX_HIP(hipSetDevice(ix->device));
    hipStream_t st = nullptr;
    int rc;
    if ((rc = ctx_stream_of(ix, &st)) != SPX_OK) return rc;
    if (n) {
        QuietOnError quiet(st);
        SPX_HIP(hipMemcpyAsync(out, ix->mems_scr[spx_index::M_OUT].p, n * sizeof(spm_match), hipMemcpyDeviceToHost, st));
        if (ix->mems_ready_docs)
            SPX_HIP(hipMemcpyAsync(out_docs, ix->mems_scr[spx_index::M_OUT_DOCS].p, n * 4, hipMemcpyDeviceToHost, st));
        if ((rc = ctx_wait(ix, st)) != SPX_OK) return rc;
        quiet.done(SPX_OK);
    }
    ix->mems_ready.ok = false;
    return SPX_OK;
}

}  // extern "C"
