// spx_genome_kernels.h -- what spx_cover.hip (the coverage) and spx_call.hip (the pileup and the calls) share: two products
// that accumulate spx_map.hip's mappings into arrays over the forward genome and report records over tiles of it.  On the
// device the sequence table, the tiles, the head of a mapping with its checks, the op predicates and the block's sums; on
// the host everything that works on a spx_index::GenomeAcc and differs between the two only in the words of a GenomeKind.
// Each translation unit gets its own copy (the library is built without relocatable device code).
#pragma once
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <initializer_list>

#include "../../include/spumoni_map.h"
#include "spx_internal.h"

namespace spx {
namespace {

constexpr uint32_t OP_I = SPG_OP_I, OP_D = SPG_OP_D, OP_N = SPG_OP_N, OP_S = SPE_OP_S, OP_EQ = SPG_OP_EQ, OP_X = SPG_OP_X;
constexpr int PER_THREAD = 16, TILE = 256 * PER_THREAD;  // positions of a tile: a block of 256 threads, 16 each

struct Table {
    const uint64_t* P;  // n_seqs * strands + 1
    uint64_t n_seqs;
    uint32_t strands;
    uint64_t G;
};

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

// The block's tile [t0, t1) of the forward genome and the thread's positions [p0, p1) in it (none: p0 >= p1)
struct Tile {
    uint64_t t0, t1, p0, p1;
};
__device__ inline Tile tile_of(uint64_t G) {
    Tile x;
    x.t0 = (uint64_t)blockIdx.x * TILE;
    x.t1 = x.t0 + TILE < G ? x.t0 + TILE : G;
    x.p0 = x.t0 + (uint64_t)threadIdx.x * PER_THREAD;
    x.p1 = x.p0 + PER_THREAD < x.t1 ? x.p0 + PER_THREAD : x.t1;
    return x;
}

struct MapHead {
    uint32_t s;
    bool rev;
    uint64_t pos, span, i0, ne;  // pos: F[s] + target_start; span: target_end - target_start
    uint64_t r0, len;            // READS: where the read's bytes start, and how many
};
// Read q's spn_mapping and entry offsets of an add's arguments (t, map, ioffs, in_entries), checked against the table;
// with READS the offsets of its bytes too (roffs, in_chars).  0: unmapped, 1: the record and the offsets pass, 2: they do not
template <bool READS, typename Args>
__device__ inline int map_head(const Args& a, uint64_t q, MapHead& h) {
    const uint4 w1 = a.map[3 * q + 1];
    if (w1.x == SPN_UNMAPPED) return 0;
    const uint4 w0 = a.map[3 * q];
    const uint64_t ts = (uint64_t)w0.x | ((uint64_t)w0.y << 32), te = (uint64_t)w0.z | ((uint64_t)w0.w << 32);
    const uint64_t i0 = a.ioffs[q], i1 = a.ioffs[q + 1];
    uint64_t r0 = 0, r1 = 0, in_chars = 0;
    if constexpr (READS) {
        r0 = a.roffs[q];
        r1 = a.roffs[q + 1];
        in_chars = a.in_chars;
    }
    if (w1.x >= a.t.n_seqs || i1 < i0 || i1 > a.in_entries || r1 < r0 || r1 > in_chars || ts > te) return 2;
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

// N sums leave a block of four wavefronts as one set of atomics
template <int N>
__device__ inline void block_counts(unsigned long long* part, unsigned long long* to, unsigned long long (&v)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = wave_sum(v[i]);
    const uint32_t wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) part[wv * N + i] = v[i];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const unsigned long long s = part[threadIdx.x] + part[N + threadIdx.x] + part[2 * N + threadIdx.x] + part[3 * N + threadIdx.x];
        if (s) atomicAdd(to + threadIdx.x, s);
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------

using GenomeAcc = spx_index::GenomeAcc;

// What tells the two products apart in the shared code: the words of their messages, the counter words of their three
// steps (the error bits last), how many of the add's words add up in acc, and the size of an output record.
struct GenomeKind {
    const char *reset, *what, *per_base;  // "spd_cover_reset", "the coverage", "about 12 per base"
    const char *begin, *fetch, *out_arg;  // "spd_cover_runs_begin", "spd_cover_runs_fetch", "out_runs"
    int words[3], nacc;
    size_t record_bytes;
};

inline Table table_of(const spx_index* ix) {
    return Table{ix->map_P, ix->map_seq_lengths.size(), ix->map_strands, ix->n_text / ix->map_strands};
}
inline uint64_t tiles_of(uint64_t G) { return (G + TILE - 1) / TILE; }

// exactly `bytes`: the arrays of a genome are not given the scratch buffers' head-room
inline int exact(spx_index::Scratch& sc, size_t bytes) {
    if (sc.cap >= bytes) return SPX_OK;
    if (sc.p) (void)hipFree(sc.p);
    sc.p = nullptr;
    sc.cap = 0;
    SPX_HIP(hipMalloc(&sc.p, bytes));
    sc.cap = bytes;
    return SPX_OK;
}

inline void add_reset(spx_index* ix, GenomeAcc& ga) {
    product_reset(ix, ga.step[GenomeAcc::ADD]);
    std::lock_guard<std::mutex> g(ix->mu);
    std::memset(ga.acc, 0, sizeof ga.acc);
}

// Waits for what a step enqueued last and takes its counters and its time.  Takes ix->mu.
inline int step_collect(spx_index* ix, GenomeAcc& ga, const GenomeKind& k, int step) {
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    spx_index::Product& p = ga.step[step];
    const int words = k.words[step];
    SPX_HIP(hipEventSynchronize(p.ev1));
    unsigned long long c[16] = {};
    SPX_HIP(hipMemcpy(c, p.counters.p, (size_t)words * 8, hipMemcpyDeviceToHost));
    SPX_HIP(hipEventElapsedTime(&ga.step_ms[step], p.ev0, p.ev1));
    if (step == GenomeAcc::ADD)
        for (int i = 0; i < k.nacc; ++i) ga.acc[i] += c[i];
    if (step == GenomeAcc::OUT) ga.n_out = c[0];
    p.error = step == GenomeAcc::OUT ? c[words - 1] : p.error | c[words - 1];
    p.pending = false;
    return SPX_OK;
}

inline int collect_all(spx_index* ix, GenomeAcc& ga, const GenomeKind& k) {
    int rc;
    for (int step = 0; step < 3; ++step)
        if (ga.step[step].pending && (rc = step_collect(ix, ga, k, step)) != SPX_OK) return rc;
    return SPX_OK;
}
inline bool have_any(const GenomeAcc& ga) { return ga.step[0].have || ga.step[1].have || ga.step[2].have; }

// The host forms' arrays are there and belong to the table in force.  The caller holds host_mu.
inline int need_arrays(spx_index* ix, const GenomeAcc& ga, const GenomeKind& k, const char* who) {
    int rc;
    if ((rc = need_table(ix, who)) != SPX_OK) return rc;
    if (ga.dropped) {
        set_error("%s: spn_set_sequences replaced the sequence table after %s and dropped %s: reset again", who, k.reset, k.what);
        return SPX_E_ARG;
    }
    if (!ga.G) {
        set_error("%s without a successful %s before it", who, k.reset);
        return SPX_E_ARG;
    }
    return SPX_OK;
}

// the arrays sized for a genome -- the product's first GenomeAcc::ARRAYS slots of its own -- and the records
static_assert(GenomeAcc::S_RECORDS + 1 == GenomeAcc::S_OWN && spx_index::D_OUT + 1 == GenomeAcc::S_OWN + GenomeAcc::ARRAYS &&
                  spx_index::PL_DEL + 1 == GenomeAcc::S_OWN + GenomeAcc::ARRAYS && spx_index::PL_ROFFS < GenomeAcc::S_COUNT,
              "drop_arrays frees S_RECORDS and the ARRAYS slots behind it; every slot lies in scr");
inline void drop_arrays(GenomeAcc& ga) {
    for (int i = GenomeAcc::S_RECORDS; i < GenomeAcc::S_OWN + GenomeAcc::ARRAYS; ++i) {
        spx_index::Scratch& sc = ga.scr[i];
        if (sc.p) (void)hipFree(sc.p);
        sc.p = nullptr;
        sc.cap = 0;
    }
    ga.G = 0;
    ga.ready = false;
}

inline void release_acc(GenomeAcc& ga) {
    for (auto& sc : ga.scr)
        if (sc.p) (void)hipFree(sc.p);
    for (auto& p : ga.step) product_release(p);
}

inline void acc_table_changed(GenomeAcc& ga) {
    // (a kernel of an earlier call may still read the old table or the arrays)
    for (auto& p : ga.step)
        if (p.have && p.ev1) (void)hipEventSynchronize(p.ev1);  // (a reset sets `have` for the stats and creates no event)
    if (!ga.G) return;
    drop_arrays(ga);
    ga.dropped = true;
}

// A reset's arrays: what must grow is summed and compared with the free memory before anything is allocated, each array
// gets exactly its bytes, those that accumulate are zeroed.  The caller holds host_mu and has set the device.
struct ArraySpec {
    int slot;
    size_t bytes;
    bool zeroed;
};
inline int reset_arrays(spx_index* ix, GenomeAcc& ga, const GenomeKind& k, uint64_t G, std::initializer_list<ArraySpec> arrays) {
    size_t need = 0;
    for (const ArraySpec& s : arrays)
        if (ga.scr[s.slot].cap < s.bytes) need += s.bytes;
    size_t free_b = 0, total_b = 0;
    SPX_HIP(hipMemGetInfo(&free_b, &total_b));
    int rc;
    {
        std::lock_guard<std::mutex> g(ix->mu);
        if (need > free_b) {
            set_error("%s: %s of %llu bases needs %llu more bytes of device memory (%s), %llu are free", k.reset, k.what,
                      (unsigned long long)G, (unsigned long long)need, k.per_base, (unsigned long long)free_b);
            return SPX_E_UNSUPPORTED;
        }
        for (const ArraySpec& s : arrays)
            if ((rc = exact(ga.scr[s.slot], s.bytes)) != SPX_OK) {
                drop_arrays(ga);
                return rc;
            }
    }
    hipStream_t st = nullptr;
    if ((rc = ctx_stream_of(ix, &st)) != SPX_OK) return rc;
    for (const ArraySpec& s : arrays)
        if (s.zeroed) SPX_HIP(hipMemsetAsync(ga.scr[s.slot].p, 0, s.bytes, st));
    if ((rc = ctx_wait(ix, st)) != SPX_OK) return rc;
    add_reset(ix, ga);
    ga.G = G;
    ga.dropped = false;
    ga.dirty = true;
    ga.ready = false;
    ga.step[GenomeAcc::ADD].have = true;  // (the stats of no adds are zeros)
    return SPX_OK;
}

// The list of one call and both add kernels on st, between the step's two events.  Takes ix->mu.
template <typename Args>
int add_enqueue(spx_index* ix, GenomeAcc& ga, const GenomeKind& k, Args& a, hipStream_t st, void (*lane)(Args), void (*wave)(Args)) {
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    a.t = table_of(ix);
    a.sw = (uint64_t)ga.sw;
    void* p = nullptr;
    int rc;
    if ((rc = ga.scr[GenomeAcc::S_LONG].reserve(a.nreads * 8 + 8, &p)) != SPX_OK) return rc;
    a.longs = (uint64_t*)p;
    return product_enqueue(ga.step[GenomeAcc::ADD], k.words[GenomeAcc::ADD], st, [&](void* counters) -> int {
        a.c = (decltype(a.c))counters;
        if (!a.nreads) return SPX_OK;
        const unsigned grid = (unsigned)std::min<uint64_t>((a.nreads + 255) / 256, 1024);
        lane<<<grid, 256, 0, st>>>(a);
        SPX_HIP(hipGetLastError());
        wave<<<(unsigned)std::min<uint64_t>((a.nreads + 3) / 4, 2048), 256, 0, st>>>(a);
        SPX_HIP(hipGetLastError());
        return SPX_OK;
    });
}

// The finish step: hipcub's inclusive sum of a difference array and what `then` enqueues behind it.  Takes ix->mu.
template <typename Then>
int finish_enqueue(spx_index* ix, GenomeAcc& ga, const GenomeKind& k, const uint32_t* d_diff, uint32_t* d_sum, hipStream_t st, Then&& then) {
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    const Table t = table_of(ix);
    size_t cub_bytes = 0;
    SPX_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, cub_bytes, d_diff, d_sum, t.G, (hipStream_t) nullptr));
    void* cub = nullptr;
    int rc;
    if ((rc = ga.scr[GenomeAcc::S_CUB].reserve(cub_bytes + 16, &cub)) != SPX_OK) return rc;
    return product_enqueue(ga.step[GenomeAcc::FIN], k.words[GenomeAcc::FIN], st, [&](void*) -> int {
        SPX_HIP(hipcub::DeviceScan::InclusiveSum(cub, cub_bytes, d_diff, d_sum, t.G, st));
        return then(t);
    });
}

// The host form of the finish, when something was added since the last one: `enqueue` is the product's finish on the
// handle's arrays.  The caller holds host_mu.
template <typename Enqueue>
int finish_host(spx_index* ix, GenomeAcc& ga, const GenomeKind& k, Enqueue&& enqueue) {
    if (!ga.dirty) return SPX_OK;
    hipStream_t st = nullptr;
    int rc;
    if ((rc = ctx_stream_of(ix, &st)) != SPX_OK) return rc;
    if ((rc = enqueue(st)) != SPX_OK) return rc;
    if ((rc = ctx_wait(ix, st)) != SPX_OK) return rc;
    if ((rc = step_collect(ix, ga, k, GenomeAcc::FIN)) != SPX_OK) return rc;
    ga.dirty = false;
    return SPX_OK;
}

// The records over the tiles (a: t, ntiles, tcnt, toffs, c), count -> exclusive sum -> write as in spx_mems.hip.  `count`
// launches the kernel that fills tcnt, `write` those that read toffs.  count without write: the tiles' counts and their
// scan only; write without count: the second half of the host form, which sizes its records from the count before it
// writes them.  Takes ix->mu.
template <typename Args, typename Count, typename Write>
int tiles_enqueue(spx_index* ix, GenomeAcc& ga, const GenomeKind& k, Args& a, hipStream_t st, bool count, bool write, Count&& do_count,
                  Write&& do_write) {
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    a.t = table_of(ix);
    a.ntiles = tiles_of(a.t.G);
    void* p = nullptr;
    int rc;
    if ((rc = ga.scr[GenomeAcc::S_TCNT].reserve((a.ntiles + 1) * 8, &p)) != SPX_OK) return rc;
    a.tcnt = (uint64_t*)p;
    if ((rc = ga.scr[GenomeAcc::S_TOFFS].reserve((a.ntiles + 1) * 8, &p)) != SPX_OK) return rc;
    a.toffs = (uint64_t*)p;
    size_t cub_bytes = 0;
    SPX_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, a.tcnt, a.toffs, a.ntiles + 1, (hipStream_t) nullptr));
    void* cub = nullptr;
    if ((rc = ga.scr[GenomeAcc::S_CUB2].reserve(cub_bytes + 16, &cub)) != SPX_OK) return rc;
    auto launch = [&](void* counters) -> int {
        a.c = (decltype(a.c))counters;
        if (count) {
            do_count();
            SPX_HIP(hipGetLastError());
            SPX_HIP(hipcub::DeviceScan::ExclusiveSum(cub, cub_bytes, a.tcnt, a.toffs, a.ntiles + 1, st));
        }
        return write ? do_write() : SPX_OK;
    };
    spx_index::Product& out = ga.step[GenomeAcc::OUT];
    if (count) return product_enqueue(out, k.words[GenomeAcc::OUT], st, launch);
    // the second half of the host form: the same counters, the step's end moved behind the write
    if ((rc = launch(out.counters.p)) != SPX_OK) return rc;
    SPX_HIP(hipEventRecord(out.ev1, st));
    return SPX_OK;
}

// The host form above it: `finish` brings the arrays up to date, then count, the one wait of the records' own, the records
// at their exact size (a.rec, a.cap), write.  `enqueue(a, st, count, write)` is the product's call of tiles_enqueue.  The
// caller holds host_mu and has checked the arrays.
template <typename Args, typename Finish, typename Enqueue>
int records_begin(spx_index* ix, GenomeAcc& ga, const GenomeKind& k, Args& a, uint64_t* n, Finish&& finish, Enqueue&& enqueue) {
    SPX_HIP(hipSetDevice(ix->device));
    ga.ready = false;
    hipStream_t st = nullptr;
    int rc;
    if ((rc = finish()) != SPX_OK) return rc;
    if ((rc = ctx_stream_of(ix, &st)) != SPX_OK) return rc;
    void* p = nullptr;
    if ((rc = ga.scr[GenomeAcc::S_NOUT].reserve(8, &p)) != SPX_OK) return rc;
    a.count = (uint64_t*)p;
    if ((rc = enqueue(a, st, true, false)) != SPX_OK) return rc;
    if ((rc = ctx_wait(ix, st)) != SPX_OK) return rc;
    uint64_t total = 0;
    SPX_HIP(hipMemcpy(&total, a.toffs + a.ntiles, 8, hipMemcpyDeviceToHost));
    if ((rc = ga.scr[GenomeAcc::S_RECORDS].reserve((total + 1) * k.record_bytes, &p)) != SPX_OK) return rc;
    a.rec = (decltype(a.rec))p;
    a.cap = total;
    if ((rc = enqueue(a, st, false, true)) != SPX_OK) return rc;
    if ((rc = ctx_wait(ix, st)) != SPX_OK) return rc;
    if ((rc = step_collect(ix, ga, k, GenomeAcc::OUT)) != SPX_OK) return rc;
    ga.ready = true;
    ga.ready_n = total;
    *n = total;
    return SPX_OK;
}

inline int records_fetch(spx_index* ix, GenomeAcc spx_index::*acc, const GenomeKind& k, void* out) {
    if (!ix) {
        set_error("index must be non-null");
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> hg(ix->host_mu);
    GenomeAcc& ga = ix->*acc;
    if (!ga.ready) {
        set_error("%s without a successful %s before it", k.fetch, k.begin);
        return SPX_E_ARG;
    }
    if (ga.ready_n && !out) {
        set_error("%s must be non-null", k.out_arg);
        return SPX_E_ARG;
    }
    ga.ready = false;
    if (!ga.ready_n) return SPX_OK;
    SPX_HIP(hipSetDevice(ix->device));
    SPX_HIP(hipMemcpy(out, ga.scr[GenomeAcc::S_RECORDS].p, ga.ready_n * k.record_bytes, hipMemcpyDeviceToHost));
    return SPX_OK;
}

// [first, first + count) lies in the forward genome the arrays were sized for
inline int check_range(const GenomeAcc& ga, const char* who, uint64_t first, uint64_t count) {
    if (first > ga.G || count > ga.G - first) {
        set_error("%s: [%llu, %llu + %llu) does not lie in the forward genome of %llu bases", who, (unsigned long long)first,
                  (unsigned long long)first, (unsigned long long)count, (unsigned long long)ga.G);
        return SPX_E_ARG;
    }
    return SPX_OK;
}

}  // namespace
}  // namespace spx
