// spx_build.hip -- the index builder (include/spumoni_build.h): text -> run-length BWT, thresholds, SA samples and
// document ids on one gfx950 device.  The output is bit-identical to synth.index_from_text.
//
// Phases (each one frees its temporaries before the next; peak about 33 bytes per character, in phase 1):
//   1  suffix array by prefix doubling over the groups that are still unsorted (Larsson-Sadakane): a first sort of
//      every suffix by its first 8 bytes, then rounds over the elements of non-singleton groups only, keyed by
//      (group head << 32) | rank[sa + h] with every key built before any rank changes;
//   2  LCP by Kasai's Phi method in chunks of CHUNK text positions, 8 bytes per compare;
//   3  BWT runs: run starts compacted, heads gathered;
//   5  SA samples at run starts / ends and their document ids (before 4: the SA can go then);
//   4  thresholds: runs paired with the previous run of the same letter by a stable sort on the head byte, every
//      interval answered by a range minimum over (LCP << 32) | pos: block minima + a sparse table over the blocks.
#include <hipcub/hipcub.hpp>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/spumoni_build.h"
#include "spx_internal.h"

struct spb_build {
    uint64_t n = 0, r = 0;
    bool samples = false;
    std::vector<uint8_t> heads;
    std::vector<uint32_t> starts, thr, ssa, esa;
    std::vector<uint16_t> ds, de;
};

namespace spx {
namespace {

constexpr int BT = 256;                  // threads per block
constexpr uint64_t LCP_CHUNK = 4096;     // text positions per thread of the PLCP pass (each starts from scratch)
constexpr uint32_t RMQ_SHIFT = 6;        // range-minimum blocks of 64 positions
constexpr uint32_t NONE = 0xffffffffu;   // Phi of the first suffix (positions are < n <= 2^32 - 1)
constexpr uint64_t TEXT_PAD = 16;        // zero bytes after the terminator: 8-byte windows never leave the buffer

inline unsigned nblk(uint64_t m) { return (unsigned)((m + BT - 1) / BT); }

struct Mem {  // device bytes held by the build, and the most it held at once
    uint64_t cur = 0, peak = 0;
};

struct Buf {  // RAII device buffer that counts itself in a Mem
    Mem* m = nullptr;
    void* p = nullptr;
    size_t bytes = 0;
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { release(); }
    hipError_t alloc(Mem& mem, size_t b) {
        release();
        m = &mem;
        hipError_t e = hipMalloc(&p, b ? b : 1);
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        bytes = b ? b : 1;
        m->cur += bytes;
        if (m->cur > m->peak) m->peak = m->cur;
        return hipSuccess;
    }
    void release() {
        if (p) {
            (void)hipFree(p);
            m->cur -= bytes;
        }
        p = nullptr;
        bytes = 0;
    }
    template <class T>
    T* as() const {
        return (T*)p;
    }
};

struct Stream {
    hipStream_t s = nullptr;
    ~Stream() {
        if (s) (void)hipStreamDestroy(s);
    }
};

// ---- phase 1: suffix array --------------------------------------------------------------------------------------

// the 8 bytes T[i .. i + 8) as a big-endian integer (integer order = lexicographic order), from two aligned words
__device__ inline uint64_t window8(const uint64_t* T64, uint64_t i) {
    const uint64_t a = T64[i >> 3], b = T64[(i >> 3) + 1];
    const uint32_t sh = (uint32_t)(i & 7) * 8;
    const uint64_t w = sh ? (a >> sh) | (b << (64 - sh)) : a;
    return __builtin_bswap64(w);
}

__global__ void k_first_keys(const uint64_t* T64, uint64_t n, uint64_t* key, uint32_t* val) {
    const uint64_t i = blockIdx.x * (uint64_t)BT + threadIdx.x;
    if (i >= n) return;
    key[i] = window8(T64, i);
    val[i] = (uint32_t)i;
}

// round keys: (group head of s << 32) | group head of s + h, for every active suffix s (s + h < n: the terminator is
// unique, so a suffix that shares its first h characters with another is longer than h)
__global__ void k_round_keys(const uint32_t* act, uint64_t m, const uint32_t* rank, uint64_t h, uint64_t n,
                             uint64_t* key) {
    const uint64_t j = blockIdx.x * (uint64_t)BT + threadIdx.x;
    if (j >= m) return;
    const uint64_t s = act[j];
    key[j] = ((uint64_t)rank[s] << 32) | (s + h < n ? rank[s + h] : 0u);
}

// first round: slot j of the sorted keys is SA position j
__global__ void k_first_place(const uint64_t* key, const uint32_t* val, uint64_t m, uint32_t* sa, uint32_t* newhead) {
    const uint64_t j = blockIdx.x * (uint64_t)BT + threadIdx.x;
    if (j >= m) return;
    sa[j] = val[j];
    newhead[j] = (j == 0 || key[j] != key[j - 1]) ? (uint32_t)j : 0u;
}

// later rounds: the active slots of one old group are consecutive and the old group's SA positions are
// [head, head + size): first[j] = the group's first slot (after a max-scan)
__global__ void k_old_group_first(const uint64_t* key, uint64_t m, uint32_t* first) {
    const uint64_t j = blockIdx.x * (uint64_t)BT + threadIdx.x;
    if (j >= m) return;
    first[j] = (j == 0 || (key[j] >> 32) != (key[j - 1] >> 32)) ? (uint32_t)j : 0u;
}

__global__ void k_place(const uint64_t* key, const uint32_t* val, const uint32_t* first, uint64_t m, uint64_t n,
                        uint32_t* sa, uint32_t* newhead) {
    const uint64_t j = blockIdx.x * (uint64_t)BT + threadIdx.x;
    if (j >= m) return;
    const uint64_t p = (key[j] >> 32) + (j - first[j]);
    if (p < n) sa[p] = val[j];  // (always: the group's slots are its SA positions)
    newhead[j] = (j == 0 || key[j] != key[j - 1]) ? (uint32_t)p : 0u;
}

// new ranks (after the max-scan of newhead) and the elements that stay active (not a singleton group)
__global__ void k_rank_flags(const uint64_t* key, const uint32_t* val, const uint32_t* newhead, uint64_t m,
                             uint32_t* rank, uint8_t* keep) {
    const uint64_t j = blockIdx.x * (uint64_t)BT + threadIdx.x;
    if (j >= m) return;
    rank[val[j]] = newhead[j];
    const bool b0 = j == 0 || key[j] != key[j - 1];
    const bool b1 = j + 1 == m || key[j + 1] != key[j];
    keep[j] = (b0 && b1) ? 0 : 1;
}

// ---- phase 2: LCP ------------------------------------------------------------------------------------------------

__global__ void k_phi(const uint32_t* sa, uint64_t n, uint32_t* phi) {
    const uint64_t i = blockIdx.x * (uint64_t)BT + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = sa[i];
    if (s < n) phi[s] = i ? sa[i - 1] : NONE;
}

// PLCP over [t * LCP_CHUNK, ..) in place over Phi: the first value from scratch, then PLCP[j + 1] >= PLCP[j] - 1.
// A comparison never passes the terminator (unique, and 0 where the other side is >= 2).
__global__ void k_plcp(const uint64_t* T64, uint64_t n, uint32_t* phi, unsigned long long* compares) {
    const uint64_t t = blockIdx.x * (uint64_t)BT + threadIdx.x;
    const uint64_t j0 = t * LCP_CHUNK;
    if (j0 >= n) return;
    const uint64_t j1 = j0 + LCP_CHUNK < n ? j0 + LCP_CHUNK : n;
    uint64_t l = 0, cmp = 0;
    for (uint64_t j = j0; j < j1; ++j) {
        const uint32_t k = phi[j];
        if (k == NONE) {
            phi[j] = 0;
            l = 0;
            continue;
        }
        while (j + l < n && k + l < n) {  // (always left through the break: the terminator differs)
            ++cmp;
            const uint64_t x = window8(T64, j + l) ^ window8(T64, k + l);
            if (x) {
                l += (uint64_t)__builtin_clzll(x) >> 3;  // big-endian windows: the first byte that differs
                break;
            }
            l += 8;
        }
        phi[j] = (uint32_t)l;
        l = l ? l - 1 : 0;
    }
    atomicAdd(compares, (unsigned long long)cmp);
}

__global__ void k_lcp_gather(const uint32_t* sa, const uint32_t* plcp, uint64_t n, uint32_t* lcp) {
    const uint64_t i = blockIdx.x * (uint64_t)BT + threadIdx.x;
    if (i >= n) return;
    lcp[i] = plcp[sa[i]];
}

// ---- phase 3: runs -----------------------------------------------------------------------------------------------

__global__ void k_bwt(const uint8_t* T, const uint32_t* sa, uint64_t n, uint8_t* bwt) {
    const uint64_t i = blockIdx.x * (uint64_t)BT + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = sa[i];
    bwt[i] = T[s ? s - 1 : n - 1];
}

__global__ void k_run_flags(const uint8_t* bwt, uint64_t n, uint8_t* flag) {
    const uint64_t i = blockIdx.x * (uint64_t)BT + threadIdx.x;
    if (i >= n) return;
    flag[i] = (i == 0 || bwt[i] != bwt[i - 1]) ? 1 : 0;
}

__global__ void k_heads(const uint8_t* bwt, const uint32_t* starts, uint64_t r, uint8_t* heads) {
    const uint64_t k = blockIdx.x * (uint64_t)BT + threadIdx.x;
    if (k >= r) return;
    heads[k] = bwt[starts[k]];
}

// ---- phase 5: samples and document ids -----------------------------------------------------------------------------

__device__ inline uint16_t doc_of(const uint64_t* ends, uint32_t nd, uint64_t v) {  // #ends <= v
    uint32_t lo = 0, hi = nd;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ends[mid] <= v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return (uint16_t)lo;
}

__global__ void k_samples(const uint32_t* sa, const uint32_t* starts, uint64_t r, uint64_t n, const uint64_t* ends,
                          uint32_t nd, uint32_t* ssa, uint32_t* esa, uint16_t* ds, uint16_t* de) {
    const uint64_t k = blockIdx.x * (uint64_t)BT + threadIdx.x;
    if (k >= r) return;
    const uint64_t last = (k + 1 < r ? (uint64_t)starts[k + 1] : n) - 1;
    const uint32_t a = sa[starts[k]], b = sa[last];
    const uint32_t sa_ = a ? a - 1 : (uint32_t)(n - 1), sb = b ? b - 1 : (uint32_t)(n - 1);
    ssa[k] = sa_;
    esa[k] = sb;
    ds[k] = doc_of(ends, nd, sa_);
    de[k] = doc_of(ends, nd, sb);
}

// ---- phase 4: thresholds -----------------------------------------------------------------------------------------

__global__ void k_iota(uint32_t* v, uint64_t m) {
    const uint64_t k = blockIdx.x * (uint64_t)BT + threadIdx.x;
    if (k < m) v[k] = (uint32_t)k;
}

__device__ inline uint64_t lkey(const uint32_t* lcp, uint64_t i) { return ((uint64_t)lcp[i] << 32) | i; }

__global__ void k_block_min(const uint32_t* lcp, uint64_t n, uint64_t nb, uint64_t* lev0) {
    const uint64_t b = blockIdx.x * (uint64_t)BT + threadIdx.x;
    if (b >= nb) return;
    const uint64_t lo = b << RMQ_SHIFT, hi = (lo + (1ull << RMQ_SHIFT)) < n ? lo + (1ull << RMQ_SHIFT) : n;
    uint64_t m = ~0ull;
    for (uint64_t i = lo; i < hi; ++i) {
        const uint64_t v = lkey(lcp, i);
        m = v < m ? v : m;
    }
    lev0[b] = m;
}

__global__ void k_sparse_level(const uint64_t* prev, uint64_t nb, uint64_t half, uint64_t* out) {
    const uint64_t b = blockIdx.x * (uint64_t)BT + threadIdx.x;
    if (b + 2 * half > nb) return;
    const uint64_t x = prev[b], y = prev[b + half];
    out[b] = x < y ? x : y;
}

__device__ inline uint64_t scan_min(const uint32_t* lcp, uint64_t lo, uint64_t hi, uint64_t m) {  // [lo, hi]
    for (uint64_t i = lo; i <= hi; ++i) {
        const uint64_t v = lkey(lcp, i);
        m = v < m ? v : m;
    }
    return m;
}

// thr of every run from its position q in the stable order by head byte
__global__ void k_thresholds(const uint8_t* hs, const uint32_t* order, const uint32_t* starts, uint64_t r,
                             const uint32_t* lcp, const uint64_t* table, uint64_t nb, uint32_t* thr) {
    const uint64_t q = blockIdx.x * (uint64_t)BT + threadIdx.x;
    if (q >= r) return;
    const uint32_t k = order[q];
    if (q == 0 || hs[q] != hs[q - 1]) {
        thr[k] = 0;
        return;
    }
    const uint64_t lo = starts[order[q - 1] + 1], hi = starts[k];  // (end of the previous run, start of run k]
    const uint64_t bl = lo >> RMQ_SHIFT, bh = hi >> RMQ_SHIFT;
    uint64_t m = ~0ull;
    if (bl == bh) {
        m = scan_min(lcp, lo, hi, m);
    } else {
        m = scan_min(lcp, lo, ((bl + 1) << RMQ_SHIFT) - 1, m);
        m = scan_min(lcp, bh << RMQ_SHIFT, hi, m);
        if (bl + 1 < bh) {
            const uint64_t a = bl + 1, len = bh - a;
            const uint32_t lg = 63 - __builtin_clzll(len);
            const uint64_t x = table[lg * nb + a], y = table[lg * nb + bh - (1ull << lg)];
            m = x < m ? x : m;
            m = y < m ? y : m;
        }
    }
    thr[k] = (uint32_t)(m & 0xffffffffu);
}

// ---- driver ------------------------------------------------------------------------------------------------------

#define SPB_HIP(call) SPX_HIP(call)
#define SPB_LAUNCH() SPX_HIP(hipGetLastError())

struct Timer {
    bool on;
    hipStream_t st;
    std::chrono::steady_clock::time_point t0;
    int phase(const char* name, const std::string& extra, uint64_t cur_bytes) {
        if (!on) return SPX_OK;
        SPB_HIP(hipStreamSynchronize(st));
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[spb] %-10s %9.1f ms  device %.3f GB%s%s\n", name,
                std::chrono::duration<double, std::milli>(t1 - t0).count(), cur_bytes / 1e9, extra.empty() ? "" : "  ",
                extra.c_str());
        t0 = t1;
        return SPX_OK;
    }
};

int bits_of(uint64_t v) {
    int b = 0;
    while (v) {
        ++b;
        v >>= 1;
    }
    return b;
}

// temporary bytes of the library calls of phase 1 for m elements (the largest call; sizes only, nothing runs)
int phase1_temp(uint64_t m, size_t& out) {
    size_t a = 0, b = 0, c = 0;
    hipcub::DoubleBuffer<uint64_t> kb(nullptr, nullptr);
    hipcub::DoubleBuffer<uint32_t> vb(nullptr, nullptr);
    SPB_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, a, kb, vb, m, 0, 64));
    SPB_HIP(hipcub::DeviceScan::InclusiveScan(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, hipcub::Max(), m));
    SPB_HIP(hipcub::DeviceSelect::Flagged(nullptr, c, (uint32_t*)nullptr, (uint8_t*)nullptr, (uint32_t*)nullptr,
                                          (uint64_t*)nullptr, (int64_t)m));
    out = std::max(a, std::max(b, c));
    return SPX_OK;
}

int build(spb_build& B, const uint8_t* text, uint64_t n_text, const std::vector<uint64_t>& doc_ends, bool samples) {
    const uint64_t n = n_text + 1;
    Mem mem;
    Stream S;
    SPB_HIP(hipStreamCreateWithFlags(&S.s, hipStreamNonBlocking));
    hipStream_t st = S.s;
    Timer tm{getenv("SPX_TIMING") != nullptr, st, std::chrono::steady_clock::now()};

    // ---- memory: phase 1 holds the most (text, SA, ranks, two key and two value buffers of n); refuse up front
    size_t temp1 = 0;
    if (int rc = phase1_temp(n, temp1)) return rc;
    const uint64_t tbytes = ((n + 7) & ~7ull) + TEXT_PAD;
    const uint64_t need = tbytes + 4 * n + 4 * n + 16 * n + 8 * n + temp1 + 64 + (64ull << 20);
    size_t fr = 0, tot = 0;
    SPB_HIP(hipMemGetInfo(&fr, &tot));
    if (need > fr) {
        set_error("the build of %llu characters does not fit on the device: it needs %llu bytes of device memory, "
                  "%llu bytes are free (of %llu)",
                  (unsigned long long)n_text, (unsigned long long)need, (unsigned long long)fr,
                  (unsigned long long)tot);
        return SPX_E_ARG;
    }

    Buf T, SA, RK, K0, K1, V0, V1, tmp, cnt;
    SPB_HIP(T.alloc(mem, tbytes));
    SPB_HIP(hipMemsetAsync(T.p, 0, tbytes, st));
    SPB_HIP(hipMemcpyAsync(T.p, text, n_text, hipMemcpyHostToDevice, st));  // T[n - 1] = 0: the terminator
    SPB_HIP(SA.alloc(mem, 4 * n));
    SPB_HIP(RK.alloc(mem, 4 * n));
    SPB_HIP(K0.alloc(mem, 8 * n));
    SPB_HIP(K1.alloc(mem, 8 * n));
    SPB_HIP(V0.alloc(mem, 4 * n));
    SPB_HIP(V1.alloc(mem, 4 * n));
    SPB_HIP(tmp.alloc(mem, temp1 + 16));
    SPB_HIP(cnt.alloc(mem, 64));
    if (int rc = tm.phase("upload", "", mem.cur)) return rc;

    // ---- phase 1: suffix array
    const uint64_t* T64 = T.as<uint64_t>();
    uint32_t* sa = SA.as<uint32_t>();
    uint32_t* rank = RK.as<uint32_t>();
    uint64_t* d_count = cnt.as<uint64_t>();
    std::string rounds_log;
    uint64_t m = n, h = 8;
    int rounds = 0;
    uint32_t* act = nullptr;  // active suffixes in SA order (after the first round)
    while (m > 0) {
        uint64_t* kin = K0.as<uint64_t>();
        uint32_t* vin;
        if (rounds == 0) {
            vin = V0.as<uint32_t>();
            k_first_keys<<<nblk(n), BT, 0, st>>>(T64, n, kin, vin);
        } else {
            vin = act;
            k_round_keys<<<nblk(m), BT, 0, st>>>(act, m, rank, h, n, kin);
        }
        SPB_LAUNCH();
        uint32_t* valt = vin == V0.as<uint32_t>() ? V1.as<uint32_t>() : V0.as<uint32_t>();
        hipcub::DoubleBuffer<uint64_t> kb(kin, K1.as<uint64_t>());
        hipcub::DoubleBuffer<uint32_t> vb(vin, valt);
        const int end_bit = rounds == 0 ? 64 : 32 + bits_of(n);
        size_t tb = temp1;
        SPB_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, kb, vb, m, 0, end_bit, st));
        const uint64_t* key = kb.Current();
        const uint32_t* val = vb.Current();
        uint32_t* X = (uint32_t*)kb.Alternate();  // 8m free bytes: two u32 arrays of m
        uint32_t* Y = X + m;
        if (rounds == 0) {
            k_first_place<<<nblk(m), BT, 0, st>>>(key, val, m, sa, Y);
            SPB_LAUNCH();
        } else {
            k_old_group_first<<<nblk(m), BT, 0, st>>>(key, m, X);
            SPB_LAUNCH();
            tb = temp1;
            SPB_HIP(hipcub::DeviceScan::InclusiveScan(tmp.p, tb, X, X, hipcub::Max(), m, st));
            k_place<<<nblk(m), BT, 0, st>>>(key, val, X, m, n, sa, Y);
            SPB_LAUNCH();
        }
        tb = temp1;
        SPB_HIP(hipcub::DeviceScan::InclusiveScan(tmp.p, tb, Y, Y, hipcub::Max(), m, st));
        uint8_t* keep = (uint8_t*)X;
        k_rank_flags<<<nblk(m), BT, 0, st>>>(key, val, Y, m, rank, keep);
        SPB_LAUNCH();
        uint32_t* vout = vb.Alternate();
        tb = temp1;
        SPB_HIP(hipcub::DeviceSelect::Flagged(tmp.p, tb, val, keep, vout, d_count, (int64_t)m, st));
        uint64_t next = 0;
        SPB_HIP(hipMemcpyAsync(&next, d_count, 8, hipMemcpyDeviceToHost, st));
        SPB_HIP(hipStreamSynchronize(st));
        if (tm.on) rounds_log += (rounds ? " " : "") + std::to_string(m);
        act = vout;
        m = next;
        if (rounds > 0) h *= 2;
        ++rounds;
        if (rounds > 40) {  // h >= 2^40 > n: impossible unless the text has a second terminator
            set_error("suffix sorting did not converge (text must not contain bytes 0 or 1)");
            return SPX_E_ARG;
        }
    }
    tmp.release();
    K0.release();
    K1.release();
    V0.release();
    V1.release();
    if (int rc = tm.phase("sa", "rounds " + std::to_string(rounds) + ", sorted per round: " + rounds_log, mem.cur))
        return rc;

    // ---- phase 2: LCP (into the rank buffer)
    Buf PHI;
    SPB_HIP(PHI.alloc(mem, 4 * n));
    uint32_t* phi = PHI.as<uint32_t>();
    unsigned long long* d_cmp = (unsigned long long*)cnt.p;
    SPB_HIP(hipMemsetAsync(d_cmp, 0, 8, st));
    k_phi<<<nblk(n), BT, 0, st>>>(sa, n, phi);
    SPB_LAUNCH();
    const uint64_t nchunks = (n + LCP_CHUNK - 1) / LCP_CHUNK;
    k_plcp<<<nblk(nchunks), BT, 0, st>>>(T64, n, phi, d_cmp);
    SPB_LAUNCH();
    uint32_t* lcp = rank;
    k_lcp_gather<<<nblk(n), BT, 0, st>>>(sa, phi, n, lcp);
    SPB_LAUNCH();
    unsigned long long compares = 0;
    SPB_HIP(hipMemcpyAsync(&compares, d_cmp, 8, hipMemcpyDeviceToHost, st));
    SPB_HIP(hipStreamSynchronize(st));
    PHI.release();
    if (int rc = tm.phase("lcp", std::to_string(compares) + " compares of 8 bytes (" +
                                     std::to_string(nchunks) + " chunks of " + std::to_string(LCP_CHUNK) + ")",
                          mem.cur))
        return rc;

    // ---- phase 3: runs
    Buf BW, FL, ST, HD;
    SPB_HIP(BW.alloc(mem, n));
    SPB_HIP(FL.alloc(mem, n));
    SPB_HIP(ST.alloc(mem, 4 * n));
    k_bwt<<<nblk(n), BT, 0, st>>>(T.as<uint8_t>(), sa, n, BW.as<uint8_t>());
    SPB_LAUNCH();
    k_run_flags<<<nblk(n), BT, 0, st>>>(BW.as<uint8_t>(), n, FL.as<uint8_t>());
    SPB_LAUNCH();
    {
        hipcub::CountingInputIterator<uint32_t> iota(0);
        size_t tb = 0;
        SPB_HIP(hipcub::DeviceSelect::Flagged(nullptr, tb, iota, FL.as<uint8_t>(), ST.as<uint32_t>(), d_count,
                                              (int64_t)n, st));
        SPB_HIP(tmp.alloc(mem, tb + 16));
        SPB_HIP(hipcub::DeviceSelect::Flagged(tmp.p, tb, iota, FL.as<uint8_t>(), ST.as<uint32_t>(), d_count,
                                              (int64_t)n, st));
    }
    uint64_t r = 0;
    SPB_HIP(hipMemcpyAsync(&r, d_count, 8, hipMemcpyDeviceToHost, st));
    SPB_HIP(hipStreamSynchronize(st));
    tmp.release();
    FL.release();
    T.release();
    const uint32_t* starts = ST.as<uint32_t>();
    SPB_HIP(HD.alloc(mem, r));
    k_heads<<<nblk(r), BT, 0, st>>>(BW.as<uint8_t>(), starts, r, HD.as<uint8_t>());
    SPB_LAUNCH();
    BW.release();
    B.n = n;
    B.r = r;
    B.heads.resize(r);
    B.starts.resize(r);
    SPB_HIP(hipMemcpyAsync(B.heads.data(), HD.p, r, hipMemcpyDeviceToHost, st));
    SPB_HIP(hipMemcpyAsync(B.starts.data(), starts, 4 * r, hipMemcpyDeviceToHost, st));
    SPB_HIP(hipStreamSynchronize(st));
    if (int rc = tm.phase("runs", "r " + std::to_string(r), mem.cur)) return rc;

    // ---- phase 5: samples and document ids (the SA goes after this)
    if (samples) {
        Buf SS, ES, DS, DE, EN;
        SPB_HIP(SS.alloc(mem, 4 * r));
        SPB_HIP(ES.alloc(mem, 4 * r));
        SPB_HIP(DS.alloc(mem, 2 * r));
        SPB_HIP(DE.alloc(mem, 2 * r));
        SPB_HIP(EN.alloc(mem, 8 * doc_ends.size()));
        SPB_HIP(hipMemcpyAsync(EN.p, doc_ends.data(), 8 * doc_ends.size(), hipMemcpyHostToDevice, st));
        k_samples<<<nblk(r), BT, 0, st>>>(sa, starts, r, n, EN.as<uint64_t>(), (uint32_t)doc_ends.size(),
                                           SS.as<uint32_t>(), ES.as<uint32_t>(), DS.as<uint16_t>(), DE.as<uint16_t>());
        SPB_LAUNCH();
        B.ssa.resize(r);
        B.esa.resize(r);
        B.ds.resize(r);
        B.de.resize(r);
        SPB_HIP(hipMemcpyAsync(B.ssa.data(), SS.p, 4 * r, hipMemcpyDeviceToHost, st));
        SPB_HIP(hipMemcpyAsync(B.esa.data(), ES.p, 4 * r, hipMemcpyDeviceToHost, st));
        SPB_HIP(hipMemcpyAsync(B.ds.data(), DS.p, 2 * r, hipMemcpyDeviceToHost, st));
        SPB_HIP(hipMemcpyAsync(B.de.data(), DE.p, 2 * r, hipMemcpyDeviceToHost, st));
        SPB_HIP(hipStreamSynchronize(st));
        B.samples = true;
    }
    SA.release();
    if (samples)
        if (int rc = tm.phase("samples", "", mem.cur)) return rc;

    // ---- phase 4: thresholds
    const uint64_t nb = (n + (1ull << RMQ_SHIFT) - 1) >> RMQ_SHIFT;
    const int levels = bits_of(nb);  // level L holds minima of 2^L blocks
    Buf TB, IO, HS, OR, TH;
    SPB_HIP(TB.alloc(mem, 8 * nb * levels));
    uint64_t* table = TB.as<uint64_t>();
    k_block_min<<<nblk(nb), BT, 0, st>>>(lcp, n, nb, table);
    SPB_LAUNCH();
    for (int L = 1; L < levels; ++L) {
        const uint64_t half = 1ull << (L - 1);
        k_sparse_level<<<nblk(nb), BT, 0, st>>>(table + (L - 1) * nb, nb, half, table + L * nb);
        SPB_LAUNCH();
    }
    SPB_HIP(IO.alloc(mem, 4 * r));
    SPB_HIP(HS.alloc(mem, r));
    SPB_HIP(OR.alloc(mem, 4 * r));
    {
        size_t tb = 0;
        SPB_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, HD.as<uint8_t>(), HS.as<uint8_t>(), IO.as<uint32_t>(),
                                                   OR.as<uint32_t>(), r, 0, 8, st));
        SPB_HIP(tmp.alloc(mem, tb + 16));
        k_iota<<<nblk(r), BT, 0, st>>>(IO.as<uint32_t>(), r);
        SPB_LAUNCH();
        // LSD radix sort is stable: the runs of one letter stay in ascending order
        SPB_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, HD.as<uint8_t>(), HS.as<uint8_t>(), IO.as<uint32_t>(),
                                                   OR.as<uint32_t>(), r, 0, 8, st));
    }
    tmp.release();
    IO.release();
    HD.release();
    SPB_HIP(TH.alloc(mem, 4 * r));
    k_thresholds<<<nblk(r), BT, 0, st>>>(HS.as<uint8_t>(), OR.as<uint32_t>(), starts, r, lcp, table, nb,
                                         TH.as<uint32_t>());
    SPB_LAUNCH();
    B.thr.resize(r);
    SPB_HIP(hipMemcpyAsync(B.thr.data(), TH.p, 4 * r, hipMemcpyDeviceToHost, st));
    SPB_HIP(hipStreamSynchronize(st));
    if (int rc = tm.phase("thresholds", std::to_string(levels) + " sparse-table levels over " + std::to_string(nb) +
                                            " blocks",
                          mem.cur))
        return rc;
    if (tm.on)
        fprintf(stderr, "[spb] n %llu r %llu peak device %llu bytes (%.2f B/char)\n", (unsigned long long)n,
                (unsigned long long)r, (unsigned long long)mem.peak, (double)mem.peak / (double)n);
    return SPX_OK;
}

}  // namespace
}  // namespace spx

using namespace spx;

extern "C" {

spb_build* spb_build_from_text(const uint8_t* text, uint64_t n_text, const uint64_t* doc_lengths, uint32_t n_docs,
                               int with_samples, int device) {
    if (select_device(device) != SPX_OK) return nullptr;
    if (!text || n_text == 0) {
        set_error("text is null or empty");
        return nullptr;
    }
    if (n_text >= 0xffffffffull) {
        set_error("text of %llu characters: the builder takes fewer than 2^32 - 1 (positions are 32-bit)",
                  (unsigned long long)n_text);
        return nullptr;
    }
    if (memchr(text, 0, n_text) || memchr(text, 1, n_text)) {
        set_error("text bytes must be >= 2 (0 and 1 are the terminator)");
        return nullptr;
    }
    std::vector<uint64_t> ends;  // cumulative document ends, the last one + 1 (it absorbs the terminator)
    if (doc_lengths) {
        if (n_docs == 0 || n_docs > 65535) {
            set_error("%u documents: the builder takes 1 to 65535", n_docs);
            return nullptr;
        }
        uint64_t sum = 0;
        for (uint32_t d = 0; d < n_docs; ++d) {
            sum += doc_lengths[d];
            ends.push_back(sum);
        }
        if (sum != n_text) {
            set_error("document lengths sum to %llu, the text has %llu characters", (unsigned long long)sum,
                      (unsigned long long)n_text);
            return nullptr;
        }
    } else {
        ends.push_back(n_text);
    }
    ends.back() += 1;
    spb_build* b = new (std::nothrow) spb_build;
    if (!b) {
        set_error("out of host memory");
        return nullptr;
    }
    int rc;
    try {
        rc = build(*b, text, n_text, ends, with_samples != 0);
    } catch (const std::bad_alloc&) {
        set_error("out of host memory");
        rc = SPX_E_ARG;
    }
    if (rc != SPX_OK) {
        delete b;
        return nullptr;
    }
    return b;
}

int spb_build_stats(const spb_build* b, uint64_t* n, uint64_t* r) {
    if (!b) {
        set_error("build is null");
        return SPX_E_ARG;
    }
    if (n) *n = b->n;
    if (r) *r = b->r;
    return SPX_OK;
}

int spb_build_copy(const spb_build* b, uint8_t* heads, uint64_t* lens, uint64_t* thr, uint64_t* ssa, uint64_t* esa,
                   uint64_t* doc_start, uint64_t* doc_end) {
    if (!b) {
        set_error("build is null");
        return SPX_E_ARG;
    }
    if (!b->samples && (ssa || esa || doc_start || doc_end)) {
        set_error("the build has no SA samples (with_samples was 0)");
        return SPX_E_ARG;
    }
    const uint64_t r = b->r;
    if (heads) memcpy(heads, b->heads.data(), r);
    for (uint64_t k = 0; k < r; ++k) {
        if (lens) lens[k] = (k + 1 < r ? (uint64_t)b->starts[k + 1] : b->n) - b->starts[k];
        if (thr) thr[k] = b->thr[k];
        if (ssa) ssa[k] = b->ssa[k];
        if (esa) esa[k] = b->esa[k];
        if (doc_start) doc_start[k] = b->ds[k];
        if (doc_end) doc_end[k] = b->de[k];
    }
    return SPX_OK;
}

void spb_build_free(spb_build* b) { delete b; }

}  // extern "C"
