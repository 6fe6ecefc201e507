// spx_align_kernels.h -- what spx_align.hip (the alignments) and spx_cigar.hip (the same alignments with their path)
// share: the arguments, the counters, the count over the chain records, the walk back over pred with every input checked,
// and the reduction of a read's gaps into its record.  Each translation unit gets its own copy of the kernels (the
// library is built without relocatable device code); the fills between the walk and the reduction are each file's own.
#pragma once
#include "../../include/spumoni_align.h"
#include "spx_internal.h"

namespace spx {
namespace {

constexpr uint32_t LANE_MAX = 16;     // both sides up to this: one lane's table
constexpr uint32_t FILL_LIMIT = 4096;  // the largest max_fill: sizes the LDS of the wavefront fills
constexpr uint32_t EDIT = 1u << 16;

struct AlignCounters {  // device; zeroed in front of every launch
    unsigned long long reads, aligned, gaps, filled, cells;
    unsigned long long nbig;   // the lane fill -> the wavefront fill: entries of the list
    unsigned long long error;  // bit 0: a read failed the walk's checks; bit 1: a read's gaps did not fit the capacity
};
constexpr int ALIGN_WORDS = sizeof(AlignCounters) / 8;
struct AlignArgs {
    const uint8_t* R;
    const uint64_t* roffs;
    const uint4* M;
    const uint64_t* moffs;
    uint64_t nreads;
    const uint4* chains;  // three per read
    const uint32_t* pred;
    const uint8_t* T;
    uint64_t n_text;
    uint32_t max_fill;
    uint64_t cap;
    uint4* out;  // three per read
    uint64_t* cnt;    // nreads + 1: gaps per read, then a 0
    uint64_t* goffs;  // nreads + 1
    uint4* gaps;      // cap: a, b, edits, matches
    ulonglong2* desc;  // cap: where A starts in R, where B starts in T
    uint32_t* list;    // cap
    AlignCounters* c;
};

// A read's chain record and what the offsets say, checked: the same in the count and in the walk.
struct ChainOf {
    uint4 w0, w1, w2;
    uint64_t o, ro, read_len;
    uint32_t h, n, first, last;
    bool chained, sane;
};
__device__ inline ChainOf chain_of(const AlignArgs& a, uint64_t q) {
    ChainOf c;
    c.w0 = a.chains[3 * q];
    c.w1 = a.chains[3 * q + 1];
    c.w2 = a.chains[3 * q + 2];
    c.o = a.moffs[q];
    const uint64_t e = a.moffs[q + 1];
    c.ro = a.roffs[q];
    const uint64_t re = a.roffs[q + 1];
    c.n = c.w1.w;
    c.first = c.w2.x;
    c.last = c.w2.y;
    c.chained = !(c.w0.x == 0xffffffffu && c.w0.y == 0xffffffffu);
    const bool ranges = e >= c.o && e - c.o < (1ull << 32) && re >= c.ro && re - c.ro < (1ull << 32);
    c.h = ranges ? (uint32_t)(e - c.o) : 0u;
    c.read_len = ranges ? re - c.ro : 0;
    c.sane = ranges && c.n >= 1 && c.n <= c.h && c.last < c.h && c.first <= c.last && c.n - 1 <= c.last - c.first;
    return c;
}

__global__ __launch_bounds__(256) void k_align_count(AlignArgs a) {
    const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (q > a.nreads) return;
    uint64_t n = 0;
    if (q < a.nreads) {
        const ChainOf c = chain_of(a, q);
        if (c.chained && c.sane) n = c.n - 1;
    }
    a.cnt[q] = n;
}

__device__ inline void write_unaligned(const AlignArgs& a, uint64_t q) {
    a.out[3 * q] = make_uint4(0xffffffffu, 0xffffffffu, 0, 0);
    a.out[3 * q + 1] = make_uint4(0, 0, 0, 0);
    a.out[3 * q + 2] = make_uint4(0, 0, 0, SPC_NO_DOC);
}

__global__ __launch_bounds__(256) void k_align_walk(AlignArgs a) {
    const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= a.nreads) return;
    const ChainOf c = chain_of(a, q);
    if (!c.chained) {
        write_unaligned(a, q);
        return;
    }
    if (!c.sane) {
        atomicOr(&a.c->error, 1ull);
        write_unaligned(a, q);
        return;
    }
    const uint64_t g0 = a.goffs[q], g1 = a.goffs[q + 1];  // (g1 - g0 == n - 1: the count saw the same record)
    const bool fits = g1 <= a.cap || g0 == g1;  // (a chain of one anchor has no gaps: it always fits)
    bool ok = fits;
    if (!fits) atomicOr(&a.c->error, 2ull);
    uint32_t i = c.last;
    uint4 mi = a.M[c.o + i];
    uint64_t base = 0;
    for (uint32_t step = 0; ok && step + 1 < c.n; ++step) {
        const uint32_t j = a.pred[c.o + i];
        if (j == SPC_NO_PRED || j >= i || j < c.first) {
            ok = false;
            break;
        }
        const uint4 mj = a.M[c.o + j];
        const uint64_t yi = (uint64_t)mi.x | ((uint64_t)mi.y << 32), yj = (uint64_t)mj.x | ((uint64_t)mj.y << 32);
        const uint64_t xe_i = (uint64_t)mi.z + mi.w, xe_j = (uint64_t)mj.z + mj.w;  // the ends in the read: exact in 64 bits
        // the ends in the text: y + l wraps only when y is within 2^32 of 2^64, and then the order test below fails
        const uint64_t ye_i = yi + mi.w, ye_j = yj + mj.w;
        if (ye_i < yi || ye_j < yj || xe_i <= xe_j || ye_i <= ye_j || xe_i > c.read_len) {
            ok = false;
            break;
        }
        const uint64_t ex = xe_i - xe_j, ey = ye_i - ye_j;  // >= 1
        uint64_t keep = mi.w;
        keep = ex < keep ? ex : keep;
        keep = ey < keep ? ey : keep;
        const uint64_t ga = ex - keep, gb = ey - keep;
        // keep >= 1 needs l_i >= 1; a gap in the text that is read lies inside the text
        if (keep == 0 || ga > 0xffffffffull || gb > 0xffffffffull || (gb != 0 && (ye_j > a.n_text || gb > a.n_text - ye_j))) {
            ok = false;
            break;
        }
        const uint64_t g = g0 + (c.n - 2 - step);  // in [g0, g1), below cap
        a.gaps[g] = make_uint4((uint32_t)ga, (uint32_t)gb, 0, 0);
        a.desc[g] = make_ulonglong2(c.ro + xe_j, ye_j);
        base += keep;
        i = j;
        mi = mj;
    }
    ok = ok && i == c.first && (uint64_t)mi.z + mi.w <= c.read_len && mi.w >= 1;
    if (!ok) {
        if (fits) atomicOr(&a.c->error, 1ull);
        write_unaligned(a, q);
        // the read's places in the table hold empty gaps: the fill and the reduce read nothing that was not written
        const uint64_t end = g1 < a.cap ? g1 : a.cap;
        for (uint64_t g = g0; g < end; ++g) {
            a.gaps[g] = make_uint4(0, 0, 0, 0);
            a.desc[g] = make_ulonglong2(0, 0);
        }
        return;
    }
    base += mi.w;  // at most the end of the last anchor in the read (the kept parts do not overlap): below 2^32
    // the record's first version: matches = l_first + the sum of keep, and -- until the reduction writes the edits there --
    // l_first itself, which is what spx_cigar.hip's emit needs beside the gaps to lay the anchors out
    a.out[3 * q] = c.w0;
    a.out[3 * q + 1] = make_uint4(c.w1.x, c.w1.y, (uint32_t)base, mi.w);
    a.out[3 * q + 2] = make_uint4(c.n, 0, 0, c.w2.w);
}

// A lane per read, a block over a stride of reads: what is counted leaves a block as one set of atomics (one per wavefront
// was 62 000 atomics on four words for 10^6 reads, and they alone took 0.7 ms).
__global__ __launch_bounds__(256) void k_align_reduce(AlignArgs a) {
    __shared__ unsigned long long part[4][4];
    unsigned long long n_aligned = 0, n_gaps = 0, n_filled = 0, n_cells = 0;
    for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < a.nreads; q += (uint64_t)gridDim.x * 256) {
        const uint4 w0 = a.out[3 * q];
        if (w0.x == 0xffffffffu && w0.y == 0xffffffffu) continue;
        uint4 w1 = a.out[3 * q + 1], w2 = a.out[3 * q + 2];
        const uint64_t g0 = a.goffs[q], g1 = a.goffs[q + 1];  // (an aligned read's gaps are all below cap)
        uint64_t matches = w1.z, edits = 0, unfilled = 0, skipped = 0;
        for (uint64_t g = g0; g < g1; ++g) {
            const uint4 gp = a.gaps[g];
            if (gp.z == SPA_UNFILLED) {
                unfilled++;
                skipped += gp.x > gp.y ? gp.x : gp.y;
            } else {
                edits += gp.z;
                matches += gp.w;
                n_filled++;
                if (gp.x >= 1 && gp.y >= 1 && !(gp.x == 1 && gp.y == 1)) n_cells += (unsigned long long)gp.x * gp.y;
            }
        }
        // (under the input contract both sums stay below 2^32; outside it they saturate)
        w1.z = (uint32_t)(matches > 0xffffffffull ? 0xffffffffull : matches);
        w1.w = (uint32_t)(edits > 0xffffffffull ? 0xffffffffull : edits);
        w2.y = (uint32_t)unfilled;
        w2.z = (uint32_t)(skipped > 0xffffffffull ? 0xffffffffull : skipped);
        a.out[3 * q + 1] = w1;
        a.out[3 * q + 2] = w2;
        n_aligned++;
        n_gaps += g1 - g0;
    }
    n_aligned = wave_sum(n_aligned);
    n_gaps = wave_sum(n_gaps);
    n_filled = wave_sum(n_filled);
    n_cells = wave_sum(n_cells);
    const uint32_t wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wv][0] = n_aligned;
        part[wv][1] = n_gaps;
        part[wv][2] = n_filled;
        part[wv][3] = n_cells;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const unsigned long long v = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        unsigned long long* c = threadIdx.x == 0 ? &a.c->aligned : threadIdx.x == 1 ? &a.c->gaps : threadIdx.x == 2 ? &a.c->filled : &a.c->cells;
        if (v) atomicAdd(c, v);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.c->reads = a.nreads;
}

int check_align_params(const spx_index* ix, const spa_params* p) {
    if (!ix) {
        set_error("index must be non-null");
        return SPX_E_ARG;
    }
    if (!p) {
        set_error("align params must be non-null");
        return SPX_E_ARG;
    }
    if (p->max_fill < 1 || p->max_fill > FILL_LIMIT) {
        set_error("max_fill must be 1 .. 4096");
        return SPX_E_ARG;
    }
    return SPX_OK;
}

// The six scratch slots the alignments and both CIGARs have alike, reserved before any kernel is enqueued (a buffer that
// grows is freed first: a device-wide wait): the gap counts, their offsets and the per-gap table unless they are the
// caller's arrays, where each gap's strings start, the list of the gaps that take a wavefront, and the scans' space -- for
// the scan of the counts and `other_scans` bytes at least.  The caller holds ix->mu and has set the device.
static_assert(spx_index::TB_CNT == spx_index::L_CNT && spx_index::TB_GOFFS == spx_index::L_GOFFS && spx_index::TB_GAPS == spx_index::L_GAPS &&
                  spx_index::TB_DESC == spx_index::L_DESC && spx_index::TB_LIST == spx_index::L_LIST && spx_index::TB_CUB == spx_index::L_CUB,
              "reserve_gaps fills the slots of either product");
int reserve_gaps(spx_index::Scratch* scr, AlignArgs& a, bool own_goffs, bool own_gaps, size_t other_scans, size_t* cub_bytes, void** cub) {
    void* p = nullptr;
    int rc;
    if ((rc = scr[spx_index::L_CNT].reserve((a.nreads + 1) * 8, &p)) != SPX_OK) return rc;
    a.cnt = (uint64_t*)p;
    if (own_goffs) {
        if ((rc = scr[spx_index::L_GOFFS].reserve((a.nreads + 1) * 8, &p)) != SPX_OK) return rc;
        a.goffs = (uint64_t*)p;
    }
    if (own_gaps) {
        if ((rc = scr[spx_index::L_GAPS].reserve(a.cap * 16 + 16, &p)) != SPX_OK) return rc;
        a.gaps = (uint4*)p;
    }
    if ((rc = scr[spx_index::L_DESC].reserve(a.cap * 16 + 16, &p)) != SPX_OK) return rc;
    a.desc = (ulonglong2*)p;
    if ((rc = scr[spx_index::L_LIST].reserve(a.cap * 4 + 16, &p)) != SPX_OK) return rc;
    a.list = (uint32_t*)p;
    *cub_bytes = 0;
    SPX_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, *cub_bytes, a.cnt, a.goffs, a.nreads + 1, (hipStream_t) nullptr));
    *cub_bytes = std::max(*cub_bytes, other_scans);
    return scr[spx_index::L_CUB].reserve(*cub_bytes + 16, cub);
}

}  // namespace
}  // namespace spx
