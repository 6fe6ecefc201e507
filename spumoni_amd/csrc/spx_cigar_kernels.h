// spx_cigar_kernels.h -- what spx_cigar.hip (the CIGARs) and spx_extend.hip (the same CIGARs taken to the read's ends)
// share: the plan, the tracing fills with their walk back, the emit and the host code that reserves, enqueues and
// collects them.  The ends come in at three places, each templated or switched on `ends`: the emit lays a read's two end
// paths and its clips around the gaps' steps (emit_read<WRITE, ENDS>), the launches call the extension's own kernels
// through EndHooks (their sizes in the plan, their fill in front of the emit, the records' update behind the reduction),
// and a TraceView names the scratch, the Product (counters, events, step times) and the waiting entries of the product
// that is calling.
// With ENDS false every kernel is the code spx_cigar.hip had.  Each translation unit gets its own copy of the kernels
// (the library is built without relocatable device code).
#pragma once
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/spumoni_cigar.h"
#include "spx_align_kernels.h"

namespace spx {
namespace {

// (tools/cigar_bench.py and tools/extend_bench.py print the scratch these three and ENDS_GRID give: keep them in step)
constexpr uint32_t TRACE_LDS_WORDS = 2048;       // a wavefront's trace in LDS: 8 KiB
constexpr uint64_t TRACE_BUDGET = 64ull << 20;   // bytes of trace buffers in device memory, all wavefronts together
constexpr uint64_t PATH_LIMIT = 1ull << 28;      // words of path scratch the device form reserves at most
constexpr uint64_t ENDS_GRID = 16384;            // wavefronts of the ends' launch at most (8 a SIMD are 8192 in flight)
constexpr uint64_t OVER = ~0ull;

struct CigarCounters {  // device; zeroed in front of every launch
    AlignCounters a;    // (nbig: the gaps whose trace fits LDS)
    unsigned long long nbig2;  // the gaps whose trace goes to device memory
    unsigned long long entries, path_words, ops_bound, fill_ticks, back_ticks;
    unsigned long long ends, extended, band_cells, clipped;  // the extension's: spx_extend.hip
};
constexpr int CIGAR_WORDS = sizeof(CigarCounters) / 8;
static_assert(CIGAR_WORDS <= spx_index::Product::WORDS, "Product::acc holds a word of every counter");
// the words of Product::acc by name (a.reads .. a.cells are words 0 .. 4, as in the alignments), and the error word
#define SPX_CIGAR_WORD(m) ((int)(offsetof(CigarCounters, m) / 8))
enum {
    CW_ERROR = SPX_CIGAR_WORD(a.error), CW_ENTRIES = SPX_CIGAR_WORD(entries), CW_PATH_WORDS = SPX_CIGAR_WORD(path_words),
    CW_OPS_BOUND = SPX_CIGAR_WORD(ops_bound), CW_FILL_TICKS = SPX_CIGAR_WORD(fill_ticks), CW_BACK_TICKS = SPX_CIGAR_WORD(back_ticks),
    CW_ENDS = SPX_CIGAR_WORD(ends), CW_EXTENDED = SPX_CIGAR_WORD(extended), CW_BAND_CELLS = SPX_CIGAR_WORD(band_cells),
    CW_CLIPPED = SPX_CIGAR_WORD(clipped)
};
#undef SPX_CIGAR_WORD
struct CigarArgs {
    AlignArgs a;
    uint64_t* pw;     // cap + 1: words of path per gap, then a 0
    uint64_t* poffs;  // cap + 1
    uint32_t* path;
    uint64_t path_cap;
    uint32_t* trace;  // gridDim of the second wave launch * trace_stride words
    uint64_t trace_stride;
    uint64_t* ocnt;   // nreads + 1: entries per read, then a 0
    uint64_t* ooffs;  // nreads + 1
    uint32_t* ops;
    uint64_t op_cap;
    CigarCounters* c;
    // the ends (spx_extend.hip; unused by the CIGARs): end 2 q is read q's left one, 2 q + 1 its right one
    uint32_t max_extend, band, mismatch, indel;
    uint64_t* epw;     // 2 nreads + 1: words of path per end, then a 0
    uint64_t* epoffs;  // 2 nreads + 1: an end's path stands at path[poffs[cap] + epoffs[e]]
    uint4* eres;       // two per end: (i, j, score, edits), (steps, cells, a, 0)
    uint32_t* etrace;  // gridDim of the ends' launch * etrace_stride words
    uint64_t etrace_stride;
    uint4* out_ends;   // 2 nreads, or null
};
constexpr uint32_t OP_S = 4;  // SPE_OP_S (spx_extend.hip holds the two together with a static_assert)

__device__ inline uint32_t path_words_of(uint32_t ga, uint32_t gb) { return (ga + gb + 15) / 16; }

// A lane per gap (and per read, for the anchors' share of the bound), a block over a stride of both: the two sums leave a
// block as one pair of atomics (one pair per wavefront was 0.3 ms on 10^6 reads: 40 000 atomics on two words).
__global__ __launch_bounds__(256) void k_cigar_plan(CigarArgs ca) {
    __shared__ unsigned long long part[4][2];
    const AlignArgs& a = ca.a;
    const uint64_t total = a.goffs[a.nreads] < a.cap ? a.goffs[a.nreads] : a.cap;
    const uint64_t span = a.cap + 1 > a.nreads ? a.cap + 1 : a.nreads;
    unsigned long long words = 0, bound = 0;
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < span; t += (uint64_t)gridDim.x * 256) {
        if (t <= a.cap) {
            unsigned long long w = 0;
            if (t < total) {
                const uint4 gp = a.gaps[t];
                const uint32_t ga = gp.x, gb = gp.y;
                if (ga > a.max_fill || gb > a.max_fill) {
                    bound += (unsigned long long)(ga >> 28) + (gb >> 28) + 2;
                } else if (ga == 0 || gb == 0) {
                    bound += (ga | gb) != 0;
                } else if (ga == 1 && gb == 1) {
                    bound += 1;
                } else {
                    w = path_words_of(ga, gb);
                    bound += (unsigned long long)ga + gb;
                }
            }
            ca.pw[t] = w;
            words += w;
        }
        if (t < a.nreads) {
            const uint4 w0 = a.out[3 * t];
            // an anchor's kept part is one run: the parts add up to less than 2^32 characters, 16 full entries at the most
            if (!(w0.x == 0xffffffffu && w0.y == 0xffffffffu)) bound += (unsigned long long)a.out[3 * t + 2].x + 16;
        }
    }
    words = wave_sum(words);
    bound = wave_sum(bound);
    if ((threadIdx.x & 63) == 0) {
        part[threadIdx.x >> 6][0] = words;
        part[threadIdx.x >> 6][1] = bound;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const unsigned long long v = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (v) atomicAdd(threadIdx.x == 0 ? &ca.c->path_words : &ca.c->ops_bound, v);
    }
}

// One lane's table as fill_lane has it, with each row's directions packed into one word of the lane's column of LDS
// (dirs[(i - 1) * 256]), and the walk back from (a, b): the steps go to `path`, 16 a word, when there is room.  Returns
// the corner's cell.
__device__ inline uint32_t trace_lane(const uint8_t* A, const uint8_t* B, uint32_t a, uint32_t b, uint32_t* dirs, uint32_t* path) {
    uint32_t row[LANE_MAX + 1];
    uint8_t bc[LANE_MAX];
#pragma unroll
    for (uint32_t j = 0; j < LANE_MAX; ++j) bc[j] = j < b ? B[j] : 0;
#pragma unroll
    for (uint32_t j = 0; j <= LANE_MAX; ++j) row[j] = j * EDIT | 0xffffu;
    for (uint32_t i = 1; i <= a; ++i) {
        const uint8_t ac = A[i - 1];
        uint32_t diag = row[0], left = i * EDIT | 0xffffu, dw = 0;
        row[0] = left;
#pragma unroll
        for (uint32_t j = 1; j <= LANE_MAX; ++j) {
            const uint32_t up = row[j];
            const bool eq = ac == bc[j - 1];
            const uint32_t d = eq ? diag - 1 : diag + EDIT, u = up + EDIT, l = left + EDIT;
            uint32_t v = u < l ? u : l;
            v = d < v ? d : v;
            const uint32_t code = d == v ? (eq ? 0u : 1u) : (u == v ? 2u : 3u);
            dw |= code << (2 * (j - 1));
            diag = up;
            left = v;
            row[j] = v;  // (columns past b hold values nothing reads: a column depends on those to its left alone)
        }
        dirs[(i - 1) * 256] = dw;
    }
    uint32_t r = row[1];
#pragma unroll
    for (uint32_t j = 2; j <= LANE_MAX; ++j) r = j == b ? row[j] : r;
    if (path) {
        uint32_t i = a, j = b, k = 0, acc = 0;
        while (i | j) {  // at most a + b steps: ceil((a + b) / 16) words
            const uint32_t code = i == 0 ? 3u : j == 0 ? 2u : (dirs[(i - 1) * 256] >> (2 * (j - 1))) & 3u;
            acc |= code << (2 * (k & 15));
            if ((k & 15) == 15) {
                path[k >> 4] = acc;
                acc = 0;
            }
            ++k;
            i -= code != 3u;
            j -= code != 2u;
        }
        if (k & 15) path[k >> 4] = acc;
    }
    return r;
}

__global__ __launch_bounds__(256) void k_trace_small(CigarArgs ca) {
    __shared__ uint32_t dirs[LANE_MAX * 256];
    const AlignArgs& a = ca.a;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t total = a.goffs[a.nreads] < a.cap ? a.goffs[a.nreads] : a.cap;
    bool big = false, big2 = false;
    if (g < total) {
        const uint4 gp = a.gaps[g];
        const uint32_t ga = gp.x, gb = gp.y;
        uint32_t edits, matches = 0;
        if (ga > a.max_fill || gb > a.max_fill) {
            edits = SPA_UNFILLED;
        } else if (ga == 0 || gb == 0) {
            edits = ga > gb ? ga : gb;
        } else {
            const ulonglong2 d = a.desc[g];
            const uint8_t *A = a.R + d.x, *B = a.T + d.y;
            if (ga == 1 && gb == 1) {
                matches = A[0] == B[0];
                edits = 1 - matches;
            } else if (ga <= LANE_MAX && gb <= LANE_MAX) {
                const uint64_t p0 = ca.poffs[g];
                const bool room = p0 + path_words_of(ga, gb) <= ca.path_cap;
                const uint32_t v = trace_lane(A, B, ga, gb, dirs + threadIdx.x, room ? ca.path + p0 : nullptr);
                edits = v >> 16;
                matches = 0xffffu - (v & 0xffffu);
            } else {
                big = (uint64_t)ga * ((gb + 15) / 16) <= TRACE_LDS_WORDS;
                big2 = !big;
                edits = 0;
            }
        }
        if (!big && !big2) a.gaps[g] = make_uint4(ga, gb, edits, matches);
    }
    // the gaps that need a wavefront: one atomic per wavefront and list, and a list's order does not matter -- a gap's
    // result goes to the gap's own place.  Those whose trace fits LDS stand from the front of the list, the others from
    // its end (nbig + nbig2 <= total <= cap: the two never meet)
    const unsigned long long mask = __ballot(big), mask2 = __ballot(big2);
    if (mask) {
        const int leader = __ffsll(mask) - 1;
        unsigned long long at = 0;
        if ((int)lane == leader) at = atomicAdd(&ca.c->a.nbig, (unsigned long long)__popcll(mask));
        at = __shfl(at, leader);
        if (big) a.list[at + __popcll(mask & ((1ull << lane) - 1))] = (uint32_t)g;
    }
    if (mask2) {
        const int leader = __ffsll(mask2) - 1;
        unsigned long long at = 0;
        if ((int)lane == leader) at = atomicAdd(&ca.c->nbig2, (unsigned long long)__popcll(mask2));
        at = __shfl(at, leader);
        if (big2) a.list[a.cap - 1 - (at + __popcll(mask2 & ((1ull << lane) - 1)))] = (uint32_t)g;
    }
}

// A wavefront per listed gap: align's k_fill_wave (strips of 64 rows, a lane per row, an anti-diagonal a step) with the
// direction of every cell kept: lane r packs 16 consecutive columns of its row into one word and stores it to
// tr[(i - 1) * wpr + w], wpr = ceil(b / 16).  GLOBAL: tr is the wavefront's own buffer in device memory, else LDS.
// Dynamic LDS: bound[max_fill + 1], the trace (not GLOBAL), then B.
template <bool GLOBAL>
__global__ __launch_bounds__(64) void k_trace_wave(CigarArgs ca) {
    extern __shared__ uint32_t lds[];
    const AlignArgs& a = ca.a;
    uint32_t* bound = lds;
    uint32_t* tr = GLOBAL ? ca.trace + (size_t)blockIdx.x * ca.trace_stride : lds + a.max_fill + 1;
    uint8_t* Bs = (uint8_t*)(lds + a.max_fill + 1 + (GLOBAL ? 0 : TRACE_LDS_WORDS));
    const uint32_t lane = threadIdx.x;
    const unsigned long long n = __shfl(GLOBAL ? ca.c->nbig2 : ca.c->a.nbig, 0);
    unsigned long long t_fill = 0, t_back = 0;
    for (unsigned long long k = blockIdx.x; k < n; k += gridDim.x) {
        const unsigned long long t0 = wall_clock64();
        const uint64_t g = a.list[GLOBAL ? a.cap - 1 - k : k];
        const uint4 gp = a.gaps[g];
        const uint32_t ga = __shfl(gp.x, 0), gb = __shfl(gp.y, 0);  // (1 .. max_fill: k_trace_small listed it)
        const ulonglong2 d = a.desc[g];
        const uint8_t *A = a.R + d.x, *B = a.T + d.y;
        const uint32_t wpr = (gb + 15) / 16;  // (ga * wpr words fit tr: the list's kind, or max_fill * ceil(max_fill / 16))
        __syncthreads();  // (the gap before is done with the LDS and the trace)
        for (uint32_t j = lane; j <= gb; j += 64) bound[j] = j * EDIT | 0xffffu;
        for (uint32_t j = lane; j < gb; j += 64) Bs[j] = B[j];
        __syncthreads();
        const uint32_t nstrips = (ga + 63) / 64;
        for (uint32_t s = 0; s < nstrips; ++s) {
            const uint32_t i = s * 64 + lane + 1;
            const bool row_ok = i <= ga;
            const uint32_t rows = ga - s * 64 < 64 ? ga - s * 64 : 64;
            const uint8_t ac = row_ok ? A[i - 1] : 0;
            uint32_t left = i * EDIT | 0xffffu, diag = (i - 1) * EDIT | 0xffffu, cur = left, dw = 0;
            const uint32_t steps = gb + rows - 1;
            for (uint32_t st = 0; st < steps; ++st) {
                const int32_t j = (int32_t)st - (int32_t)lane + 1;
                const bool act = row_ok && j >= 1 && j <= (int32_t)gb;
                uint32_t up = __shfl_up(cur, 1);
                if (act) {
                    if (lane == 0) up = bound[j];
                    const bool eq = ac == Bs[j - 1];
                    const uint32_t dg = eq ? diag - 1 : diag + EDIT, u = up + EDIT, l = left + EDIT;
                    uint32_t v = u < l ? u : l;
                    v = dg < v ? dg : v;
                    const uint32_t code = dg == v ? (eq ? 0u : 1u) : (u == v ? 2u : 3u);
                    const uint32_t sh = (uint32_t)(j - 1) & 15;
                    dw |= code << (2 * sh);
                    if (sh == 15 || j == (int32_t)gb) {
                        tr[(size_t)(i - 1) * wpr + ((uint32_t)(j - 1) >> 4)] = dw;
                        dw = 0;
                    }
                    diag = up;
                    left = v;
                    cur = v;
                    if (lane == rows - 1) bound[j] = v;
                }
            }
            __syncthreads();
        }
        if (GLOBAL) __threadfence_block();
        __syncthreads();  // (every lane's trace words are visible to the wavefront)
        const unsigned long long t1 = wall_clock64();
        const uint32_t v = bound[gb];
        const uint64_t p0 = ca.poffs[g];
        if (p0 + path_words_of(ga, gb) <= ca.path_cap) {  // (else the emit leaves the read unaligned: overflow)
            uint32_t* path = ca.path + p0;
            // the same walk in every lane.  The cache: lane r holds the word of row i0 - r in the column of words wj0
            uint32_t i = ga, j = gb, kk = 0, acc = 0, i0 = 0, wj0 = 0xffffffffu, pref = 0;
            while (i | j) {
                uint32_t code;
                if (i == 0) {
                    code = 3u;
                } else if (j == 0) {
                    code = 2u;
                } else {
                    const uint32_t wj = (j - 1) >> 4;
                    if (wj != wj0 || i0 - i > 63) {  // (i <= i0 always: the walk only goes up)
                        i0 = i;
                        wj0 = wj;
                        pref = lane < i0 ? tr[(size_t)(i0 - lane - 1) * wpr + wj] : 0;
                    }
                    code = (__shfl(pref, (int)(i0 - i)) >> (2 * ((j - 1) & 15))) & 3u;
                }
                acc |= code << (2 * (kk & 15));
                if ((kk & 15) == 15) {
                    if (lane == 0) path[kk >> 4] = acc;
                    acc = 0;
                }
                ++kk;
                i -= code != 3u;
                j -= code != 2u;
            }
            if ((kk & 15) && lane == 0) path[kk >> 4] = acc;
        }
        if (lane == 0) a.gaps[g] = make_uint4(ga, gb, v >> 16, 0xffffu - (v & 0xffffu));
        const unsigned long long t2 = wall_clock64();
        t_fill += t1 - t0;
        t_back += t2 - t1;
    }
    if (lane == 0 && (t_fill | t_back)) {
        atomicAdd(&ca.c->fill_ticks, t_fill);
        atomicAdd(&ca.c->back_ticks, t_back);
    }
}

__device__ inline uint32_t op_of_step(uint32_t code) {
    return code == 0 ? SPG_OP_EQ : code == 1 ? SPG_OP_X : code == 2 ? SPG_OP_I : SPG_OP_D;
}

// A read's entries: counted, or (WRITE) written to dst.  OVER: one of the read's paths had no room.  ENDS: the clip and
// the left end's steps in front of the first anchor, the right end's steps and the clip behind the last; an end's path
// is stored from its end point to (0, 0), which for the left end is the read's order.
template <bool WRITE, bool ENDS>
__device__ inline uint64_t emit_read(const CigarArgs& ca, uint64_t q, uint32_t* dst) {
    const AlignArgs& a = ca.a;
    const uint4 w0 = a.out[3 * q];
    if (w0.x == 0xffffffffu && w0.y == 0xffffffffu) return 0;
    const uint4 w1 = a.out[3 * q + 1];  // the walk's version: z = l_first + the sum of keep, w = l_first
    const uint64_t g0 = a.goffs[q], g1 = a.goffs[q + 1];  // (an aligned read's gaps are all below cap)
    if (g1 > g0 && ca.poffs[g1] > ca.path_cap) return OVER;
    const uint64_t ebase = ENDS ? ca.poffs[a.cap] : 0;
    if (ENDS && ebase + ca.epoffs[2 * q + 2] > ca.path_cap) return OVER;
    uint32_t op = ENDS ? OP_S : SPG_OP_EQ;
    uint64_t len = ENDS ? w1.x - ca.eres[4 * q].x : w1.w, n = 0, kept = w1.w;
    auto flush = [&]() {
        if (ENDS && !len) return;
        const uint64_t full = (len - 1) / SPG_MAX_LENGTH;  // (len >= 1)
        if (WRITE) {
            for (uint64_t f = 0; f < full; ++f) dst[n + f] = SPG_MAX_LENGTH << 4 | op;
            dst[n + full] = (uint32_t)(len - full * SPG_MAX_LENGTH) << 4 | op;
        }
        n += full + 1;
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
    auto push_end = [&](uint32_t side) {  // the steps of one end in the read's order
        const uint32_t* p = ca.path + ebase + ca.epoffs[2 * q + side];
        const uint32_t steps = ca.eres[4 * q + 2 * side + 1].x;  // (at most a + b: within the end's words)
        uint32_t cw = 0xffffffffu, word = 0;
        for (uint32_t t = 0; t < steps; ++t) {
            const uint32_t idx = side ? steps - 1 - t : t;
            if ((idx >> 4) != cw) {
                cw = idx >> 4;
                word = p[cw];
            }
            push(op_of_step((word >> (2 * (idx & 15))) & 3u), 1);
        }
    };
    if (ENDS) {
        push_end(0);
        push(SPG_OP_EQ, w1.w);
    }
    for (uint64_t g = g0; g < g1; ++g) {
        const uint4 gp = a.gaps[g];
        const uint32_t ga = gp.x, gb = gp.y;
        if (gp.z == SPA_UNFILLED) {
            push(SPG_OP_I, ga);
            push(SPG_OP_N, gb);
        } else if (ga == 0 || gb == 0) {
            push(ga ? SPG_OP_I : SPG_OP_D, ga | gb);
        } else if (ga == 1 && gb == 1) {
            push(gp.w ? SPG_OP_EQ : SPG_OP_X, 1);
        } else {
            const uint32_t* p = ca.path + ca.poffs[g];
            const uint32_t steps = gp.z + gp.w;  // (at most a + b: within the gap's words)
            uint32_t cw = 0xffffffffu, word = 0;
            for (uint32_t t = 0; t < steps; ++t) {
                const uint32_t idx = steps - 1 - t;
                if ((idx >> 4) != cw) {
                    cw = idx >> 4;
                    word = p[cw];
                }
                const uint32_t code = (word >> (2 * (idx & 15))) & 3u;
                push(code == 0 ? SPG_OP_EQ : code == 1 ? SPG_OP_X : code == 2 ? SPG_OP_I : SPG_OP_D, 1);
            }
        }
        // the kept part of the anchor behind the gap ends where the next gap's A starts; the last one takes the rest
        const uint64_t keep = g + 1 < g1 ? a.desc[g + 1].x - a.desc[g].x - ga : (uint64_t)w1.z - kept;
        push(SPG_OP_EQ, keep);
        kept += keep;
    }
    if (ENDS) {
        push_end(1);
        // (the plan checked the record's spans against the read: the end point lies within it)
        push(OP_S, a.roffs[q + 1] - a.roffs[q] - w1.y - ca.eres[4 * q + 2].x);
    }
    flush();
    return n;
}

template <bool ENDS>
__global__ __launch_bounds__(256) void k_cigar_count(CigarArgs ca) {
    const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (q > ca.a.nreads) return;
    uint64_t n = 0;
    if (q < ca.a.nreads) {
        n = emit_read<false, ENDS>(ca, q, nullptr);
        if (n == OVER) n = 0;
    }
    ca.ocnt[q] = n;
}

template <bool ENDS>
__global__ __launch_bounds__(256) void k_cigar_write(CigarArgs ca) {
    const AlignArgs& a = ca.a;
    const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long n = 0;
    if (q < a.nreads) {
        const uint4 w0 = a.out[3 * q];
        if (!(w0.x == 0xffffffffu && w0.y == 0xffffffffu)) {
            const uint64_t o0 = ca.ooffs[q], o1 = ca.ooffs[q + 1];
            // (an aligned read has at least one entry: no entries means that a path of its had no room)
            if (o1 == o0 || o1 > ca.op_cap) {
                atomicOr(&ca.c->a.error, 2ull);
                write_unaligned(a, q);
            } else {
                n = emit_read<true, ENDS>(ca, q, ca.ops + o0);
            }
        }
    }
    n = wave_sum(n);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&ca.c->entries, n);
}


int check_cigar_pointers(const spx_index* ix, const char* what) {
    if (!ix->text) {
        set_error("%s need the text (spx_index_set_text / spx_index_rebuild_text)", what);
        return SPX_E_ARG;
    }
    return SPX_OK;
}

struct CigarPlan {  // what the host works out before anything is enqueued
    size_t cub_bytes = 0;
    void* cub = nullptr;
    unsigned grid_global = 1, grid_ends = 1;
    size_t lds_local = 0, lds_global = 0;
};

// The extension's own kernels, enqueued by spx_extend.hip: the ends' sizes behind the walk over pred (a read whose spans
// fail its checks leaves the plan unaligned), their fill and walk back in front of the emit, the records' update behind
// the reduction.
struct EndHooks {
    int (*plan)(CigarArgs& ca, const CigarPlan& plan, hipStream_t st);
    int (*fill)(CigarArgs& ca, const CigarPlan& plan, hipStream_t st);
    int (*finish)(CigarArgs& ca, hipStream_t st);
};
// The product that is calling: its scratch (TB_COUNT slots), its counters and times, the entries that wait for its _fetch,
// the extension's kernels and its names.  Steps: 0 plan, 1 lane fills, 2 wavefront fills, 3 emit, 4 reduce, 5 the ends.
struct TraceView {
    spx_index::Scratch* scr;
    spx_index::Product* p;
    spx_index::Ready* ready;
    const EndHooks* ends;  // null: the CIGARs
    const char* what;  // the product in a message: "the CIGARs", "the extended CIGARs"
    const char* begin_name;
    const char* fetch_name;
};

// words of trace one end needs at most: a lane owns a diagonal of the band, 16 rows a word
inline uint64_t end_trace_words(uint32_t max_extend, uint32_t band) { return (uint64_t)((max_extend + 15) / 16) * (2 * band + 1); }

// The scratch of one call but the path and (host form) the entries.  Takes ix->mu.
int cigar_reserve(spx_index* ix, const TraceView& tv, CigarArgs& ca, bool own_ooffs, CigarPlan* plan) {
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    AlignArgs& a = ca.a;
    spx_index::Scratch* scr = tv.scr;
    void* p = nullptr;
    int rc;
    if ((rc = scr[spx_index::TB_PW].reserve((a.cap + 1) * 8, &p)) != SPX_OK) return rc;
    ca.pw = (uint64_t*)p;
    if ((rc = scr[spx_index::TB_POFFS].reserve((a.cap + 1) * 8, &p)) != SPX_OK) return rc;
    ca.poffs = (uint64_t*)p;
    if ((rc = scr[spx_index::TB_OCNT].reserve((a.nreads + 1) * 8, &p)) != SPX_OK) return rc;
    ca.ocnt = (uint64_t*)p;
    if (own_ooffs) {
        if ((rc = scr[spx_index::TB_OOFFS].reserve((a.nreads + 1) * 8, &p)) != SPX_OK) return rc;
        ca.ooffs = (uint64_t*)p;
    }
    // the wavefronts' trace buffers: sized by max_fill alone, the grid shrinking as it grows
    const uint64_t per_block = (uint64_t)a.max_fill * ((a.max_fill + 15) / 16);  // words
    ca.trace_stride = per_block;
    uint64_t grid = TRACE_BUDGET / (per_block * 4);
    grid = std::min<uint64_t>(std::max<uint64_t>(grid, 1), 4096);
    grid = std::max<uint64_t>(std::min<uint64_t>(grid, a.cap), 1);
    plan->grid_global = (unsigned)grid;
    if ((rc = scr[spx_index::TB_TRACE].reserve(grid * per_block * 4, &p)) != SPX_OK) return rc;
    ca.trace = (uint32_t*)p;
    plan->lds_global = ((size_t)a.max_fill + 1) * 4 + a.max_fill;
    plan->lds_local = plan->lds_global + TRACE_LDS_WORDS * 4;
    size_t b2 = 0, b3 = 0;
    SPX_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, b2, ca.pw, ca.poffs, a.cap + 1, (hipStream_t) nullptr));
    if (tv.ends) {
        if ((rc = scr[spx_index::TB_EPW].reserve((2 * a.nreads + 1) * 8, &p)) != SPX_OK) return rc;
        ca.epw = (uint64_t*)p;
        if ((rc = scr[spx_index::TB_EPOFFS].reserve((2 * a.nreads + 1) * 8, &p)) != SPX_OK) return rc;
        ca.epoffs = (uint64_t*)p;
        if ((rc = scr[spx_index::TB_ERES].reserve(a.nreads * 64 + 16, &p)) != SPX_OK) return rc;
        ca.eres = (uint4*)p;
        // an end's trace goes to device memory only when the parameters let it outgrow LDS: a buffer per wavefront then,
        // within the same budget
        const uint64_t words = end_trace_words(ca.max_extend, ca.band);
        uint64_t egrid = std::min<uint64_t>(std::max<uint64_t>(2 * a.nreads, 1), ENDS_GRID);
        ca.etrace_stride = 0;
        if (words > TRACE_LDS_WORDS) {
            ca.etrace_stride = words;
            egrid = std::min<uint64_t>(egrid, std::max<uint64_t>(TRACE_BUDGET / (words * 4), 1));
        }
        plan->grid_ends = (unsigned)egrid;
        if ((rc = scr[spx_index::TB_ETRACE].reserve(egrid * ca.etrace_stride * 4 + 16, &p)) != SPX_OK) return rc;
        ca.etrace = (uint32_t*)p;
        SPX_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, b3, ca.epw, ca.epoffs, 2 * a.nreads + 1, (hipStream_t) nullptr));
    }
    return reserve_gaps(scr, a, true, true, std::max(b2, b3), &plan->cub_bytes, &plan->cub);
}
int cigar_reserve_path(spx_index* ix, const TraceView& tv, CigarArgs& ca, uint64_t words) {
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    void* p = nullptr;
    int rc;
    if ((rc = tv.scr[spx_index::TB_PATH].reserve(words * 4 + 16, &p)) != SPX_OK) return rc;
    ca.path = (uint32_t*)p;
    ca.path_cap = words;
    return SPX_OK;
}

// The plan on st (inside product_enqueue's launch, which has marked step 0).
int launch_plan(const TraceView& tv, CigarArgs& ca, const CigarPlan& plan, hipStream_t st) {
    size_t cub_bytes = plan.cub_bytes;
    AlignArgs& a = ca.a;
    int rc;
    const unsigned read_grid = (unsigned)((a.nreads + 1 + 255) / 256);
    k_align_count<<<read_grid, 256, 0, st>>>(a);
    SPX_HIP(hipGetLastError());
    SPX_HIP(hipcub::DeviceScan::ExclusiveSum(plan.cub, cub_bytes, a.cnt, a.goffs, a.nreads + 1, st));
    k_align_walk<<<read_grid, 256, 0, st>>>(a);
    SPX_HIP(hipGetLastError());
    if (tv.ends && (rc = tv.ends->plan(ca, plan, st)) != SPX_OK) return rc;
    k_cigar_plan<<<(unsigned)std::min<uint64_t>((std::max<uint64_t>(a.cap + 1, a.nreads) + 255) / 256, 1024), 256, 0, st>>>(ca);
    SPX_HIP(hipGetLastError());
    SPX_HIP(hipcub::DeviceScan::ExclusiveSum(plan.cub, cub_bytes, ca.pw, ca.poffs, a.cap + 1, st));
    return SPX_OK;
}
// The step the fills, the emit and the reduction begin with: the ends' or the lane fills'.
inline int trace_first_step(const TraceView& tv) { return tv.ends ? 5 : 1; }
// The fills, the emit and the reduction on st (inside product_enqueue's launch).  at_open: the launch begins here and
// product_enqueue has opened with trace_first_step, which needs no mark of its own.
int launch_trace(const TraceView& tv, CigarArgs& ca, const CigarPlan& plan, bool at_open, hipStream_t st) {
    size_t cub_bytes = plan.cub_bytes;
    AlignArgs& a = ca.a;
    spx_index::Product& p = *tv.p;
    auto begin = [&](int step) -> int { return at_open && step == trace_first_step(tv) ? SPX_OK : product_mark(p, step, st); };
    int rc;
    const unsigned read_grid = (unsigned)((a.nreads + 1 + 255) / 256);
    if (tv.ends) {
        if ((rc = begin(5)) != SPX_OK) return rc;
        if ((rc = tv.ends->fill(ca, plan, st)) != SPX_OK) return rc;
    }
    if ((rc = begin(1)) != SPX_OK) return rc;
    if (a.cap) {
        // (the number of gaps is the device's: the grid covers the capacity, and lanes past the total leave at once)
        k_trace_small<<<(unsigned)((a.cap + 255) / 256), 256, 0, st>>>(ca);
        SPX_HIP(hipGetLastError());
    }
    if ((rc = product_mark(p, 2, st)) != SPX_OK) return rc;
    if (a.cap) {
        k_trace_wave<false><<<(unsigned)std::min<uint64_t>(a.cap, 4096), 64, plan.lds_local, st>>>(ca);
        SPX_HIP(hipGetLastError());
        k_trace_wave<true><<<plan.grid_global, 64, plan.lds_global, st>>>(ca);
        SPX_HIP(hipGetLastError());
    }
    if ((rc = product_mark(p, 3, st)) != SPX_OK) return rc;
    if (tv.ends)
        k_cigar_count<true><<<read_grid, 256, 0, st>>>(ca);
    else
        k_cigar_count<false><<<read_grid, 256, 0, st>>>(ca);
    SPX_HIP(hipGetLastError());
    SPX_HIP(hipcub::DeviceScan::ExclusiveSum(plan.cub, cub_bytes, ca.ocnt, ca.ooffs, a.nreads + 1, st));
    if (tv.ends)
        k_cigar_write<true><<<read_grid, 256, 0, st>>>(ca);
    else
        k_cigar_write<false><<<read_grid, 256, 0, st>>>(ca);
    SPX_HIP(hipGetLastError());
    if ((rc = product_mark(p, 4, st)) != SPX_OK) return rc;
    k_align_reduce<<<std::min(read_grid, 1024u), 256, 0, st>>>(a);
    SPX_HIP(hipGetLastError());
    if (tv.ends && (rc = tv.ends->finish(ca, st)) != SPX_OK) return rc;
    return SPX_OK;
}

// One or both phases on st, between the product's two events: the time from ev0 on is the first step's of the first
// phase there is (no step's for a batch without reads: its step times are zeros).  Takes ix->mu.
int cigar_enqueue(spx_index* ix, const TraceView& tv, CigarArgs& ca, const CigarPlan& plan, bool first, bool second, hipStream_t st) {
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    return product_enqueue(*tv.p, CIGAR_WORDS, st, [&](void* counters) -> int {
        ca.c = (CigarCounters*)counters;
        ca.a.c = &ca.c->a;
        int rc;
        if (!ca.a.nreads) {
            SPX_HIP(hipMemsetAsync(ca.ooffs, 0, 8, st));
            return SPX_OK;
        }
        if (first && (rc = launch_plan(tv, ca, plan, st)) != SPX_OK) return rc;
        if (second && (rc = launch_trace(tv, ca, plan, !first, st)) != SPX_OK) return rc;
        return SPX_OK;
    }, !ca.a.nreads ? -1 : first ? 0 : trace_first_step(tv));
}
int cigar_error_code(const TraceView& tv) {
    if (tv.p->error & 1) {
        set_error(tv.ends ? "a read's chain failed the walk's checks (pred, anchors, first / last, a link of negative length, a gap "
                            "outside the read or the text, or spans outside the read or the text): such a read is left unaligned"
                          : "a read's chain failed the walk's checks (pred, anchors, first / last, a link of negative length, or a gap "
                            "outside the read or the text): such a read is left unaligned");
        return SPX_E_FORMAT;
    }
    return SPX_OK;
}

// What the four parameters of the extension are to the kernels (zeros for the CIGARs) and the ends a caller asked for.
struct EndParams {
    uint32_t max_extend = 0, band = 0, mismatch = 0, indel = 0;
};
inline void set_end_params(CigarArgs& ca, const EndParams& ep) {
    ca.max_extend = ep.max_extend;
    ca.band = ep.band;
    ca.mismatch = ep.mismatch;
    ca.indel = ep.indel;
}
// words of path the ends of nreads reads take at most: a + b steps each, b <= a + band
inline uint64_t end_path_bound(uint64_t nreads, const EndParams& ep) {
    return 2 * nreads * ((2ull * ep.max_extend + ep.band + 15) / 16);
}

// The device form of both products, behind the checks of the parameters.
int trace_device(spx_index* ix, const TraceView& tv, const uint8_t* d_reads, const uint64_t* d_read_offsets, const spm_match* d_matches,
                 const uint64_t* d_match_offsets, uint64_t nreads, const spc_chain* d_chains, const uint32_t* d_pred,
                 const spa_params* params, const EndParams& ep, uint64_t gap_capacity, uint64_t op_capacity, spa_alignment* d_out,
                 uint64_t* d_out_op_offsets, uint32_t* d_out_ops, void* d_out_ends, void* stream) {
    int rc;
    if ((rc = check_cigar_pointers(ix, tv.what)) != SPX_OK) return rc;
    if (!d_out_op_offsets || (op_capacity && !d_out_ops) ||
        (nreads && (!d_reads || !d_read_offsets || !d_matches || !d_match_offsets || !d_chains || !d_pred || !d_out))) {
        set_error("d_reads, d_read_offsets, d_matches, d_match_offsets, d_chains, d_pred, d_out, d_out_op_offsets and d_out_ops "
                  "must be non-null");
        return SPX_E_ARG;
    }
    if (gap_capacity > 0xffffffffull || op_capacity > 0xffffffffull) {
        set_error("gap_capacity and op_capacity must be at most 2^32 - 1");
        return SPX_E_ARG;
    }
    if ((((uintptr_t)d_matches | (uintptr_t)d_chains | (uintptr_t)d_out | (uintptr_t)d_out_ends) & 15) != 0 ||
        (((uintptr_t)d_read_offsets | (uintptr_t)d_match_offsets | (uintptr_t)d_out_op_offsets) & 7) != 0 ||
        (((uintptr_t)d_pred | (uintptr_t)d_out_ops) & 3) != 0) {
        set_error(tv.ends ? "d_matches, d_chains, d_out and d_out_ends must be 16-byte aligned (records are read and written as 16-byte "
                            "vectors), the 64-bit arrays 8-byte, d_pred and d_out_ops 4-byte aligned"
                          : "d_matches, d_chains and d_out must be 16-byte aligned (records are read and written as 16-byte vectors), "
                            "the 64-bit arrays 8-byte, d_pred and d_out_ops 4-byte aligned");
        return SPX_E_ARG;
    }
    product_reset(ix, *tv.p);
    CigarArgs ca{};
    AlignArgs& a = ca.a;
    a.R = d_reads;
    a.roffs = d_read_offsets;
    a.M = (const uint4*)d_matches;
    a.moffs = d_match_offsets;
    a.nreads = nreads;
    a.chains = (const uint4*)d_chains;
    a.pred = d_pred;
    a.T = ix->text;
    a.n_text = ix->n_text;
    a.max_fill = params->max_fill;
    a.cap = gap_capacity;
    a.out = (uint4*)d_out;
    ca.ooffs = d_out_op_offsets;
    ca.ops = d_out_ops;
    ca.op_cap = op_capacity;
    set_end_params(ca, ep);
    ca.out_ends = (uint4*)d_out_ends;
    CigarPlan plan;
    if ((rc = cigar_reserve(ix, tv, ca, false, &plan)) != SPX_OK) return rc;
    // every scratch byte before the first kernel: the path by what the host knows
    const uint64_t words = std::min<uint64_t>(gap_capacity * ((params->max_fill + 7) / 8) + (tv.ends ? end_path_bound(nreads, ep) : 0),
                                              PATH_LIMIT);
    if ((rc = cigar_reserve_path(ix, tv, ca, words)) != SPX_OK) return rc;
    return cigar_enqueue(ix, tv, ca, plan, true, true, (hipStream_t)stream);
}

// The host pair of both products.  spa_align_batch's steps with the cigar kernels in place of the align kernels, in two
// phases: behind the plan the host waits for the words of path and the bound of the entries, reserves both and enqueues
// the rest.
int trace_begin(spx_index* ix, const TraceView& tv, int digest_kind, uint32_t k, uint32_t w, const uint8_t* seqs, const uint64_t* offsets,
                uint64_t nreads, uint64_t min_length, int want_docs, const spc_params* chain_params, const spa_params* align_params,
                const EndParams& ep, spa_alignment* out_alignments, spc_chain* out_chains, uint64_t* out_values, void* out_ends,
                uint64_t* n_entries) {
    int rc;
    if ((rc = chain_check_params(ix, chain_params)) != SPX_OK) return rc;
    if ((rc = check_batch(ix, tv.what, BATCH_MIN_LENGTH | BATCH_TEXT | BATCH_ONE_PIECE, min_length, digest_kind, want_docs,
                          !n_entries || (nreads && (!seqs || !offsets || !out_alignments))
                              ? "seqs, offsets, out_alignments and n_entries must be non-null"
                              : nullptr,
                          offsets, nreads)) != SPX_OK)
        return rc;
    std::lock_guard<std::mutex> hg(ix->host_mu);
    SPX_HIP(hipSetDevice(ix->device));
    product_reset(ix, *tv.p);
    product_reset(ix, ix->chain);
    tv.ready->ok = false;
    *n_entries = 0;
    if (nreads == 0) {
        tv.p->have = ix->chain.have = true;  // (the stats of an empty batch are zeros)
        ready_publish(*tv.ready, 0, 0);
        return SPX_OK;
    }
    spx_index::Scratch* scr = tv.scr;
    void *d_chains = nullptr, *d_out = nullptr, *d_ends = nullptr;
    if ((rc = scr[spx_index::TB_CHAINS].reserve(nreads * sizeof(spc_chain), &d_chains)) != SPX_OK) return rc;
    if ((rc = scr[spx_index::TB_OUT].reserve(nreads * sizeof(spa_alignment), &d_out)) != SPX_OK) return rc;
    if (tv.ends && out_ends && (rc = scr[spx_index::TB_ENDS].reserve(nreads * 32, &d_ends)) != SPX_OK) return rc;
    std::vector<uint64_t> match_offsets(nreads + 1);
    uint64_t n = 0;
    rc = mems_begin_staged(
        ix, digest_kind, k, w, seqs, offsets, nreads, min_length, want_docs, match_offsets.data(), out_values, &n, true,
        [&](const MemsOnDevice& m) -> int {
            void* d_pred = nullptr;
            int r;
            if ((r = scr[spx_index::TB_PRED].reserve(m.n * 4 + 16, &d_pred)) != SPX_OK) return r;
            CigarArgs ca{};
            AlignArgs& a = ca.a;
            a.R = m.reads;
            a.roffs = m.read_offsets;
            a.M = (const uint4*)m.records;
            a.moffs = m.match_offsets;
            a.nreads = m.nreads;
            a.chains = (const uint4*)d_chains;
            a.pred = (const uint32_t*)d_pred;
            a.T = ix->text;
            a.n_text = ix->n_text;
            a.max_fill = align_params->max_fill;
            a.cap = m.n;  // (a chain of h anchors has h - 1 gaps: the number of matches always suffices)
            a.out = (uint4*)d_out;
            set_end_params(ca, ep);
            ca.out_ends = (uint4*)d_ends;
            CigarPlan plan;
            if ((r = cigar_reserve(ix, tv, ca, true, &plan)) != SPX_OK) return r;
            if ((r = spc_chain_device(ix, (const spm_match*)m.records, m.docs, m.match_offsets, m.nreads, chain_params,
                                      (spc_chain*)d_chains, nullptr, (uint32_t*)d_pred, m.stream)) != SPX_OK)
                return r;
            if ((r = cigar_enqueue(ix, tv, ca, plan, true, false, m.stream)) != SPX_OK) return r;
            // the one wait that spa_align_batch does not have: the path's words and the bound of the entries are the
            // device's, and both buffers have their size before the fills are enqueued
            if ((r = product_collect(ix, *tv.p, CIGAR_WORDS, CIGAR_WORDS, CW_ERROR)) != SPX_OK) return r;
            if ((r = cigar_reserve_path(ix, tv, ca, tv.p->acc[CW_PATH_WORDS])) != SPX_OK) return r;
            ca.op_cap = std::min<uint64_t>(tv.p->acc[CW_OPS_BOUND], 0xffffffffull);
            void* d_ops = nullptr;
            if ((r = scr[spx_index::TB_OPS].reserve(ca.op_cap * 4 + 16, &d_ops)) != SPX_OK) return r;
            ca.ops = (uint32_t*)d_ops;
            if ((r = cigar_enqueue(ix, tv, ca, plan, false, true, m.stream)) != SPX_OK) return r;
            SPX_HIP(hipMemcpyAsync(out_alignments, d_out, m.nreads * sizeof(spa_alignment), hipMemcpyDeviceToHost, m.stream));
            if (out_chains)
                SPX_HIP(hipMemcpyAsync(out_chains, d_chains, m.nreads * sizeof(spc_chain), hipMemcpyDeviceToHost, m.stream));
            if (d_ends) SPX_HIP(hipMemcpyAsync(out_ends, d_ends, m.nreads * 32, hipMemcpyDeviceToHost, m.stream));
            return SPX_OK;
        });
    if (rc != SPX_OK) return rc;
    spc_chain_stats cs;
    if ((rc = spc_last_chain_stats(ix, &cs)) != SPX_OK) return rc;
    if ((rc = product_collect(ix, *tv.p, CIGAR_WORDS, CIGAR_WORDS, CW_ERROR)) != SPX_OK) return rc;
    if ((rc = cigar_error_code(tv)) != SPX_OK) return rc;
    if (tv.p->error & 2) {
        set_error("internal: the bound of the entries did not hold");
        return SPX_E_FORMAT;
    }
    *n_entries = tv.p->acc[CW_ENTRIES];
    ready_publish(*tv.ready, *n_entries, nreads);
    return SPX_OK;
}

int trace_fetch(spx_index* ix, const TraceView& tv, uint64_t* out_op_offsets, uint32_t* out_ops) {
    return ready_fetch(ix, *tv.ready, tv.scr[spx_index::TB_OOFFS], tv.scr[spx_index::TB_OPS], tv.fetch_name, tv.begin_name, out_op_offsets,
                       out_ops);
}

}  // namespace
}  // namespace spx
