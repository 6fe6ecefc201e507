// spx_extend.hip -- the extended CIGARs (include/spumoni_extend.h): the CIGARs of spx_cigar.hip taken to
// the read's ends.  Plan, tracing fills, emit and reduction are spx_cigar_kernels.h's, shared with spx_cigar.hip; this
// file adds the three kernels of the ends, which the shared launches call through EndHooks, and the product's C-ABI.
//
//   sizes    (in the plan, behind the walk over pred) a lane per read: the record's spans are checked against the read
//            and the text -- they come from the chain record, which the walk copies and does not check --, each end's
//            a and b give its words of path (a + b steps at most, 16 a word) and its share of the entries' bound, and a
//            device scan places the ends' paths behind the gaps' in the one path scratch;
//   ends     (in front of the gaps' fills) a wavefront per end, grid-stride.  A and B are staged in LDS in the order the
//            table reads them, so the left end is the right end's code on reversed strings.  The wavefront marches the
//            anti-diagonals s = i + j.  On one anti-diagonal only the diagonals D = j - i + band of s's parity have a
//            cell -- at most 64 of the 2 * band + 1 <= 127 --, so lane k owns the two diagonals 2 k and 2 k + 1 and
//            computes the one that is live.  A cell's diagonal neighbour is the lane's own value of two steps back; of
//            its up and left neighbours one is the lane's value of the other diagonal and one a neighbour lane's, so
//            that a step costs one cross-lane read and no LDS for the values.  Each lane keeps its best (score, s, i)
//            in registers -- within a lane s only grows, so a strict comparison keeps the first -- and one butterfly at
//            the end applies the tie rule.  Two bits a cell go to a trace in which a lane owns its diagonals: the word
//            (i - 1) / 16 * (2 * band + 1) + D holds rows 16 at a time, so no two lanes write one word; the trace is in
//            LDS when ceil(a / 16) * (2 * band + 1) words fit TRACE_LDS_WORDS and else in a buffer the wavefront owns.
//            The walk back is the same walk in every lane, with the last trace word kept in a register (a diagonal run
//            of 16 steps reads it once); lane 0 writes the steps, from the end point to (0, 0), to the path scratch;
//   update   (behind the reduction) a lane per read moves the spans, adds the ends' matches and edits, writes the ends on
//            request and counts.
// An end with a = 0 or b = 0 has its end point at (0, 0) by the rule (every other cell is a run of indels) and takes no
// table.
//
// Control flow: every loop that holds a shuffle or a barrier has a trip count that depends on the wavefront alone: a, b and
// the end point are the same in every lane.
#include <climits>

#include "../../include/spumoni_extend.h"
#include "spx_cigar_kernels.h"

namespace spx {
namespace {

constexpr uint32_t EXTEND_LIMIT = 4096, BAND_LIMIT = 63;
static_assert(OP_S == SPE_OP_S, "the shared emit's clip code is the header's");

// One end of an aligned read whose spans the plan has checked: the table reads A[(i - 1) * dir] and B[(j - 1) * dir].
struct EndOf {
    uint32_t a, b;
    const uint8_t *A, *B;
    int dir;
};
__device__ inline EndOf end_of(const CigarArgs& ca, uint64_t q, uint32_t side, const uint4& w0, const uint4& w1) {
    const AlignArgs& al = ca.a;
    const uint64_t ro = al.roffs[q], len = al.roffs[q + 1] - ro;
    const uint64_t ts = (uint64_t)w0.x | ((uint64_t)w0.y << 32), te = (uint64_t)w0.z | ((uint64_t)w0.w << 32);
    EndOf e;
    if (side == 0) {
        e.a = w1.x < ca.max_extend ? w1.x : ca.max_extend;
        const uint64_t room = ts;
        e.b = room < (uint64_t)e.a + ca.band ? (uint32_t)room : e.a + ca.band;
        e.A = al.R + ro + w1.x - 1;
        e.B = al.T + ts - 1;
        e.dir = -1;
    } else {
        const uint64_t rest = len - w1.y;
        e.a = rest < ca.max_extend ? (uint32_t)rest : ca.max_extend;
        const uint64_t room = al.n_text - te;
        e.b = room < (uint64_t)e.a + ca.band ? (uint32_t)room : e.a + ca.band;
        e.A = al.R + ro + w1.y;
        e.B = al.T + te;
        e.dir = 1;
    }
    return e;
}
__device__ inline bool is_unaligned(const uint4& w0) { return w0.x == 0xffffffffu && w0.y == 0xffffffffu; }

// A lane per read, a block over a stride of reads: the two sums leave a block as one pair of atomics, as in k_cigar_plan
// (one pair per wavefront took 0.4 ms on 10^6 reads).
__global__ __launch_bounds__(256) void k_ext_sizes(CigarArgs ca) {
    __shared__ unsigned long long part[4][2];
    const AlignArgs& al = ca.a;
    unsigned long long words = 0, bound = 0;
    for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q <= al.nreads; q += (uint64_t)gridDim.x * 256) {
        if (q == al.nreads) {
            ca.epw[2 * q] = 0;
            break;
        }
        uint64_t w[2] = {0, 0};
        const uint4 w0 = al.out[3 * q];
        if (!is_unaligned(w0)) {
            const uint4 w1 = al.out[3 * q + 1];
            const uint64_t len = al.roffs[q + 1] - al.roffs[q];  // (the walk has checked the offsets)
            const uint64_t ts = (uint64_t)w0.x | ((uint64_t)w0.y << 32), te = (uint64_t)w0.z | ((uint64_t)w0.w << 32);
            if (w1.x > w1.y || w1.y > len || ts > te || te > al.n_text) {
                atomicOr(&ca.c->a.error, 1ull);
                write_unaligned(al, q);
                // as in the walk: the read's places in the table hold empty gaps, so that no fill works for a discarded read
                const uint64_t g0 = al.goffs[q], g1 = al.goffs[q + 1] < al.cap ? al.goffs[q + 1] : al.cap;
                for (uint64_t g = g0; g < g1; ++g) {
                    al.gaps[g] = make_uint4(0, 0, 0, 0);
                    al.desc[g] = make_ulonglong2(0, 0);
                }
            } else {
                for (uint32_t side = 0; side < 2; ++side) {
                    const EndOf e = end_of(ca, q, side, w0, w1);
                    if (e.a && e.b) {
                        w[side] = path_words_of(e.a, e.b);
                        bound += (unsigned long long)e.a + e.b;
                    }
                }
                bound += 2 * 17;  // the clips: below 2^32 characters each, 17 entries at the most
            }
        }
        ca.epw[2 * q] = w[0];
        ca.epw[2 * q + 1] = w[1];
        words += w[0] + w[1];
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

// The table of one end, the same code for a trace in LDS and one in device memory.  Returns with the end point and its
// score in every lane, and the cells this lane evaluated in *cells.
__device__ inline void end_fill(const uint8_t* As, const uint8_t* Bs, uint32_t a, uint32_t b, uint32_t band, int mismatch, int indel,
                                uint32_t* tr, uint32_t lane, uint32_t* end_i, uint32_t* end_j, int* score, uint32_t* cells) {
    const uint32_t nl = 2 * band + 1;
    int v0 = 0, v1 = 0;  // the lane's last cell on its diagonals 2 lane and 2 lane + 1
    int bv = (2 * lane == band || 2 * lane + 1 == band) ? 0 : INT_MIN;  // (0, 0) is a cell
    uint32_t bs = 0, bi = 0, dw0 = 0, dw1 = 0, n = 0;
    const uint32_t steps = a + b;
    for (uint32_t s = 1; s <= steps; ++s) {
        const uint32_t p = (s + band) & 1;
        const int nb = p ? __shfl_down(v0, 1) : __shfl_up(v1, 1);
        const uint32_t D = 2 * lane + p;
        const int t = (int)(s + band) - (int)D;  // 2 i
        const uint32_t i = (uint32_t)t >> 1;
        const int js = (int)s - (int)i;
        if (D < nl && t >= 0 && i <= a && js >= 0 && (uint32_t)js <= b) {
            const uint32_t j = (uint32_t)js;
            const int own = p ? v1 : v0, other = p ? v0 : v1;
            const int up = p ? nb : other, left = p ? other : nb;
            int v = INT_MIN;
            uint32_t code = 0;
            if (i >= 1 && j >= 1) {
                const bool eq = As[i - 1] == Bs[j - 1];
                v = eq ? own + 1 : own - mismatch;
                code = eq ? 0u : 1u;
            }
            if (i >= 1 && D + 1 < nl) {
                const int c = up - indel;
                if (c > v) {
                    v = c;
                    code = 2u;
                }
            }
            if (j >= 1 && D >= 1) {
                const int c = left - indel;
                if (c > v) {
                    v = c;
                    code = 3u;
                }
            }
            if (p)
                v1 = v;
            else
                v0 = v;
            if (i >= 1) {  // (row 0 is walked left without a trace)
                const uint32_t sh = (i - 1) & 15;
                uint32_t dw = (p ? dw1 : dw0) | code << (2 * sh);
                if (sh == 15 || i == a || j == b) {  // the word is full, or the diagonal ends here
                    tr[(size_t)((i - 1) >> 4) * nl + D] = dw;
                    dw = 0;
                }
                if (p)
                    dw1 = dw;
                else
                    dw0 = dw;
            }
            if (v > bv) {
                bv = v;
                bs = s;
                bi = i;
            }
            ++n;
        }
    }
    for (int m = 32; m > 0; m >>= 1) {  // the largest score, then the smallest i + j, then the smallest i
        const int ov = __shfl_xor(bv, m);
        const uint32_t os = __shfl_xor(bs, m), oi = __shfl_xor(bi, m);
        if (ov > bv || (ov == bv && (os < bs || (os == bs && oi < bi)))) {
            bv = ov;
            bs = os;
            bi = oi;
        }
    }
    *end_i = bi;
    *end_j = bs - bi;
    *score = bv;
    *cells = n;
}

// Dynamic LDS of k_ext_ends: the trace (what the largest end the parameters allow asks for, TRACE_LDS_WORDS at the most),
// max_extend characters of A and max_extend + band of B.  512 / 16: 5.3 KB a wavefront; 4096 / 63: 16.3 KB.
__host__ __device__ inline uint32_t lds_trace_words(uint32_t max_extend, uint32_t band) {
    const uint64_t w = (uint64_t)((max_extend + 15) / 16) * (2 * band + 1);
    return w < TRACE_LDS_WORDS ? (uint32_t)w : TRACE_LDS_WORDS;
}
inline size_t ends_lds_bytes(uint32_t max_extend, uint32_t band) {
    return (size_t)lds_trace_words(max_extend, band) * 4 + ((max_extend + 3) & ~3u) + ((max_extend + band + 4) & ~3u);
}

__global__ __launch_bounds__(64) void k_ext_ends(CigarArgs ca) {
    extern __shared__ uint32_t lds[];  // ends_lds_bytes: the trace, A, B -- sized by the parameters, not by their limits
    uint32_t* trl = lds;
    uint8_t* As = (uint8_t*)(lds + lds_trace_words(ca.max_extend, ca.band));
    uint8_t* Bs = As + ((ca.max_extend + 3) & ~3u);
    const AlignArgs& al = ca.a;
    const uint32_t lane = threadIdx.x;
    const uint32_t nl = 2 * ca.band + 1;
    const uint64_t ebase = ca.poffs[al.cap];
    for (uint64_t e = blockIdx.x; e < 2 * al.nreads; e += gridDim.x) {
        const uint64_t q = e >> 1;
        const uint32_t side = (uint32_t)(e & 1);
        const uint4 w0 = al.out[3 * q];
        uint32_t a = 0, b = 0;
        EndOf eo{};
        if (!is_unaligned(w0)) {
            eo = end_of(ca, q, side, w0, al.out[3 * q + 1]);
            a = eo.a;
            b = eo.b;
        }
        if (a == 0 || b == 0) {  // the end point is (0, 0); the table's other cells are a run of indels within the band
            const uint32_t run = a > b ? a : b;
            if (lane == 0) {
                ca.eres[2 * e] = make_uint4(0, 0, 0, 0);
                ca.eres[2 * e + 1] = make_uint4(0, run < ca.band ? run : ca.band, a, 0);
            }
            continue;
        }
        __syncthreads();  // (the end before is done with the LDS)
        for (uint32_t i = lane; i < a; i += 64) As[i] = eo.A[(long)i * eo.dir];
        for (uint32_t j = lane; j < b; j += 64) Bs[j] = eo.B[(long)j * eo.dir];
        __syncthreads();
        const uint64_t twords = (uint64_t)((a + 15) / 16) * nl;
        const bool global = twords > TRACE_LDS_WORDS;  // (then etrace_stride = the largest an end can ask for: the host's)
        uint32_t* trg = ca.etrace + (size_t)blockIdx.x * ca.etrace_stride;
        uint32_t ei, ej, n;
        int score;
        if (global) {
            end_fill(As, Bs, a, b, ca.band, (int)ca.mismatch, (int)ca.indel, trg, lane, &ei, &ej, &score, &n);
            __threadfence_block();
        } else {
            end_fill(As, Bs, a, b, ca.band, (int)ca.mismatch, (int)ca.indel, trl, lane, &ei, &ej, &score, &n);
        }
        __syncthreads();  // (every lane's trace words are visible to the wavefront)
        unsigned long long cells = wave_sum((unsigned long long)n);
        const uint64_t p0 = ebase + ca.epoffs[e];
        const bool room = p0 + path_words_of(a, b) <= ca.path_cap;  // (else the emit leaves the read unaligned: overflow)
        uint32_t* path = ca.path + p0;
        // the same walk in every lane; `word` is the trace word read last
        uint32_t i = ei, j = ej, kk = 0, acc = 0, edits = 0, cw = 0xffffffffu, word = 0;
        while ((i | j) && kk < a + b) {
            uint32_t code;
            if (i == 0) {
                code = 3u;
            } else if (j == 0) {
                code = 2u;
            } else {
                const uint32_t wi = ((i - 1) >> 4) * nl + (j + ca.band - i);
                if (wi != cw) {
                    cw = wi;
                    word = global ? trg[wi] : trl[wi];
                }
                code = (word >> (2 * ((i - 1) & 15))) & 3u;
            }
            edits += code != 0;
            acc |= code << (2 * (kk & 15));
            if ((kk & 15) == 15) {
                if (room && lane == 0) path[kk >> 4] = acc;
                acc = 0;
            }
            ++kk;
            i -= code != 3u;
            j -= code != 2u;
        }
        if ((kk & 15) && room && lane == 0) path[kk >> 4] = acc;
        if (lane == 0) {
            ca.eres[2 * e] = make_uint4(ei, ej, (uint32_t)score, edits);
            ca.eres[2 * e + 1] = make_uint4(kk, (uint32_t)cells, a, 0);
        }
    }
}

// A lane per read, a block over a stride of reads, behind the reduction: the record takes the ends in.
__global__ __launch_bounds__(256) void k_ext_update(CigarArgs ca) {
    __shared__ unsigned long long part[4][4];
    const AlignArgs& al = ca.a;
    unsigned long long n_ends = 0, n_ext = 0, n_cells = 0, n_clip = 0;
    for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < al.nreads; q += (uint64_t)gridDim.x * 256) {
        uint4 w0 = al.out[3 * q];
        if (is_unaligned(w0)) {
            if (ca.out_ends) ca.out_ends[2 * q] = ca.out_ends[2 * q + 1] = make_uint4(0, 0, 0, 0);
            continue;
        }
        uint4 w1 = al.out[3 * q + 1];
        const uint4 l0 = ca.eres[4 * q], l1 = ca.eres[4 * q + 1], r0 = ca.eres[4 * q + 2], r1 = ca.eres[4 * q + 3];
        const uint64_t ts = ((uint64_t)w0.x | ((uint64_t)w0.y << 32)) - l0.y, te = ((uint64_t)w0.z | ((uint64_t)w0.w << 32)) + r0.y;
        w0 = make_uint4((uint32_t)ts, (uint32_t)(ts >> 32), (uint32_t)te, (uint32_t)(te >> 32));
        w1.x -= l0.x;
        w1.y += r0.x;
        w1.z += (l1.x - l0.w) + (r1.x - r0.w);  // the '=' of a path: its steps but its edits
        w1.w += l0.w + r0.w;
        al.out[3 * q] = w0;
        al.out[3 * q + 1] = w1;
        if (ca.out_ends) {
            ca.out_ends[2 * q] = l0;
            ca.out_ends[2 * q + 1] = r0;
        }
        n_ends += (l1.z != 0) + (r1.z != 0);
        n_ext += ((l0.x | l0.y) != 0) + ((r0.x | r0.y) != 0);
        n_cells += (unsigned long long)l1.y + r1.y;
        n_clip += (unsigned long long)w1.x + (al.roffs[q + 1] - al.roffs[q] - w1.y);
    }
    n_ends = wave_sum(n_ends);
    n_ext = wave_sum(n_ext);
    n_cells = wave_sum(n_cells);
    n_clip = wave_sum(n_clip);
    const uint32_t wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wv][0] = n_ends;
        part[wv][1] = n_ext;
        part[wv][2] = n_cells;
        part[wv][3] = n_clip;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const unsigned long long v = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        unsigned long long* c = threadIdx.x == 0 ? &ca.c->ends : threadIdx.x == 1 ? &ca.c->extended : threadIdx.x == 2 ? &ca.c->band_cells : &ca.c->clipped;
        if (v) atomicAdd(c, v);
    }
}

int hook_plan(CigarArgs& ca, const CigarPlan& plan, hipStream_t st) {
    size_t cub_bytes = plan.cub_bytes;
    k_ext_sizes<<<(unsigned)std::min<uint64_t>((ca.a.nreads + 1 + 255) / 256, 1024), 256, 0, st>>>(ca);
    SPX_HIP(hipGetLastError());
    SPX_HIP(hipcub::DeviceScan::ExclusiveSum(plan.cub, cub_bytes, ca.epw, ca.epoffs, 2 * ca.a.nreads + 1, st));
    return SPX_OK;
}
int hook_fill(CigarArgs& ca, const CigarPlan& plan, hipStream_t st) {
    k_ext_ends<<<plan.grid_ends, 64, ends_lds_bytes(ca.max_extend, ca.band), st>>>(ca);
    SPX_HIP(hipGetLastError());
    return SPX_OK;
}
int hook_finish(CigarArgs& ca, hipStream_t st) {
    k_ext_update<<<(unsigned)std::min<uint64_t>((ca.a.nreads + 255) / 256, 1024), 256, 0, st>>>(ca);
    SPX_HIP(hipGetLastError());
    return SPX_OK;
}
const EndHooks HOOKS{hook_plan, hook_fill, hook_finish};

TraceView extend_view(spx_index* ix) {
    return TraceView{ix->extend_scr, &ix->extend, &ix->extend_ready, &HOOKS, "the extended CIGARs", "spe_extend_begin", "spe_extend_fetch"};
}

int check_extend_params(const spe_params* p, EndParams* ep) {
    if (!p) {
        set_error("extend params must be non-null");
        return SPX_E_ARG;
    }
    if (p->max_extend < 1 || p->max_extend > EXTEND_LIMIT) {
        set_error("max_extend must be 1 .. 4096");
        return SPX_E_ARG;
    }
    if (p->band > BAND_LIMIT) {
        set_error("band must be 0 .. 63");
        return SPX_E_ARG;
    }
    if (p->mismatch > 65535 || p->indel > 65535) {
        set_error("mismatch and indel must be 0 .. 65535");
        return SPX_E_ARG;
    }
    ep->max_extend = p->max_extend;
    ep->band = p->band;
    ep->mismatch = p->mismatch;
    ep->indel = p->indel;
    return SPX_OK;
}

}  // namespace

void release_extend(spx_index* ix) { release(ix->extend_scr, spx_index::TB_COUNT, &ix->extend); }

}  // namespace spx

using namespace spx;

extern "C" {

int spe_extend_device(spx_index* ix, const uint8_t* d_reads, const uint64_t* d_read_offsets, const spm_match* d_matches,
                      const uint64_t* d_match_offsets, uint64_t nreads, const spc_chain* d_chains, const uint32_t* d_pred,
                      const spa_params* params, const spe_params* extend_params, uint64_t gap_capacity, uint64_t op_capacity,
                      spa_alignment* d_out, uint64_t* d_out_op_offsets, uint32_t* d_out_ops, spe_end* d_out_ends, void* stream) {
    int rc = check_align_params(ix, params);
    if (rc != SPX_OK) return rc;
    EndParams ep;
    if ((rc = check_extend_params(extend_params, &ep)) != SPX_OK) return rc;
    return trace_device(ix, extend_view(ix), d_reads, d_read_offsets, d_matches, d_match_offsets, nreads, d_chains, d_pred, params, ep,
                        gap_capacity, op_capacity, d_out, d_out_op_offsets, d_out_ops, d_out_ends, stream);
}

int spe_last_extend_stats(spx_index* ix, spe_extend_stats* out) {
    if (!ix || !out) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    if (!ix->extend.have) {
        set_error("no extended CIGARs have been computed on this index yet");
        return SPX_E_ARG;
    }
    const spx_index::Product& p = ix->extend;
    if (p.pending) {
        const int rc = product_collect(ix, ix->extend, CIGAR_WORDS, CIGAR_WORDS, CW_ERROR);
        if (rc != SPX_OK) return rc;
    }
    out->reads = p.acc[0];
    out->aligned_reads = p.acc[1];
    out->gaps = p.acc[2];
    out->filled_gaps = p.acc[3];
    out->cells = p.acc[4];
    out->entries = p.acc[CW_ENTRIES];
    out->path_words = p.acc[CW_PATH_WORDS];
    out->ends = p.acc[CW_ENDS];
    out->extended_ends = p.acc[CW_EXTENDED];
    out->band_cells = p.acc[CW_BAND_CELLS];
    out->clipped = p.acc[CW_CLIPPED];
    out->error = (uint32_t)(p.error & 1);
    out->overflow = (uint32_t)((p.error >> 1) & 1);
    out->kernel_ms = p.ms;
    for (int i = 0; i < 6; ++i) out->step_ms[i] = p.step_ms[i];
    out->reserved = 0;
    return cigar_error_code(extend_view(ix));
}

int spe_extend_begin(spx_index* ix, int digest_kind, uint32_t k, uint32_t w, const uint8_t* seqs, const uint64_t* offsets,
                     uint64_t nreads, uint64_t min_length, int want_docs, const spc_params* chain_params,
                     const spa_params* align_params, const spe_params* extend_params, spa_alignment* out_alignments,
                     spc_chain* out_chains, uint64_t* out_values, spe_end* out_ends, uint64_t* n_entries) {
    if (spx_device_count() <= 0) {
        set_error("no HIP device visible: the extended CIGARs are computed on the GPU and there is no CPU fallback");
        return SPX_E_NODEVICE;
    }
    int rc = check_align_params(ix, align_params);
    if (rc != SPX_OK) return rc;
    EndParams ep;
    if ((rc = check_extend_params(extend_params, &ep)) != SPX_OK) return rc;
    return trace_begin(ix, extend_view(ix), digest_kind, k, w, seqs, offsets, nreads, min_length, want_docs, chain_params, align_params,
                       ep, out_alignments, out_chains, out_values, out_ends, n_entries);
}

int spe_extend_fetch(spx_index* ix, uint64_t* out_op_offsets, uint32_t* out_ops) {
    if (!ix) {
        set_error("index must be non-null");
        return SPX_E_ARG;
    }
    return trace_fetch(ix, extend_view(ix), out_op_offsets, out_ops);
}

}  // extern "C"
