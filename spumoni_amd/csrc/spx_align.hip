// spx_align.hip -- the alignments (include/spumoni_align.h): per read, its best chain (spx_chain.hip)
// turned into a chain-constrained global alignment -- every gap between two consecutive anchors filled by an exact
// edit-distance dynamic programme -- as one 48-byte record, and on request the per-gap table.
//
// Four steps on one stream, nothing returns to the host between them:
//   count    a lane per read: max(anchors - 1, 0) of a chain that passes the checks on its record, and a device scan
//            gives gap_offsets;
//   walk     a lane per read follows pred from `last` back to `first`: a serial pointer chase (the chain kernel keeps no
//            list of a chain's anchors).  Every link is checked -- the inputs are untrusted --, its gap (a, b and where A
//            and B start) goes to its final place gap_offsets[q] + anchors - 2 - step, so the order of the table is a
//            function of the input, and l_first + the sum of keep is the record's first version;
//   fill     the unit of work is the GAP, not the read.  k_fill_small gives every gap a lane: a gap that is not filled, an
//            empty side and 1 x 1 need no table; sides up to 16 are one lane's table, a row of 17 cells in registers; the
//            others go to a list (one atomic per wavefront), and k_fill_wave gives each of those a wavefront: strips of 64
//            rows, a lane per row, marching the anti-diagonals.  The neighbour above comes by __shfl_up (an exchange through
//            LDS would cost a write, a barrier and a read a step), the row above a strip and B stand in LDS;
//   reduce   a lane per read adds its gaps to the record.  Integer sums: the same input gives the same bytes.
// A cell is ONE uint32_t: edits << 16 | (0xFFFF - matches).  edits <= a + b <= 8192 < 2^16 and matches <= min(a, b) <=
// 4096 < 0xFFFF, so neither field carries into the other; unsigned order on the word is the lexicographic order (fewer
// edits, then more matches), adding 1 << 16 is an edit and subtracting 1 a match: the optimum is one unsigned min of three.
//
// Control flow: every loop that holds a shuffle, a ballot or a barrier has a trip count that depends on the wavefront alone.
//
// The arguments, the counters and the kernels of count, walk and reduce stand in spx_align_kernels.h, which spx_cigar.hip
// includes too; the fills below are this file's own.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <vector>

#include "spx_align_kernels.h"

namespace spx {
namespace {

// One lane's table: sides 1 .. 16, a row of 17 cells in registers (every index below is a constant after unrolling).
__device__ inline uint32_t fill_lane(const uint8_t* A, const uint8_t* B, uint32_t a, uint32_t b) {
    uint32_t row[LANE_MAX + 1];
    uint8_t bc[LANE_MAX];
#pragma unroll
    for (uint32_t j = 0; j < LANE_MAX; ++j) bc[j] = j < b ? B[j] : 0;
#pragma unroll
    for (uint32_t j = 0; j <= LANE_MAX; ++j) row[j] = j * EDIT | 0xffffu;
    for (uint32_t i = 1; i <= a; ++i) {
        const uint8_t ac = A[i - 1];
        uint32_t diag = row[0], left = i * EDIT | 0xffffu;
        row[0] = left;
#pragma unroll
        for (uint32_t j = 1; j <= LANE_MAX; ++j) {
            const uint32_t up = row[j];
            uint32_t v = (up < left ? up : left) + EDIT;
            const uint32_t d = ac == bc[j - 1] ? diag - 1 : diag + EDIT;
            v = d < v ? d : v;
            diag = up;
            left = v;
            row[j] = v;  // (columns past b hold values nothing reads: a column depends on those to its left alone)
        }
    }
    uint32_t r = row[1];
#pragma unroll
    for (uint32_t j = 2; j <= LANE_MAX; ++j) r = j == b ? row[j] : r;
    return r;
}

__global__ __launch_bounds__(256) void k_fill_small(AlignArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t total = a.goffs[a.nreads] < a.cap ? a.goffs[a.nreads] : a.cap;
    bool big = false;
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
                const uint32_t v = fill_lane(A, B, ga, gb);
                edits = v >> 16;
                matches = 0xffffu - (v & 0xffffu);
            } else {
                big = true;
                edits = 0;
            }
        }
        if (!big) a.gaps[g] = make_uint4(ga, gb, edits, matches);
    }
    // the gaps that need a wavefront: one atomic per wavefront, and the list's order does not matter -- a gap's result
    // goes to the gap's own place
    const unsigned long long mask = __ballot(big);
    if (mask) {
        const int leader = __ffsll(mask) - 1;
        unsigned long long at = 0;
        if ((int)lane == leader) at = atomicAdd(&a.c->nbig, (unsigned long long)__popcll(mask));
        at = __shfl(at, leader);
        if (big) a.list[at + __popcll(mask & ((1ull << lane) - 1))] = (uint32_t)g;  // (nbig <= total <= cap)
    }
}

// A wavefront per listed gap: strips of 64 rows of the table (row i belongs to character A[i - 1]), lane r of a strip
// holds row 64 s + r + 1 and, at step d, column d - r + 1: an anti-diagonal a step.  What a cell needs: its left
// neighbour is the lane's own last value, the one above is the last value of the lane with the row above (a shuffle up
// by one), the diagonal one what that shuffle brought a step earlier.  The first row of a strip reads the row
// above it from `bound`, where the last row of the strip before wrote it (behind the reader: column d - 63 is written
// when column d + 1 is read), and B stands in LDS beside it.
__global__ __launch_bounds__(64) void k_fill_wave(AlignArgs a) {
    __shared__ uint32_t bound[FILL_LIMIT + 1];
    __shared__ uint8_t Bs[FILL_LIMIT];
    const uint32_t lane = threadIdx.x;
    const unsigned long long nbig = __shfl(a.c->nbig, 0);
    for (unsigned long long k = blockIdx.x; k < nbig; k += gridDim.x) {
        const uint64_t g = a.list[k];
        const uint4 gp = a.gaps[g];
        const uint32_t ga = __shfl(gp.x, 0), gb = __shfl(gp.y, 0);  // (1 .. max_fill <= FILL_LIMIT: k_fill_small listed it)
        const ulonglong2 d = a.desc[g];
        const uint8_t *A = a.R + d.x, *B = a.T + d.y;
        __syncthreads();  // (the gap before is done with the LDS)
        for (uint32_t j = lane; j <= gb; j += 64) bound[j] = j * EDIT | 0xffffu;
        for (uint32_t j = lane; j < gb; j += 64) Bs[j] = B[j];
        __syncthreads();
        const uint32_t nstrips = (ga + 63) / 64;
        for (uint32_t s = 0; s < nstrips; ++s) {
            const uint32_t i = s * 64 + lane + 1;
            const bool row_ok = i <= ga;
            const uint32_t rows = ga - s * 64 < 64 ? ga - s * 64 : 64;
            const uint8_t ac = row_ok ? A[i - 1] : 0;
            uint32_t left = i * EDIT | 0xffffu, diag = (i - 1) * EDIT | 0xffffu, cur = left;
            const uint32_t steps = gb + rows - 1;
            for (uint32_t st = 0; st < steps; ++st) {
                const int32_t j = (int32_t)st - (int32_t)lane + 1;
                const bool act = row_ok && j >= 1 && j <= (int32_t)gb;
                uint32_t up = __shfl_up(cur, 1);
                if (act) {
                    if (lane == 0) up = bound[j];
                    uint32_t v = (up < left ? up : left) + EDIT;
                    const uint32_t dg = ac == Bs[j - 1] ? diag - 1 : diag + EDIT;
                    v = dg < v ? dg : v;
                    diag = up;
                    left = v;
                    cur = v;
                    if (lane == rows - 1) bound[j] = v;
                }
            }
            __syncthreads();
        }
        if (lane == 0) {
            const uint32_t v = bound[gb];
            a.gaps[g] = make_uint4(ga, gb, v >> 16, 0xffffu - (v & 0xffffu));
        }
    }
}

// The scratch of one call, reserved before any of its kernels is enqueued (a buffer that grows is freed first: a
// device-wide wait).  Takes ix->mu.
int align_reserve(spx_index* ix, AlignArgs& a, bool own_goffs, bool own_gaps, size_t* cub_bytes, void** cub) {
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    return reserve_gaps(ix->align_scr, a, own_goffs, own_gaps, 0, cub_bytes, cub);
}

// The align kernels on st, between the index's two events, with a mark where each of the four steps begins (none for a
// batch without reads: its step times are zeros).  Takes ix->mu.
int align_enqueue(spx_index* ix, AlignArgs& a, size_t cub_bytes, void* cub, hipStream_t st) {
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    spx_index::Product& p = ix->align;
    return product_enqueue(p, ALIGN_WORDS, st, [&](void* counters) -> int {
        a.c = (AlignCounters*)counters;
        int rc;
        if (!a.nreads) {
            SPX_HIP(hipMemsetAsync(a.goffs, 0, 8, st));
            return SPX_OK;
        }
        const unsigned read_grid = (unsigned)((a.nreads + 1 + 255) / 256);
        k_align_count<<<read_grid, 256, 0, st>>>(a);
        SPX_HIP(hipGetLastError());
        SPX_HIP(hipcub::DeviceScan::ExclusiveSum(cub, cub_bytes, a.cnt, a.goffs, a.nreads + 1, st));
        if ((rc = product_mark(p, 1, st)) != SPX_OK) return rc;
        k_align_walk<<<read_grid, 256, 0, st>>>(a);
        SPX_HIP(hipGetLastError());
        if ((rc = product_mark(p, 2, st)) != SPX_OK) return rc;
        if (a.cap) {
            // (the number of gaps is the device's: the grid covers the capacity, and lanes past the total leave at once)
            k_fill_small<<<(unsigned)((a.cap + 255) / 256), 256, 0, st>>>(a);
            SPX_HIP(hipGetLastError());
            k_fill_wave<<<(unsigned)std::min<uint64_t>(a.cap, 4096), 64, 0, st>>>(a);
            SPX_HIP(hipGetLastError());
        }
        if ((rc = product_mark(p, 3, st)) != SPX_OK) return rc;
        k_align_reduce<<<std::min(read_grid, 1024u), 256, 0, st>>>(a);
        SPX_HIP(hipGetLastError());
        return SPX_OK;
    }, a.nreads ? 0 : -1);
}
int align_error_code(const spx_index* ix) {
    if (ix->align.error & 1) {
        set_error("a read's chain failed the walk's checks (pred, anchors, first / last, a link of negative length, or a gap "
                  "outside the read or the text): such a read is left unaligned");
        return SPX_E_FORMAT;
    }
    return SPX_OK;
}

}  // namespace

void release_align(spx_index* ix) { release(ix->align_scr, spx_index::L_COUNT, &ix->align); }

}  // namespace spx

using namespace spx;

extern "C" {

int spa_align_device(spx_index* ix, const uint8_t* d_reads, const uint64_t* d_read_offsets, const spm_match* d_matches,
                     const uint64_t* d_match_offsets, uint64_t nreads, const spc_chain* d_chains, const uint32_t* d_pred,
                     const spa_params* params, uint64_t gap_capacity, spa_alignment* d_out, uint64_t* d_out_gap_offsets,
                     spa_gap* d_out_gaps, void* stream) {
    int rc = check_align_params(ix, params);
    if (rc != SPX_OK) return rc;
    if (!ix->text) {
        set_error("the alignments need the text (spx_index_set_text / spx_index_rebuild_text)");
        return SPX_E_ARG;
    }
    if (nreads && (!d_reads || !d_read_offsets || !d_matches || !d_match_offsets || !d_chains || !d_pred || !d_out)) {
        set_error("d_reads, d_read_offsets, d_matches, d_match_offsets, d_chains, d_pred and d_out must be non-null");
        return SPX_E_ARG;
    }
    if (gap_capacity > 0xffffffffull) {
        set_error("gap_capacity must be at most 2^32 - 1");
        return SPX_E_ARG;
    }
    if ((((uintptr_t)d_matches | (uintptr_t)d_chains | (uintptr_t)d_out | (uintptr_t)d_out_gaps) & 15) != 0 ||
        (((uintptr_t)d_read_offsets | (uintptr_t)d_match_offsets | (uintptr_t)d_out_gap_offsets) & 7) != 0 ||
        ((uintptr_t)d_pred & 3) != 0) {
        set_error("d_matches, d_chains, d_out and d_out_gaps must be 16-byte aligned (records are read and written as 16-byte "
                  "vectors), the 64-bit arrays 8-byte and d_pred 4-byte aligned");
        return SPX_E_ARG;
    }
    product_reset(ix, ix->align);
    AlignArgs a{};
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
    a.goffs = d_out_gap_offsets;
    a.gaps = (uint4*)d_out_gaps;
    size_t cub_bytes = 0;
    void* cub = nullptr;
    if ((rc = align_reserve(ix, a, !d_out_gap_offsets, !d_out_gaps, &cub_bytes, &cub)) != SPX_OK) return rc;
    return align_enqueue(ix, a, cub_bytes, cub, (hipStream_t)stream);
}

int spa_last_align_stats(spx_index* ix, spa_align_stats* out) {
    if (!ix || !out) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    if (!ix->align.have) {
        set_error("no alignments have been computed on this index yet");
        return SPX_E_ARG;
    }
    if (ix->align.pending) {
        const int rc = product_collect(ix, ix->align, ALIGN_WORDS, 5);
        if (rc != SPX_OK) return rc;
    }
    out->reads = ix->align.acc[0];
    out->aligned_reads = ix->align.acc[1];
    out->gaps = ix->align.acc[2];
    out->filled_gaps = ix->align.acc[3];
    out->cells = ix->align.acc[4];
    out->error = (uint32_t)(ix->align.error & 1);
    out->overflow = (uint32_t)((ix->align.error >> 1) & 1);
    out->kernel_ms = ix->align.ms;
    for (int i = 0; i < 4; ++i) out->step_ms[i] = ix->align.step_ms[i];
    return align_error_code(ix);
}

// spc_chain_batch's steps (mems_begin_staged, the chain kernel behind k_mems_write) with pred kept in scratch, the reads'
// characters kept where the walk read them, and the align kernels behind the chain kernel on the same stream.
int spa_align_batch(spx_index* ix, int digest_kind, uint32_t k, uint32_t w, const uint8_t* seqs, const uint64_t* offsets,
                    uint64_t nreads, uint64_t min_length, int want_docs, const spc_params* chain_params,
                    const spa_params* align_params, spa_alignment* out_alignments, spc_chain* out_chains, uint64_t* out_values) {
    if (spx_device_count() <= 0) {
        set_error("no HIP device visible: the alignments are computed on the GPU and there is no CPU fallback");
        return SPX_E_NODEVICE;
    }
    int rc = check_align_params(ix, align_params);
    if (rc != SPX_OK) return rc;
    if ((rc = chain_check_params(ix, chain_params)) != SPX_OK) return rc;
    if ((rc = check_batch(ix, "the alignments", BATCH_MIN_LENGTH | BATCH_TEXT | BATCH_ONE_PIECE, min_length, digest_kind, want_docs,
                          nreads && (!seqs || !offsets || !out_alignments) ? "seqs, offsets and out_alignments must be non-null" : nullptr,
                          offsets, nreads)) != SPX_OK)
        return rc;
    std::lock_guard<std::mutex> hg(ix->host_mu);
    SPX_HIP(hipSetDevice(ix->device));
    product_reset(ix, ix->align);
    product_reset(ix, ix->chain);
    if (nreads == 0) {
        ix->align.have = ix->chain.have = true;  // (the stats of an empty batch are zeros)
        return SPX_OK;
    }
    // what is sized by the reads, before anything is enqueued; what is sized by the matches when their number is known
    // (as the records themselves are), before the chain and the align kernels are enqueued
    void *d_chains = nullptr, *d_out = nullptr;
    if ((rc = ix->align_scr[spx_index::L_CHAINS].reserve(nreads * sizeof(spc_chain), &d_chains)) != SPX_OK) return rc;
    if ((rc = ix->align_scr[spx_index::L_OUT].reserve(nreads * sizeof(spa_alignment), &d_out)) != SPX_OK) return rc;
    std::vector<uint64_t> match_offsets(nreads + 1);
    uint64_t n = 0;
    rc = mems_begin_staged(
        ix, digest_kind, k, w, seqs, offsets, nreads, min_length, want_docs, match_offsets.data(), out_values, &n, true,
        [&](const MemsOnDevice& m) -> int {
            void* d_pred = nullptr;
            int r;
            if ((r = ix->align_scr[spx_index::L_PRED].reserve(m.n * 4 + 16, &d_pred)) != SPX_OK) return r;
            AlignArgs a{};
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
            size_t cub_bytes = 0;
            void* cub = nullptr;
            if ((r = align_reserve(ix, a, true, true, &cub_bytes, &cub)) != SPX_OK) return r;
            if ((r = spc_chain_device(ix, (const spm_match*)m.records, m.docs, m.match_offsets, m.nreads, chain_params,
                                      (spc_chain*)d_chains, nullptr, (uint32_t*)d_pred, m.stream)) != SPX_OK)
                return r;
            if ((r = align_enqueue(ix, a, cub_bytes, cub, m.stream)) != SPX_OK) return r;
            SPX_HIP(hipMemcpyAsync(out_alignments, d_out, m.nreads * sizeof(spa_alignment), hipMemcpyDeviceToHost, m.stream));
            if (out_chains)
                SPX_HIP(hipMemcpyAsync(out_chains, d_chains, m.nreads * sizeof(spc_chain), hipMemcpyDeviceToHost, m.stream));
            return SPX_OK;
        });
    if (rc != SPX_OK) return rc;
    spc_chain_stats cs;
    if ((rc = spc_last_chain_stats(ix, &cs)) != SPX_OK) return rc;
    if ((rc = product_collect(ix, ix->align, ALIGN_WORDS, 5)) != SPX_OK) return rc;
    return align_error_code(ix);
}

}  // extern "C"
