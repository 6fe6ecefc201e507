// spx_cigar.hip -- the CIGARs (include/spumoni_cigar.h): the alignments of spx_align.hip with their path.
// The count over the chain records, the walk back over pred and the reduction are spx_align.hip's own kernels
// (spx_align_kernels.h); between them the tables are filled once more with the way each cell came from remembered, walked
// back, and the steps handed out as merged runs.  The kernels and the host code that drives them stand in
// spx_cigar_kernels.h, which spx_extend.hip includes too; this file is the product's C-ABI over them.
//
// Two phases on one stream; the device form enqueues both at once, the host form waits between them to size its scratch:
//   plan     count, scan and the walk over pred as in align; then a lane per gap: the words of path the gap needs --
//            a + b steps of four kinds at most, two bits each, 16 a word --, an upper bound of its entries, and a device
//            scan that places every gap's path;
//   small    a lane per gap, as align's: no table for a gap that is not filled, an empty side or 1 x 1; sides up to 16
//            are one lane's table, and the row's 16 directions one word in a column of LDS that the lane owns (a row
//            index that is not a constant would send a register array to scratch memory); the lane walks back at once
//            and writes its path words.  The others go to two lists, one from either end of one buffer;
//   wave     a wavefront per listed gap marching anti-diagonals as align's.  Each lane packs the directions of 16
//            consecutive columns of its row into one word and stores it to the wavefront's trace buffer: in LDS when
//            a * ceil(b / 16) words fit TRACE_LDS_WORDS (the first list), else in a buffer of max_fill * ceil(max_fill /
//            16) words that the wavefront owns for every gap of its grid-stride loop (the second list; the grid shrinks
//            as max_fill grows so that the buffers stay within TRACE_BUDGET).  The same wavefront then walks the gap
//            back, all lanes in step: 64 rows' words of one column of words are fetched at once, a lane a row, and read
//            through a shuffle until the path leaves them -- a dependent load per 64 rows or 16 columns, not per row;
//   emit     a lane per read goes over its anchors and gaps twice, decoding the path bits: the first pass counts the
//            merged entries, a device scan gives op_offsets, the second pass writes.  A read whose entries do not fit
//            comes back unaligned here, before the reduction counts it;
//   reduce   as in align.
// A step is two bits: 0 '=', 1 'X', 2 'I' (up), 3 'D' (left) -- the direction and, for a diagonal, whether the characters
// were equal, so that the walk back reads no character.  A gap's path is stored in the order of the walk back, from
// (a, b) to (0, 0): edits + matches steps, and the emit reads it from its end.
//
// Control flow: every loop that holds a shuffle, a ballot or a barrier has a trip count that depends on the wavefront alone
// (the walk back is the same walk in every lane).
#include "spx_cigar_kernels.h"

namespace spx {
namespace {

TraceView cigar_view(spx_index* ix) {
    return TraceView{ix->cigar_scr, &ix->cigar, &ix->cigar_ready, nullptr, "the CIGARs", "spg_cigar_begin", "spg_cigar_fetch"};
}

}  // namespace

void release_cigar(spx_index* ix) { release(ix->cigar_scr, spx_index::TB_COUNT, &ix->cigar); }

}  // namespace spx

using namespace spx;

extern "C" {

int spg_cigar_device(spx_index* ix, const uint8_t* d_reads, const uint64_t* d_read_offsets, const spm_match* d_matches,
                     const uint64_t* d_match_offsets, uint64_t nreads, const spc_chain* d_chains, const uint32_t* d_pred,
                     const spa_params* params, uint64_t gap_capacity, uint64_t op_capacity, spa_alignment* d_out,
                     uint64_t* d_out_op_offsets, uint32_t* d_out_ops, void* stream) {
    const int rc = check_align_params(ix, params);
    if (rc != SPX_OK) return rc;
    return trace_device(ix, cigar_view(ix), d_reads, d_read_offsets, d_matches, d_match_offsets, nreads, d_chains, d_pred, params,
                        EndParams{}, gap_capacity, op_capacity, d_out, d_out_op_offsets, d_out_ops, nullptr, stream);
}

int spg_last_cigar_stats(spx_index* ix, spg_cigar_stats* out) {
    if (!ix || !out) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    if (!ix->cigar.have) {
        set_error("no CIGARs have been computed on this index yet");
        return SPX_E_ARG;
    }
    const spx_index::Product& p = ix->cigar;
    if (p.pending) {
        const int rc = product_collect(ix, ix->cigar, CIGAR_WORDS, CIGAR_WORDS, CW_ERROR);
        if (rc != SPX_OK) return rc;
    }
    out->reads = p.acc[0];
    out->aligned_reads = p.acc[1];
    out->gaps = p.acc[2];
    out->filled_gaps = p.acc[3];
    out->cells = p.acc[4];
    out->entries = p.acc[CW_ENTRIES];
    out->path_words = p.acc[CW_PATH_WORDS];
    out->wave_fill_ticks = p.acc[CW_FILL_TICKS];
    out->wave_back_ticks = p.acc[CW_BACK_TICKS];
    out->error = (uint32_t)(p.error & 1);
    out->overflow = (uint32_t)((p.error >> 1) & 1);
    out->kernel_ms = p.ms;
    for (int i = 0; i < 5; ++i) out->step_ms[i] = p.step_ms[i];
    return cigar_error_code(cigar_view(ix));
}

int spg_cigar_begin(spx_index* ix, int digest_kind, uint32_t k, uint32_t w, const uint8_t* seqs, const uint64_t* offsets,
                    uint64_t nreads, uint64_t min_length, int want_docs, const spc_params* chain_params,
                    const spa_params* align_params, spa_alignment* out_alignments, spc_chain* out_chains, uint64_t* out_values,
                    uint64_t* n_entries) {
    if (spx_device_count() <= 0) {
        set_error("no HIP device visible: the CIGARs are computed on the GPU and there is no CPU fallback");
        return SPX_E_NODEVICE;
    }
    const int rc = check_align_params(ix, align_params);
    if (rc != SPX_OK) return rc;
    return trace_begin(ix, cigar_view(ix), digest_kind, k, w, seqs, offsets, nreads, min_length, want_docs, chain_params, align_params,
                       EndParams{}, out_alignments, out_chains, out_values, nullptr, n_entries);
}

int spg_cigar_fetch(spx_index* ix, uint64_t* out_op_offsets, uint32_t* out_ops) {
    if (!ix) {
        set_error("index must be non-null");
        return SPX_E_ARG;
    }
    return trace_fetch(ix, cigar_view(ix), out_op_offsets, out_ops);
}

}  // extern "C"
