/*
 * spumoni_cigar.h -- C-ABI of the CIGARs in libspumoni_gpu.so (gfx950): for every read, the alignment of
 * spumoni_align.h -- the same 48-byte record with the same values -- and beside it the PATH of that alignment as a list
 * of operations: where the matches, substitutions, insertions and deletions are.  The tables of spumoni_align.h are
 * filled once more with the way each cell came from remembered, and walked back on the device.
 *
 * The rule (ours; spumoni_amd/cigar.py: cigar_reference is the specification, and the tests hold the kernels to it bit
 * for bit).  Anchors, pred, links, keep, t, the gaps A (a read characters) and B (b text characters), max_fill and
 * "filled" are exactly those of spumoni_align.h.  A read's operations are the concatenation, in chain order, of
 *   1. l_first x '=' for the chain's first anchor;
 *   2. for every link: the operations of its gap, then keep x '='.
 * The operations of a gap:
 *   - a = 0: b x 'D'.  b = 0: a x 'I'.  Both 0: nothing.
 *   - not filled: a x 'I', then b x 'N'.
 *   - filled, a and b >= 1: W[i][j] is the one word per cell of the align tables, edits << 16 | (0xFFFF - matches), with
 *     W[i][0] = i << 16 | 0xFFFF and W[0][j] = j << 16 | 0xFFFF.  dir[i][j] is the FIRST, in the order diagonal, up,
 *     left, of the three candidates whose value equals W[i][j]: diagonal = W[i-1][j-1] - 1 when A[i-1] == B[j-1] and
 *     W[i-1][j-1] + (1 << 16) otherwise, up = W[i-1][j] + (1 << 16), left = W[i][j-1] + (1 << 16).  Start at (a, b)
 *     and follow dir to (0, 0); along row 0 go left, along column 0 go up.  A diagonal step is '=' on equal characters
 *     and 'X' otherwise, an up step consumes a read character and is 'I', a left step consumes a text character and is
 *     'D'.  The gap's operations are those steps read from (0, 0) to (a, b).  The fixed order makes the path unique; it
 *     is the only tie rule.  (1 x 1 needs no table: '=' or 'X'.)
 * Adjacent equal operations are merged over the whole read, across the borders of anchors and gaps too.  One ENTRY is
 * a uint32_t, length << 4 | op, with the BAM codes below; a merged run longer than SPG_MAX_LENGTH is written as
 * consecutive entries, all full but the last.  A read without a chain has no entries.
 * What follows from the rule, over a read's entries: the sum of '=' is `matches`; 'X' + 'I' + 'D' is `edits` plus the
 * 'I' of its unfilled gaps; 'N' plus the 'I' of the unfilled gaps is the a + b of those gaps; the read characters
 * consumed ('=', 'X', 'I') are read_end - read_start and the text characters consumed ('=', 'X', 'D', 'N') are
 * ref_end - ref_start.
 *
 * Conventions: those of spumoni_gpu.h (0 or a negative SPX_E* code, message in spx_last_error(), NO CPU fallback).
 */
#ifndef SPUMONI_CIGAR_H
#define SPUMONI_CIGAR_H

#include <stdint.h>

#include "spumoni_align.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPG_OP_I 1u /* a read character without a text character */
#define SPG_OP_D 2u /* a text character without a read character */
#define SPG_OP_N 3u /* text characters skipped: the text side of a gap that is not filled */
#define SPG_OP_EQ 7u /* equal characters */
#define SPG_OP_X 8u  /* unequal characters */
#define SPG_MAX_LENGTH 0x0FFFFFFFu /* 2^28 - 1: the longest run one entry holds */

/* of the most recent spg_* call on an index: what spa_align_stats reports (a read that came back unaligned for want of
 * capacity counts in none of them), the entries of the aligned reads, error (non-zero: a read failed the walk's checks;
 * the call then returns SPX_E_FORMAT), overflow (non-zero: a read's gaps did not fit gap_capacity, its entries did not
 * fit op_capacity or its path did not fit the path scratch), the words of path scratch (16 steps each) the call's gaps
 * asked for, the HIP-event time of the cigar kernels alone and of their five steps -- plan (count, scan, walk over
 * pred, path sizes), the tracing fill of the gaps a lane takes, the tracing fill and walk back of the gaps a wavefront
 * takes, emit (count, scan, write), reduce -- and, summed over the wavefronts of the third step, the ticks of the
 * constant 100 MHz clock spent filling and spent walking back. */
typedef struct spg_cigar_stats {
    uint64_t reads;
    uint64_t aligned_reads;
    uint64_t gaps;
    uint64_t filled_gaps;
    uint64_t cells;
    uint64_t entries;
    uint64_t path_words;
    uint64_t wave_fill_ticks;
    uint64_t wave_back_ticks;
    uint32_t error;
    uint32_t overflow;
    float kernel_ms;
    float step_ms[5];
} spg_cigar_stats;

/* Device form, asynchronous on `stream` (a hipStream_t as void*, NULL = default stream), no host wait inside; composes
 * behind spc_chain_device on the same stream.  The inputs, gap_capacity and their alignment are spa_align_device's.
 * d_out gets one record per read, d_out_op_offsets (nreads + 1 entries) the exclusive sum of the reads' entry counts,
 * and read q's entries stand from d_out_ops[d_out_op_offsets[q]] on.  op_capacity bounds d_out_ops (at most 2^32 - 1):
 * entries of rank >= op_capacity are not written, a read whose entries do not all fit writes none, comes back unaligned
 * (its count stays in the offsets, so that a second call can be sized from d_out_op_offsets[nreads]) and the stats
 * report the overflow, as with gap_capacity.  The path scratch is the index's and is sized before the first kernel from
 * what the host knows: min(gap_capacity * ceil(max_fill / 8), 2^28) words; a read whose paths end beyond it comes back
 * unaligned and counts in overflow likewise (2^28 words are 2^32 steps: more than one piece of reads can ask for within
 * the limits of spg_cigar_begin).
 * Every input is untrusted exactly as in spa_align_device: the same five bad inputs leave the read unaligned and
 * spg_last_cigar_stats returns SPX_E_FORMAT; no access leaves a buffer that the offsets describe.  d_out_ops and
 * d_pred must be 4-byte aligned.  The same input gives the same bytes. */
int spg_cigar_device(spx_index *ix, const uint8_t *d_reads, const uint64_t *d_read_offsets, const spm_match *d_matches,
                     const uint64_t *d_match_offsets, uint64_t nreads, const spc_chain *d_chains,
                     const uint32_t *d_pred, const spa_params *params, uint64_t gap_capacity, uint64_t op_capacity,
                     spa_alignment *d_out, uint64_t *d_out_op_offsets, uint32_t *d_out_ops, void *stream);
/* Host pair, shaped like spm_mems_begin / spm_mems_fetch because the size of the answer is not known beforehand.
 * _begin takes spa_align_batch's arguments, runs the whole pipeline, fills out_alignments (and out_chains, out_values:
 * may be NULL) and returns the number of entries in *n_entries.  It waits on the host once more than spa_align_batch:
 * behind the walk over pred, for the words of path the gaps need and an upper bound of the entries, so that both
 * scratch buffers have their size before the fills are enqueued; no read overflows.  The entries wait in the handle for
 * _fetch, the next call on the index from the same thread: out_op_offsets gets nreads + 1 offsets, out_ops n_entries
 * entries.  One piece per call: at most 32 Mi characters and 4 Mi reads (SPX_E_ARG beyond). */
int spg_cigar_begin(spx_index *ix, int digest_kind, uint32_t k, uint32_t w, const uint8_t *seqs,
                    const uint64_t *offsets, uint64_t nreads, uint64_t min_length, int want_docs,
                    const spc_params *chain_params, const spa_params *align_params, spa_alignment *out_alignments,
                    spc_chain *out_chains, uint64_t *out_values, uint64_t *n_entries);
int spg_cigar_fetch(spx_index *ix, uint64_t *out_op_offsets, uint32_t *out_ops);
/* Statistics of the most recent spg_* call on ix (synchronises with it). */
int spg_last_cigar_stats(spx_index *ix, spg_cigar_stats *out);

#ifdef __cplusplus
}
#endif

#endif /* SPUMONI_CIGAR_H */
