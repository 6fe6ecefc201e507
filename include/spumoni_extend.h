/*
 * spumoni_extend.h -- C-ABI of the extended CIGARs in libspumoni_gpu.so (gfx950): for every read, the alignment and
 * the CIGAR of spumoni_cigar.h taken to the read's ends.  Both ends of the chain are extended by a banded dynamic
 * programme whose end point is not known beforehand, the record's spans, matches and edits include the extensions, the
 * CIGAR carries their operations, and what is left of the read on either side appears as 'S': the read-consuming
 * operations of an aligned read add up to the read's length.
 *
 * The rule (ours; spumoni_amd/extend.py: extend_reference is the specification, and the tests hold the kernels to it
 * bit for bit).  Everything of spumoni_align.h and spumoni_cigar.h holds unchanged for the part between the chain's
 * first and last anchor; R, T, the record and the entries are as there.  len is the read's length in the characters
 * the walk saw, n_text the text's length.
 *   - THE RIGHT END of an aligned read: a = min(len - read_end, max_extend) and A = R[read_end, read_end + a);
 *     b = min(n_text - ref_end, a + band) and B = T[ref_end, ref_end + b).
 *   - THE TABLE S[i][j] is defined for 0 <= i <= a, 0 <= j <= b and |j - i| <= band.  S[0][0] = 0.  Every other cell
 *     is the largest of its candidates whose source cell is in the table: diagonal S[i-1][j-1] + 1 when
 *     A[i-1] == B[j-1], else S[i-1][j-1] - mismatch; up S[i-1][j] - indel; left S[i][j-1] - indel.  The cells fit
 *     32 bits signed: the lowest reachable value is above -2^30.
 *   - THE END POINT is the cell of the largest S; among equal cells the one with the smallest i + j, among those the one
 *     with the smallest i.  (0, 0) is a cell, so an extension is taken only when it gains.
 *   - THE PATH is walked back from the end point to (0, 0) by the FIRST, in the order diagonal, up, left, of the
 *     in-table candidates that equals the cell.  A diagonal step is '=' or 'X', an up step 'I', a left step 'D'; the
 *     steps are read from (0, 0) outwards.  These two fixed orders are the only tie rules.
 *   - THE LEFT END is the same table on the reversed strings: a = min(read_start, max_extend),
 *     b = min(ref_start, a + band), A = reverse(R[read_start - a, read_start)), B = reverse(T[ref_start - b, ref_start)).
 *     Its steps, read from the end point back to (0, 0), are the operations in read order.
 *   - THE RECORD is spa_alignment.  read_start and ref_start move down by the left end point's i and j, read_end and
 *     ref_end move up by the right end point's i and j; matches and edits grow by the '=' and by the X + I + D of both
 *     paths; anchors, unfilled, skipped and doc are spumoni_align.h's.
 *   - THE ENTRIES of an aligned read are, in this order: read_start x 'S' (the new value), the left path, the
 *     operations of spumoni_cigar.h, the right path, (len - read_end) x 'S'; merged and split as there over all those
 *     borders.  A read without a chain has ref_start = SPA_UNALIGNED, zeros elsewhere and no entries.
 * What follows from the rule, over an aligned read's entries: '=', 'X', 'I' and 'S' add up to len, and the
 * text-consuming operations to ref_end - ref_start.
 *
 * Limits: an extension compares plain bytes and may cross a sequence boundary, as spumoni_place.h's does; the costs are
 * linear; there is no x-drop, so the whole band is evaluated; one chain per read and one device, as in spumoni_align.h.
 *
 * Conventions: those of spumoni_gpu.h (0 or a negative SPX_E* code, message in spx_last_error(), NO CPU fallback).
 */
#ifndef SPUMONI_EXTEND_H
#define SPUMONI_EXTEND_H

#include <stdint.h>

#include "spumoni_cigar.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPE_OP_S 4u /* read characters outside the alignment (the BAM code of a soft clip) */

/* Any value out of range: SPX_E_ARG.  An equal column scores +1. */
typedef struct spe_params { /* 16 bytes */
    uint32_t max_extend;    /* 1 .. 4096: the largest end side that is extended (default 512) */
    uint32_t band;          /* 0 .. 63: how far the extension may drift off the diagonal (default 16) */
    uint32_t mismatch;      /* 0 .. 65535: cost of an unequal column (default 4) */
    uint32_t indel;         /* 0 .. 65535: cost of an 'I' or a 'D' (default 6) */
} spe_params;

typedef struct spe_end { /* 16 bytes: one end of a read; two per read, left then right */
    uint32_t read_chars; /* the end point's i: read characters the extension took */
    uint32_t text_chars; /* the end point's j: text characters it took */
    int32_t score;       /* S at the end point, >= 0 */
    uint32_t edits;      /* X + I + D of its path */
} spe_end;

/* of the most recent spe_* call on an index: what spg_cigar_stats counts (matches, edits and entries with the ends in
 * them; a read that came back unaligned for want of capacity counts in none), then over the aligned reads the ends
 * looked at (a >= 1), the ends extended (an end point other than (0, 0)), the band cells evaluated (the cells of the
 * tables but (0, 0)) and the read characters clipped; error and overflow as there (the path scratch holds the ends'
 * paths too); the HIP-event time of the kernels alone and of their six steps: spg_cigar_stats' five -- the plan with
 * the ends' sizes in it, the reduce with the records' update in it -- and, last, the ends. */
typedef struct spe_extend_stats {
    uint64_t reads;
    uint64_t aligned_reads;
    uint64_t gaps;
    uint64_t filled_gaps;
    uint64_t cells;
    uint64_t entries;
    uint64_t path_words;
    uint64_t ends;
    uint64_t extended_ends;
    uint64_t band_cells;
    uint64_t clipped;
    uint32_t error;
    uint32_t overflow;
    float kernel_ms;
    float step_ms[6];
    uint32_t reserved;
} spe_extend_stats;

/* Device form, asynchronous on `stream`, no host wait inside; spg_cigar_device's arguments with the extension's
 * parameters and, on request, the ends: d_out_ends (2 * nreads records, 16-byte aligned, may be NULL) gets read q's
 * left end at 2 q and its right end at 2 q + 1, zeros for a read that comes back unaligned.
 * Every input is untrusted exactly as in spg_cigar_device: the same bad inputs, and a chain record whose spans do not
 * lie in the read and in the text in order, leave the read unaligned and spe_last_extend_stats returns SPX_E_FORMAT; no
 * access leaves a buffer that the offsets describe, and no end reads before T[0] or at or beyond T[n_text].
 * op_capacity and gap_capacity behave as there.  The path scratch holds the ends' paths behind the gaps', a + b steps
 * an end at most, and is sized before the first kernel from what the host knows:
 * min(gap_capacity * ceil(max_fill / 8) + 2 * nreads * ceil((2 * max_extend + band) / 16), 2^28) words; a read whose
 * paths end beyond it comes back unaligned, its count stays in the offsets, and overflow is set.  The reservation
 * follows max_extend, not the reads (their lengths are the device's): at the defaults 65 words an end, 520 MB for 10^6
 * reads whatever their length.  A caller whose reads are short should pass a max_extend no larger than its longest read
 * -- the results are the same, a = min(.., max_extend) is then the read's own limit -- and reserves that much less; the
 * host pair needs no such care, it reserves what the plan counted. */
int spe_extend_device(spx_index *ix, const uint8_t *d_reads, const uint64_t *d_read_offsets, const spm_match *d_matches,
                      const uint64_t *d_match_offsets, uint64_t nreads, const spc_chain *d_chains,
                      const uint32_t *d_pred, const spa_params *params, const spe_params *extend_params,
                      uint64_t gap_capacity, uint64_t op_capacity, spa_alignment *d_out, uint64_t *d_out_op_offsets,
                      uint32_t *d_out_ops, spe_end *d_out_ends, void *stream);
/* Host pair: spg_cigar_begin / spg_cigar_fetch with the extension's parameters and the ends (out_ends: 2 * nreads
 * records, may be NULL).  _begin waits on the host exactly where spg_cigar_begin waits -- the ends' sizes need only the
 * chain records and the read offsets, and are part of the plan --; no read overflows.  One piece per call: at most
 * 32 Mi characters and 4 Mi reads (SPX_E_ARG beyond). */
int spe_extend_begin(spx_index *ix, int digest_kind, uint32_t k, uint32_t w, const uint8_t *seqs,
                     const uint64_t *offsets, uint64_t nreads, uint64_t min_length, int want_docs,
                     const spc_params *chain_params, const spa_params *align_params, const spe_params *extend_params,
                     spa_alignment *out_alignments, spc_chain *out_chains, uint64_t *out_values, spe_end *out_ends,
                     uint64_t *n_entries);
int spe_extend_fetch(spx_index *ix, uint64_t *out_op_offsets, uint32_t *out_ops);
/* Statistics of the most recent spe_* call on ix (synchronises with it). */
int spe_last_extend_stats(spx_index *ix, spe_extend_stats *out);

#ifdef __cplusplus
}
#endif

#endif /* SPUMONI_EXTEND_H */
