/*
 * spumoni_align.h -- C-ABI of the alignments in libspumoni_gpu.so (gfx950): for every read, its best chain
 * (spumoni_chain.h) turned into a chain-constrained global alignment -- every gap between two consecutive anchors of
 * the chain filled by an exact edit-distance dynamic programme on the device -- as one 48-byte record: edits, matches
 * and spans.  No CIGAR, no traceback: the numbers below are unique without one.
 *
 * The rule (ours; spumoni_amd/align.py: align_reference is the specification, and the tests hold the kernels to it bit
 * for bit).  A read's anchors, pred and its chain record (first, last, anchors) are those of spumoni_chain.h.  R is the
 * read's characters as the walk saw them (the digested read under digestion), T the text the index holds; characters
 * are compared as plain bytes.
 *   - LINKS.  Walk pred from `last` back to `first`.  For every link j -> i of the chain, with ex and ey as in
 *     spumoni_chain.h: keep = min(l_i, ex, ey) and t = l_i - keep: the head of anchor i that overlaps j in the read or
 *     in the text is cut off (an eligible link has keep >= 1).  The GAP of the link is A = R[x_j + l_j, x_i + t) with
 *     a = |A| = ex - keep and B = T[y_j + l_j, y_i + t) with b = |B| = ey - keep: both are >= 0, and one of them is 0
 *     whenever the anchors overlap.
 *   - FILLING.  A gap is FILLED when a <= max_fill and b <= max_fill.  Its result is the pair (edits, matches): edits is
 *     the Levenshtein distance of A and B (substitution, insertion and deletion cost 1 each), matches the largest
 *     number of columns of equal characters among the alignments of that cost.  Both add up along an alignment, so the
 *     pair is a lexicographic optimum and unique: no tie rule, no traceback.  a = 0 or b = 0 gives (max(a, b), 0).  A gap
 *     that is not filled has edits = SPA_UNFILLED and matches = 0.
 *   - THE RECORD.  Spans, anchors and doc are the chain record's.  matches = l_first + the sum of keep over the links
 *     + the sum of the gap matches over the filled gaps; edits = the sum of the gap edits over the filled gaps;
 *     unfilled = the number of gaps not filled; skipped = the sum of max(a, b) over those, saturating at 2^32 - 1.
 *     A chain of one anchor: matches = l, edits = 0.  A read without a chain: ref_start = SPA_UNALIGNED,
 *     doc = SPC_NO_DOC, zeros elsewhere.
 *
 * Conventions: those of spumoni_gpu.h (0 or a negative SPX_E* code, message in spx_last_error(), NO CPU fallback).
 */
#ifndef SPUMONI_ALIGN_H
#define SPUMONI_ALIGN_H

#include <stdint.h>

#include "spumoni_chain.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPA_UNALIGNED UINT64_MAX /* spa_alignment::ref_start of a read without a chain */
#define SPA_UNFILLED 0xFFFFFFFFu /* spa_gap::edits of a gap larger than max_fill */

/* Any value out of range: SPX_E_ARG. */
typedef struct spa_params {
    uint32_t max_fill; /* 1 .. 4096: the largest gap side that is filled (default 512) */
} spa_params;

typedef struct spa_alignment { /* 48 bytes */
    uint64_t ref_start;        /* from the chain record */
    uint64_t ref_end;          /* from the chain record */
    uint32_t read_start;       /* from the chain record */
    uint32_t read_end;         /* from the chain record */
    uint32_t matches;          /* l_first + sum of keep + sum of the filled gaps' matches */
    uint32_t edits;            /* sum of the filled gaps' edits */
    uint32_t anchors;          /* from the chain record */
    uint32_t unfilled;         /* gaps larger than max_fill */
    uint32_t skipped;          /* sum of max(a, b) over those, saturating at 2^32 - 1 */
    uint32_t doc;              /* from the chain record */
} spa_alignment;

typedef struct spa_gap { /* 16 bytes: one link of a chain */
    uint32_t a;          /* read characters between the two anchors */
    uint32_t b;          /* text characters between them */
    uint32_t edits;      /* SPA_UNFILLED: not filled */
    uint32_t matches;
} spa_gap;

/* of the most recent spa_* call on an index: the reads it looked at and those that came back aligned, the gaps of the
 * aligned reads and how many of them were filled, the table cells evaluated (a * b of every filled gap with a, b >= 1
 * that is not 1 x 1), error (non-zero: a read failed the walk's checks; the call then returns SPX_E_FORMAT), overflow
 * (non-zero: a read's gaps did not fit gap_capacity), the HIP-event time of the align kernels alone and of their four
 * steps: count and scan, walk, fill, reduce. */
typedef struct spa_align_stats {
    uint64_t reads;
    uint64_t aligned_reads;
    uint64_t gaps;
    uint64_t filled_gaps;
    uint64_t cells;
    uint32_t error;
    uint32_t overflow;
    float kernel_ms;
    float step_ms[4];
} spa_align_stats;

/* Device form, asynchronous on `stream` (a hipStream_t as void*, NULL = default stream); composes behind
 * spc_chain_device on the same stream.  Read q's characters are d_reads[d_read_offsets[q] .. d_read_offsets[q + 1]),
 * its anchors d_matches[d_match_offsets[q] .. d_match_offsets[q + 1]) with d_pred at the same indices (what
 * spc_chain_device wrote to d_out_pred) and its chain d_chains[q].  The index must hold the text.  d_out gets one
 * record per read.  The per-gap table, on request: d_out_gap_offsets (nreads + 1 entries, may be NULL) is the
 * exclusive sum of max(anchors - 1, 0), and read q's gaps stand in chain order from d_out_gaps[d_out_gap_offsets[q]]
 * on (may be NULL: the table then lives in the index's scratch).  gap_capacity bounds the table either way (at most
 * 2^32 - 1; the number of matches always suffices): gaps of rank >= gap_capacity are not written, a read whose gaps do
 * not all fit comes back unaligned, and the stats report the overflow.
 * Every input is untrusted: a read whose pred does not decrease strictly, leaves [first, last], takes more or fewer
 * than `anchors` steps to `first`, whose links have keep < 1 (a gap of negative length), whose chain anchors leave the
 * read, or whose gap leaves the text comes back unaligned and spa_last_align_stats returns SPX_E_FORMAT; no access
 * leaves a buffer that the offsets describe.  d_matches, d_chains, d_out and d_out_gaps must be 16-byte aligned, the
 * 64-bit arrays 8-byte, d_pred 4-byte.  The same input gives the same bytes. */
int spa_align_device(spx_index *ix, const uint8_t *d_reads, const uint64_t *d_read_offsets, const spm_match *d_matches,
                     const uint64_t *d_match_offsets, uint64_t nreads, const spc_chain *d_chains,
                     const uint32_t *d_pred, const spa_params *params, uint64_t gap_capacity, spa_alignment *d_out,
                     uint64_t *d_out_gap_offsets, spa_gap *d_out_gaps, void *stream);
/* Host form: reads in (upper-cased, concatenated at offsets[0 .. nreads]), one record per read out.  digest_kind, k,
 * w, min_length, want_docs and chain_params as in spc_chain_batch, whose steps it takes with pred kept on the device
 * and the align kernels behind the chain kernel on the same stream; out_chains (the chain records) and out_values
 * (the values per read after digestion) may be NULL.  One piece per call: at most 32 Mi characters and 4 Mi reads
 * (SPX_E_ARG beyond). */
int spa_align_batch(spx_index *ix, int digest_kind, uint32_t k, uint32_t w, const uint8_t *seqs,
                    const uint64_t *offsets, uint64_t nreads, uint64_t min_length, int want_docs,
                    const spc_params *chain_params, const spa_params *align_params, spa_alignment *out_alignments,
                    spc_chain *out_chains, uint64_t *out_values);
/* Statistics of the most recent spa_* call on ix (synchronises with it). */
int spa_last_align_stats(spx_index *ix, spa_align_stats *out);

#ifdef __cplusplus
}
#endif

#endif /* SPUMONI_ALIGN_H */
