/*
 * spumoni_chain.h -- C-ABI of the chains in libspumoni_gpu.so (gfx950): for every read, the best collinear chain of
 * its matches (spumoni_mems.h) as one 48-byte record, reduced on the device from the match records the match kernels
 * leave in device memory.
 *
 * The rule (ours; spumoni_amd/chain.py: chain_reference is the specification, and the tests hold the kernel to it bit
 * for bit).  The ANCHORS of a read are its match records in the order spm_mems_device writes them: x = read_pos,
 * y = ref_pos, l = length and, with ids, a document D.  Input contract: x + l < 2^32 and y + l < 2^63 for every
 * anchor, which holds for what the match kernels deliver; outside it the result is undefined, but no access goes out
 * of bounds.
 *   - a candidate predecessor of anchor i is j with i - lookback <= j < i inside the same read.  In signed 64-bit
 *     arithmetic: dx = x_i - x_j, dy = y_i - y_j, ex = dx + l_i - l_j, ey = dy + l_i - l_j (the differences of the
 *     ends), d = |dx - dy|;
 *   - j is ELIGIBLE when dx >= 1, dy >= 1, ex >= 1, ey >= 1, dx <= max_dist, dy <= max_dist, d <= max_gap and, with
 *     ids, D_j == D_i;
 *   - its candidate score is c_j = f[j] + min(l_i, ex, ey) - gap_penalty * d, and f[i] = max(l_i, max c_j);
 *   - pred[i] is none (SPC_NO_PRED) when l_i >= every candidate: the anchor alone wins a tie.  Otherwise it is the
 *     LARGEST j that reaches the maximum, counted from the read's first anchor;
 *   - 1 <= f[i] <= x_i + l_i < 2^32 by induction: scores are uint32_t;
 *   - the best chain ends at the SMALLEST i with the largest f[i]; walking pred from there gives the record.
 * A read without anchors: ref_start = SPC_UNCHAINED, doc = SPC_NO_DOC, zeros elsewhere.
 *
 * Conventions: those of spumoni_gpu.h (0 or a negative SPX_E* code, message in spx_last_error(), NO CPU fallback).
 */
#ifndef SPUMONI_CHAIN_H
#define SPUMONI_CHAIN_H

#include <stdint.h>

#include "spumoni_mems.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPC_UNCHAINED UINT64_MAX  /* spc_chain::ref_start of a read without anchors */
#define SPC_NO_DOC 0xFFFFFFFFu    /* spc_chain::doc without ids, or of a read without anchors */
#define SPC_NO_PRED 0xFFFFFFFFu   /* d_out_pred of an anchor that starts its chain */

/* Any value out of range: SPX_E_ARG. */
typedef struct spc_params {
    uint32_t lookback;    /* 1 .. 64: the predecessors an anchor looks at (default 64) */
    uint32_t max_dist;    /* 1 .. 2^31 - 1: the largest dx and dy (default 5000) */
    uint32_t max_gap;     /* 0 .. 2^31 - 1: the largest d (default 500) */
    uint32_t gap_penalty; /* 0 .. 65535: what a unit of d costs (default 1) */
} spc_params;

typedef struct spc_chain { /* 48 bytes */
    uint64_t ref_start;    /* y of the first anchor */
    uint64_t ref_end;      /* y + l of the last anchor */
    uint32_t read_start;   /* x of the first anchor */
    uint32_t read_end;     /* x + l of the last anchor */
    uint32_t score;        /* f of the chain's end */
    uint32_t anchors;      /* number of anchors in the chain */
    uint32_t first;        /* index of the first anchor within the read's range */
    uint32_t last;         /* index of the last anchor within the read's range */
    uint32_t gap;          /* sum of d along the chain, saturating at 2^32 - 1 */
    uint32_t doc;          /* D of the last anchor, SPC_NO_DOC without ids */
} spc_chain;

/* of the most recent spc_* call on an index: reads and anchors it looked at, the reads that got a chain and the anchors
 * in those chains, the eligible pairs the recurrence evaluated, and the HIP-event time of the chain kernel alone. */
typedef struct spc_chain_stats {
    uint64_t reads;
    uint64_t anchors;
    uint64_t chained_reads;
    uint64_t chain_anchors;
    uint64_t candidates;
    float kernel_ms;
} spc_chain_stats;

/* Device form, asynchronous on `stream` (a hipStream_t as void*, NULL = default stream); composes behind
 * spm_mems_device on the same stream: nothing returns to the host between the records and the chains.  Read q's
 * anchors are d_matches[d_match_offsets[q] .. d_match_offsets[q + 1]) and, when given, the same range of
 * d_match_docs (NULL: no ids); d_match_offsets[0] need not be 0.  d_out gets one record per read; d_out_score and
 * d_out_pred (each may be NULL) get f and pred of every anchor at the anchor's index in d_matches: the whole table
 * of the dynamic programme.  d_matches and d_out must be 16-byte aligned, d_match_offsets 8-byte, the others 4-byte.
 * Decreasing offsets or a read of 2^32 anchors or more are reported by spc_last_chain_stats (SPX_E_FORMAT); such a
 * read counts as one without anchors.  The same input gives the same bytes. */
int spc_chain_device(spx_index *ix, const spm_match *d_matches, const uint32_t *d_match_docs,
                     const uint64_t *d_match_offsets, uint64_t nreads, const spc_params *params, spc_chain *d_out,
                     uint32_t *d_out_score, uint32_t *d_out_pred, void *stream);
/* Host form: reads in (upper-cased, concatenated at offsets[0 .. nreads]), one record per read out.  digest_kind, k,
 * w, min_length and want_docs as in spm_mems_begin, whose steps it takes -- digestion, the MS walk, the length
 * extension, the count of the matches, a host wait, the records at their exact size -- with the chain kernel behind
 * them on the same stream; 48 bytes per read come back, and the values per read after digestion (out_values, may be
 * NULL).  One piece per call: at most 32 Mi characters and 4 Mi reads (SPX_E_ARG beyond). */
int spc_chain_batch(spx_index *ix, int digest_kind, uint32_t k, uint32_t w, const uint8_t *seqs,
                    const uint64_t *offsets, uint64_t nreads, uint64_t min_length, int want_docs,
                    const spc_params *params, spc_chain *out_chains, uint64_t *out_values);
/* Statistics of the most recent spc_* call on ix (synchronises with it). */
int spc_last_chain_stats(spx_index *ix, spc_chain_stats *out);

#ifdef __cplusplus
}
#endif

#endif /* SPUMONI_CHAIN_H */
