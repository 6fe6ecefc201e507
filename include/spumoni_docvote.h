/*
 * spumoni_docvote.h -- C-ABI of the document votes in libspumoni_gpu.so (gfx950): one record per read that says
 * which document the read belongs to and how clear that is, reduced on the device from the per-position lengths and
 * document ids a query leaves in device memory.
 *
 * The rule (ours: the reference stops at the per-position files, src/compute_ms_pml.cpp:1003-1010; it is what
 * SPUMONI 2's multi-class experiments compute from those two files).  For a read with values L[0..m) and document
 * ids D[0..m), as spx_query_batch* returns them in either mode:
 *   - position i VOTES when L[i] >= min_length; voters = number of voting positions;
 *   - votes[d] = voting positions with D[i] == d;
 *   - top_doc = the document with the most votes, the SMALLEST id among equals; top_votes its count;
 *   - second_votes = the largest count among the other documents, 0 when there is none;
 *   - no voter (also: an empty read): voters = top_votes = second_votes = 0, top_doc = SPV_NO_DOC.
 * spumoni_amd/docvote.py: votes_reference is the same rule in numpy; the tests hold the kernels to it bit for bit.
 *
 * Conventions: those of spumoni_gpu.h (0 or a negative SPX_E* code, message in spx_last_error(), NO CPU fallback).
 * Document ids are those of the index (<= 65535); 0xFFFFFFFF is not a document id.
 */
#ifndef SPUMONI_DOCVOTE_H
#define SPUMONI_DOCVOTE_H

#include <stdint.h>

#include "spumoni_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPV_NO_DOC 0xFFFFFFFFu

typedef struct spv_vote { /* 16 bytes */
    uint32_t voters;
    uint32_t top_doc;
    uint32_t top_votes;
    uint32_t second_votes;
} spv_vote;

/* of the most recent spv_* call on an index: reads taken by each kernel path (several reads per wavefront; a
 * workgroup per read, counted in LDS; several workgroups per read), reads without a value, voting positions, the
 * workgroup tiles the long reads were cut into, and the HIP-event time of the vote kernels alone. */
typedef struct spv_votes_stats {
    uint64_t reads_short;
    uint64_t reads_medium;
    uint64_t reads_long;
    uint64_t reads_empty;
    uint64_t voting_positions;
    uint64_t long_tiles;
    float kernel_ms;
} spv_votes_stats;

/* Device form, asynchronous on `stream` (a hipStream_t as void*, NULL = default stream); composes after
 * spx_query_batch_device*() on the same stream.  value_bits 16 or 32 = width of BOTH arrays.  Read q's values are
 * d_lengths[d_offsets[q] .. d_offsets[q + 1]) and the same of d_docs; d_lengths, d_docs and d_out must be 16-byte
 * aligned (the values are read as the 16-byte vectors the walk stored).  total_values = d_offsets[nreads] -
 * d_offsets[0] or an upper bound: it sizes the index's scratch, and a batch that holds more is reported by
 * spv_last_votes_stats (SPX_E_FORMAT), as is a read of 2^32 values or more; the records of such a call are undefined. */
int spv_votes_device(spx_index *ix, const void *d_lengths, const void *d_docs, int value_bits,
                     const uint64_t *d_offsets, uint64_t nreads, uint64_t total_values,
                     uint64_t min_length, spv_vote *d_out, void *stream);
/* Host form: reads in (upper-cased, concatenated at offsets[0 .. nreads]), 16 bytes per read out.  digest_kind 0 /
 * SPX_DIGEST_PROMOTED / SPX_DIGEST_DNA with k and w as in spx_digest_batch.  Digestion, walk (with document ids), MS
 * length extension where mode is SPX_MODE_MS (needs spx_index_set_text / _rebuild_text), and the votes all stay on the
 * device; the per-position arrays exist only in the library's scratch (16-bit when every read is shorter than 65536
 * characters, 32-bit otherwise).  Large batches run as a pipeline of pieces.  out_values (may be NULL): values per
 * read after digestion -- 0 is the caller's "empty after digestion" case (compute_ms_pml.cpp:926-931). */
int spv_assign_batch(spx_index *ix, int mode, int digest_kind, uint32_t k, uint32_t w, const uint8_t *seqs,
                     const uint64_t *offsets, uint64_t nreads, uint64_t min_length, spv_vote *out,
                     uint64_t *out_values);
/* Statistics of the most recent spv_* call on ix (synchronises with it). */
int spv_last_votes_stats(spx_index *ix, spv_votes_stats *out);

#ifdef __cplusplus
}
#endif

#endif /* SPUMONI_DOCVOTE_H */
