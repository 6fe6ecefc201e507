/*
 * spumoni_mems.h -- C-ABI of the matches in libspumoni_gpu.so (gfx950): for every read, the positions where a new
 * exact match with the text starts and is long enough, as (read position, length, text position), reduced on the
 * device from the per-position MS lengths and pointers an MS query leaves in device memory.
 *
 * The rule (ours: the reference stops at the per-position files; MONI ships the same reduction as `moni mems`).  For
 * a read with lengths L[0..m) and pointers P[0..m), as spx_query_batch* returns them in MS mode, and optionally
 * document ids D[0..m):
 *   - position i STARTS a match when i == 0 or L[i] >= L[i - 1].  The extension (compute_ms_pml.cpp:802-810) gives
 *     L[i] >= L[i - 1] - 1, with equality exactly where the match of i - 1 merely continues;
 *   - a start is REPORTED when L[i] >= min_length.  min_length >= 1 (0: SPX_E_ARG): positions of length 0 are where
 *     the wrapped and placeholder pointers live, and they never come out;
 *   - the record: ref_pos = P[i] verbatim, read_pos = i, length = L[i]; with ids, D[i] goes to a parallel array;
 *   - records are ordered by read, then by read_pos; match_offsets[0 .. nreads] (CSR) says where each read's records
 *     start: an empty read, or a read without a reported start, has an empty range;
 *   - the last value of the read before never influences a read's first position;
 *   - digested reads are reported in digested coordinates, like every other output.
 * The rule is defined on the arrays, not on the text: text[ref_pos .. ref_pos + length) equals the read at read_pos,
 * and the match cannot be extended to the right.  Where the lengths under-report after a letter the text does not
 * have, a reported match is still exact but may not be maximal.
 * spumoni_amd/mems.py: mems_reference is the same rule in numpy; the tests hold the kernels to it bit for bit.
 *
 * Conventions: those of spumoni_gpu.h (0 or a negative SPX_E* code, message in spx_last_error(), NO CPU fallback).
 */
#ifndef SPUMONI_MEMS_H
#define SPUMONI_MEMS_H

#include <stdint.h>

#include "spumoni_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spm_match { /* 16 bytes */
    uint64_t ref_pos;
    uint32_t read_pos;
    uint32_t length;
} spm_match;

/* of the most recent spm_* call on an index: the values it looked at, the reported starts, the records it wrote
 * (matches > written: the capacity was too small), the longest reported length, and the HIP-event time of the
 * match kernels alone. */
typedef struct spm_mems_stats {
    uint64_t values;
    uint64_t matches;
    uint64_t written;
    uint64_t longest;
    float kernel_ms;
} spm_mems_stats;

/* Device form, asynchronous on `stream` (a hipStream_t as void*, NULL = default stream); composes after
 * spx_query_batch_device*() in MS mode on the same stream: nothing returns to the host between the walk and the
 * records.  value_bits 16 or 32 = width of d_lengths and, when given, of d_docs (NULL: no ids; then d_out_docs is not
 * written).  Read q's values are d_lengths[d_offsets[q] .. d_offsets[q + 1]), the same of d_pointers and d_docs;
 * d_lengths, d_docs and d_out must be 16-byte aligned (the lengths are read as the 16-byte vectors the walk stored;
 * the pointers and ids are read at reported starts only).  total_values = d_offsets[nreads] - d_offsets[0] or an upper
 * bound: it sizes the index's scratch, and a batch that holds more is reported by spm_last_mems_stats
 * (SPX_E_FORMAT), as is a read of 2^32 values or more; the output of such a call is undefined.
 * d_match_offsets (nreads + 1) is always complete.  Records (and ids) of rank >= out_capacity are not written and
 * nothing is written past the capacity (d_out / d_out_docs may be NULL when it is 0): a caller can size a second
 * call from d_match_offsets[nreads].  The same input gives the same bytes. */
int spm_mems_device(spx_index *ix, const void *d_lengths, int value_bits, const uint64_t *d_pointers,
                    const void *d_docs, const uint64_t *d_offsets, uint64_t nreads, uint64_t total_values,
                    uint64_t min_length, uint64_t *d_match_offsets, spm_match *d_out, uint64_t out_capacity,
                    uint32_t *d_out_docs, void *stream);
/* Host pair: reads in (upper-cased, concatenated at offsets[0 .. nreads]), records out.  digest_kind 0 /
 * SPX_DIGEST_PROMOTED / SPX_DIGEST_DNA with k and w as in spx_digest_batch.  _begin runs digestion, the MS walk, the
 * length extension (needs spx_index_set_text / _rebuild_text) and the match kernels on the device, allocates the
 * records at their exact size once they are counted, and copies back match_offsets alone (nreads + 1), the values
 * per read after digestion (out_values, may be NULL) and the number of records (n_matches); the per-position arrays
 * exist only in the library's scratch (16-bit when every read is shorter than 65536 characters).  The records wait
 * in the handle for _fetch, the next call on the index from the same thread: out gets n_matches records, out_docs
 * (NULL unless want_docs) as many ids.  One piece per call: feed batches of at most 32 Mi characters. */
int spm_mems_begin(spx_index *ix, int digest_kind, uint32_t k, uint32_t w, const uint8_t *seqs,
                   const uint64_t *offsets, uint64_t nreads, uint64_t min_length, int want_docs,
                   uint64_t *match_offsets, uint64_t *out_values, uint64_t *n_matches);
int spm_mems_fetch(spx_index *ix, spm_match *out, uint32_t *out_docs);
/* Statistics of the most recent spm_* call on ix (synchronises with it). */
int spm_last_mems_stats(spx_index *ix, spm_mems_stats *out);

#ifdef __cplusplus
}
#endif

#endif /* SPUMONI_MEMS_H */
