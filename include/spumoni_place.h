/*
 * spumoni_place.h -- C-ABI of the placements in libspumoni_gpu.so (gfx950): for every read, where it sits on the
 * indexed text and how well it fits there -- its longest match, extended to both sides without gaps under an x-drop
 * rule -- as one 32-byte record, computed on the device from the per-position MS lengths and pointers an MS query
 * leaves in device memory, the reads and the text the index holds.
 *
 * The rule (ours: the reference stops at the per-position files; MONI ships the step as `moni extend`).  For a read
 * with characters R[0..m) as the walk saw them (digested under -m / -a), lengths L[0..m) and pointers P[0..m) as
 * spx_query_batch* returns them in MS mode, optionally document ids D[0..m), and the text T[0..n_text) of the index
 * (spx_index_set_text / spx_index_rebuild_text):
 *   - SEED: i* is the smallest i with L[i] = max L.  The read is UNPLACED when m == 0 or L[i*] < min_seed (min_seed
 *     >= 1; 0: SPX_E_ARG).  The last value of the read before never influences a read's first position;
 *   - DIAGONAL: read position j faces text position P[i*] - i* + j;
 *   - RIGHT EXTENSION: from read position e = i* + L[i*] and text position te = P[i*] + L[i*] (modulo 2^64), over
 *     K = min(m - e, n_text - te) steps, 0 where either is not positive: defined for any arrays, also inconsistent
 *     ones.  s_0 = 0, s_k = s_(k-1) + 1 where R[e + k - 1] == T[te + k - 1] and s_(k-1) - mismatch_penalty where not.
 *     stop is the smallest k >= 1 with max_(u <= k) s_u - s_k > x_drop (a drop EQUAL to x_drop does not stop), or K
 *     if there is none; right is the smallest k in [0, stop] that maximises s_k;
 *   - LEFT EXTENSION: the mirror image, step k comparing R[i* - k] with T[P[i*] - k], K = min(i*, P[i*]) -- and 0
 *     for a pointer behind the text (P[i*] > n_text: inconsistent arrays), which has nothing in front of it to compare;
 *   - RECORD: ref_start = P[i*] - left, read_start = i* - left, read_end = i* + L[i*] + right, matches = L[i*] plus
 *     the equal characters inside the two extensions (both modulo 2^32; consistent arrays never get there),
 *     seed_pos = i*, seed_len = L[i*], doc = D[i*] or SPP_NO_DOC without ids;
 *   - an unplaced read: ref_start = SPP_UNPLACED, doc = SPP_NO_DOC, every other field 0.
 * mismatch_penalty 0 .. 65535, x_drop 0 .. 2^31 - 1 (outside: SPX_E_ARG).  What follows from the rule:
 *   - mismatch_penalty = 0 never drops: it clips only trailing mismatches, and matches / (read_end - read_start) is
 *     then the Hamming identity of the overlap of read and text on the diagonal;
 *   - the seed's characters are trusted, not compared again;
 *   - an extension may run across a sequence boundary of the concatenated text;
 *   - where the lengths under-report after a letter the text does not have, the seed is still
 *     exact but may not be the longest;
 *   - digested reads are placed in digested coordinates, on the digested text, like every other output.
 * spumoni_amd/place.py: place_reference is the same rule in numpy; the tests hold the kernels to it bit for bit.
 *
 * Conventions: those of spumoni_gpu.h (0 or a negative SPX_E* code, message in spx_last_error(), NO CPU fallback).
 */
#ifndef SPUMONI_PLACE_H
#define SPUMONI_PLACE_H

#include <stdint.h>

#include "spumoni_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPP_NO_DOC 0xFFFFFFFFu
#define SPP_UNPLACED UINT64_MAX

typedef struct spp_placement { /* 32 bytes */
    uint64_t ref_start;
    uint32_t read_start;
    uint32_t read_end;
    uint32_t matches;
    uint32_t seed_pos;
    uint32_t seed_len;
    uint32_t doc;
} spp_placement;

/* of the most recent spp_* call on an index: the values it looked at, the reads it placed, the sum of their seed_len,
 * the sum of left + right, and the HIP-event time of the placement kernels alone. */
typedef struct spp_place_stats {
    uint64_t values;
    uint64_t placed;
    uint64_t seed_values;
    uint64_t extended_values;
    float kernel_ms;
} spp_place_stats;

/* Device form, asynchronous on `stream` (a hipStream_t as void*, NULL = default stream); composes after
 * spx_query_batch_device*() in MS mode on the same stream: nothing returns to the host between the walk and the
 * records.  Read q's characters are d_seqs[d_offsets[q] .. d_offsets[q + 1]) -- d_seqs under the walk's contract,
 * readable for round_up(total, 4) + 32 bytes, any alignment -- and its values the same range of d_lengths, d_pointers
 * and d_docs.  value_bits 16 or 32 = width of d_lengths and, when given, of d_docs (NULL: no ids).  d_lengths and
 * d_out must be 16-byte aligned (the lengths are read as the 16-byte vectors the walk stored: the array is readable up
 * to the next multiple of 16 bytes), d_pointers and d_offsets 8-byte; pointers and ids are read at the seed only.
 * total_values = d_offsets[nreads] - d_offsets[0] or an upper bound: a read that ends behind it is not looked at and
 * comes back unplaced, and spp_last_place_stats reports the call (SPX_E_FORMAT), as it does a read of 2^32 values or
 * more or decreasing offsets.  The index must hold its text: without it the call is refused (spx_index_set_text /
 * spx_index_rebuild_text).  d_out gets nreads records.  The same input gives the same bytes. */
int spp_place_device(spx_index *ix, const uint8_t *d_seqs, const void *d_lengths, int value_bits,
                     const uint64_t *d_pointers, const void *d_docs, const uint64_t *d_offsets, uint64_t nreads,
                     uint64_t total_values, uint64_t min_seed, uint32_t mismatch_penalty, uint64_t x_drop,
                     spp_placement *d_out, void *stream);
/* Host form: reads in (upper-cased, concatenated at offsets[0 .. nreads]), nreads records out; out_values (may be
 * NULL) gets the values per read after digestion.  digest_kind 0 / SPX_DIGEST_PROMOTED / SPX_DIGEST_DNA with k and w
 * as in spx_digest_batch; want_docs needs an index with a document array.  Digestion, the MS walk, the length
 * extension and the placement run on the device on pieces of at most 32 Mi characters, and 32 bytes per read come
 * back; the per-position arrays exist only in the library's scratch (16-bit when every read is shorter than 65536
 * characters).  Under digestion the kernels read the digested reads at the offsets of the concatenation: the call
 * forces the concatenating pass (the "digest_parked" option is held at 1 while it runs). */
int spp_place_batch(spx_index *ix, int digest_kind, uint32_t k, uint32_t w, const uint8_t *seqs,
                    const uint64_t *offsets, uint64_t nreads, uint64_t min_seed, uint32_t mismatch_penalty,
                    uint64_t x_drop, int want_docs, spp_placement *out, uint64_t *out_values);
/* Statistics of the most recent spp_* call on ix (synchronises with it). */
int spp_last_place_stats(spx_index *ix, spp_place_stats *out);

#ifdef __cplusplus
}
#endif

#endif /* SPUMONI_PLACE_H */
