/*
 * spumoni_cover.h -- C-ABI of the coverage in libspumoni_gpu.so (gfx950): per-base depth and mismatch counts along every
 * sequence's forward strand and a summary per sequence, accumulated on the device over any number of batches of the
 * mappings of spumoni_map.h.  One small table comes back in place of a PAF file.
 *
 * The rule (ours; spumoni_amd/cover.py: cover_reference, summary_reference and runs_reference are the specification, and
 * the tests hold the kernels to them bit for bit).  Per index the input is the sequence table of spn_set_sequences: the
 * lengths L[0 .. n_seqs).  F[s] is the sum of the lengths before sequence s, G = F[n_seqs] the length of the forward
 * genome; coordinates are 64-bit.  Per read the input is an spn_mapping and the read's entries (length << 4 | op).
 *   - A MAPPED READ (seq = s, target_start = a, target_end = b) is walked from pos = a over its entries other than 'S',
 *     in order; they run along the forward strand on either strand.  '=' n: depth[F[s] + pos .. + n) += 1, then
 *     pos += n.  'X' n: the same, and mism[...] += 1 over the same range.  'D' n and 'N' n: pos += n -- a deleted or
 *     skipped base is not covered.  'I' n: nothing per base.  Per sequence reads[s] += 1 and indels[s] += the 'I' and 'D'
 *     lengths.  The strand field does not enter the rule.
 *   - AN UNMAPPED READ (seq = SPN_UNMAPPED) adds nothing.
 *   - THE CHECKS.  Every input is untrusted.  A read is skipped whole, and error is set, when s >= n_seqs; when
 *     a <= b <= L[s] does not hold; when an operation is none of the six; when an 'S' stands between two other entries;
 *     when the text-consuming lengths ('=', 'X', 'D', 'N') do not add up to b - a; when the read's offsets decrease or end
 *     beyond in_entries.  No access leaves a buffer; a skipped read leaves no partial sums behind.
 *   - THE ARRAYS.  diff[G + 1] is the difference array of depth in 32-bit modular arithmetic: depth[i] = diff[0] + ... +
 *     diff[i]; a stretch of '=' and 'X' columns between two 'D' / 'N' is one interval and costs one +1 and one -1.
 *     mism[G] counts the 'X' columns per position.  seq_counts[2 * n_seqs]: reads[s] at 2 * s, indels[s] at 2 * s + 1.
 *   - THE SUMMARY per sequence is spd_seq_cover: covered -- the positions with depth > 0; bases -- the sum of depth;
 *     mismatches -- the sum of mism; indels, reads; max_depth.
 *   - THE RUNS: inside each sequence the maximal runs of equal depth, in (sequence, start) order, as spd_run: start and
 *     end in the sequence, seq, depth, and mismatches -- the sum of mism over the run modulo 2^32.  Runs with
 *     depth < min_depth are left out; with min_depth = 0 the runs of a sequence partition it.  A run never crosses a
 *     sequence border, even where the depth is the same on both sides.
 *   - THE CONTRACT: fewer than 2^32 mapped reads are added between two resets, so no depth can wrap.  The host forms
 *     count and refuse with SPX_E_ARG; for the device forms it is the caller's contract.
 * Everything is a sum: the same input gives the same bytes, in any order of adds.
 *
 * Limits: depth for digested indexes is not defined (the mappings' are not); a deleted base is not covered; one depth
 * for both strands; one device.
 *
 * Conventions: those of spumoni_gpu.h (0 or a negative SPX_E* code, message in spx_last_error(), NO CPU fallback).
 */
#ifndef SPUMONI_COVER_H
#define SPUMONI_COVER_H

#include <stdint.h>

#include "spumoni_map.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spd_seq_cover { /* 48 bytes */
    uint64_t covered;
    uint64_t bases;
    uint64_t mismatches;
    uint64_t indels;
    uint64_t reads;
    uint32_t max_depth;
    uint32_t reserved;
} spd_seq_cover;

typedef struct spd_run { /* 32 bytes */
    uint64_t start; /* in the sequence */
    uint64_t end;
    uint32_t seq;
    uint32_t depth;
    uint32_t mismatches;
    uint32_t reserved;
} spd_run;

/* Of the most recent spd_cover_* calls on an index.  The adds since the last spd_cover_reset (host forms) or of the last
 * spd_cover_add_device: the reads, the mapped ones among them, those added and those skipped by the checks, the intervals
 * and the atomic adds they cost (two per interval, one per 'X' column); runs: what the last runs call counted, kept or
 * not by run_capacity.  error: a read failed the checks; overflow: the runs did not fit run_capacity.  The HIP-event
 * time of the last add, finish and runs step in step_ms[0 .. 2], kernel_ms their sum. */
typedef struct spd_cover_stats {
    uint64_t reads;
    uint64_t mapped;
    uint64_t added;
    uint64_t skipped;
    uint64_t intervals;
    uint64_t atomics;
    uint64_t runs;
    uint32_t error;
    uint32_t overflow;
    float kernel_ms;
    float step_ms[3];
} spd_cover_stats;

/* Device forms: asynchronous on `stream`, no host wait inside, the caller's buffers.  All need the sequence table.
 *
 * _add_device: d_mappings (16-byte aligned), d_op_offsets (nreads + 1) and d_ops are spn_map_device's outputs,
 * in_entries the entries d_ops holds.  d_diff: G + 1 words, d_mism: G words, d_seq_counts: 2 * n_seqs 64-bit words; the
 * batch is added to what they hold (zeros at first).  A read that fails the checks above adds nothing and
 * spd_last_cover_stats returns SPX_E_FORMAT. */
int spd_cover_add_device(spx_index *ix, const spn_mapping *d_mappings, const uint64_t *d_op_offsets, const uint32_t *d_ops,
                         uint64_t in_entries, uint64_t nreads, uint32_t *d_diff, uint32_t *d_mism, uint64_t *d_seq_counts,
                         void *stream);
/* _finish_device: d_depth[G] gets the running sum of d_diff, d_out[n_seqs] (8-byte aligned) the summary.  d_diff, d_mism
 * and d_seq_counts stay as they are, so that more can be added. */
int spd_cover_finish_device(spx_index *ix, const uint32_t *d_diff, const uint32_t *d_mism, const uint64_t *d_seq_counts,
                            uint32_t *d_depth, spd_seq_cover *d_out, void *stream);
/* _runs_device: d_runs (8-byte aligned) gets the runs of depth >= min_depth, run_capacity of them at the most, *d_count
 * how many there are; runs beyond run_capacity are not written, the count is kept and overflow is set. */
int spd_cover_runs_device(spx_index *ix, const uint32_t *d_depth, const uint32_t *d_mism, uint32_t min_depth,
                          uint64_t run_capacity, spd_run *d_runs, uint64_t *d_count, void *stream);

/* Host forms, with the arrays in the handle: about 12 bytes per base of the forward genome.  They go with the index; a
 * clone of an index that has them starts with arrays of its own, empty; spn_set_sequences drops them, and the next call says so.
 *
 * _reset allocates them, or zeroes the ones there are.  SPX_E_ARG without a sequence table; SPX_E_UNSUPPORTED with a
 * message that names the bytes when they do not fit the device. */
int spd_cover_reset(spx_index *ix);
/* _add_batch: spn_map_begin's arguments.  Runs that pipeline and adds the mappings where it left them on the device; the
 * entries never come back (spn_map_fetch has nothing to fetch afterwards).  out_mappings (may be NULL) gets the nreads
 * records.  SPX_E_ARG when the batch would take the mapped reads since the reset to 2^32 or beyond: nothing is added. */
int spd_cover_add_batch(spx_index *ix, int digest_kind, uint32_t k, uint32_t w, const uint8_t *seqs, const uint64_t *offsets,
                        uint64_t nreads, uint64_t min_length, int want_docs, const spc_params *chain_params,
                        const spa_params *align_params, const spe_params *extend_params, spn_mapping *out_mappings);
/* out[n_seqs] in table order. */
int spd_cover_summary(spx_index *ix, spd_seq_cover *out, uint64_t n_seqs);
/* _runs_begin counts the runs of depth >= min_depth and writes them on the device, *n_runs of them; _runs_fetch copies
 * them to out_runs[*n_runs]. */
int spd_cover_runs_begin(spx_index *ix, uint32_t min_depth, uint64_t *n_runs);
int spd_cover_runs_fetch(spx_index *ix, spd_run *out_runs);
/* A slice of the raw arrays: depth and mism of the positions [first, first + count) of the forward genome (F[s] + the
 * position in sequence s); either output may be NULL. */
int spd_cover_depth(spx_index *ix, uint64_t first, uint64_t count, uint32_t *out_depth, uint32_t *out_mism);
/* Statistics of the most recent spd_cover_* calls on ix (synchronises with them). */
int spd_last_cover_stats(spx_index *ix, spd_cover_stats *out);

#ifdef __cplusplus
}
#endif

#endif /* SPUMONI_COVER_H */
