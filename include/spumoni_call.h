/*
 * spumoni_call.h -- C-ABI of the pileup and the calls in libspumoni_gpu.so (gfx950): per base of every sequence's forward
 * strand, which letters the reads carried where they disagreed with the reference, how many insertions start there and how
 * many reads delete it -- accumulated on the device beside the coverage of spumoni_cover.h -- and the single-nucleotide
 * calls these counts support.  The calls come back in place of a PAF file and a second pass over the reads.
 *
 * The rule (ours; spumoni_amd/call.py: pileup_reference and calls_reference are the specification, and the tests hold the
 * kernels to them bit for bit).  Per index the input is the sequence table of spn_set_sequences, with F[s], G and the piece
 * starts P as in spumoni_cover.h, and the text: the forward piece of sequence s starts at P[s * strands].  Per read the
 * input is an spn_mapping, the read's entries as spn_map_device writes them (length << 4 | op, along the forward strand on
 * either strand) and the read's bytes as given: R, with nreads + 1 offsets.
 *   - LETTER CODES.  A byte has code 0, 1, 2, 3 for A/a, C/c, G/g, T/t and code 4 ("other") for anything else.
 *   - THE ORIENTED READ is the read itself on strand 0.  On any other strand its position j is read byte len - 1 - j, and
 *     a code c < 4 becomes 3 - c; 4 stays 4.  The entries of a reverse mapping are already turned round, so walking them
 *     over the oriented read is the same walk on both strands.
 *   - A MAPPED READ (seq = s, target_start = a, target_end = b) is walked from pos = a, j = 0 over all its entries in
 *     order.  'S' n: j += n.  '=' n: pos += n, j += n.  'X' n: for each of the n columns alt[4 * (F[s] + pos) + c] += 1
 *     where c < 4 is the oriented read's code at j, other[F[s] + pos] += 1 where c = 4; then pos and j advance.  'I' n:
 *     ins[F[s] + pos] += 1, j += n -- pos is the next text position.  'D' n: del[F[s] + pos .. + n) += 1, kept as one +1
 *     and one -1 in the difference array ddiff; pos += n.  'N' n: pos += n.
 *   - AN UNMAPPED READ (seq = SPN_UNMAPPED) adds nothing.
 *   - THE CHECKS.  Every input is untrusted.  A read is checked whole before anything is added and skipped whole, with
 *     error set, when it fails one of: all the checks of spumoni_cover.h; the read-consuming lengths ('=', 'X', 'I', 'S')
 *     add up to the read's length by its offsets; the read's offsets do not decrease and do not end beyond in_chars; no
 *     'I' stands behind the last text-consuming column ('=', 'X', 'D', 'N' of a length above 0) -- there pos would be b,
 *     and F[s] + b may be G.  spn_map_device's mappings end with '=' and never fail the last one.  No access leaves a
 *     buffer; a skipped read leaves no partial sums behind.
 *   - THE ARRAYS.  alt[4 * G], other[G], ins[G] and ddiff[G + 1] are 32-bit words in modular arithmetic; del[G] is ddiff's
 *     running sum.  That is 28 bytes per forward base beside the coverage's 12.
 *   - THE CALLS come from depth and mism of the coverage and the arrays above; the parameters are min_depth >= 1,
 *     min_alt >= 1 and min_permille in 0 .. 1000.  At position i of sequence s, ref is the text byte at P[s * strands] + i;
 *     the candidates are the codes 0 .. 3 other than ref's own code (all four when ref has code 4); the called allele is
 *     the candidate with the largest alt count, the lowest code among equals.  The position is a call when
 *     depth >= min_depth, that count >= min_alt and count * 1000 >= min_permille * depth, in 64-bit integers: no floating
 *     point anywhere.  Calls come in (sequence, position) order as spl_call.  ref_count is depth - mism[i]: the host
 *     derives it.
 *   - THE CONTRACT is the coverage's: fewer than 2^32 mapped reads between two resets.
 * Everything is a sum: the same input gives the same bytes, in any order of adds.
 *
 * Limits: indel alleles are not called, del and ins are evidence only; no genotypes or qualities; the sequence the
 * counts imply is spumoni_consensus.h's product; one count for both strands; one device; no digested indexes.
 *
 * Conventions: those of spumoni_gpu.h (0 or a negative SPX_E* code, message in spx_last_error(), NO CPU fallback).
 */
#ifndef SPUMONI_CALL_H
#define SPUMONI_CALL_H

#include <stdint.h>

#include "spumoni_cover.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spl_call { /* 48 bytes */
    uint64_t pos;     /* position in the sequence, 0-based */
    uint32_t seq;
    uint32_t depth;
    uint32_t alt[4];  /* by letter code */
    uint32_t other;
    uint32_t del;
    uint32_t ins;
    uint8_t ref;      /* the text byte */
    uint8_t allele;   /* code */
    uint16_t reserved;
} spl_call;

/* Of the most recent spl_* calls on an index.  The adds since the last spl_call_reset (host forms) or of the last
 * spl_pileup_add_device: the reads, the mapped ones among them, those added and those skipped by the checks; all 'X'
 * columns and those of code 4 among them; the 'I' and the 'D' entries; the atomic adds they cost (one per 'X' column and
 * per 'I', two per 'D').  calls: what the last calls step counted, kept or not by call_capacity.  error: a read failed
 * the checks; overflow: the calls did not fit call_capacity.  The HIP-event time of the last add, finish and calls step. */
typedef struct spl_call_stats {
    uint64_t reads;
    uint64_t mapped;
    uint64_t added;
    uint64_t skipped;
    uint64_t x_columns;
    uint64_t other_columns;
    uint64_t insertions;
    uint64_t deletions;
    uint64_t atomics;
    uint64_t calls;
    uint32_t error;
    uint32_t overflow;
    float step_ms[3];
    uint32_t reserved;
} spl_call_stats;

/* Device forms: asynchronous on `stream`, no host wait inside, the caller's buffers.  All need the sequence table.
 *
 * _add_device: d_mappings (16-byte aligned), d_op_offsets (nreads + 1) and d_ops are spn_map_device's outputs, in_entries
 * the entries d_ops holds; d_reads and d_read_offsets (nreads + 1) the reads' bytes, in_chars of them.  d_alt: 4 * G words
 * (16-byte aligned), d_other and d_ins: G words, d_ddiff: G + 1 words; the batch is added to what they hold (zeros at
 * first).  A read that fails the checks adds nothing and spl_last_call_stats returns SPX_E_FORMAT. */
int spl_pileup_add_device(spx_index *ix, const spn_mapping *d_mappings, const uint64_t *d_op_offsets, const uint32_t *d_ops,
                          uint64_t in_entries, const uint8_t *d_reads, const uint64_t *d_read_offsets, uint64_t in_chars,
                          uint64_t nreads, uint32_t *d_alt, uint32_t *d_other, uint32_t *d_ins, uint32_t *d_ddiff, void *stream);
/* _finish_device: d_del[G] gets the running sum of d_ddiff, which stays as it is. */
int spl_pileup_finish_device(spx_index *ix, const uint32_t *d_ddiff, uint32_t *d_del, void *stream);
/* _calls_device: d_depth and d_mism are spd_cover_finish_device's and spd_cover_add_device's.  d_calls (16-byte aligned)
 * gets the calls, call_capacity of them at the most, *d_count how many there are; calls beyond call_capacity are not
 * written, the count is kept and overflow is set.  SPX_E_ARG for parameters outside their ranges. */
int spl_calls_device(spx_index *ix, const uint32_t *d_depth, const uint32_t *d_mism, const uint32_t *d_alt, const uint32_t *d_other,
                     const uint32_t *d_ins, const uint32_t *d_del, uint32_t min_depth, uint32_t min_alt, uint32_t min_permille,
                     uint64_t call_capacity, spl_call *d_calls, uint64_t *d_count, void *stream);

/* Host forms, with the arrays in the handle beside the coverage's: about 28 bytes per base of the forward genome more.
 * They go with the index; a clone of an index that has them starts with arrays of its own, empty; spn_set_sequences drops
 * them, and the next call says so.
 *
 * _reset does what spd_cover_reset does and allocates the pileup's arrays, or zeroes the ones there are.  SPX_E_ARG
 * without a sequence table; SPX_E_UNSUPPORTED with a message that names the bytes when they do not fit the device. */
int spl_call_reset(spx_index *ix);
/* _add_batch: spd_cover_add_batch's arguments.  One spn_map_begin, then the coverage's add and the pileup's add on the
 * records and entries where it left them: depth and allele counts always speak of the same reads.  The reads' bytes
 * seqs[offsets[0] .. offsets[nreads]) are copied to the device once more, asynchronously, in front of spn_map_begin. */
int spl_call_add_batch(spx_index *ix, int digest_kind, uint32_t k, uint32_t w, const uint8_t *seqs, const uint64_t *offsets,
                       uint64_t nreads, uint64_t min_length, int want_docs, const spc_params *chain_params,
                       const spa_params *align_params, const spe_params *extend_params, spn_mapping *out_mappings);
/* _calls_begin counts the calls and writes them on the device, *n_calls of them; _calls_fetch copies them to
 * out_calls[*n_calls]. */
int spl_calls_begin(spx_index *ix, uint32_t min_depth, uint32_t min_alt, uint32_t min_permille, uint64_t *n_calls);
int spl_calls_fetch(spx_index *ix, spl_call *out_calls);
/* A slice of the raw arrays: the positions [first, first + count) of the forward genome; out_alt gets 4 * count words.
 * Any output may be NULL. */
int spl_pileup_counts(spx_index *ix, uint64_t first, uint64_t count, uint32_t *out_alt, uint32_t *out_other, uint32_t *out_ins,
                      uint32_t *out_del);
/* Statistics of the most recent spl_* calls on ix (synchronises with them). */
int spl_last_call_stats(spx_index *ix, spl_call_stats *out);

#ifdef __cplusplus
}
#endif

#endif /* SPUMONI_CALL_H */
