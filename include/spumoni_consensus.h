/*
 * spumoni_consensus.h -- C-ABI of the consensus in libspumoni_gpu.so (gfx950): the sequence that the coverage of
 * spumoni_cover.h and the pileup of spumoni_call.h imply for every sequence of the table, decided per base and laid out as
 * FASTA body text on the device.  It comes back in place of 40 bytes of counts per base, or of a .vcf and a patched
 * reference.
 *
 * The rule (ours; spumoni_amd/consensus.py: consensus_reference is the specification, and the tests hold the kernels to it
 * byte for byte).  Integers only, no floating point.  The input is the sequence table -- F[s], G and the piece starts P as in
 * spumoni_cover.h --, the text, depth[G] of spd_cover_finish_device, and alt[4 * G], ins[G] and del[G] of
 * spl_pileup_add_device and spl_pileup_finish_device; other and mism do not enter.  The parameters are spl_calls_device's
 * min_depth >= 1, min_alt >= 1 and min_permille in 0 .. 1000, a mask byte (0: "write the reference's byte") and line_width
 * in 0 .. 2^31 - 1 (0: one line per sequence).
 *   - THE DECISION at position i of sequence s: g = F[s] + i, ref = text[P[s * strands] + i], d = depth[g], dl = del[g],
 *     span = d + dl, all sums and products in 64 bits.  The first rule that holds decides:
 *       1. span < min_depth: MASKED -- emits mask, or ref when mask is 0;
 *       2. dl >= min_alt and dl * 1000 >= min_permille * span: DELETED -- emits nothing;
 *       3. d < min_depth: MASKED, as in rule 1;
 *       4. SUBSTITUTED -- emits "ACGT"[allele]: the best candidate is the calls' (the codes other than ref's own, the largest
 *          alt count, the lowest code among equals); the rule holds when its count >= min_alt and
 *          count * 1000 >= min_permille * d.  Among the positions rules 1 - 3 leave, these are spl_calls_device's calls
 *          at the same three thresholds;
 *       5. KEPT -- emits ref as it is, case included.
 *   - AN INSERTION SITE is a position that rule 1 does not mask with ins[g] >= min_alt and
 *     ins[g] * 1000 >= min_permille * span.  Sites are counted, not applied: the pileup keeps how many insertions start at
 *     a base, not their letters.
 *   - THE BODY is one byte buffer for all sequences in table order.  Sequence s contributes its emitted bytes in position
 *     order, a '\n' behind every line_width-th letter and a '\n' behind the last letter unless one was just written; with
 *     line_width 0 only the final '\n'.  A sequence with no emitted letter contributes no bytes.  So
 *     body_bytes(s) = letters + (line_width ? ceil(letters / line_width) : (letters > 0)), and body_start is the running
 *     sum of body_bytes.
 *   - THE RECORDS: one sps_seq per sequence.  kept = letters - substituted - masked.
 *
 * Limits: insertions are flagged, not applied; a deletion counts where the reads' alignments put it, and forward and reverse
 * reads can put one deletion at the two ends of a repeat and split its count; one decision for both strands; no IUPAC codes,
 * no qualities; one device; no digested indexes; the coverage's limits (spumoni_cover.h).
 *
 * Conventions: those of spumoni_gpu.h (0 or a negative SPX_E* code, message in spx_last_error(), NO CPU fallback).
 */
#ifndef SPUMONI_CONSENSUS_H
#define SPUMONI_CONSENSUS_H

#include <stdint.h>

#include "spumoni_call.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sps_params { /* 20 bytes */
    uint32_t min_depth;    /* >= 1 (default 2) */
    uint32_t min_alt;      /* >= 1 (default 2) */
    uint32_t min_permille; /* 0 .. 1000 (default 500) */
    uint32_t line_width;   /* 0 .. 2^31 - 1 (default 60); 0: one line per sequence */
    uint8_t mask;          /* the byte of a masked position (default 'N'); 0: the reference's byte */
    uint8_t reserved[3];
} sps_params;

typedef struct sps_seq { /* 48 bytes */
    uint64_t body_start;  /* where the sequence's bytes start in the body */
    uint64_t letters;     /* emitted letters: kept + substituted + masked */
    uint64_t substituted;
    uint64_t deleted;
    uint64_t masked;
    uint64_t ins_sites;
} sps_seq;

/* Of the most recent sps_* call on an index: the positions judged (G) and how they were decided, the insertion sites, the
 * letters and the bytes of the body, kept or not by body_capacity.  overflow: the body did not fit body_capacity.  The
 * HIP-event time of the count, the scans and the write. */
typedef struct sps_consensus_stats {
    uint64_t positions;
    uint64_t kept;
    uint64_t substituted;
    uint64_t deleted;
    uint64_t masked;
    uint64_t ins_sites;
    uint64_t letters;
    uint64_t bytes;
    uint32_t overflow;
    float step_ms[3];
} sps_consensus_stats;

/* Device form: asynchronous on `stream`, no host wait inside, the caller's buffers.  Needs the sequence table.  d_depth,
 * d_ins and d_del: G words (4-byte aligned), d_alt: 4 * G words (16-byte aligned); they stay as they are.  d_records
 * (8-byte aligned) gets n_seqs records, d_body the body, body_capacity bytes of it at the most, *d_count (8-byte aligned)
 * the body's total bytes: bytes at offsets >= body_capacity are not written, the records and the count are still complete
 * and overflow is set.  d_body may be NULL when body_capacity is 0.  SPX_E_ARG for parameters outside their ranges. */
int sps_consensus_device(spx_index *ix, const uint32_t *d_depth, const uint32_t *d_alt, const uint32_t *d_ins, const uint32_t *d_del,
                         const sps_params *params, uint64_t body_capacity, sps_seq *d_records, uint8_t *d_body, uint64_t *d_count,
                         void *stream);

/* Host forms, on the handle's arrays of spl_call_reset / spl_call_add_batch: the refusals of spl_calls_begin without a
 * sequence table or without the arrays; after spn_set_sequences the next call says that the arrays are gone; a clone starts
 * with nothing to fetch; an sps_consensus_device call on the handle between _begin and _fetch drops what waits for the fetch.
 *
 * _begin finishes the coverage and the pileup when something was added since, then counts and writes on the device:
 * *n_bytes gets the body's bytes.  _fetch copies the records to out_records[n_seqs] and the body to out_body[*n_bytes]
 * (may be NULL when that is 0). */
int sps_consensus_begin(spx_index *ix, const sps_params *params, uint64_t *n_bytes);
int sps_consensus_fetch(spx_index *ix, sps_seq *out_records, uint8_t *out_body);
/* Statistics of the most recent sps_* call on ix (synchronises with it). */
int sps_last_consensus_stats(spx_index *ix, sps_consensus_stats *out);

#ifdef __cplusplus
}
#endif

#endif /* SPUMONI_CONSENSUS_H */
