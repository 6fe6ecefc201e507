/*
 * spumoni_map.h -- C-ABI of the mappings in libspumoni_gpu.so (gfx950): for every read, the extended alignment of
 * spumoni_extend.h in the coordinates of the sequence it lies on -- which sequence, which strand, where in it -- and its
 * CIGAR along that sequence's forward strand: what a line of PAF says.
 *
 * The rule (ours; spumoni_amd/map.py: map_reference is the specification, and the tests hold the kernels to it bit for
 * bit).  The input per read is the record and the entries of spumoni_extend.h and the read's length len; per index the
 * sequence table: the lengths of the sequences in text order and `strands`.  Without digestion the text is every
 * sequence followed at once, when strands == 2, by its reverse complement, and nothing between them: the pieces.
 * P[0 .. np] are the piece starts, P[np] = n_text.  Piece p belongs to sequence p / strands, it is the reverse piece when
 * p % strands == 1, and Lp = P[p + 1] - P[p] is the sequence's length.  For an aligned read:
 *   - THE COLUMNS: the entries other than 'S' expanded, in order.  A column has an operation and a text position t:
 *     ref_start plus the text characters consumed before it.  A text-consuming column ('=', 'X', 'D', 'N') lies in the
 *     piece that holds its t.
 *   - THE HOME PIECE is the piece with the most '=' columns, among equals the lowest p.
 *   - THE KEPT PART runs from the first '=' column in the home piece through the last one, with every column between
 *     them; text positions are monotone, so all of them lie in the home piece.  An alignment that lies in one piece and
 *     begins and ends with '=' is kept whole.  Read-consuming columns in front of the kept part join the left clip, those
 *     behind it the right clip; text-only columns outside it disappear.
 *   - THE RECORD is spn_mapping.  target_start = t_first - P[p], target_end = t_last + 1 - P[p]; on a reverse piece they
 *     become Lp - end and Lp - start: forward coordinates of the sequence.  read_start and read_end are the kept part's,
 *     in the read as given.  matches: '=' over the kept columns; edits: X + I + D over them ('N' is not counted, so this
 *     can differ from spumoni_extend.h's edits where a gap was not filled); block: the kept columns other than 'N';
 *     cut: SPN_CUT_LEFT when a column other than 'S' was removed on the left in text order, SPN_CUT_RIGHT on the right.
 *   - THE ENTRIES: the left clip, the kept operations and the right clip, merged and split as in spumoni_cigar.h
 *     (SPG_MAX_LENGTH).  On a reverse piece the whole list is reversed, so that the operations run along the forward
 *     sequence: PAF's convention for '-'.
 *   - A read that spumoni_extend.h left unaligned has seq = SPN_UNMAPPED, zeros elsewhere and no entries.
 * What follows from the rule, over a mapped read's entries: '=', 'X', 'I' and 'S' add up to len; '=', 'X', 'D' and 'N'
 * to target_end - target_start, which is at most Lp; the first and the last entry that is not 'S' are '='.
 *
 * Limits: the extension still compares plain bytes across a border and the mapping repairs that afterwards, by cutting;
 * one chain per read, so no mapping quality and no secondary mappings; one device.
 *
 * Conventions: those of spumoni_gpu.h (0 or a negative SPX_E* code, message in spx_last_error(), NO CPU fallback).
 */
#ifndef SPUMONI_MAP_H
#define SPUMONI_MAP_H

#include <stdint.h>

#include "spumoni_extend.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPN_UNMAPPED 0xFFFFFFFFu
#define SPN_CUT_LEFT 1u
#define SPN_CUT_RIGHT 2u

typedef struct spn_mapping { /* 48 bytes */
    uint64_t target_start;   /* in the sequence's forward strand */
    uint64_t target_end;
    uint32_t seq;            /* index into the sequence table, SPN_UNMAPPED: none */
    uint32_t strand;         /* 0 forward, 1 reverse */
    uint32_t read_start;     /* of the kept part, in the read as given */
    uint32_t read_end;
    uint32_t matches;
    uint32_t edits;
    uint32_t block;
    uint32_t cut;
} spn_mapping;

/* of the most recent spn_map_* call on an index, over the mapped reads (a read that came back unmapped for want of
 * capacity counts in none): the reads cut on either side, the reads on a reverse piece, their entries in and out, the
 * read characters that cuts moved into clips; error and overflow; the HIP-event time of the map kernels alone and of
 * their two steps: locate and count with the scan behind it, write. */
typedef struct spn_map_stats {
    uint64_t reads;
    uint64_t mapped;
    uint64_t cut_reads;
    uint64_t reverse_reads;
    uint64_t entries_in;
    uint64_t entries_out;
    uint64_t cut_chars;
    uint32_t error;
    uint32_t overflow;
    float kernel_ms;
    float step_ms[2];
    uint32_t reserved;
} spn_map_stats;

/* Copies the sequence table to the device and holds it in the handle; it is released with the index, and a clone made
 * afterwards has its own copy.  SPX_E_ARG for strands outside 1 .. 2, a length of zero, n_seqs == 0 and a total
 * (the lengths times strands) that is not the text's length.  Without a table every spn_map_* call returns SPX_E_ARG with
 * a message that says so. */
int spn_set_sequences(spx_index *ix, const uint64_t *seq_lengths, uint64_t n_seqs, uint32_t strands);

/* Device form, asynchronous on `stream`, no host wait inside.  d_alignments, d_op_offsets and d_ops are
 * spe_extend_device's outputs for the reads of d_read_offsets (nreads + 1).  d_out gets nreads records (16-byte aligned),
 * d_out_op_offsets nreads + 1 offsets, d_out_ops the entries, op_capacity of them at the most (<= 2^32 - 1).
 * Every input is untrusted: a record whose spans do not lie in [0, len] and [0, n_text] in order, or a read of 2^32
 * characters or more; entries whose read or text sums disagree with the spans or with len ('S' stands only in front of
 * the first and behind the last other entry); an operation that is none of the six; an aligned read without any '=':
 * each leaves the read unmapped, and spn_last_map_stats returns SPX_E_FORMAT.  No access leaves a buffer that the offsets
 * describe: a read whose input offsets decrease or end beyond in_entries is such a read.  A read whose entries do not fit
 * op_capacity comes back unmapped, its count stays in the offsets, and overflow is set.  The kernels read neither the
 * text nor the reads. */
int spn_map_device(spx_index *ix, const spa_alignment *d_alignments, const uint64_t *d_op_offsets, const uint32_t *d_ops,
                   uint64_t in_entries, const uint64_t *d_read_offsets, uint64_t nreads, uint64_t op_capacity,
                   spn_mapping *d_out, uint64_t *d_out_op_offsets, uint32_t *d_out_ops, void *stream);
/* Host pair: spe_extend_begin's arguments, the whole pipeline from the reads to the mappings.  out_mappings gets nreads
 * records; out_alignments (may be NULL) the spa_alignment records, for anchors and doc.  _begin waits on the host where
 * spe_extend_begin waits and once more for the entry count; no read overflows.  The piece limits are spe_extend_begin's. */
int spn_map_begin(spx_index *ix, int digest_kind, uint32_t k, uint32_t w, const uint8_t *seqs, const uint64_t *offsets,
                  uint64_t nreads, uint64_t min_length, int want_docs, const spc_params *chain_params,
                  const spa_params *align_params, const spe_params *extend_params, spn_mapping *out_mappings,
                  spa_alignment *out_alignments, uint64_t *n_entries);
int spn_map_fetch(spx_index *ix, uint64_t *out_op_offsets, uint32_t *out_ops);
/* Statistics of the most recent spn_map_* call on ix (synchronises with it). */
int spn_last_map_stats(spx_index *ix, spn_map_stats *out);

#ifdef __cplusplus
}
#endif

#endif /* SPUMONI_MAP_H */
