/*
 * spumoni_reftext.h -- C-ABI of the reference text preparation in libspumoni_gpu.so (gfx950).
 *
 * Turns the bytes of FASTA files into the text `spumoni build` indexes: every sequence upper-cased (ASCII a-z),
 * followed by its reverse complement unless rev_comp is 0, each of the two pieces digested on its own when a
 * digestion is asked for.  Parsing, compaction, the reverse complement and the digestion run on the device
 * (DESIGN.md 4.8); the specification is read_fasta and main of spumoni_amd/build_index.py:
 *   - a line ends at '\n'; a line whose first byte is '>' is a header, every other line is a sequence line with its
 *     leading and trailing ASCII whitespace (space, \t, \n, \r, \v, \f) removed, whitespace inside it kept;
 *   - headers and file starts delimit the sequences; lines before a file's first header form a sequence; a file's
 *     end closes its last sequence; empty sequences are dropped;
 *   - the complement is the seqtk table of the reference (src/refbuilder.cpp): A<->T, C<->G, R<->Y, K<->M, B<->V,
 *     D<->H, U->A; every other byte below 128 maps to itself except '`', which the table maps to '@'.  For A, C,
 *     G, T and N this is synth.revcomp; synth.revcomp maps the other IUPAC codes to 0, so build_index.py refuses
 *     what this accepts.
 *
 * Conventions
 *   - errors: NULL or a negative SPX_E* code of spumoni_gpu.h; the message is in spx_last_error().
 *   - there is NO CPU fallback: without a gfx950 device spr_text_from_fasta fails with SPX_E_NODEVICE.
 *   - a sequence byte 0, 1 or >= 128 is refused (SPX_E_FORMAT); the message starts "file #<i>" (0-based) and names
 *     the sequence by its header.
 *   - 64-bit offsets throughout: the input and the undigested text may exceed 2^32.
 *   - the byte-proportional device buffers are checked against the device's free memory before anything is
 *     allocated (the message names the bytes needed and free); all device memory is released before a call
 *     returns, the results are held in host memory.
 *   - SPX_TIMING=1 in the environment prints per-phase times and the peak device bytes ("[spr]" lines).
 */
#ifndef SPUMONI_REFTEXT_H
#define SPUMONI_REFTEXT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spr_text spr_text;

/* bytes: the input files' bytes back to back (already inflated), host memory; file_ends[i]: end of file i in bytes
 * (non-decreasing, file_ends[n_files - 1] == n_bytes).  digest_kind: 0 (none), SPX_DIGEST_PROMOTED or SPX_DIGEST_DNA
 * of spumoni_gpu.h, with k and w as in spx_digest_batch.  max_text (0: no limit): a text longer than this is refused
 * with SPX_E_UNSUPPORTED ("the text has <n> characters, ..."); without digestion before the text is made. */
spr_text *spr_text_from_fasta(const uint8_t *bytes, uint64_t n_bytes, const uint64_t *file_ends, uint32_t n_files,
                              int rev_comp, int digest_kind, uint32_t k, uint32_t w, uint64_t max_text, int device);
/* n_text: characters of the text; n_seqs: non-empty sequences; n_fwd: their characters, case preserved */
int spr_text_stats(const spr_text *t, uint64_t *n_text, uint64_t *n_seqs, uint64_t *n_fwd);
/* Each pointer may be NULL.  text: n_text bytes; file_text_lengths: n_files text characters each file contributes;
 * fwd: the n_fwd sequence bytes as they are in the files (no case change), sequence after sequence; seq_ends: n_seqs
 * cumulative ends of the sequences in fwd; seq_file: n_seqs file numbers. */
int spr_text_copy(const spr_text *t, uint8_t *text, uint64_t *file_text_lengths, uint8_t *fwd, uint64_t *seq_ends,
                  uint32_t *seq_file);
/* The sequences' names, for the sequence table of `spumoni build -s` (spumoni_amd/map.py: sequence_name): a header's
 * bytes behind '>' up to the first ASCII whitespace; seq<k>, k the sequence's 1-based ordinal over all files, for an
 * empty name and for the lines before a file's first header.  Each pointer may be NULL.  n_name_bytes: the bytes of all
 * names together; names: those bytes, name after name; name_ends: n_seqs cumulative ends of the names in `names`. */
int spr_text_names(const spr_text *t, uint8_t *names, uint64_t *name_ends, uint64_t *n_name_bytes);
void spr_text_free(spr_text *t);

#ifdef __cplusplus
}
#endif

#endif /* SPUMONI_REFTEXT_H */
