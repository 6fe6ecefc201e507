/*
 * spumoni_build.h -- C-ABI of the index builder in libspumoni_gpu.so (gfx950).
 *
 * Turns a text into the raw per-run arrays that spx_index_from_runs (spumoni_gpu.h) and the raw run
 * files take: run heads and lengths of the BWT, thresholds, SA samples at run starts / ends and the
 * document id of every sample.  The suffix array, LCP array and range minima are computed on the
 * device.
 *
 * Conventions
 *   - errors: NULL or a negative SPX_E* code of spumoni_gpu.h; the message is in spx_last_error().
 *   - there is NO CPU fallback: without a gfx950 device spb_build_from_text fails with SPX_E_NODEVICE.
 *   - limits: 1 <= n_text < 2^32 - 1 (positions are 32-bit), every text byte >= 2 (0 and 1 are the
 *     terminator), 1 <= n_docs <= 65535 and the document lengths sum to n_text.
 *   - a build that does not fit in the device's free memory is refused before anything is allocated;
 *     the message names the bytes needed and the bytes free.
 *
 * The output is that of the specification in spumoni_amd/synth.py (index_from_text): a terminator 0 is
 * appended (n = n_text + 1, its run's head is 0); thr[k] is the first arg-min of the LCP over (end of
 * the previous run of the same letter, start of run k], 0 for the first run of a letter; ssa / esa are
 * (SA[start] - 1) mod n and (SA[end] - 1) mod n; a sample's document id is the number of cumulative
 * document ends at or below it, the last document absorbing the terminator.
 */
#ifndef SPUMONI_BUILD_H
#define SPUMONI_BUILD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spb_build spb_build;

/* text: host bytes >= 2, no terminator; doc_lengths NULL => one document.  All device memory is released before
 * this returns (the result is held in host memory) so that spx_index_from_runs has the device to itself. */
spb_build *spb_build_from_text(const uint8_t *text, uint64_t n_text, const uint64_t *doc_lengths,
                               uint32_t n_docs, int with_samples, int device);
/* n = n_text + 1, r = runs of the BWT */
int spb_build_stats(const spb_build *b, uint64_t *n, uint64_t *r);
/* r values into each array that is not NULL; ssa .. doc_end need a build with samples (SPX_E_ARG otherwise) */
int spb_build_copy(const spb_build *b, uint8_t *heads, uint64_t *lens, uint64_t *thr, uint64_t *ssa,
                   uint64_t *esa, uint64_t *doc_start, uint64_t *doc_end);
void spb_build_free(spb_build *b);

#ifdef __cplusplus
}
#endif

#endif /* SPUMONI_BUILD_H */
