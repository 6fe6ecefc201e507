/* brute_ms.c -- matching statistics from first principles, for the tests of the query path.
 *
 * Plain C99, nothing from the product or the oracle.  ms[i] of a read is the length of the longest prefix of
 * read[i:] that occurs somewhere in the text.  It is found by binary search for read[i:] over the suffix array of the
 * text (the `sa` of brute_index.c: n_text + 1 entries, the empty suffix first), comparing character by character: the
 * longest common prefix with any suffix is the one with a neighbour of the place where read[i:] would be inserted.
 *
 * Two things keep long matches affordable; neither changes what is searched:
 *   - a comparison starts at min(lcp with the lower bound, lcp with the upper bound): every suffix between two that
 *     share d characters with the pattern shares them too;
 *   - the occurrence found for position i - 1, moved one to the right, still matches ms[i - 1] - 1 characters.  It is
 *     extended directly, and since it then sorts before or behind read[i:], it serves as one bound of the search:
 *     whatever matches longer lies on the other side of it, and all of that side is searched.
 *
 * tests/brute.py compiles this file into a shared object and calls brute_ms through ctypes; with -DBRUTE_MS_MAIN it is
 * a stand-alone program over a few built-in inputs (run under ASan / UBSan by tests/test_ms_math_cpu.py). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* Characters that pat[0 .. m) and the suffix text[s .. n_text) have in common, counted from `from` (which the caller
 * knows to be common); *greater = 1 iff the pattern sorts behind the suffix (the suffix ended, or its next character
 * is smaller), 0 iff the pattern is a prefix of the suffix or sorts before it. */
static uint64_t common(const uint8_t* text, uint64_t n_text, uint64_t s, const uint8_t* pat, uint64_t m, uint64_t from,
                       int* greater) {
    uint64_t d = from;
    while (d < m && s + d < n_text && pat[d] == text[s + d]) ++d;
    if (d == m)
        *greater = 0;
    else if (s + d == n_text)
        *greater = 1;
    else
        *greater = pat[d] > text[s + d];
    return d;
}

/* ms[offs[q] + i] for every read q and position i.  sa: the suffix array of text + terminator, n_text + 1 entries.
 * Returns 0, or -1 for a bad argument (sa is no permutation of 0 .. n_text, offsets that fall) or no memory. */
int brute_ms(const uint8_t* text, uint64_t n_text, const uint32_t* sa, const uint8_t* seqs, const uint64_t* offs,
             uint64_t nreads, uint32_t* ms) {
    const uint64_t n = n_text + 1;
    if (!text || !sa || !offs || n >= 0xffffffffull) return -1;
    uint32_t* isa = (uint32_t*)malloc(n * sizeof(uint32_t));
    if (!isa) return -1;
    memset(isa, 0xff, n * sizeof(uint32_t));
    for (uint64_t k = 0; k < n; ++k) {
        if (sa[k] >= n || isa[sa[k]] != 0xffffffffu) {
            free(isa);
            return -1;
        }
        isa[sa[k]] = (uint32_t)k;
    }
    for (uint64_t q = 0; q < nreads; ++q) {
        if (offs[q + 1] < offs[q]) {
            free(isa);
            return -1;
        }
        const uint8_t* read = seqs + offs[q];
        const uint64_t m = offs[q + 1] - offs[q];
        uint64_t at = 0, have = 0; /* text[at .. at + have) == read[i .. i + have): the previous answer, shifted */
        for (uint64_t i = 0; i < m; ++i) {
            const uint8_t* pat = read + i;
            const uint64_t pm = m - i;
            int64_t lo = -1, hi = (int64_t)n; /* suffix lo sorts before the pattern, suffix hi does not */
            uint64_t llcp = 0, rlcp = 0, lat = 0, rat = 0;
            int greater;
            if (have > 0) {
                const uint64_t d = common(text, n_text, at, pat, pm, have, &greater);
                if (greater) {
                    lo = isa[at];
                    llcp = d;
                    lat = at;
                } else {
                    hi = isa[at];
                    rlcp = d;
                    rat = at;
                }
            }
            while (hi - lo > 1 && rlcp < pm) {
                const int64_t mid = lo + (hi - lo) / 2;
                const uint64_t d = common(text, n_text, sa[mid], pat, pm, llcp < rlcp ? llcp : rlcp, &greater);
                if (greater) {
                    lo = mid;
                    llcp = d;
                    lat = sa[mid];
                } else {
                    hi = mid;
                    rlcp = d;
                    rat = sa[mid];
                }
            }
            const uint64_t best = llcp > rlcp ? llcp : rlcp;
            ms[offs[q] + i] = (uint32_t)best;
            at = (llcp > rlcp ? lat : rat) + 1;
            have = best ? best - 1 : 0;
        }
    }
    free(isa);
    return 0;
}

#ifdef BRUTE_MS_MAIN
static const uint8_t* g_t;
static uint64_t g_n_text;

static int cmp_suffix(const void* pa, const void* pb) {
    const uint64_t a = *(const uint32_t*)pa, b = *(const uint32_t*)pb;
    const uint64_t la = g_n_text - a, lb = g_n_text - b;
    const int c = memcmp(g_t + a, g_t + b, la < lb ? la : lb);
    if (c) return c;
    return la < lb ? -1 : la > lb ? 1 : 0;
}

/* the definition itself: try every text position */
static uint32_t slow_ms(const uint8_t* text, uint64_t n_text, const uint8_t* pat, uint64_t m) {
    uint64_t best = 0;
    for (uint64_t s = 0; s < n_text; ++s) {
        uint64_t d = 0;
        while (d < m && s + d < n_text && pat[d] == text[s + d]) ++d;
        if (d > best) best = d;
    }
    return (uint32_t)best;
}

static int run(const char* name, const uint8_t* text, uint64_t n_text, const uint8_t* seqs, const uint64_t* offs,
               uint64_t nreads, uint64_t* sum) {
    const uint64_t n = n_text + 1, tot = offs[nreads];
    uint32_t* sa = (uint32_t*)malloc(n * 4);
    uint32_t* ms = (uint32_t*)malloc((tot + 1) * 4);
    int bad = 0;
    if (!sa || !ms) return 1;
    for (uint64_t i = 0; i < n; ++i) sa[i] = (uint32_t)i;
    g_t = text;
    g_n_text = n_text;
    qsort(sa, n, sizeof(uint32_t), cmp_suffix);
    if (brute_ms(text, n_text, sa, seqs, offs, nreads, ms) != 0) bad = 1;
    uint64_t h = 0xcbf29ce484222325ull, longest = 0;
    for (uint64_t q = 0; q < nreads && !bad; ++q)
        for (uint64_t i = offs[q]; i < offs[q + 1]; ++i) {
            if (ms[i] != slow_ms(text, n_text, seqs + i, offs[q + 1] - i)) bad = 1;
            if (ms[i] > longest) longest = ms[i];
            h = (h ^ ms[i]) * 0x100000001b3ull;
        }
    printf("%-10s n_text %llu reads %llu values %llu longest %llu checksum %016llx%s\n", name,
           (unsigned long long)n_text, (unsigned long long)nreads, (unsigned long long)tot, (unsigned long long)longest,
           (unsigned long long)h, bad ? "  WRONG" : "");
    *sum = (*sum ^ h) * 0x100000001b3ull;
    free(sa);
    free(ms);
    return bad;
}

int main(void) {
    enum { NT = 3000, NR = 2400 };
    uint8_t* text = (uint8_t*)malloc(NT);
    uint8_t* seqs = (uint8_t*)malloc(NR);
    uint64_t offs[16], sum = 0, x = 88172645463325252ull;
    int bad = 0;
    if (!text || !seqs) return 2;

    const char* t0 = "GATTACAGATTACACATTAG";
    const char* r0 = "TTACAGATTAGZGATTACAGATTACACATTAGG";
    const uint64_t o0[5] = {0, 11, 11, 12, 33}; /* an empty read, an absent letter, the whole text and one more */
    bad |= run("gattaca", (const uint8_t*)t0, strlen(t0), (const uint8_t*)r0, o0, 4, &sum);

    memset(text, 65, NT); /* one letter: every position's answer is what is left of the read, or the text's length */
    memset(seqs, 65, NR);
    seqs[700] = 67;
    offs[0] = 0, offs[1] = 1, offs[2] = 900, offs[3] = NR;
    bad |= run("one letter", text, 1000, seqs, offs, 3, &sum);

    for (int i = 0; i < NT; ++i) { /* xorshift DNA with its first 700 characters repeated at 1500 */
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        text[i] = (uint8_t)"ACGT"[x & 3];
    }
    memcpy(text + 1500, text, 700);
    memcpy(seqs, text + 1400, 900);      /* runs into the copy and out of it */
    memcpy(seqs + 900, text + NT - 300, 300); /* the text's last characters, then the batch goes on */
    memcpy(seqs + 1200, text, 1200);
    seqs[1300] ^= 6;
    offs[0] = 0, offs[1] = 900, offs[2] = 1200, offs[3] = 1200, offs[4] = NR;
    bad |= run("dna", text, NT, seqs, offs, 4, &sum);
    bad |= run("dna/short", text, 9, seqs, offs, 4, &sum);

    offs[1] = 0;
    bad |= run("no values", text, NT, seqs, offs, 1, &sum);

    free(text);
    free(seqs);
    if (bad) {
        printf("brute ms FAILED\n");
        return 1;
    }
    printf("brute ms ok %016llx\n", (unsigned long long)sum);
    return 0;
}
#endif
