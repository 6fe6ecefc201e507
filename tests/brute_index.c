/* brute_index.c -- the index of a text from first principles, for the tests of the index builder.
 *
 * Plain C99, nothing from the product or the oracle.  The suffix array is qsort over the suffixes themselves (memcmp
 * over the common length, then the shorter suffix first), the LCP array is counted character by character, and every
 * field of the index is restated over those two arrays with loops:
 *
 *   runs      maximal runs of equal characters of BWT[i] = T[SA[i] - 1] (wrapping to T[n - 1]); heads, lens
 *   thr[k]    0 for a letter's first run; otherwise the first position of the smallest LCP in
 *             (end of the previous run of the same letter, start of run k]
 *   ssa, esa  SA - 1 at the run's first / last position, wrapping to n - 1
 *   doc ids   the number of document ends <= the sample, the last end counted one later (it takes the terminator)
 *
 * T is the text plus one terminator byte 0, n = n_text + 1.  Text bytes must be >= 2.
 *
 * tests/brute.py compiles this file into a shared object and calls brute_index through ctypes; with
 * -DBRUTE_INDEX_MAIN it is a stand-alone program over a few built-in texts (run under ASan / UBSan by
 * tests/test_build_spec_cpu.py). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static const uint8_t* g_t; /* the text with its terminator, for the comparator */
static uint64_t g_n;

static int cmp_suffix(const void* pa, const void* pb) {
    const uint64_t a = *(const uint32_t*)pa, b = *(const uint32_t*)pb;
    const uint64_t la = g_n - a, lb = g_n - b;
    const int c = memcmp(g_t + a, g_t + b, la < lb ? la : lb);
    if (c) return c;
    return la < lb ? -1 : la > lb ? 1 : 0;
}

/* Every output array has room for n = n_text + 1 entries; *r_out of them are filled (sa and lcp: all n).
 * doc_lengths may be NULL: doc_start / doc_end are then left alone.  Returns 0, or -1 for a bad argument or no memory. */
int brute_index(const uint8_t* text, uint64_t n_text, const uint64_t* doc_lengths, uint32_t n_docs, uint32_t* sa,
                uint32_t* lcp, uint64_t* r_out, uint8_t* heads, uint64_t* lens, uint64_t* thr, uint64_t* ssa,
                uint64_t* esa, uint64_t* doc_start, uint64_t* doc_end) {
    const uint64_t n = n_text + 1;
    if (!text || n_text == 0 || n >= 0xffffffffull) return -1;
    for (uint64_t i = 0; i < n_text; ++i)
        if (text[i] < 2) return -1;
    uint8_t* t = (uint8_t*)malloc(n);
    uint8_t* bwt = (uint8_t*)malloc(n);
    uint64_t* starts = (uint64_t*)malloc(n * sizeof(uint64_t));
    uint32_t* doc_at = doc_lengths ? (uint32_t*)malloc(n * sizeof(uint32_t)) : NULL;
    int rc = -1;
    if (!t || !bwt || !starts || (doc_lengths && !doc_at)) goto out;
    memcpy(t, text, n_text);
    t[n - 1] = 0;

    for (uint64_t i = 0; i < n; ++i) sa[i] = (uint32_t)i;
    g_t = t;
    g_n = n;
    qsort(sa, n, sizeof(uint32_t), cmp_suffix);

    lcp[0] = 0;
    for (uint64_t i = 1; i < n; ++i) {
        const uint64_t a = sa[i - 1], b = sa[i];
        uint64_t l = 0;
        while (a + l < n && b + l < n && t[a + l] == t[b + l]) ++l;
        lcp[i] = (uint32_t)l;
    }

    for (uint64_t i = 0; i < n; ++i) bwt[i] = t[sa[i] ? sa[i] - 1 : n - 1];
    uint64_t r = 0;
    for (uint64_t i = 0; i < n; ++i)
        if (i == 0 || bwt[i] != bwt[i - 1]) starts[r++] = i;

    if (doc_lengths) { /* the document of every text position: ends passed so far */
        uint64_t end = 0, sum = 0;
        uint32_t d = 0;
        if (n_docs == 0) goto out;
        for (uint32_t k = 0; k < n_docs; ++k) sum += doc_lengths[k];
        if (sum != n_text) goto out;
        end = doc_lengths[0] + (n_docs == 1 ? 1 : 0);
        for (uint64_t p = 0; p < n; ++p) {
            while (d < n_docs && end <= p) {
                ++d;
                if (d < n_docs) end += doc_lengths[d] + (d + 1 == n_docs ? 1 : 0);
            }
            doc_at[p] = d;
        }
    }

    int64_t last_end[256];
    for (int c = 0; c < 256; ++c) last_end[c] = -1;
    for (uint64_t k = 0; k < r; ++k) {
        const uint64_t s = starts[k], e = (k + 1 < r ? starts[k + 1] : n) - 1;
        const uint8_t c = bwt[s];
        heads[k] = c;
        lens[k] = e - s + 1;
        if (last_end[c] < 0) {
            thr[k] = 0;
        } else {
            uint64_t best = (uint64_t)last_end[c] + 1;
            for (uint64_t i = best + 1; i <= s; ++i)
                if (lcp[i] < lcp[best]) best = i;
            thr[k] = best;
        }
        last_end[c] = (int64_t)e;
        ssa[k] = sa[s] ? (uint64_t)sa[s] - 1 : n - 1;
        esa[k] = sa[e] ? (uint64_t)sa[e] - 1 : n - 1;
        if (doc_lengths) {
            doc_start[k] = doc_at[ssa[k]];
            doc_end[k] = doc_at[esa[k]];
        }
    }
    *r_out = r;
    rc = 0;
out:
    free(t);
    free(bwt);
    free(starts);
    free(doc_at);
    return rc;
}

#ifdef BRUTE_INDEX_MAIN
static uint64_t mix(uint64_t h, uint64_t v) { return (h ^ v) * 0x100000001b3ull; }

static int run(const char* name, const uint8_t* text, uint64_t n_text, const uint64_t* docs, uint32_t n_docs,
               uint64_t* sum) {
    const uint64_t n = n_text + 1;
    uint32_t* sa = (uint32_t*)malloc(n * 4);
    uint32_t* lcp = (uint32_t*)malloc(n * 4);
    uint8_t* heads = (uint8_t*)malloc(n);
    uint64_t* f[6];
    uint64_t r = 0;
    for (int i = 0; i < 6; ++i) f[i] = (uint64_t*)calloc(n, 8);
    const int rc = brute_index(text, n_text, docs, n_docs, sa, lcp, &r, heads, f[0], f[1], f[2], f[3], f[4], f[5]);
    if (rc == 0) {
        uint64_t h = 0xcbf29ce484222325ull;
        for (uint64_t i = 0; i < n; ++i) h = mix(mix(h, sa[i]), lcp[i]);
        for (uint64_t k = 0; k < r; ++k) {
            h = mix(h, heads[k]);
            for (int i = 0; i < (docs ? 6 : 4); ++i) h = mix(h, f[i][k]);
        }
        printf("%-12s n %llu r %llu checksum %016llx\n", name, (unsigned long long)n, (unsigned long long)r,
               (unsigned long long)h);
        *sum = mix(*sum, h);
    } else {
        printf("%-12s refused\n", name);
    }
    free(sa);
    free(lcp);
    free(heads);
    for (int i = 0; i < 6; ++i) free(f[i]);
    return rc;
}

int main(void) {
    enum { BIG = 20000 };
    uint8_t* buf = (uint8_t*)malloc(BIG);
    uint64_t* docs = (uint64_t*)malloc(BIG * sizeof(uint64_t));
    uint64_t sum = 0, x = 88172645463325252ull;
    int bad = 0;
    if (!buf || !docs) return 2;

    const char* banana = "GATTACAGATTACACATTAG";
    const uint64_t two[2] = {7, 13};
    bad |= run("gattaca", (const uint8_t*)banana, strlen(banana), two, 2, &sum);
    bad |= run("gattaca/none", (const uint8_t*)banana, strlen(banana), NULL, 0, &sum);

    buf[0] = 255;
    const uint64_t one[1] = {1};
    bad |= run("single", buf, 1, one, 1, &sum);

    memset(buf, 65, 3000);
    const uint64_t edge[4] = {0, 2999, 0, 1}; /* empty documents in front and inside */
    bad |= run("one letter", buf, 3000, edge, 4, &sum);

    for (int i = 0; i < 4001; ++i) buf[i] = (i & 1) ? 255 : 2;
    bad |= run("period 2", buf, 4001, NULL, 0, &sum);

    for (int i = 0; i < BIG; ++i) { /* xorshift DNA, every character a document */
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        buf[i] = (uint8_t)"ACGT"[x & 3];
        docs[i] = 1;
    }
    bad |= run("dna", buf, BIG, docs, BIG, &sum);

    buf[5] = 1; /* a byte below 2 is refused, nothing is read past the text */
    if (run("bad byte", buf, 100, NULL, 0, &sum) != -1) bad = 1;

    free(buf);
    free(docs);
    if (bad) {
        printf("brute index FAILED\n");
        return 1;
    }
    printf("brute index ok %016llx\n", (unsigned long long)sum);
    return 0;
}
#endif
