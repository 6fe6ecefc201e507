// spx_reftext.hip -- reference text preparation (include/spumoni_reftext.h): FASTA bytes -> the text `spumoni build`
// indexes, on one gfx950 device.  The output is that of read_fasta + main in spumoni_amd/build_index.py,
// with the reference's complement table.
//
// Everything is parallel over bytes (a chromosome may be one line of 2.5e8 characters).  The line structure is two small
// automata: forward, the state before a byte (line start / header line / sequence line with nothing kept yet / sequence
// line past its first non-blank byte); backward, whether a non-blank byte follows in the same line.  A byte's transition
// is a function on the states (a byte), functions compose associatively, so
//   pass 0  every tile of 4096 bytes composes its bytes' functions (block scan over the 16-byte runs of its threads);
//   scan    one block turns the tiles' functions into every tile's entry states;
//   pass 1  with the entry states known each byte knows whether it is kept and whether a sequence starts there: per
//           tile counts, exclusive sums over the tiles;
//   pass 2  the same, now writing the kept bytes compacted (case preserved) and the start of every sequence candidate
//           (a file start or a header line) in the kept stream;
//   then    candidates with no kept byte are dropped, and one pass writes every sequence upper-cased and its reverse
//           complement; the digestion, when asked for, is the library's own (launch_digest) over all pieces at once.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/spumoni_reftext.h"
#include "spx_internal.h"

struct spr_text {
    uint32_t n_files = 0;
    std::vector<uint8_t> text, fwd;
    std::vector<uint64_t> file_len, seq_ends;
    std::vector<uint32_t> seq_file;
    std::vector<uint8_t> names;       // the sequences' names back to back (spr_text_names)
    std::vector<uint64_t> name_ends;  // their cumulative ends
};

namespace spx {
namespace {

constexpr int RT = 256;                       // threads per block
constexpr int PER = 16;                       // bytes per thread
constexpr uint64_t TILE = (uint64_t)RT * PER;  // bytes per tile
constexpr int SCAN_T = 1024;                  // threads of the tile-state scan

// forward states
constexpr uint32_t S_LS = 0, S_HDR = 1, S_NONE = 2, S_SEEN = 3;
// forward transition functions: f(s) = (F >> 2s) & 3
constexpr uint32_t F_NL = 0x00;                                            // '\n': everything -> line start
constexpr uint32_t F_GT = S_HDR | S_HDR << 2 | S_SEEN << 4 | S_SEEN << 6;   // '>'
constexpr uint32_t F_WS = S_NONE | S_HDR << 2 | S_NONE << 4 | S_SEEN << 6;  // blank
constexpr uint32_t F_CH = S_SEEN | S_HDR << 2 | S_SEEN << 4 | S_SEEN << 6;  // anything else
constexpr uint32_t F_ID = 0 | 1 << 2 | 2 << 4 | 3 << 6;
// backward functions on {0, 1} ("a non-blank byte follows in the line"): g(r) = (G >> r) & 1
constexpr uint32_t G_ID = 2, G_0 = 0, G_1 = 3;

__device__ __forceinline__ bool blank(uint32_t c) { return c == ' ' || (c >= 9 && c <= 13); }
__device__ __forceinline__ uint32_t fwd_fn(uint32_t c) { return c == '\n' ? F_NL : c == '>' ? F_GT : blank(c) ? F_WS : F_CH; }
__device__ __forceinline__ uint32_t bwd_fn(uint32_t c) { return c == '\n' ? G_0 : blank(c) ? G_ID : G_1; }
__device__ __forceinline__ uint32_t fapply(uint32_t f, uint32_t s) { return (f >> (2 * s)) & 3; }
__device__ __forceinline__ uint32_t gapply(uint32_t g, uint32_t r) { return (g >> r) & 1; }
__device__ __forceinline__ uint32_t fcomp(uint32_t g, uint32_t f) {  // g after f
    uint32_t r = 0;
    for (uint32_t s = 0; s < 4; ++s) r |= fapply(g, fapply(f, s)) << (2 * s);
    return r;
}
__device__ __forceinline__ uint32_t gcomp(uint32_t g, uint32_t f) {  // g after f
    return gapply(g, gapply(f, 0)) | gapply(g, gapply(f, 1)) << 1;
}
__device__ __forceinline__ uint8_t upper(uint8_t c) { return (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c; }
// the seqtk table of the reference (src/refbuilder.cpp): upper case only reaches it here
__device__ __forceinline__ uint8_t comp(uint8_t c) {
    switch (c) {
        case 'A': return 'T';
        case 'T': return 'A';
        case 'U': return 'A';
        case 'C': return 'G';
        case 'G': return 'C';
        case 'R': return 'Y';
        case 'Y': return 'R';
        case 'K': return 'M';
        case 'M': return 'K';
        case 'B': return 'V';
        case 'V': return 'B';
        case 'D': return 'H';
        case 'H': return 'D';
        case '`': return '@';
        default: return c;
    }
}

struct ParseArgs {
    const uint8_t* in;
    uint64_t n;
    const uint64_t* file_ends;
    uint32_t n_files;
    uint8_t* tile_f;           // pass 0 out: forward function of each tile
    uint8_t* tile_g;           // pass 0 out: backward function of each tile
    const uint8_t* fin;        // passes 1, 2: forward state entering each tile
    const uint8_t* bin;        // passes 1, 2: backward state after each tile
    uint64_t* tile_kept;       // pass 1 out / pass 2 in (exclusive sums)
    uint64_t* tile_brk;
    uint8_t* kept;             // pass 2 out
    uint64_t* cand_start;      // pass 2 out: kept bytes before each candidate
    uint32_t* cand_file;
    unsigned long long* bad;   // pass 2: first input position of a kept byte 0, 1 or >= 128
};

// Hillis-Steele inclusive scan over the block's threads of a (non-commutative) composition; `right` scans from the
// last thread down.  Returns the exclusive value.
template <class Op>
__device__ uint32_t block_scan_fn(uint32_t* sh, uint32_t v, uint32_t id, bool right, Op op) {
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < RT; d <<= 1) {
        uint32_t x = v;
        if (!right && t >= d) x = op(v, sh[t - d]);
        if (right && t + d < RT) x = op(v, sh[t + d]);
        __syncthreads();
        sh[t] = v = x;
        __syncthreads();
    }
    uint32_t ex = id;
    if (!right && t > 0) ex = sh[t - 1];
    if (right && t + 1 < RT) ex = sh[t + 1];
    __syncthreads();
    return ex;
}
__device__ uint64_t block_excl_sum(uint64_t* sh, uint64_t v) {
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < RT; d <<= 1) {
        const uint64_t x = t >= d ? v + sh[t - d] : v;
        __syncthreads();
        sh[t] = v = x;
        __syncthreads();
    }
    const uint64_t ex = t > 0 ? sh[t - 1] : 0;
    __syncthreads();
    return ex;
}

template <int PASS>
__global__ void __launch_bounds__(RT) k_parse(const ParseArgs a) {
    __shared__ uint32_t shf[RT];
    __shared__ uint64_t shu[RT];
    const uint64_t tile = blockIdx.x;
    const uint64_t lo = tile * TILE + (uint64_t)threadIdx.x * PER;
    const uint64_t hi = lo + PER < a.n ? lo + PER : a.n;
    // per byte of the thread: file start / last byte of its file
    uint32_t fs = 0, fl = 0, f = 0;
    uint8_t c[PER];
    if (lo < a.n) {
        uint32_t l = 0, h = a.n_files;  // first file whose end is above lo
        while (l < h) {
            const uint32_t m = (l + h) / 2;
            if (a.file_ends[m] > lo) h = m;
            else l = m + 1;
        }
        f = l;
        uint32_t ff = f;
        for (uint64_t i = lo; i < hi; ++i) {
            while (a.file_ends[ff] <= i) ++ff;
            const uint64_t start = ff ? a.file_ends[ff - 1] : 0;
            const uint32_t j = (uint32_t)(i - lo);
            fs |= (uint32_t)(i == start) << j;
            fl |= (uint32_t)(i + 1 == a.file_ends[ff]) << j;
            c[j] = a.in[i];
        }
    }
    const uint32_t nb = lo < a.n ? (uint32_t)(hi - lo) : 0;
    uint32_t F = F_ID, G = G_ID;
    for (uint32_t j = 0; j < nb; ++j) {
        uint32_t fj = fwd_fn(c[j]);
        if ((fs >> j) & 1) fj = fapply(fj, S_LS) * 0x55u;  // entered from a line start whatever came before
        F = fcomp(fj, F);
    }
    for (uint32_t j = nb; j-- > 0;) {
        uint32_t gj = bwd_fn(c[j]);
        if ((fl >> j) & 1) gj = gapply(gj, 0) * 3u;  // nothing follows in the line
        G = gcomp(gj, G);
    }
    const uint32_t Fx = block_scan_fn(shf, F, F_ID, false, [](uint32_t v, uint32_t prev) { return fcomp(v, prev); });
    const uint32_t Gx = block_scan_fn(shf, G, G_ID, true, [](uint32_t v, uint32_t next) { return gcomp(v, next); });
    if (PASS == 0) {
        if (threadIdx.x == RT - 1) a.tile_f[tile] = (uint8_t)fcomp(F, Fx);
        if (threadIdx.x == 0) a.tile_g[tile] = (uint8_t)gcomp(G, Gx);
        return;
    }
    uint32_t s = fapply(Fx, a.fin[tile]);
    uint32_t r = gapply(Gx, a.bin[tile]);  // after the thread's last byte
    uint32_t follow = 0;                    // bit j: a non-blank byte follows byte j in its line
    for (uint32_t j = nb; j-- > 0;) {
        if ((fl >> j) & 1) r = 0;
        follow |= r << j;
        r = gapply(bwd_fn(c[j]), r);
    }
    uint32_t keep = 0, brk = 0;
    for (uint32_t j = 0; j < nb; ++j) {
        if ((fs >> j) & 1) s = S_LS;
        const uint32_t ch = c[j];
        const bool hs = s == S_LS && ch == '>';
        const bool in_header = hs || s == S_HDR;
        const bool k = !in_header && ch != '\n' && (!blank(ch) || (s == S_SEEN && ((follow >> j) & 1)));
        keep |= (uint32_t)k << j;
        brk |= (uint32_t)(hs || ((fs >> j) & 1)) << j;
        s = fapply(fwd_fn(ch), s);
    }
    if (PASS == 1) {
        const uint64_t kc = __popc(keep), bc = __popc(brk);
        const uint64_t kx = block_excl_sum(shu, kc);
        const uint64_t bx = block_excl_sum(shu, bc);
        if (threadIdx.x == RT - 1) {
            a.tile_kept[tile] = kx + kc;
            a.tile_brk[tile] = bx + bc;
        }
        return;
    }
    uint64_t ko = a.tile_kept[tile] + block_excl_sum(shu, __popc(keep));
    uint64_t bo = a.tile_brk[tile] + block_excl_sum(shu, __popc(brk));
    uint32_t ff = f;
    for (uint32_t j = 0; j < nb; ++j) {
        const uint64_t i = lo + j;
        while (a.file_ends[ff] <= i) ++ff;
        if ((brk >> j) & 1) {
            a.cand_start[bo] = ko;
            a.cand_file[bo] = ff;
            ++bo;
        }
        if ((keep >> j) & 1) {
            const uint8_t ch = c[j];
            a.kept[ko++] = ch;
            if (ch < 2 || ch >= 128) atomicMin(a.bad, (unsigned long long)i);
        }
    }
}

// every tile's entry states from the tiles' functions: one block, a contiguous range of tiles per thread
__global__ void __launch_bounds__(SCAN_T) k_tile_states(const uint8_t* tf, const uint8_t* tg, uint64_t ntiles,
                                                        uint8_t* fin, uint8_t* bin) {
    __shared__ uint8_t sf[SCAN_T], sg[SCAN_T], ef[SCAN_T], eg[SCAN_T];
    const uint32_t t = threadIdx.x;
    const uint64_t per = (ntiles + SCAN_T - 1) / SCAN_T;
    const uint64_t lo = t * per < ntiles ? t * per : ntiles;
    const uint64_t hi = lo + per < ntiles ? lo + per : ntiles;
    uint32_t F = F_ID, G = G_ID;
    for (uint64_t i = lo; i < hi; ++i) F = fcomp(tf[i], F);
    for (uint64_t i = hi; i-- > lo;) G = gcomp(tg[i], G);
    sf[t] = (uint8_t)F;
    sg[t] = (uint8_t)G;
    __syncthreads();
    if (t == 0) {
        uint32_t s = S_LS, r = 0;
        for (uint32_t j = 0; j < SCAN_T; ++j) {
            ef[j] = (uint8_t)s;
            s = fapply(sf[j], s);
        }
        for (uint32_t j = SCAN_T; j-- > 0;) {
            eg[j] = (uint8_t)r;
            r = gapply(sg[j], r);
        }
    }
    __syncthreads();
    uint32_t s = ef[t], r = eg[t];
    for (uint64_t i = lo; i < hi; ++i) {
        fin[i] = (uint8_t)s;
        s = fapply(tf[i], s);
    }
    for (uint64_t i = hi; i-- > lo;) {
        bin[i] = (uint8_t)r;
        r = gapply(tg[i], r);
    }
}

// candidates that kept no byte are dropped: flag[c] = 1 for the others (flag[n_cand] = 0)
__global__ void k_seq_flags(const uint64_t* cand_start, uint64_t n_cand, uint64_t* flag) {
    const uint64_t c = blockIdx.x * (uint64_t)RT + threadIdx.x;
    if (c <= n_cand) flag[c] = c < n_cand && cand_start[c + 1] > cand_start[c];
}
__global__ void k_seq_scatter(const uint64_t* cand_start, const uint32_t* cand_file, const uint64_t* flag_ex,
                              uint64_t n_cand, uint64_t* seq_start, uint32_t* seq_file) {
    const uint64_t c = blockIdx.x * (uint64_t)RT + threadIdx.x;
    if (c < n_cand && cand_start[c + 1] > cand_start[c]) {
        seq_start[flag_ex[c]] = cand_start[c];
        seq_file[flag_ex[c]] = cand_file[c];
    }
}

// every sequence upper-cased at text position (rc ? 2 : 1) * start, followed by its reverse complement when rc
__global__ void __launch_bounds__(RT) k_text(const uint8_t* kept, uint64_t n_kept, const uint64_t* seq_start,
                                             uint64_t n_seqs, int rc, uint8_t* text) {
    const uint64_t lo = (blockIdx.x * (uint64_t)RT + threadIdx.x) * PER;
    if (lo >= n_kept) return;
    const uint64_t hi = lo + PER < n_kept ? lo + PER : n_kept;
    uint64_t l = 0, h = n_seqs;  // last sequence starting at or before lo
    while (h - l > 1) {
        const uint64_t m = (l + h) / 2;
        if (seq_start[m] <= lo) l = m;
        else h = m;
    }
    uint64_t q = l;
    for (uint64_t p = lo; p < hi; ++p) {
        while (seq_start[q + 1] <= p) ++q;
        const uint64_t s = seq_start[q], len = seq_start[q + 1] - s;
        const uint8_t ch = upper(kept[p]);
        if (rc) {
            text[2 * s + (p - s)] = ch;
            text[2 * s + len + (len - 1 - (p - s))] = comp(ch);
        } else {
            text[p] = ch;
        }
    }
}

// the pieces as reads for the digestion: a sequence, then (rc) its reverse complement
__global__ void k_piece_offs(const uint64_t* seq_start, uint64_t n_seqs, int rc, uint64_t* offs) {
    const uint64_t q = blockIdx.x * (uint64_t)RT + threadIdx.x;
    if (q > n_seqs) return;
    const uint64_t s = seq_start[q];
    if (!rc) {
        offs[q] = s;
        return;
    }
    offs[2 * q] = 2 * s;
    if (q < n_seqs) offs[2 * q + 1] = 2 * s + (seq_start[q + 1] - s);
}

// ---- driver ------------------------------------------------------------------------------------------------------

struct Mem {
    uint64_t cur = 0, peak = 0;
};
struct Buf {  // RAII device buffer that counts itself in a Mem
    Mem* m = nullptr;
    void* p = nullptr;
    size_t bytes = 0;
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { release(); }
    hipError_t alloc(Mem& mem, size_t b) {
        release();
        m = &mem;
        hipError_t e = hipMalloc(&p, b ? b : 1);
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        bytes = b ? b : 1;
        m->cur += bytes;
        if (m->cur > m->peak) m->peak = m->cur;
        return hipSuccess;
    }
    void release() {
        if (p) {
            (void)hipFree(p);
            m->cur -= bytes;
        }
        p = nullptr;
        bytes = 0;
    }
    template <class T>
    T* as() const {
        return (T*)p;
    }
};
struct Stream {
    hipStream_t s = nullptr;
    ~Stream() {
        if (s) (void)hipStreamDestroy(s);
    }
};
struct IndexHandle {  // a minimal index: the digestion's scratch and character hashes live in one
    spx_index* ix = nullptr;
    ~IndexHandle() {
        if (ix) spx_index_free(ix);
    }
};
struct Timer {
    bool on;
    hipStream_t st;
    std::chrono::steady_clock::time_point t0;
    int phase(const char* name, const std::string& extra, uint64_t cur_bytes) {
        if (!on) return SPX_OK;
        SPX_HIP(hipStreamSynchronize(st));
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[spr] %-10s %9.1f ms  device %.3f GB%s%s\n", name,
                std::chrono::duration<double, std::milli>(t1 - t0).count(), cur_bytes / 1e9, extra.empty() ? "" : "  ",
                extra.c_str());
        t0 = t1;
        return SPX_OK;
    }
};

inline unsigned nblk(uint64_t m) { return (unsigned)((m + RT - 1) / RT); }

int excl_sum(uint64_t* v, uint64_t count, Buf& tmp, Mem& mem, hipStream_t st) {
    size_t tb = 0;
    SPX_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, v, v, count, st));
    if (tmp.bytes < tb) SPX_HIP(tmp.alloc(mem, tb));
    SPX_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, v, v, count, st));
    return SPX_OK;
}

// the message of a refused byte: the file, and the sequence by its header (host bytes: an error path only)
void refuse_byte(const uint8_t* bytes, const uint64_t* file_ends, uint32_t n_files, uint64_t pos) {
    uint32_t f = 0;
    while (f + 1 < n_files && file_ends[f] <= pos) ++f;
    const uint64_t start = f ? file_ends[f - 1] : 0;
    std::string name = "(the lines before the first header)";
    for (uint64_t i = pos; i > start;) {  // the header line above pos, if any
        const uint8_t* nl = (const uint8_t*)memrchr(bytes + start, '\n', i - start);
        const uint64_t ls = nl ? (uint64_t)(nl - bytes) + 1 : start;
        if (bytes[ls] == '>' && ls < pos) {
            uint64_t e = ls + 1;
            while (e < file_ends[f] && bytes[e] != '\n' && bytes[e] != '\r' && e - ls < 80) ++e;
            name = "'" + std::string((const char*)bytes + ls, (const char*)bytes + e) + "'";
            break;
        }
        if (!nl) break;
        i = ls - 1;
    }
    set_error("file #%u, sequence %s: byte 0x%02x at offset %llu of the file; bytes 0, 1 and >= 128 are not accepted",
              f, name.c_str(), (unsigned)bytes[pos], (unsigned long long)(pos - start));
}

// The names of the sequences that kept a byte, in the order of the parse, from the host's copy of the input (one memchr
// per line; a sequence line is looked at until its first kept byte): a header's bytes behind '>' up to the first ASCII
// whitespace; seq<k>, k the sequence's 1-based ordinal over all files, for an empty name and for the lines before a
// file's first header.  The line rules are the parse's: a line ends at '\n', a line whose first byte is '>' is a header,
// a file's start and end delimit like a header, a sequence keeps a byte when one of its lines has a non-blank byte.
void sequence_names(spr_text& R, const uint8_t* bytes, const uint64_t* file_ends, uint32_t n_files) {
    auto is_blank = [](uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); };
    uint64_t ordinal = 0;
    for (uint32_t f = 0; f < n_files; ++f) {
        const uint64_t end = file_ends[f];
        uint64_t pos = f ? file_ends[f - 1] : 0, h0 = 0, h1 = 0;  // [h0, h1): the open sequence's header behind '>'
        bool kept = false;
        auto close = [&]() {
            if (!kept) return;
            ++ordinal;
            uint64_t e = h0;
            while (e < h1 && !is_blank(bytes[e])) ++e;
            if (e > h0) {
                R.names.insert(R.names.end(), bytes + h0, bytes + e);
            } else {
                const std::string name = "seq" + std::to_string(ordinal);
                R.names.insert(R.names.end(), name.begin(), name.end());
            }
            R.name_ends.push_back(R.names.size());
        };
        while (pos < end) {
            const uint8_t* nl = (const uint8_t*)memchr(bytes + pos, '\n', end - pos);
            const uint64_t le = nl ? (uint64_t)(nl - bytes) : end;
            if (bytes[pos] == '>') {
                close();
                h0 = pos + 1;
                h1 = le;
                kept = false;
            } else if (!kept) {
                for (uint64_t i = pos; i < le && !kept; ++i) kept = !is_blank(bytes[i]);
            }
            pos = le + 1;
        }
        close();
    }
}

int too_long(uint64_t n_text, uint64_t max_text) {
    set_error("the text has %llu characters, more than max_text (%llu)", (unsigned long long)n_text,
              (unsigned long long)max_text);
    return SPX_E_UNSUPPORTED;
}

int prepare(spr_text& R, const uint8_t* bytes, uint64_t n, const uint64_t* file_ends, uint32_t n_files, int rc,
            int kind, uint32_t k, uint32_t w, uint64_t max_text, int device) {
    Mem mem;
    Stream S;
    SPX_HIP(hipStreamCreateWithFlags(&S.s, hipStreamNonBlocking));
    hipStream_t st = S.s;
    Timer tm{getenv("SPX_TIMING") != nullptr, st, std::chrono::steady_clock::now()};
    const uint64_t ntiles = (n + TILE - 1) / TILE;

    // ---- memory, before anything is allocated: parsing holds the input, the kept bytes and the tile arrays; the text
    // phase the kept bytes, the text and (digestion) its output and the digestion's scratch
    const uint64_t U = rc ? 2 * n : n;  // the most the undigested text can be
    const uint64_t textb = (U + 15) / 16 * 16 + 32;
    uint64_t dig = 0;
    if (kind) {
        const uint64_t chunks = U / 240 + U / 2 + 2;  // (pieces: at most one per two input bytes)
        dig = spx_digest_capacity(kind, k, U) + (U + 64) * 5 / 4 + chunks * 20 * 5 / 4 + U / 2 * 32 + U / 4096 * 48;
    }
    const uint64_t p1 = (n + 16) + n + ntiles * 24 + (64ull << 20);
    const uint64_t p2 = n + textb + dig + (64ull << 20);
    const uint64_t need = std::max(p1, p2) + (64ull << 20);
    size_t fr = 0, tot = 0;
    SPX_HIP(hipMemGetInfo(&fr, &tot));
    if (need > fr) {
        set_error("preparing %llu input bytes does not fit on the device: it needs %llu bytes of device memory, "
                  "%llu bytes are free (of %llu)",
                  (unsigned long long)n, (unsigned long long)need, (unsigned long long)fr, (unsigned long long)tot);
        return SPX_E_ARG;
    }

    Buf IN, FE, TF, TG, FIN, BIN, TK, TB, BAD, KEPT, CS, CF, tmp;
    uint64_t n_kept = 0, n_cand = 0;
    SPX_HIP(IN.alloc(mem, n + 16));
    SPX_HIP(FE.alloc(mem, 8ull * n_files));
    SPX_HIP(hipMemcpyAsync(IN.p, bytes, n, hipMemcpyHostToDevice, st));
    SPX_HIP(hipMemcpyAsync(FE.p, file_ends, 8ull * n_files, hipMemcpyHostToDevice, st));
    if (int rc2 = tm.phase("upload", std::to_string(n) + " bytes, " + std::to_string(n_files) + " files", mem.cur))
        return rc2;
    if (ntiles) {
        SPX_HIP(TF.alloc(mem, ntiles));
        SPX_HIP(TG.alloc(mem, ntiles));
        SPX_HIP(FIN.alloc(mem, ntiles));
        SPX_HIP(BIN.alloc(mem, ntiles));
        SPX_HIP(TK.alloc(mem, 8 * (ntiles + 1)));
        SPX_HIP(TB.alloc(mem, 8 * (ntiles + 1)));
        SPX_HIP(BAD.alloc(mem, 8));
        SPX_HIP(hipMemsetAsync(TK.p, 0, 8 * (ntiles + 1), st));
        SPX_HIP(hipMemsetAsync(TB.p, 0, 8 * (ntiles + 1), st));
        SPX_HIP(hipMemsetAsync(BAD.p, 0xff, 8, st));
        ParseArgs a{};
        a.in = IN.as<uint8_t>();
        a.n = n;
        a.file_ends = FE.as<uint64_t>();
        a.n_files = n_files;
        a.tile_f = TF.as<uint8_t>();
        a.tile_g = TG.as<uint8_t>();
        a.fin = FIN.as<uint8_t>();
        a.bin = BIN.as<uint8_t>();
        a.tile_kept = TK.as<uint64_t>();
        a.tile_brk = TB.as<uint64_t>();
        a.bad = BAD.as<unsigned long long>();
        k_parse<0><<<(unsigned)ntiles, RT, 0, st>>>(a);
        SPX_HIP(hipGetLastError());
        k_tile_states<<<1, SCAN_T, 0, st>>>(a.tile_f, a.tile_g, ntiles, FIN.as<uint8_t>(), BIN.as<uint8_t>());
        SPX_HIP(hipGetLastError());
        k_parse<1><<<(unsigned)ntiles, RT, 0, st>>>(a);
        SPX_HIP(hipGetLastError());
        if (int e = excl_sum(a.tile_kept, ntiles + 1, tmp, mem, st)) return e;
        if (int e = excl_sum(a.tile_brk, ntiles + 1, tmp, mem, st)) return e;
        SPX_HIP(hipMemcpyAsync(&n_kept, a.tile_kept + ntiles, 8, hipMemcpyDeviceToHost, st));
        SPX_HIP(hipMemcpyAsync(&n_cand, a.tile_brk + ntiles, 8, hipMemcpyDeviceToHost, st));
        SPX_HIP(hipStreamSynchronize(st));
        // the candidates' arrays are the only ones sized by the records, not the bytes: checked once they are counted
        SPX_HIP(hipMemGetInfo(&fr, &tot));
        if (12 * (n_cand + 1) + (n_kept + 16) + (64ull << 20) > fr) {
            set_error("preparing %llu input bytes does not fit on the device: %llu sequence records need %llu more bytes "
                      "of device memory, %llu bytes are free",
                      (unsigned long long)n, (unsigned long long)n_cand, (unsigned long long)(12 * (n_cand + 1) + n_kept),
                      (unsigned long long)fr);
            return SPX_E_ARG;
        }
        SPX_HIP(KEPT.alloc(mem, n_kept + 16));
        SPX_HIP(CS.alloc(mem, 8 * (n_cand + 1)));
        SPX_HIP(CF.alloc(mem, 4 * (n_cand + 1)));
        a.kept = KEPT.as<uint8_t>();
        a.cand_start = CS.as<uint64_t>();
        a.cand_file = CF.as<uint32_t>();
        k_parse<2><<<(unsigned)ntiles, RT, 0, st>>>(a);
        SPX_HIP(hipGetLastError());
        SPX_HIP(hipMemcpyAsync(a.cand_start + n_cand, &n_kept, 8, hipMemcpyHostToDevice, st));
        unsigned long long bad = 0;
        SPX_HIP(hipMemcpyAsync(&bad, a.bad, 8, hipMemcpyDeviceToHost, st));
        SPX_HIP(hipStreamSynchronize(st));
        if (bad != ~0ull) {
            refuse_byte(bytes, file_ends, n_files, bad);
            return SPX_E_FORMAT;
        }
        // undigested, the text's length is known now: refused before it is made
        if (!kind && max_text && (rc ? 2 * n_kept : n_kept) > max_text) return too_long(rc ? 2 * n_kept : n_kept, max_text);
        if (int rc2 = tm.phase("parse", std::to_string(ntiles) + " tiles, " + std::to_string(n_kept) +
                                            " sequence bytes, " + std::to_string(n_cand) + " records",
                               mem.cur))
            return rc2;
        IN.release();
        FE.release();
        TF.release();
        TG.release();
        FIN.release();
        BIN.release();
        TK.release();
        TB.release();
    }

    // ---- the sequences that kept a byte
    uint64_t n_seqs = 0;
    Buf FL, SS, SF;
    if (n_cand) {
        SPX_HIP(FL.alloc(mem, 8 * (n_cand + 1)));
        k_seq_flags<<<nblk(n_cand + 1), RT, 0, st>>>(CS.as<uint64_t>(), n_cand, FL.as<uint64_t>());
        SPX_HIP(hipGetLastError());
        if (int e = excl_sum(FL.as<uint64_t>(), n_cand + 1, tmp, mem, st)) return e;
        SPX_HIP(hipMemcpyAsync(&n_seqs, FL.as<uint64_t>() + n_cand, 8, hipMemcpyDeviceToHost, st));
        SPX_HIP(hipStreamSynchronize(st));
    }
    SPX_HIP(SS.alloc(mem, 8 * (n_seqs + 1)));
    SPX_HIP(SF.alloc(mem, 4 * (n_seqs + 1)));
    if (n_seqs)
        k_seq_scatter<<<nblk(n_cand), RT, 0, st>>>(CS.as<uint64_t>(), CF.as<uint32_t>(), FL.as<uint64_t>(), n_cand,
                                                   SS.as<uint64_t>(), SF.as<uint32_t>());
    SPX_HIP(hipGetLastError());
    SPX_HIP(hipMemcpyAsync(SS.as<uint64_t>() + n_seqs, &n_kept, 8, hipMemcpyHostToDevice, st));
    R.fwd.resize(n_kept);
    R.seq_ends.resize(n_seqs + 1);
    R.seq_file.resize(n_seqs);
    if (n_kept) SPX_HIP(hipMemcpyAsync(R.fwd.data(), KEPT.p, n_kept, hipMemcpyDeviceToHost, st));
    SPX_HIP(hipMemcpyAsync(R.seq_ends.data(), SS.p, 8 * (n_seqs + 1), hipMemcpyDeviceToHost, st));
    if (n_seqs) SPX_HIP(hipMemcpyAsync(R.seq_file.data(), SF.p, 4 * n_seqs, hipMemcpyDeviceToHost, st));
    SPX_HIP(hipStreamSynchronize(st));
    FL.release();
    CS.release();
    CF.release();

    // ---- text: every sequence and (rc) its reverse complement
    const uint64_t n_und = rc ? 2 * n_kept : n_kept;
    const uint64_t npieces = rc ? 2 * n_seqs : n_seqs;
    Buf TXT, OFFS;
    SPX_HIP(TXT.alloc(mem, (n_und + 15) / 16 * 16 + 32));
    SPX_HIP(hipMemsetAsync(TXT.p, 0, TXT.bytes, st));
    SPX_HIP(OFFS.alloc(mem, 8 * (npieces + 1)));
    if (n_kept) {
        k_text<<<nblk((n_kept + PER - 1) / PER), RT, 0, st>>>(KEPT.as<uint8_t>(), n_kept, SS.as<uint64_t>(), n_seqs, rc,
                                                               TXT.as<uint8_t>());
        SPX_HIP(hipGetLastError());
    }
    k_piece_offs<<<nblk(n_seqs + 1), RT, 0, st>>>(SS.as<uint64_t>(), n_seqs, rc, OFFS.as<uint64_t>());
    SPX_HIP(hipGetLastError());
    if (int rc2 = tm.phase("text", std::to_string(n_seqs) + " sequences, " + std::to_string(n_und) + " characters",
                           mem.cur))
        return rc2;
    KEPT.release();
    SS.release();
    SF.release();

    std::vector<uint64_t> piece_offs(npieces + 1);
    if (kind && npieces) {
        IndexHandle H;
        const uint8_t head = 0;
        const uint64_t len1 = 1, thr0 = 0;
        H.ix = spx_index_from_runs(&head, &len1, &thr0, 1, nullptr, nullptr, nullptr, nullptr, 0, device);
        if (!H.ix) return SPX_E_HIP;
        const uint64_t cap = spx_digest_capacity(kind, k, n_und);
        Buf OUT, OOFF;
        SPX_HIP(OUT.alloc(mem, cap));
        SPX_HIP(OOFF.alloc(mem, 8 * (npieces + 1)));
        if (int e = launch_digest(H.ix, kind, k, w, TXT.as<uint8_t>(), OFFS.as<uint64_t>(), npieces, n_und,
                                  OUT.as<uint8_t>(), OOFF.as<uint64_t>(), st))
            return e;
        SPX_HIP(hipMemcpyAsync(piece_offs.data(), OOFF.p, 8 * (npieces + 1), hipMemcpyDeviceToHost, st));
        SPX_HIP(hipStreamSynchronize(st));
        // the digestion's scratch lives in the index handle, not in `mem`: counted into the peak here
        uint64_t scr = 0;
        for (int i = 0; i < spx_index::NDIGSCR; ++i) scr += H.ix->digest_scr[i].cap;
        mem.peak = std::max(mem.peak, mem.cur + scr);
        if (max_text && piece_offs[npieces] > max_text) return too_long(piece_offs[npieces], max_text);
        if (int rc2 = tm.phase("digest", std::to_string(npieces) + " pieces -> " + std::to_string(piece_offs[npieces]) +
                                             " characters",
                               mem.cur))
            return rc2;
        TXT.release();
        R.text.resize(piece_offs[npieces]);
        if (!R.text.empty()) SPX_HIP(hipMemcpyAsync(R.text.data(), OUT.p, R.text.size(), hipMemcpyDeviceToHost, st));
        SPX_HIP(hipStreamSynchronize(st));
    } else {
        SPX_HIP(hipMemcpyAsync(piece_offs.data(), OFFS.p, 8 * (npieces + 1), hipMemcpyDeviceToHost, st));
        R.text.resize(n_und);
        if (n_und) SPX_HIP(hipMemcpyAsync(R.text.data(), TXT.p, n_und, hipMemcpyDeviceToHost, st));
        SPX_HIP(hipStreamSynchronize(st));
    }
    R.file_len.assign(n_files, 0);
    for (uint64_t q = 0; q < npieces; ++q) R.file_len[R.seq_file[rc ? q / 2 : q]] += piece_offs[q + 1] - piece_offs[q];
    R.seq_ends.erase(R.seq_ends.begin());
    if (int rc2 = tm.phase("download", std::to_string(R.text.size()) + " text characters", mem.cur)) return rc2;
    if (tm.on)
        fprintf(stderr, "[spr] input %llu bytes -> text %llu characters, peak device %llu bytes (%.2f B/input byte)\n",
                (unsigned long long)n, (unsigned long long)R.text.size(), (unsigned long long)mem.peak,
                n ? (double)mem.peak / (double)n : 0.0);
    return SPX_OK;
}

}  // namespace
}  // namespace spx

using namespace spx;

extern "C" {

spr_text* spr_text_from_fasta(const uint8_t* bytes, uint64_t n_bytes, const uint64_t* file_ends, uint32_t n_files,
                              int rev_comp, int digest_kind, uint32_t k, uint32_t w, uint64_t max_text, int device) {
    if (select_device(device) != SPX_OK) return nullptr;
    if ((!bytes && n_bytes) || !file_ends || n_files == 0) {
        set_error("bytes / file_ends are null or there are no files");
        return nullptr;
    }
    for (uint32_t i = 0; i < n_files; ++i) {
        if ((i && file_ends[i] < file_ends[i - 1]) || file_ends[i] > n_bytes) {
            set_error("file_ends must be non-decreasing and at most n_bytes");
            return nullptr;
        }
    }
    if (file_ends[n_files - 1] != n_bytes) {
        set_error("the last file must end at n_bytes");
        return nullptr;
    }
    if (digest_kind != 0 && digest_kind != SPX_DIGEST_PROMOTED && digest_kind != SPX_DIGEST_DNA) {
        set_error("digest kind must be 0, SPX_DIGEST_PROMOTED (-m) or SPX_DIGEST_DNA (-a)");
        return nullptr;
    }
    if (digest_kind && (k < 1 || k > 4 || w < k)) {
        set_error("minimizer windows: k must be in [1, 4] and w at least k");
        return nullptr;
    }
    spr_text* t = new (std::nothrow) spr_text;
    if (!t) {
        set_error("out of host memory");
        return nullptr;
    }
    t->n_files = n_files;
    int rc;
    try {
        rc = prepare(*t, bytes, n_bytes, file_ends, n_files, rev_comp != 0, digest_kind, k, w, max_text, device);
    } catch (const std::bad_alloc&) {
        set_error("out of host memory");
        rc = SPX_E_ARG;
    }
    if (rc == SPX_OK) {
        try {
            sequence_names(*t, bytes, file_ends, n_files);
        } catch (const std::bad_alloc&) {
            set_error("out of host memory");
            rc = SPX_E_ARG;
        }
        if (rc == SPX_OK && t->name_ends.size() != t->seq_file.size()) {
            set_error("internal: the headers name %llu sequences, the parse found %llu", (unsigned long long)t->name_ends.size(),
                      (unsigned long long)t->seq_file.size());
            rc = SPX_E_FORMAT;
        }
    }
    if (rc != SPX_OK) {
        delete t;
        return nullptr;
    }
    return t;
}

int spr_text_stats(const spr_text* t, uint64_t* n_text, uint64_t* n_seqs, uint64_t* n_fwd) {
    if (!t) {
        set_error("text is null");
        return SPX_E_ARG;
    }
    if (n_text) *n_text = t->text.size();
    if (n_seqs) *n_seqs = t->seq_file.size();
    if (n_fwd) *n_fwd = t->fwd.size();
    return SPX_OK;
}

int spr_text_copy(const spr_text* t, uint8_t* text, uint64_t* file_text_lengths, uint8_t* fwd, uint64_t* seq_ends,
                  uint32_t* seq_file) {
    if (!t) {
        set_error("text is null");
        return SPX_E_ARG;
    }
    if (text && !t->text.empty()) memcpy(text, t->text.data(), t->text.size());
    if (file_text_lengths) memcpy(file_text_lengths, t->file_len.data(), 8ull * t->n_files);
    if (fwd && !t->fwd.empty()) memcpy(fwd, t->fwd.data(), t->fwd.size());
    if (seq_ends && !t->seq_ends.empty()) memcpy(seq_ends, t->seq_ends.data(), 8 * t->seq_ends.size());
    if (seq_file && !t->seq_file.empty()) memcpy(seq_file, t->seq_file.data(), 4 * t->seq_file.size());
    return SPX_OK;
}

int spr_text_names(const spr_text* t, uint8_t* names, uint64_t* name_ends, uint64_t* n_name_bytes) {
    if (!t) {
        set_error("text is null");
        return SPX_E_ARG;
    }
    if (names && !t->names.empty()) memcpy(names, t->names.data(), t->names.size());
    if (name_ends && !t->name_ends.empty()) memcpy(name_ends, t->name_ends.data(), 8 * t->name_ends.size());
    if (n_name_bytes) *n_name_bytes = t->names.size();
    return SPX_OK;
}

void spr_text_free(spr_text* t) { delete t; }

}  // extern "C"
