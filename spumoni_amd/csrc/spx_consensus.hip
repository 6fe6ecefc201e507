// spx_consensus.hip -- the consensus (include/spumoni_consensus.h): per base of every sequence's forward
// strand the byte that the coverage's depth and the pileup's alt, ins and del imply -- kept, substituted, deleted or masked
// --, compacted per sequence and laid out as FASTA body text on the device; and the product's C-ABI.  The kernels read the
// four arrays, the piece starts of the sequence table and the text (the forward piece of sequence s starts at
// P[s * strands]); they change nothing of the ten products before this one.
//
//   count    k_cons_count, a block per tile of 4096 positions, a thread per 16 consecutive ones, as the calls of
//            spx_call.hip.  A thread decides its positions and leaves the emitted byte of each (0: deleted; the text's bytes
//            are >= 2) in `emit` as one 16-byte store.  The five per-sequence counters go into the records: where the tile
//            lies in one sequence the block's sums leave as one set of atomics, where it crosses borders a thread adds what
//            it has at every border it walks across (a tile may hold thousands of one-base sequences).  The tile's letters
//            go to tcnt, the totals to the counters.
//   scans    hipcub's exclusive sum over the tiles' letters; k_cons_pairs makes (letters, body bytes) of every sequence and
//            one exclusive scan of the pairs gives each sequence's first letter rank and its body_start.
//   write    k_cons_write, a block per tile again.  It reads `emit` -- the decision is not made twice --, ranks its letters
//            by a block scan and places letter k of sequence s at body_start[s] + k + k / line_width; the letter in front
//            of a newline writes it.  The bytes of a tile are one contiguous range of the body whatever borders it holds
//            (a sequence's last newline belongs to its last letter): the block stages the range in LDS, shifted so that
//            LDS dwords are the body's aligned dwords, and stores it as lane-contiguous dwords with byte ends.
//
// Control flow: every block-wide scan, sum and __syncthreads stands outside the loops and conditions of a thread's own.
#include "../../include/spumoni_consensus.h"
#include "spx_genome_kernels.h"

namespace spx {
namespace {

struct ConsCounters {  // device; zeroed in front of every launch
    unsigned long long letters, substituted, deleted, masked, ins_sites, bytes;
    unsigned long long error;  // bit 1: the body did not fit body_capacity
};
constexpr int CONS_WORDS = sizeof(ConsCounters) / 8;
constexpr int REC_WORDS = sizeof(sps_seq) / 8;  // body_start, then the five counters in ConsCounters' order
static_assert(REC_WORDS == 6 && CONS_WORDS == 7, "the records' counters follow body_start in the counters' order");

struct Pair {  // of a sequence; behind the scan: of the sequences in front of it
    unsigned long long letters, bytes;
};
struct PairSum {
    __host__ __device__ Pair operator()(const Pair& a, const Pair& b) const { return Pair{a.letters + b.letters, a.bytes + b.bytes}; }
};

struct ConsArgs {
    Table t;
    const uint8_t* text;
    const uint32_t* depth;
    const uint4* alt;
    const uint32_t* ins;
    const uint32_t* del;
    uint32_t min_depth, min_alt, min_permille, line_width, mask;
    uint64_t cap, ntiles;
    unsigned long long* rec;  // REC_WORDS per sequence: sps_seq
    uint4* emit;              // ntiles * TILE bytes
    uint64_t* tcnt;           // ntiles + 1: letters in a tile, then a 0
    uint64_t* toffs;          // ntiles + 1
    Pair* pairs;              // n_seqs + 1: a sequence's letters and bytes, then zeros
    Pair* starts;             // n_seqs + 1
    uint8_t* body;
    uint64_t* count;
    ConsCounters* c;
};

enum : uint32_t { KEPT, SUBSTITUTED, DELETED, MASKED, INS_SITE = 4 };  // a decision: the class, INS_SITE or-ed in

__device__ inline uint32_t code_of(uint8_t b) {  // 0 .. 3 for A/a, C/c, G/g, T/t, 4 for every other byte
    const uint32_t u = b & 0xdfu;
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 4u;
}

// Position p of the forward genome, whose reference byte is ref: the decision, and in *out the emitted byte (0: none)
__device__ inline uint32_t decide(const ConsArgs& a, uint64_t p, uint8_t ref, uint8_t* out) {
    const unsigned long long d = a.depth[p], dl = a.del[p], span = d + dl, share = a.min_permille;
    *out = a.mask ? (uint8_t)a.mask : ref;
    if (span < a.min_depth) return MASKED;
    const unsigned long long in = a.ins[p];
    const uint32_t site = in >= a.min_alt && in * 1000ull >= share * span ? INS_SITE : 0u;
    if (dl >= a.min_alt && dl * 1000ull >= share * span) {
        *out = 0;
        return DELETED | site;
    }
    if (d < a.min_depth) return MASKED | site;
    const uint4 al = a.alt[p];
    const uint32_t rc = code_of(ref), cnt[4] = {al.x, al.y, al.z, al.w};
    uint32_t best = rc == 0 ? 1u : 0u;  // the lowest candidate
#pragma unroll
    for (uint32_t c = 1; c < 4; ++c)
        if (c != rc && c > best && cnt[c] > cnt[best]) best = c;
    if (cnt[best] >= a.min_alt && (unsigned long long)cnt[best] * 1000ull >= share * d) {
        *out = (uint8_t)("ACGT"[best]);
        return SUBSTITUTED | site;
    }
    *out = ref;
    return KEPT | site;
}

__global__ __launch_bounds__(256) void k_cons_count(ConsArgs a) {
    __shared__ unsigned long long part[4 * 5];
    const Tile x = tile_of(a.t.G);
    // (the same for the whole block) the tile's first sequence, and whether the tile ends in it
    const uint64_t s_first = seq_of(a.t, x.t0);
    const bool one = seq_start(a.t, s_first + 1) >= x.t1;
    unsigned long long mine[5] = {}, total[5] = {};  // of the thread's sequence so far; of all its positions
    union {
        uint4 v;
        uint8_t b[PER_THREAD];
    } out;
    out.v = make_uint4(0, 0, 0, 0);
    if (x.p0 < x.p1) {
        uint64_t s = one ? s_first : seq_of(a.t, x.p0), lo = seq_start(a.t, s), hi = seq_start(a.t, s + 1);
        const uint8_t* ref_at = a.text + a.t.P[s * a.t.strands] - lo;  // the reference byte of p is ref_at[p]
        for (uint64_t p = x.p0; p < x.p1; ++p) {
            if (p == hi) {  // (only in a tile of several sequences)
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    if (mine[i]) atomicAdd(a.rec + s * REC_WORDS + 1 + i, mine[i]);
                    mine[i] = 0;
                }
                s += 1;
                lo = hi;
                hi = seq_start(a.t, s + 1);
                ref_at = a.text + a.t.P[s * a.t.strands] - lo;
            }
            const uint8_t ref = ref_at[p];
            uint8_t e;
            const uint32_t dec = decide(a, p, ref, &e);
            out.b[p - x.p0] = e;
            const uint32_t cls = dec & 3u;
            const unsigned long long add[5] = {e != 0, cls == SUBSTITUTED, cls == DELETED, cls == MASKED, (dec & INS_SITE) != 0};
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                mine[i] += add[i];
                total[i] += add[i];
            }
        }
        if (!one) {
#pragma unroll
            for (int i = 0; i < 5; ++i)
                if (mine[i]) atomicAdd(a.rec + s * REC_WORDS + 1 + i, mine[i]);
        }
    }
    a.emit[(uint64_t)blockIdx.x * 256 + threadIdx.x] = out.v;  // (a thread without positions: zeros, no letters)
    // the block's sums: to the counters, to the tile's count and, in a tile of one sequence, to its record
#pragma unroll
    for (int i = 0; i < 5; ++i) total[i] = wave_sum(total[i]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < 5; ++i) part[(threadIdx.x >> 6) * 5 + i] = total[i];
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const unsigned long long sum = part[threadIdx.x] + part[5 + threadIdx.x] + part[10 + threadIdx.x] + part[15 + threadIdx.x];
        if (sum) {
            atomicAdd(&a.c->letters + threadIdx.x, sum);
            if (one) atomicAdd(a.rec + s_first * REC_WORDS + 1 + threadIdx.x, sum);
        }
        if (threadIdx.x == 0) {
            a.tcnt[blockIdx.x] = sum;
            if (blockIdx.x == 0) a.tcnt[a.ntiles] = 0;
        }
    }
}

// A thread per sequence, and one more for the zeros behind the last
__global__ __launch_bounds__(256) void k_cons_pairs(ConsArgs a) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s > a.t.n_seqs) return;
    Pair v{0, 0};
    if (s < a.t.n_seqs) {
        v.letters = a.rec[s * REC_WORDS + 1];
        v.bytes = v.letters + (a.line_width ? (v.letters + a.line_width - 1) / a.line_width : (v.letters > 0));
    }
    a.pairs[s] = v;
}

constexpr uint32_t STAGE_WORDS = 2 * TILE / 4 + 2;  // a newline behind every letter at the most, and the shift

__global__ __launch_bounds__(256) void k_cons_write(ConsArgs a) {
    using Scan = hipcub::BlockScan<uint32_t, 256>;
    __shared__ typename Scan::TempStorage tmp;
    __shared__ uint32_t stage[STAGE_WORDS];
    __shared__ unsigned long long first_at;  // where the tile's first letter goes in the body
    __shared__ uint32_t stage_end;           // the tile's bytes
    uint8_t* const sb = (uint8_t*)stage;
    const Tile x = tile_of(a.t.G);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t total = a.starts[a.t.n_seqs].bytes;
        *a.count = total;
        a.c->bytes = total;
        if (total > a.cap) atomicOr(&a.c->error, 2ull);
    }
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < a.t.n_seqs; s += (uint64_t)gridDim.x * 256)
        a.rec[s * REC_WORDS] = a.starts[s].bytes;
    if (threadIdx.x == 0) {
        first_at = 0;
        stage_end = 0;
    }
    __syncthreads();
    union {
        uint4 v;
        uint8_t b[PER_THREAD];
    } in;
    in.v = a.emit[(uint64_t)blockIdx.x * 256 + threadIdx.x];
    uint32_t mine = 0;
    int j0 = PER_THREAD;  // the thread's first letter
#pragma unroll
    for (int j = PER_THREAD - 1; j >= 0; --j)
        if (in.b[j]) {
            mine += 1;
            j0 = j;
        }
    uint32_t before = 0;
    Scan(tmp).ExclusiveSum(mine, before);
    const uint64_t w = a.line_width;
    // the sequence of the letter in hand: its borders, its letters, where its bytes start; the letter's rank k in it, and
    // k / w and k % w, carried along from letter to letter
    uint64_t s = 0, hi = 0, base = 0, nl = 0, k = 0, q = 0, rem = 0;
    if (mine) {
        s = seq_of(a.t, x.p0 + j0);
        hi = seq_start(a.t, s + 1);
        const Pair here = a.starts[s];
        base = here.bytes;
        nl = a.starts[s + 1].letters - here.letters;
        k = a.toffs[blockIdx.x] + before - here.letters;
        if (w) {
            q = k / w;
            rem = k % w;
        }
        if (before == 0) first_at = base + k + q;
    }
    __syncthreads();
    const uint64_t o0 = first_at;
    const uint32_t shift = (uint32_t)((uintptr_t)(a.body + o0) & 3);
    if (mine) {
        uint32_t end = 0;
        for (int j = j0; j < PER_THREAD; ++j) {
            if (!in.b[j]) continue;
            const uint64_t p = x.p0 + j;
            if (p >= hi) {  // the first letter of a later sequence
                do {
                    s += 1;
                    hi = seq_start(a.t, s + 1);
                } while (p >= hi);
                const Pair here = a.starts[s];
                base = here.bytes;
                nl = a.starts[s + 1].letters - here.letters;
                k = q = rem = 0;
            }
            uint32_t at = shift + (uint32_t)(base + k + q - o0);  // (below 2 * TILE + 3)
            if (at + 2 > STAGE_WORDS * 4) break;  // (never: the scans' sums would have to disagree with `emit`)
            sb[at++] = in.b[j];
            k += 1;
            bool newline = k == nl;
            if (w && ++rem == w) {
                rem = 0;
                q += 1;
                newline = true;
            }
            if (newline) sb[at++] = '\n';
            end = at;
        }
        atomicMax(&stage_end, end);
    }
    __syncthreads();
    // the staged range [shift, end) lies at body + o0 - shift, a dword boundary: whole dwords a lane each, the two ends
    // byte by byte; nothing at or beyond body_capacity
    uint64_t end = stage_end;
    if (end <= shift || o0 >= a.cap) return;
    if (end - shift > a.cap - o0) end = shift + (a.cap - o0);
    uint8_t* const dst = a.body + o0 - shift;
    for (uint32_t i = threadIdx.x; (uint64_t)i * 4 < end; i += 256) {
        const uint32_t b0 = i * 4;
        if (b0 >= shift && (uint64_t)b0 + 4 <= end) {
            ((uint32_t*)dst)[i] = stage[i];
        } else {
            for (uint32_t b = b0 < shift ? shift : b0; b < b0 + 4 && b < end; ++b) dst[b] = sb[b];
        }
    }
}

int check_params(const sps_params* p) {
    if (!p) {
        set_error("params must be non-null");
        return SPX_E_ARG;
    }
    if (p->min_depth < 1 || p->min_alt < 1 || p->min_permille > 1000) {
        set_error("min_depth and min_alt must be at least 1 and min_permille between 0 and 1000 (they are %u, %u, %u)", p->min_depth,
                  p->min_alt, p->min_permille);
        return SPX_E_ARG;
    }
    if (p->line_width > 0x7fffffffu) {
        set_error("line_width must be between 0 and 2147483647 (it is %u)", p->line_width);
        return SPX_E_ARG;
    }
    return SPX_OK;
}

void fill_params(ConsArgs& a, const sps_params& p) {
    a.min_depth = p.min_depth;
    a.min_alt = p.min_alt;
    a.min_permille = p.min_permille;
    a.line_width = p.line_width;
    a.mask = p.mask;
}

// The scratch of a call and, on st, `count`: the records zeroed, the count kernel (step 0) and the scans (step 1), the
// product left open behind them; `write`: the write kernel (step 2) and the product closed.  The host form sizes its body
// between the two.  Takes ix->mu.
int cons_enqueue(spx_index* ix, ConsArgs& a, hipStream_t st, bool count, bool write) {
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    a.t = table_of(ix);
    a.text = ix->text;
    a.ntiles = tiles_of(a.t.G);
    const uint64_t nseq1 = a.t.n_seqs + 1;
    spx_index::Scratch* scr = ix->cons_scr;
    void* p = nullptr;
    int rc;
    if ((rc = scr[spx_index::CS_EMIT].reserve(a.ntiles * TILE, &p)) != SPX_OK) return rc;
    a.emit = (uint4*)p;
    if ((rc = scr[spx_index::CS_TCNT].reserve((a.ntiles + 1) * 8, &p)) != SPX_OK) return rc;
    a.tcnt = (uint64_t*)p;
    if ((rc = scr[spx_index::CS_TOFFS].reserve((a.ntiles + 1) * 8, &p)) != SPX_OK) return rc;
    a.toffs = (uint64_t*)p;
    if ((rc = scr[spx_index::CS_PAIRS].reserve(nseq1 * sizeof(Pair), &p)) != SPX_OK) return rc;
    a.pairs = (Pair*)p;
    if ((rc = scr[spx_index::CS_STARTS].reserve(nseq1 * sizeof(Pair), &p)) != SPX_OK) return rc;
    a.starts = (Pair*)p;
    spx_index::Product& pr = ix->cons;
    if (count) {
        size_t tile_bytes = 0, pair_bytes = 0;
        SPX_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tile_bytes, a.tcnt, a.toffs, a.ntiles + 1, (hipStream_t) nullptr));
        SPX_HIP(hipcub::DeviceScan::ExclusiveScan(nullptr, pair_bytes, a.pairs, a.starts, PairSum(), Pair{0, 0}, nseq1, (hipStream_t) nullptr));
        void *cub = nullptr, *cub2 = nullptr;
        if ((rc = scr[spx_index::CS_CUB].reserve(tile_bytes + 16, &cub)) != SPX_OK) return rc;
        if ((rc = scr[spx_index::CS_CUB2].reserve(pair_bytes + 16, &cub2)) != SPX_OK) return rc;
        if ((rc = product_open(pr, CONS_WORDS, st, 0, &p)) != SPX_OK) return rc;
        a.c = (ConsCounters*)p;
        ix->cons_G = a.t.G;
        SPX_HIP(hipMemsetAsync(a.rec, 0, a.t.n_seqs * sizeof(sps_seq), st));
        k_cons_count<<<(unsigned)a.ntiles, 256, 0, st>>>(a);
        SPX_HIP(hipGetLastError());
        if ((rc = product_mark(pr, 1, st)) != SPX_OK) return rc;
        SPX_HIP(hipcub::DeviceScan::ExclusiveSum(cub, tile_bytes, a.tcnt, a.toffs, a.ntiles + 1, st));
        k_cons_pairs<<<(unsigned)((nseq1 + 255) / 256), 256, 0, st>>>(a);
        SPX_HIP(hipGetLastError());
        SPX_HIP(hipcub::DeviceScan::ExclusiveScan(cub2, pair_bytes, a.pairs, a.starts, PairSum(), Pair{0, 0}, nseq1, st));
        if ((rc = product_mark(pr, -1, st)) != SPX_OK) return rc;
    }
    if (!write) return SPX_OK;
    a.c = (ConsCounters*)pr.counters.p;
    if ((rc = product_mark(pr, 2, st)) != SPX_OK) return rc;
    k_cons_write<<<(unsigned)a.ntiles, 256, 0, st>>>(a);
    SPX_HIP(hipGetLastError());
    return product_close(pr, st);
}

void cons_reset(spx_index* ix) {
    product_reset(ix, ix->cons);
    std::lock_guard<std::mutex> g(ix->mu);
    ix->cons_ready = false;
}

}  // namespace

void release_consensus(spx_index* ix) { release(ix->cons_scr, spx_index::CS_COUNT, &ix->cons); }

void consensus_table_changed(spx_index* ix) {
    // (a kernel of an earlier call may still read the old table)
    if (ix->cons.have && ix->cons.ev1) (void)hipEventSynchronize(ix->cons.ev1);
    ix->cons_ready = false;
}

}  // namespace spx

using namespace spx;

extern "C" {

int sps_consensus_device(spx_index* ix, const uint32_t* d_depth, const uint32_t* d_alt, const uint32_t* d_ins, const uint32_t* d_del,
                         const sps_params* params, uint64_t body_capacity, sps_seq* d_records, uint8_t* d_body, uint64_t* d_count,
                         void* stream) {
    int rc;
    if ((rc = need_table(ix, "sps_consensus_device")) != SPX_OK) return rc;
    if (!d_depth || !d_alt || !d_ins || !d_del || !d_records || !d_count || (body_capacity && !d_body)) {
        set_error("d_depth, d_alt, d_ins, d_del, d_records, d_body and d_count must be non-null");
        return SPX_E_ARG;
    }
    if (((uintptr_t)d_alt & 15) != 0 || (((uintptr_t)d_records | (uintptr_t)d_count) & 7) != 0 ||
        (((uintptr_t)d_depth | (uintptr_t)d_ins | (uintptr_t)d_del) & 3) != 0) {
        set_error("d_alt must be 16-byte aligned, d_records and d_count 8-byte, d_depth, d_ins and d_del 4-byte aligned");
        return SPX_E_ARG;
    }
    if ((rc = check_params(params)) != SPX_OK) return rc;
    cons_reset(ix);
    ConsArgs a{};
    a.depth = d_depth;
    a.alt = (const uint4*)d_alt;
    a.ins = d_ins;
    a.del = d_del;
    fill_params(a, *params);
    a.cap = body_capacity;
    a.rec = (unsigned long long*)d_records;
    a.body = d_body;
    a.count = d_count;
    return cons_enqueue(ix, a, (hipStream_t)stream, true, true);
}

int sps_consensus_begin(spx_index* ix, const sps_params* params, uint64_t* n_bytes) {
    if (!ix || !n_bytes) {
        set_error("index and n_bytes must be non-null");
        return SPX_E_ARG;
    }
    *n_bytes = 0;
    std::lock_guard<std::mutex> hg(ix->host_mu);
    int rc;
    if ((rc = call_arrays_ready(ix, "sps_consensus_begin")) != SPX_OK) return rc;
    if ((rc = check_params(params)) != SPX_OK) return rc;
    SPX_HIP(hipSetDevice(ix->device));
    cons_reset(ix);
    if ((rc = cover_finish_host(ix)) != SPX_OK || (rc = call_finish_arrays(ix)) != SPX_OK) return rc;
    hipStream_t st = nullptr;
    if ((rc = ctx_stream_of(ix, &st)) != SPX_OK) return rc;
    const uint64_t n_seqs = ix->map_seq_lengths.size();
    ConsArgs a{};
    a.depth = (const uint32_t*)ix->cover.scr[spx_index::D_DEPTH].p;
    a.alt = (const uint4*)ix->call.scr[spx_index::PL_ALT].p;
    a.ins = (const uint32_t*)ix->call.scr[spx_index::PL_INS].p;
    a.del = (const uint32_t*)ix->call.scr[spx_index::PL_DEL].p;
    fill_params(a, *params);
    void* p = nullptr;
    if ((rc = ix->cons_scr[spx_index::CS_RECORDS].reserve(n_seqs * sizeof(sps_seq), &p)) != SPX_OK) return rc;
    a.rec = (unsigned long long*)p;
    if ((rc = ix->cons_scr[spx_index::CS_NOUT].reserve(8, &p)) != SPX_OK) return rc;
    a.count = (uint64_t*)p;
    // count and scans, the one wait of the body's own, the body at its exact size, write
    if ((rc = cons_enqueue(ix, a, st, true, false)) != SPX_OK) return rc;
    if ((rc = ctx_wait(ix, st)) != SPX_OK) return rc;
    Pair total{0, 0};
    SPX_HIP(hipMemcpy(&total, a.starts + n_seqs, sizeof total, hipMemcpyDeviceToHost));
    if ((rc = ix->cons_scr[spx_index::CS_BODY].reserve(total.bytes + 16, &p)) != SPX_OK) return rc;
    a.body = (uint8_t*)p;
    a.cap = total.bytes;
    if ((rc = cons_enqueue(ix, a, st, false, true)) != SPX_OK) return rc;
    if ((rc = ctx_wait(ix, st)) != SPX_OK) return rc;
    if ((rc = product_collect(ix, ix->cons, CONS_WORDS, CONS_WORDS - 1)) != SPX_OK) return rc;
    ix->cons_ready = true;
    ix->cons_seqs = n_seqs;
    ix->cons_bytes = total.bytes;
    *n_bytes = total.bytes;
    return SPX_OK;
}

int sps_consensus_fetch(spx_index* ix, sps_seq* out_records, uint8_t* out_body) {
    if (!ix) {
        set_error("index must be non-null");
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> hg(ix->host_mu);
    if (!ix->cons_ready) {
        set_error("sps_consensus_fetch without a successful sps_consensus_begin before it");
        return SPX_E_ARG;
    }
    if (!out_records || (ix->cons_bytes && !out_body)) {
        set_error("out_records and out_body must be non-null");
        return SPX_E_ARG;
    }
    ix->cons_ready = false;
    SPX_HIP(hipSetDevice(ix->device));
    SPX_HIP(hipMemcpy(out_records, ix->cons_scr[spx_index::CS_RECORDS].p, ix->cons_seqs * sizeof(sps_seq), hipMemcpyDeviceToHost));
    if (ix->cons_bytes) SPX_HIP(hipMemcpy(out_body, ix->cons_scr[spx_index::CS_BODY].p, ix->cons_bytes, hipMemcpyDeviceToHost));
    return SPX_OK;
}

int sps_last_consensus_stats(spx_index* ix, sps_consensus_stats* out) {
    if (!ix || !out) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    spx_index::Product& p = ix->cons;
    if (!p.have) {
        set_error("no consensus has been computed on this index yet");
        return SPX_E_ARG;
    }
    if (p.pending) {
        const int rc = product_collect(ix, p, CONS_WORDS, CONS_WORDS - 1);
        if (rc != SPX_OK) return rc;
    }
    std::memset(out, 0, sizeof *out);
    out->positions = ix->cons_G;
    out->letters = p.acc[0];
    out->substituted = p.acc[1];
    out->deleted = p.acc[2];
    out->masked = p.acc[3];
    out->ins_sites = p.acc[4];
    out->bytes = p.acc[5];
    out->kept = out->letters - out->substituted - out->masked;
    out->overflow = (uint32_t)((p.error >> 1) & 1);
    for (int i = 0; i < 3; ++i) out->step_ms[i] = p.step_ms[i];
    return SPX_OK;
}

}  // extern "C"
