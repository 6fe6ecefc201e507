// spx_walk_fast.inc -- k_walk_fast: the plain walk (reads, not chunks) over compact rows (Row32), written for the
// instruction stream.  Included by spx_walk.hip inside namespace spx { namespace { ... } }.
//
// What is computed is pml_pointers::_query / ms_pointers::_query (/root/reference/src/compute_ms_pml.cpp:238-340,
// 571-682), exactly as k_walk_lanes<MODE, DOC, true, NARROW, 0> computes it (that kernel stays for the general row
// encoding and the chunked walk's fallback, reads the rows' first 16 bytes only, and is what this one is held
// against in the tests: SPX_OLD_WALK=1).
//
// Why a second body.  Since the rows carry their likeliest destination (spx_layout.h, Row32) the walk needs fewer
// than one gather per character, and what bounds it is no longer the memory system but the instructions around
// each gather: the state machine of k_walk_lanes compiles to ~1800 instructions of which a third are exec-mask
// bookkeeping for ~80 divergent regions and a sixth are copies at their joins (every lane-level `bool` lives as a
// 64-bit lane mask in scalar registers, spilled to VGPR lanes when they run out).  Here
//   * every per-lane flag is a bit of ONE vector register (`fl`), and what a lane has to do next inside an
//     iteration a bit of another (`act`);
//   * the row a lane stands on stays packed in the registers it was loaded into (q0, q1); the embedded row is only
//     looked at in the iteration that fetched it (it is the second half of that gather), so it is not loop state;
//   * one (k, off) pair: where the lane stands, or -- while its gather is in flight -- where it lands;
//   * the walk counters are wave-level (ballot + popcount in scalar registers), the loop's exit is wave-uniform;
//   * the address of a lane's next gather is computed where the phase is decided, not by a phase switch at the
//     load: the iteration opens with `load 16 (+16) bytes at addr` for every lane;
//   * a landing whose head is known (from the row before it, or from the jump row) is not a phase of its own: the
//     lane "stands" on a row of which it has only the head (F_NOROW), and STEP sends it on to the fat slot when
//     the next character differs, or back for the row when it does not;
//   * STEP and EMIT are straight-line select code, run up to STEP_REPS times per gather (two LF steps per
//     gather when a step ends in the embedded run; the peek after each).
// Phases: Q_LAND (row of run k0), Q_FAT (fat slot; with MS samples / document ids their Aux record is the slot's
// second half and rides in the same gather), Q_STEP (nothing to fetch), and the rare ones -- Q_READ, Q_CHARS,
// Q_FATJ, Q_QS, Q_DIR, Q_SAMP (samples_start / start_runs_doc of the run a byte >= 128 stays on) -- which share
// one switch.

enum : uint32_t { Q_LAND = 0, Q_FAT = 1, Q_STEP = 2, Q_READ = 3, Q_CHARS = 4, Q_FATJ = 5, Q_QS = 6, Q_DIR = 7, Q_DONE = 8, Q_SAMP = 9, Q_START = 10, Q_WANT = 11 };
enum : uint32_t {
    F_EMB = 1,     // this iteration's gather brought the row of run LFrun along (the lane landed on a row from memory)
    F_NOROW = 2,   // the lane stands on (k, off) knowing only the head of run k (low byte of q1)
    F_QUIRK = 4,   // the jump started on a run whose head is the character itself (byte >= 128, thr_ok unset)
    F_WIDE = 16,   // the next gather is 32 bytes
    F_FADD = 32,   // the jump is looking at the slot after its block's (FAT_SINGLE)
    F_HAVEC = 64,  // the step is repeated with the character it already has (it went back for its row)
    F_SAMPD = 128  // ... and has the sample / document id of the run it stays on (Q_SAMP)
};
enum : uint32_t { A_STEP = 1, A_EMIT = 2, A_DECIDE = 4 };
#ifndef SPX_STEP_REPS
#define SPX_STEP_REPS 2
#endif
constexpr int STEP_REPS = SPX_STEP_REPS;
constexpr uint32_t OFF_LAST32 = 0xffffffffu;
// reads a wavefront takes from the batch's claim word at a time (BatchArgs::claim): 64 / 128 / 256 measured alike on the
// headline batch (profiles/dynamic_deal_ab.txt); the smallest leaves the least ragged end
#ifndef SPX_CHUNK_CLAIM
#define SPX_CHUNK_CLAIM 64
#endif
constexpr uint32_t CHUNK_CLAIM = SPX_CHUNK_CLAIM;
static_assert(CHUNK_CLAIM >= 64, "a claim covers at least one iteration's worst case: 64 lanes ending a read each");

// the value of the lane beside this one (lanes 2j and 2j + 1 exchange): DPP quad_perm [1, 0, 3, 2]
__device__ __forceinline__ uint32_t dpp_swap1(uint32_t v) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, true); }

struct alignas(16) HotLetter {  // what STEP needs of a letter, one ds_read_b128
    uint32_t bmul;     // fat block of run k = umulhi(k, bmul)
    uint32_t present;  // number_of_letter(c) != 0
    uint64_t fat0;     // address of the letter's first fat slot
};

// the same LF target as lf_target_c, plus what the walk knows about the landing before any gather: t_out = t when the
// step ends exactly in run LFrun + t (the bounding cum is a true value: t < 4 and off below the saturation mark),
// 4 otherwise
__device__ __forceinline__ void lf_target_ct(uint32_t LFrun, uint32_t LFoff, uint32_t cums, uint32_t off, uint32_t& k0,
                                             uint32_t& offp, uint32_t& t_out) {
    lf_target_c(LFrun, LFoff, cums, off, k0, offp);
    const uint32_t t = k0 - LFrun;
    t_out = (t < 4 && off <= 126) ? t : 4u;
}

// CHUNK: 0 = reads; 1 = pass 1 of the chunked walk of long-read batches (spx_internal.h): the work items are chunks,
// every chunk is walked from the default state, and besides the results the walk records a checkpoint every 16
// characters, the state at the chunk's lower end and one flag byte per character -- exactly what
// k_walk_lanes<..., 1> records; 2 = pass 2: a chunk is entered with the recorded end state of the chunk above it (Q_START)
// and walked, its results written one value at a time over the speculative ones, until the walk stands where the
// speculative walk stood at the same character -- asked at every checkpoint, whose record was fetched sixteen characters
// ahead -- or the chunk ends; what k_walk_lanes<..., 2> does, at one gather per character instead of that kernel's two or
// three in a row.
// EARLY: the next iteration's gather is issued right after the repetitions, ahead of the iteration's output flushes -- for
// launches that do not fill the chip (few long reads, the chunked walk's share, pass 2), where a wavefront's time is its
// own latency chain (gather + ~400 dependent instructions an iteration): -6 % there, and +1 % on full launches, which
// therefore keep the gather at the top of the iteration (profiles/r04_early_gather.txt).
// How the items are dealt.  By striding (a lane's next item is nlanes after its last) everywhere but in the plain walk of a
// batch with more reads than lanes (DYN; BatchArgs::claim is the word: CHUNK == 0, not EARLY).  There only the first round is strided;
// after it a lane that ends a read (Q_WANT) is handed the next index of its WAVEFRONT's reservoir -- up to two ranges of
// read indices in scalar registers, handed out by ballot + mbcnt once per iteration, after the repetitions -- and the
// wavefront refills the reservoir ahead of need with one atomicAdd(claim, CHUNK_CLAIM) by one lane, issued together with
// an iteration's gather and looked at after that gather has returned (like side_in / side_doc / side_aux), so nobody ever
// waits for the atomic alone.  Reads cost unequally (one that matches takes ~35 iterations, a random one ~48): under
// striding a lane's total is a draw, a wavefront runs as long as its slowest lane and the launch as long as its slowest
// wavefront (DESIGN.md 4.1, profiles/mix_penalty_before.txt).  Which lane walks which read is not observable.
// How the results leave (PML).  Everywhere but below: when a lane has the reset bits of 64 characters (or its read ends) the
// wavefront writes that stretch, one store per word.  For short reads that is one store per read, of a stretch that neither
// starts nor ends on a line's boundary, while the reads beside it -- same claim, other lanes -- end tens of iterations
// later: every line of the output goes to memory two or three times, in pieces (profiles/claim_output_ab.txt).
// STAGE (DYN, PML, no document ids): a wavefront's reads come in claims of 64 consecutive indices (the first round,
// wave * 64 + lane, is one too), so a claim's lengths are one contiguous stretch of the output and its class records one
// aligned KB.  A claim takes one of the wavefront's CSLOTS slots in LDS when its first read is handed out; a read of up to 64
// characters leaves its one word of reset bits and its class record there when it ends; when the claim's last read has
// ended -- counted on wave-uniform values, once per iteration -- the wavefront writes the stretch in whole aligned lines
// (the first and the last masked to the stretch) and the records as one store.  Lane l takes value l of each line and finds
// the read it belongs to through a bit map of the reads' first positions (stretches of up to 64 lines: every claim of reads
// that fit a word) or, behind it, with a cursor over the reads' bases.  What does not fit keeps the path above,
// unchanged and correct on its own: a read of more than 64 characters (all its words, and its record), an empty read (its
// record; both are only counted as ended), and every read of a claim that found no slot free.  The loop's exit needs
// nothing new: a lane is done only after its last read was counted, in the iteration that read ended in.
template <int MODE, bool DOC, bool NARROW, int CHUNK = 0, bool EARLY = false, bool DYN = false>
__global__ void __launch_bounds__(WALK_TPB) k_walk_fast(const DevIndex ix, const BatchArgs b) {
    constexpr bool AUX = (MODE == SPX_MODE_MS) || DOC;  // per-jump side data (samples / doc ids)
    constexpr bool PML = MODE == SPX_MODE_PML;
    // claim-staged output (see "How the results leave" above): the dynamic deal's PML walk without document ids
    constexpr bool STAGE = DYN && PML && !DOC;
    if (CHUNK == 2 && b.ch.round > 1 && b.ch.pending[b.ch.round] == 0) return;  // no seam was left open
    __shared__ HotLetter s_hot[256];
    // MS pointers (and, with them, the document ids) wait in LDS until the sixteen that share an aligned 128-byte line of
    // the output are there, then eight lanes write that line, two pointers each ([element][thread], rows 257 apart: the
    // readers of one lane's group hit different banks).  An entry is the pointer's low 48 bits (n < 2^40, and a pointer
    // that wrapped below zero -- Appendix C3 -- is at most a read's length below it: sign-extended when it leaves) and the
    // document id above them.
#ifndef SPX_PGRP
#define SPX_PGRP 16
#endif
    constexpr int PGRP = SPX_PGRP, PROW = WALK_TPB + 1;
    constexpr int PLPG = PGRP / 2, PNG = 64 / PLPG;  // lanes that write one group, groups written per round
    __shared__ uint64_t s_ptrs[MODE == SPX_MODE_MS && CHUNK != 2 ? PGRP * PROW : 1];
    // PML with document ids: the ids take the same way out, 32 of them (an aligned 64 bytes of the 16-bit output) per
    // group, four per writing lane ([thread][element], 68 bytes per thread: a writer's four ids are one 8-byte LDS read)
    constexpr bool DSTAGE = PML && DOC && CHUNK != 2;
    constexpr int DGRP = 32, DROW = DGRP + 2;
    __shared__ uint16_t s_docs[DSTAGE ? WALK_TPB * DROW : 1];
    const LetterInfo* const s_let = ix.letters;  // (the full letter records are only read on rare paths: from memory)
    __shared__ uint32_t s_win[8 * WALK_TPB];
    // STAGE: CSLOTS claims per wavefront wait here until their last read has ended.  Per read of a claim: where its
    // results go (written when the read is taken), and -- written when it ends, if it is no longer than one word -- its
    // reset bits, its length (0: not staged -- empty, longer than a word, or not ended) and its class record.
    // Wave-private like s_ptrs: the LDS serves a wavefront's accesses in order, nothing is shared between wavefronts.
    // 2112 bytes a claim, 25 344 a block at three claims a wavefront: 37.6 KB with the tables above, four blocks a CU.
    constexpr int CSLOTS = 3, CWAVE = CSLOTS * 64, CALL = (WALK_TPB / 64) * CWAVE;
    constexpr uint32_t C_NONE = 0xffffffffu;
    __shared__ uint64_t s_cbase[STAGE ? CALL : 1];
    __shared__ uint64_t s_cword[STAGE ? CALL : 1];
    __shared__ uint64_t s_ccls[STAGE ? 2 * CALL : 1];  // spx_class: sum_max, above | below << 32
    __shared__ uint8_t s_clen[STAGE ? CALL : 1];
    const char* const rows_b = reinterpret_cast<const char*>(ix.rows);
    const char* const fat_b = reinterpret_cast<const char*>(ix.fat);
    const uint32_t fs = ix.fat_stride;
    // a PML-only index may keep, in the second half of a 32-byte fat slot, the ROW of the run the slot's jump lands in
    // (run sLFrun: the successor's landing and, when the predecessor lands in the same run, its landing too): the step
    // after such a jump goes on from that row without a landing gather (spx_flatten.hip, SPX_FAT_LROW)
    const bool lrow = !AUX && fs == 32 && ix.aux == nullptr;
    for (int t = threadIdx.x; t < 256; t += blockDim.x) {
        const LetterInfo li = ix.letters[t];
        s_hot[t] = HotLetter{li.bmul, li.qbeg != li.qend ? 1u : 0u, (uint64_t)(uintptr_t)(fat_b + li.fbase * fs)};
    }
    __syncthreads();
    const char* const dir_b = reinterpret_cast<const char*>(ix.dirrows);
    const char* const fatj_b = reinterpret_cast<const char*>(ix.fat_js);
    const char* const q_b = reinterpret_cast<const char*>(ix.Q);
    const char* const seq_b = reinterpret_cast<const char*>(b.seqs);
    const char* const off_b = reinterpret_cast<const char*>(b.offs);
    const uint32_t R = ix.r;
    const uint32_t fs_shift = fs == 32 ? 5 : 4;
    const bool want_class = PML && CHUNK == 0 && b.out_class != nullptr;
    // PML lengths leave the walk as whole 64-character words, written by the WAVEFRONT: when a lane has collected the
    // reset bits of 64 characters (or its read ends) all 64 lanes write that stretch together -- one coalesced store
    // of 128 / 256 contiguous bytes instead of a lane's scattered stores (which is what made per-lane length stores
    // expensive: profiles/r02_store_experiments.txt) and instead of a second kernel over a bit mask
    const bool want_len = PML && CHUNK != 2 && b.out_lengths != nullptr;
    const uint32_t lpw = b.lanes_per_wave;
    const uint32_t nlanes = (uint32_t)((((uint64_t)gridDim.x * blockDim.x) >> 6) * lpw);
    const uint32_t nitems = CHUNK ? (uint32_t)*b.ch.nchunks : (uint32_t)b.nreads;  // (the launcher keeps batches of 2^31 items and more on k_walk_lanes)
    // the chunk scratch is indexed by character index relative to the batch's first character (spx_walk.hip)
    const uint64_t ch_org = CHUNK ? b.offs[0] : 0;
    uint8_t* const ch_flags = CHUNK ? b.ch.flags - (ch_org & ~7ull) : nullptr;
    WalkState* const ch_ckpt = CHUNK ? b.ch.ckpt - (ch_org >> CKPT_SHIFT) : nullptr;
    const char* const item_b = CHUNK ? reinterpret_cast<const char*>(b.ch.desc) : off_b;
    constexpr uint32_t ITEM_BYTES = CHUNK ? sizeof(ChunkDesc) : 8;
    const uint32_t tid = threadIdx.x;
    static_assert(!DYN || (CHUNK == 0 && !EARLY), "only the plain, full launch deals its reads on demand");
    uint32_t w_n0 = 0, w_e0 = 0, w_n1 = 0, w_e1 = 0;  // the reservoir: [w_n0, w_e0), then [w_n1, w_e1)
    bool w_pend = false;  // a claim goes out with the next gather / is in flight with this one
    bool w_dry = false;   // the batch has no reads beyond what the wavefront's last claim returned
    // (the first claims are spread over the first 32 iterations -- nobody needs a read before its first one ends -- or
    // every wavefront of the launch would be at the claim word in the same microsecond)
    uint32_t w_wait = DYN ? (uint32_t)((((uint64_t)blockIdx.x * blockDim.x + tid) >> 6) & 31u) + 1u : 0u;
    unsigned long long claimed = 0;

    uint32_t rd = (uint32_t)((((uint64_t)blockIdx.x * blockDim.x + tid) >> 6) * lpw) + (tid & 63);
    uint32_t ph = (rd < nitems && (tid & 63) < lpw) ? Q_READ : Q_DONE;
    const char* addr = ph == Q_READ ? item_b + (uint64_t)rd * ITEM_BYTES : item_b;
    // STAGE.  Per lane: cidx, where its read stands in the wavefront's staging area (slot * 64 + index in the claim;
    // C_NONE: the read's claim found no slot, or the read has been counted as ended).  Per wavefront, in scalar
    // registers: per slot the claim's first read, its size (0: the slot is free) and how many of its reads have not
    // ended; per range of the reservoir, what turns a read index of it into a cidx (w_cv: its claim has a slot).
    const uint32_t cw0 = (tid >> 6) * CWAVE;
    uint32_t cidx = C_NONE;
    uint32_t c_first[CSLOTS] = {0, 0, 0}, c_n[CSLOTS] = {0, 0, 0}, c_left[CSLOTS] = {0, 0, 0};
    uint32_t w_cb0 = 0, w_cb1 = 0;
    bool w_cv0 = false, w_cv1 = false, w_ct0 = false, w_ct1 = false;  // (w_ct: the range's claim has asked for a slot)
    // a claim of `count` reads from `first` on takes a free slot; when there is none its reads go out one by one, as ever
    auto take_slot = [&](uint32_t first, uint32_t count, uint32_t& cb, bool& cv) {
        const uint32_t fs_ = c_n[0] == 0 ? 0u : (c_n[1] == 0 ? 1u : (c_n[2] == 0 ? 2u : 3u));
        cv = fs_ < (uint32_t)CSLOTS;
        if (cv) {
#pragma unroll
            for (int s = 0; s < CSLOTS; ++s) {
                c_first[s] = fs_ == (uint32_t)s ? first : c_first[s];
                c_n[s] = fs_ == (uint32_t)s ? count : c_n[s];
                c_left[s] = fs_ == (uint32_t)s ? count : c_left[s];
            }
            cb = fs_ * 64 - first;
            s_clen[cw0 + fs_ * 64 + (threadIdx.x & 63)] = 0;
        }
    };
    static_assert(CSLOTS == 3, "the slots' scalars are written out by hand");
    if (STAGE) {
        // the first round is a claim too: reads [wave * 64, wave * 64 + 64), clipped to the batch, in slot 0
        const uint32_t f0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(rd - (tid & 63)));
        c_first[0] = f0;
        c_n[0] = c_left[0] = f0 < nitems ? (nitems - f0 < 64u ? nitems - f0 : 64u) : 0u;
        cidx = ph == Q_READ ? (tid & 63) : C_NONE;
        s_clen[cw0 + (tid & 63)] = 0;
    }
    uint32_t seen = 0;  // chunked walk: what the steps of this chunk reset so far (bit 0 length / sample, bit 1 document id)
    uint64_t fb = 0;    // ... and the flag bytes of the aligned group of 8 characters being collected
    uint32_t fl = 0;          // F_*
    uint32_t c = 0;           // current character
    uint64_t base = 0, ibase = 0;  // of the read: where its results go, where its characters are
    uint32_t m = 0, x = 0;
    int32_t wi = -1;          // index of the next character in the window (< 0: not there)
    uint64_t q0 = 0, q1 = 0;  // the row the lane stands on
    uint32_t k = 0, off = 0;  // where the lane stands, or lands when its gather returns
    uint32_t length = 0;      // PML length; the directory position while a jump scans the directory
    uint64_t mbits = 0;
    uint32_t nr = 0;           // index in the read of the nearest reset above the characters collected in mbits (m: none)
    uint32_t bin_lo = 0, bin_max = 0, above = 0, below = 0;
    uint64_t sum_max = 0;
    uint64_t sample = 0;       // MS pointer counter
    uint32_t doc = 0;          // current document id
    // wave-level counters (scalar registers)
    uint32_t w_jumps = 0, w_pred = 0, w_rows = 0, w_dir = 0, w_again = 0;
    // pass 2: how far down an earlier, unfounded walk of this chunk wrote (later rounds), and the record of the next
    // checkpoint below the lane (fetched when the one above it was passed)
    uint32_t tlimit = 0xffffffffu;
    V16 cka{0, 0, 0, 0}, ckb{0, 0, 0, 0};

#define WIN_AT(w) ((s_win[((uint32_t)(w) >> 2) * WALK_TPB + tid] >> (((uint32_t)(w) & 3) * 8)) & 0xffu)
#define CUR_C c
#define COUNT(var, cond) (var += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(cond)))

    // ---- the one gather of an iteration ----
    // EARLY: issued where its address is final -- after the repetitions of the iteration before, ahead of that iteration's
    // output flushes (which need nothing of it) -- so that the flushes run under its latency instead of in front of it.
    V16 ga{0, 0, 0, 0}, gb{0, 0, 0, 0};
    uint32_t side_doc = 0;
    Aux side_aux{0, 0};
    uint64_t side_in = 0;  // where the read's characters are, when that is not where its results go (BatchArgs::in_starts)
    auto issue_gather = [&]() {
        ga = V16{0, 0, 0, 0};
        gb = V16{0, 0, 0, 0};
#ifndef SPX_PAIR_MIN
#define SPX_PAIR_MIN 24
#endif
        // (by pairs only when enough lanes of the wavefront want 32 bytes: the exchange costs ~30 instructions an iteration,
        // and a wavefront of 16-byte gathers -- reads that do not match -- gets nothing for them)
        // (EARLY launches are latency chains, not short of line lookups: the exchange would only lengthen the chain)
        constexpr int pair_min = EARLY ? 65 : SPX_PAIR_MIN;
        if ((int)__popcll(__builtin_amdgcn_ballot_w64(ph != Q_DONE && (fl & F_WIDE))) < pair_min) {
            if (ph != Q_DONE) {
                ga = *reinterpret_cast<const V16*>(addr);
                if (fl & F_WIDE) gb = *reinterpret_cast<const V16*>(addr + 16);
            }
        } else
        // A 32-byte gather as two loads of the same lane costs the memory pipeline two line lookups per lane; with the two
        // halves taken by NEIGHBOURING lanes of one instruction it costs one (tools/gather_bench.hip: 39.9 -> 48.4 G
        // 32-byte gathers/s, the rate of 16-byte ones -- profiles/r04_paired_gather.txt).  So the first load instruction
        // serves the even lanes' records (the even lane takes its first 16 bytes, the odd lane beside it the second 16),
        // the second the odd lanes', and the halves change lanes by DPP.
        {
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4), aligned(4)));
            typedef const __attribute__((address_space(1))) u32x4* GV16;  // (global, not flat: the addresses go through integers)
            const bool odd = tid & 1;
            const bool live = ph != Q_DONE;  // (a lane that is done still lends itself to its neighbour)
            const uint32_t w_own = (live && (fl & F_WIDE)) ? 16u : 0u;
            const uint64_t au = (uint64_t)(uintptr_t)(live ? addr : rows_b);
            const uint64_t pu = u64of(dpp_swap1((uint32_t)au), dpp_swap1((uint32_t)(au >> 32))) + 16;  // the neighbour's second half
            const uint32_t w_for = dpp_swap1(w_own);
            // instruction 1: the even lanes' records, instruction 2: the odd lanes'; a lane loads for its neighbour only when
            // that one wants 32 bytes, and for itself unless it is done
            const uint64_t a1 = odd ? pu : au, a2 = odd ? au : pu;
            const bool do1 = odd ? w_for != 0 : live, do2 = odd ? live : w_for != 0;
            uint32_t r1x = 0, r1y = 0, r1z = 0, r1w = 0, r2x = 0, r2y = 0, r2z = 0, r2w = 0;
            if (do1) {
                const u32x4 t = *(GV16)(uintptr_t)a1;
                r1x = t.x, r1y = t.y, r1z = t.z, r1w = t.w;
            }
            if (do2) {
                const u32x4 t = *(GV16)(uintptr_t)a2;
                r2x = t.x, r2y = t.y, r2z = t.z, r2w = t.w;
            }
            // own first half; the second half is what the neighbour loaded for this lane (exchanged with every lane active: a
            // DPP read of a lane that is switched off returns nothing)
            ga = V16{odd ? r2x : r1x, odd ? r2y : r1y, odd ? r2z : r1z, odd ? r2w : r1w};
            const uint32_t zx = dpp_swap1(odd ? r1x : r2x), zy = dpp_swap1(odd ? r1y : r2y), zz = dpp_swap1(odd ? r1z : r2z),
                           zw = dpp_swap1(odd ? r1w : r2w);
            gb = V16{w_own ? zx : 0u, w_own ? zy : 0u, w_own ? zz : 0u, w_own ? zw : 0u};
        }
        // side loads of two rare phases, issued with the gather (not after it has returned: their latency would
        // stall the whole wavefront): start_runs_doc of the run a byte >= 128 stays on, the Aux of a directory position
        side_doc = 0;
        side_aux = Aux{0, 0};
        side_in = 0;
        claimed = 0;
        if (CHUNK == 0 && b.in_starts != nullptr && ph == Q_READ) side_in = b.in_starts[rd];
        if (DOC && ph == Q_SAMP) side_doc = ix.rundocs[k];
        if (AUX && ph == Q_DIR) side_aux = ix.aux[length];
        if (DYN && w_pend && (tid & 63) == 0) claimed = atomicAdd(b.claim, (unsigned long long)CHUNK_CLAIM);
    };
    if (EARLY) issue_gather();
    while (__builtin_amdgcn_ballot_w64(ph != Q_DONE) != 0) {
        if (!EARLY) issue_gather();
        uint32_t act = 0, hd = 0;
        uint32_t rflag = 0;  // chunked walk: what this iteration's first finished step reset
        bool pred_ev = false;  // this iteration's jump went to the previous run of its letter
        // fields of the jump row that answers the jump (A_DECIDE)
        uint32_t d_trun = 0, d_toff = 0, d_srun = 0, d_soff = 0, d_bits = 0;  // d_bits: Hs[8] | psame << 8 | nosucc << 9 | first << 10 | Hp[8] << 16
        Aux d_aux{0, 0};  // ... and the side data of its directory position
        bool d_lrow = false;  // gb holds the row of run d_srun (a fat slot with its landing row)
        // a completed word of reset bits, to be written out after the repetitions: characters [fxi, fxi + 64) of the read
        uint64_t fbits = 0;
        uint32_t fxi = 0;
        bool flush = false;
        // MS: this lane's group of pointers -- the positions of one aligned 128-byte line from read index pfxi up -- is
        // complete; a pointer produced after that, in the same iteration, waits in `phold` until the group has left
        bool pflush = false, pheld = false, pheld_end = false;
        uint32_t pfxi = 0;
        uint64_t phold = 0;
        COUNT(w_rows, ph == Q_LAND);
        COUNT(w_dir, ph == Q_FAT || (ph >= Q_FATJ && ph <= Q_DIR));

        if (ph == Q_LAND) {
            const uint32_t len = ga.x & 0xffffu;
            const uint32_t o = off == OFF_LAST32 ? len - 1 : off;  // predecessor landing: last position of the run
            if (o >= len) {  // the LF image lies in a later run: next row
                off = o - len;
                k++;
                addr += sizeof(Row32);
            } else {
                off = o;
                q0 = u64of(ga.x, ga.y);
                q1 = u64of(ga.z, ga.w);
                fl = (fl & ~F_NOROW) | F_EMB;
                act = A_STEP;
            }
        } else if (ph == Q_FAT) {
            const uint32_t hq = ga.x;
            const uint32_t w1l = ga.z, w1h = ga.w;  // FatRow::w1
            const bool nosucc = (w1h >> 29) & 1, esc = (w1h >> 30) & 1;
            const bool quirk = fl & F_QUIRK;
            // the block's first c-run is the successor unless it lies before k (or is k itself when the walk sits
            // on a c-run: byte >= 128, Appendix C1)
            const bool found = nosucc || hq > k || (quirk && hq == k);
            if (found && !esc && !quirk) {
                d_trun = hq - (w1l & 0x7ffffu);
                d_toff = ((w1l >> 20) | (w1h << 12)) & 0xffffu;
                d_srun = ga.y;
                // the sLFoff field: the offset when the predecessor lands in the same run (psame), else (the offset is
                // 0 then) Hp, the head of run sLFrun - 1, where the predecessor lands
                const uint32_t sfield = (w1h >> 4) & 0xffffu;
                const bool ps = (w1h >> 28) & 1;
                d_soff = ps ? sfield : 0u;
                d_bits = ((w1h >> 20) & 0xffu) | ((uint32_t)ps << 8) | ((uint32_t)nosucc << 9) | ((w1h >> 31) << 10) |
                         ((ps ? 0u : (sfield & 0xffu)) << 16);
                if (AUX) d_aux = Aux{u64of(gb.x, gb.y), u64of(gb.z, gb.w)};  // the slot's second half
                d_lrow = lrow;
                act = A_DECIDE;
            } else if (!found && (w1l & (uint32_t)FAT_SINGLE) && !(fl & F_FADD)) {
                fl |= F_FADD;  // the letter's next run lies past this block: it is the next slot's run
                addr += fs;
            } else if (found && esc && !quirk) {
                // the row did not fit the digest: the slot names its directory position
                length = ga.y;
                fl |= F_WIDE;
                ph = Q_DIR;
                addr = dir_b + (uint64_t)length * sizeof(JumpRow);
            } else {
                // a scan of the directory for the first run of the letter at or after k, from where the slot's group starts
                const uint64_t grp = ((uint64_t)(addr - fat_b) >> fs_shift) >> FJ_SHIFT;
                length = (uint32_t)grp & 3;  // which of the four entries of the aligned 16 bytes
                fl &= ~F_WIDE;
                ph = Q_FATJ;
                addr = fatj_b + ((grp * 4) & ~15ull);
            }
        } else if (ph == Q_STEP) {
            act = A_STEP;  // the repetitions ran out while the lane was standing
        } else if (ph != Q_DONE && ph != Q_SAMP && (!DYN || ph != Q_WANT)) {
            // ---- the rare phases ----
            if (ph == Q_READ) {
                if (CHUNK) {  // ChunkDesc: gend, len | flags << 29, read
                    m = ga.z & CHUNK_LEN_MASK;
                    base = u64of(ga.x, ga.y) - m;
                    seen = 0;
                    fb = 0;
                    // pass 2: a read's last chunk was right from the start; later rounds: only the chunks below open seams
                    if (CHUNK == 2 && (((ga.z >> 29) & 4) || (b.ch.round > 1 && !((ga.z >> 29) & 1)))) m = 0;
                } else {
                    base = u64of(ga.x, ga.y);
                    m = (uint32_t)(u64of(ga.z, ga.w) - base);
                    if (STAGE && cidx != C_NONE) s_cbase[cw0 + cidx] = base;  // (every read of a staged claim: the writer's map)
                }
                ibase = (CHUNK == 0 && b.in_starts != nullptr) ? side_in : base;
                if (m == 0) {
                    if (want_class) b.out_class[rd] = spx_class{0, 0, 0};
                    rd += DYN ? 0u : nlanes;
                    ph = DYN ? Q_WANT : (rd < nitems ? Q_READ : Q_DONE);
                    addr = DYN ? rows_b : item_b + (uint64_t)rd * ITEM_BYTES;
                } else {
                    if (NARROW && CHUNK == 0 && m >= 65536) atomicAdd(&b.counters->error, 1ull);  // 16-bit outputs cannot hold this read's values
                    x = m;
                    length = 0;
                    sample = ix.init_sample;  // compute_ms_pml.cpp:575
                    doc = ix.init_doc;        // :298 / :634
                    // pos = bwt_size() - 1 (:243): the same row for every read, kept in the kernel arguments
                    k = ix.init_k;
                    off = (uint32_t)ix.init_off;
                    q0 = ix.init_row.q0;
                    q1 = ix.init_row.q1;
                    fl = 0;
                    wi = -1;
                    mbits = 0;
                    nr = m;
                    if (want_class) {
                        const uint32_t w = (uint32_t)b.bin_width;
                        // m / w without a divide: bin_magic = floor(2^64 / w) + 1 (exact for m < 2^32)
                        const uint32_t q = w > 1 ? (uint32_t)__umul64hi((uint64_t)m, b.bin_magic) : m;
                        const uint32_t nb = q > 0 ? q : 1;
                        bin_lo = (nb - 1) * w;
                        bin_max = above = below = 0;
                        sum_max = 0;
                    }
                    act = A_STEP;  // (finds the window empty and asks for it)
                    if (CHUNK == 2) {
                        // round 1: the recorded end state of the chunk above (the next one); later: what the scan left
                        ph = Q_START;
                        addr = reinterpret_cast<const char*>(b.ch.round > 1 ? b.ch.reentry + rd : b.ch.ends + rd + 1);
                        fl = F_WIDE;
                        act = 0;
                    }
                }
            } else if (ph == Q_CHARS) {
                s_win[0 * WALK_TPB + tid] = ga.x;
                s_win[1 * WALK_TPB + tid] = ga.y;
                s_win[2 * WALK_TPB + tid] = ga.z;
                s_win[3 * WALK_TPB + tid] = ga.w;
                s_win[4 * WALK_TPB + tid] = gb.x;
                s_win[5 * WALK_TPB + tid] = gb.y;
                s_win[6 * WALK_TPB + tid] = gb.z;
                s_win[7 * WALK_TPB + tid] = gb.w;
                ph = Q_STEP;
                act = A_STEP;  // only entered from STEP: the lane stands on (k, off)
            } else if (CHUNK == 2 && ph == Q_START) {
                // the walk that ended the chunk above goes on into this one: it lands on (k, off)
                k = ga.x;
                length = ga.y;
                {
                    const uint64_t offp = u64of(ga.z, ga.w);
                    off = offp == OFF_END ? OFF_LAST32 : (uint32_t)offp;
                }
                sample = u64of(gb.x, gb.y);
                doc = gb.z;
                tlimit = b.ch.round > 1 ? gb.w : 0xffffffffu;  // entered again: write at least as far down as the earlier walk did
                ph = Q_LAND;
                addr = rows_b + (uint64_t)k * sizeof(Row32);
                fl = F_WIDE;
                {
                    const char* const cp = reinterpret_cast<const char*>(ch_ckpt + ((base + m - 1) >> CKPT_SHIFT));
                    cka = *reinterpret_cast<const V16*>(cp);
                    ckb = *reinterpret_cast<const V16*>(cp + 16);
                }
            } else if (ph == Q_FATJ) {
                const uint32_t lo = (length & 2) ? ga.z : ga.x, hi = (length & 2) ? ga.w : ga.y;
                length = (length & 1) ? hi : lo;  // where the slot's group starts in the directory
                fl |= F_WIDE;
                ph = Q_QS;
                addr = q_b + (uint64_t)length * 4;
            } else if (ph == Q_QS) {
                const uint32_t e[8] = {ga.x, ga.y, ga.z, ga.w, gb.x, gb.y, gb.z, gb.w};
                // Q[jdir .. jdir + 8): skip the c-runs with index < k; Q ascends and "still inside the letter's
                // range" is a prefix property too, so the entries to skip are a prefix of the window
                const uint32_t room_q = s_let[CUR_C].qend - length;
                uint32_t skip = 0;
#pragma unroll
                for (int t = 0; t < 8; ++t) skip += ((uint32_t)t < room_q && e[t] < k) ? 1u : 0u;
                length += skip;
                if (skip < 8) {
                    ph = Q_DIR;
                    addr = dir_b + (uint64_t)length * sizeof(JumpRow);
                } else {
                    addr = q_b + (uint64_t)length * 4;
                }
            } else {  // Q_DIR: the full jump row of directory position jdir (= length)
                JumpRow e;
                e.d0 = u64of(ga.x, ga.y);
                e.d1 = u64of(ga.z, ga.w);
                e.d2 = u64of(gb.x, gb.y);
                e.d3 = u64of(gb.z, gb.w);
                const uint32_t jdir = length;
                const uint32_t qbeg = s_let[CUR_C].qbeg, qend = s_let[CUR_C].qend;
                if (!(fl & F_QUIRK)) {
                    d_trun = jr_THRrun(e);
                    d_toff = (uint32_t)jr_THRoff(e);
                    d_srun = jr_sLFrun(e);
                    d_soff = (uint32_t)jr_sLFoff(e);
                    d_bits = jr_Hs(e) | ((uint32_t)jr_psame(e) << 8) | ((jdir < qend ? 0u : 1u) << 9) | ((jdir <= qbeg ? 1u : 0u) << 10);
                    if (AUX) d_aux = side_aux;
                    act = A_DECIDE;
                } else {
                    // the walk sits on run k whose head equals c >= 128 (Appendix C1) and thresholds[k] > S[k]
                    // (inconsistent thresholds): jdir is k's own directory position
                    const bool has_succ = jdir < qend;
                    const uint32_t trun = jr_THRrun(e);
                    const bool below_thr = !has_succ || (k < trun) || (k == trun && off < (uint32_t)jr_THRoff(e));
                    const uint32_t LFrun_k = (uint32_t)(q0 >> 32), LFoff_k = (uint32_t)(q0 >> 16) & 0xffffu;
                    pred_ev = below_thr;
                    if (AUX) {
                        // what the jump hands out: samples_start[k] / start_runs_doc[k] when it stays, samples_last /
                        // end_runs_doc of the position it moves back to -- run k's own (the NEXT directory position's
                        // record) when that is still inside run k, the previous c-run's otherwise
                        const Aux a = ix.aux[jdir + ((below_thr && off > 0) ? 1u : 0u)];
                        if (MODE == SPX_MODE_MS) sample = below_thr ? aux_se(a) : aux_ss(a);
                        if (DOC) doc = below_thr ? (aux_docs(a) >> 16) : (aux_docs(a) & 0xffffu);
                    }
                    if (!below_thr) {  // select(rank(pos,c),c) == pos: stay
                        k = LFrun_k;
                        off = LFoff_k + off;
                    } else if (off > 0) {  // select(rnk-1, c) = pos - 1, still inside run k
                        k = LFrun_k;
                        off = LFoff_k + off - 1;
                    } else {
                        if (jdir <= qbeg) atomicAdd(&b.counters->error, 1ull);
                        const bool ps = jr_psame(e);
                        const uint32_t srun = jr_sLFrun(e);
                        k = ps ? srun : srun - 1;
                        off = ps ? (uint32_t)jr_sLFoff(e) - 1 : OFF_LAST32;
                    }
                    length = 0;
                    fl &= ~(F_EMB | F_QUIRK);
                    rflag = 3;
                    act = A_EMIT;
                }
            }
        }
        if (AUX && ph == Q_SAMP) {
            // byte >= 128 sitting on its own run (Appendix C1): the jump stays there and hands out the run's own
            // samples_start / start_runs_doc; then the step is taken again, with them
            if (MODE == SPX_MODE_MS) sample = u64of(ga.x, ga.y);
            if (DOC) doc = side_doc & 0xffffu;
            fl |= F_SAMPD;
            ph = Q_STEP;
            act = A_STEP;
        }

        // ---- the jump row is here: compute_ms_pml.cpp:253-278 on the flat layout ----
        {
            const bool dec = act & A_DECIDE;
            const bool nosucc = (d_bits >> 9) & 1, psame = (d_bits >> 8) & 1;
            // pos < thr, with thr = n + 1 when there is no successor (:254, :270)
            const bool below_thr = nosucc || (k < d_trun) || (k == d_trun && off < d_toff);
            COUNT(w_pred, (dec && below_thr) || pred_ev);
            if (dec) {
                if (below_thr && ((d_bits >> 10) & 1)) atomicAdd(&b.counters->error, 1ull);  // rnk-- below zero: undefined upstream
                // !below: first position of the next c-run; below: last position of the previous c-run; LF of it
                const bool last = below_thr && !psame;  // ... which is the last position of run sLFrun - 1
                k = d_srun - (last ? 1u : 0u);
                off = last ? OFF_LAST32 : d_soff - (below_thr ? 1u : 0u);
                // the head of the landing run travels with the jump: Hs of run sLFrun, or (fat digests only; 0 = not known)
                // Hp of run sLFrun - 1
                hd = last ? ((d_bits >> 16) & 0xffu) : (d_bits & 0xffu);
                if (MODE == SPX_MODE_MS) sample = below_thr ? aux_se(d_aux) : aux_ss(d_aux);                    // :601 / :611
                if (DOC) doc = below_thr ? (aux_docs(d_aux) >> 16) : (aux_docs(d_aux) & 0xffffu);  // :317 / :327
                length = 0;
                // (a landing in run sLFrun whose row came with the slot: the lane stands on it like on an embedded row)
                fl = (fl & ~(F_EMB | F_QUIRK)) | ((d_lrow && !last) ? F_EMB : 0u);
                rflag = 3;
                act = A_EMIT;
            }
        }

        // ---- step / emit ----
        // Straight-line select code, STEP_REPS times (unrolled: as a loop the compiler carries the whole lane state
        // through the inner loop's header and copies it -- some 45 register moves per repetition).
#pragma unroll
        for (int rep = 0; rep < STEP_REPS; ++rep) {
            if (rep > 0 && __builtin_amdgcn_ballot_w64(act != 0) == 0) break;
            bool jumped = false;
            if (act & A_STEP) {
                // next character: auto c = pattern[m - i - 1]   (:247)  (F_HAVEC: the step is being repeated with its row)
                const bool havec = fl & F_HAVEC;
                if (!havec && wi < 0) {
                    // not in the window: fetch the 32 bytes that end at the next 4-byte boundary after it
                    const uint64_t g = ibase + x - 1;
                    const uint64_t end4 = (g + 4) & ~3ull;
                    const uint64_t wbase = end4 >= 32 ? end4 - 32 : 0;
                    wi = (int32_t)(g - wbase);
                    ph = Q_CHARS;
                    addr = seq_b + wbase;
                    fl = (fl | F_WIDE) & ~F_EMB;
                    act = 0;
                } else {
                    const uint32_t cw = WIN_AT(wi < 0 ? 0 : wi);
                    c = havec ? c : cw;
                    wi -= havec ? 0 : 1;
                    const HotLetter hl = s_hot[c];
                    const uint32_t H = (uint32_t)q1 & 0xffu;
                    const bool eq = k < R && H == c;  // pos < n && bwt[pos] == c   (:250)
                    // bytes >= 128 never match (signed-char compare): they take the jump branch, and on their own
                    // run with thresholds[k] <= S[k] <= pos the jump stays where it is (Appendix C1)
                    const bool lf = eq && (c < 128 || ((q1 >> 8) & 1));
                    const bool present = hl.present != 0;
                    // the lane knows run k by its head only and the character equals it: the step needs the row
                    const bool go_land = eq && (fl & F_NOROW);
                    // threshold jump to the next / previous c-run: its fat slot
                    const bool go_fat = !go_land && present && !lf;
                    // ... and with samples / document ids a byte >= 128 that stays on its run first fetches the run's own
                    const bool go_samp = AUX && !go_land && lf && c >= 128 && !(fl & F_SAMPD);
                    const bool fin = !(go_land || go_fat || go_samp);
                    const bool lfin = fin && present;  // match (length++) or the stay-put jump of a byte >= 128 (length = 0)
                    uint32_t tk, toff, t;
                    lf_target_ct((uint32_t)(q0 >> 32), (uint32_t)(q0 >> 16) & 0xffffu, (uint32_t)(q1 >> 32), off, tk, toff, t);
                    t = lfin ? t : 4u;
                    const char* a_land = rows_b + (uint64_t)k * sizeof(Row32);
                    const char* a_fat = reinterpret_cast<const char*>((uintptr_t)hl.fat0) + (uint64_t)fat_block(k, hl.bmul) * fs;
                    addr = go_land ? a_land : (go_fat ? a_fat : addr);
                    ph = go_land ? Q_LAND : (go_fat ? Q_FAT : ph);
                    if (go_samp) {
                        addr = reinterpret_cast<const char*>(MODE == SPX_MODE_MS ? (const void*)(ix.ss_by_run + k) : (const void*)(ix.rundocs + k));
                        ph = Q_SAMP;
                    }
                    k = lfin ? tk : k;
                    off = lfin ? toff : off;
                    if (fin && !present) {
                        // number_of_letter(c) == 0 (:249): LF(pos, c) = F[c]
                        k = s_let[c].frun;
                        off = (uint32_t)s_let[c].foff;
                        if (MODE == SPX_MODE_MS) {
                            sample = 0;                 // :581
                            if (DOC) doc = ix.doc_at0;  // :641-642 (PML keeps its document id over an absent letter)
                        }
                    }
                    if (MODE == SPX_MODE_MS) sample -= (lfin && c < 128) ? 1u : 0u;  // :582 (wraps, Appendix C3)
                    length = (lfin && c < 128) ? length + 1 : (fin ? 0u : length);
                    // what the step reset (pass 3 of the chunked walk needs to know where a wrong start value ends): a match
                    // nothing; a byte >= 128 that stays, like every jump, all of it; an absent letter the length (PML keeps
                    // its document id over it)
                    if (CHUNK) rflag = (lfin && c < 128) ? 0u : (lfin ? 3u : (MODE == SPX_MODE_MS ? 3u : 1u));
                    jumped = go_fat || (lfin && c >= 128);
                    // what is known about the landing before any gather: the embedded row (t == 0), or its head
                    hd = t < 2 ? ((uint32_t)(q1 >> (16 + 8 * t)) & 0xffu) : 0u;
                    uint32_t nf = fl & ~(F_HAVEC | F_SAMPD | (t == 0 ? 0u : F_EMB));
                    nf = go_fat ? ((nf & ~(F_QUIRK | F_FADD | F_WIDE)) | (eq ? F_QUIRK : 0u) | ((AUX || lrow) ? F_WIDE : 0u)) : nf;
                    nf = go_land ? (nf | F_WIDE | F_HAVEC) : nf;
                    nf = go_samp ? ((nf | F_HAVEC) & ~F_WIDE) : nf;
                    fl = nf;
                    act = fin ? A_EMIT : 0u;
                }
            }
            COUNT(w_jumps, jumped);
            if (CHUNK == 2) COUNT(w_again, (act & A_EMIT) != 0);
            if (act & A_EMIT) {
                // lengths[m - i - 1] = length   (:281), as one bit per character ("reset here"): shifted in from the right,
                // the bit of character p ends up at position p & 63 when the word is written (at p & 63 == 0)
                const uint32_t xi = x - 1;
                x = xi;
                // the read's results wait in LDS for the rest of its claim: it fits one word and its claim has a slot
                const bool staged = STAGE && cidx != C_NONE && m <= 64;
                (void)staged;
                bool met = false;  // pass 2: the walk stands where the speculative walk of this chunk stood
                if (CHUNK == 2) {
                    // pass 2 writes over the speculative results one value at a time (a few steps per chunk)
                    const uint64_t gi = base + xi;
                    seen |= rflag;
                    ch_flags[gi] = (uint8_t)rflag;
                    if (PML) {
                        if (NARROW)
                            reinterpret_cast<uint16_t*>(b.out_lengths)[gi] = (uint16_t)length;
                        else
                            b.out_lengths[gi] = length;
                    } else {
                        b.out_pointers[gi] = sample;
                    }
                    if (DOC) {
                        if (NARROW)
                            reinterpret_cast<uint16_t*>(b.out_docs)[gi] = (uint16_t)doc;
                        else
                            b.out_docs[gi] = doc;
                    }
                    const uint64_t my_off = off == OFF_LAST32 ? OFF_END : (uint64_t)off;
                    if (xi != 0 && (gi & ((1u << CKPT_SHIFT) - 1)) == 0) {
                        // checkpoint: the state before character gi - 1, against the speculative walk's (fetched when the
                        // checkpoint above was passed)
                        if (cka.x == k && u64of(cka.z, cka.w) == my_off && xi <= tlimit) {
                            SeamRec sr;
                            sr.t = gi;
                            sr.met = 1 | (b.ch.round << 8);
                            sr.reset_above = seen;
                            sr.ext = WalkState{k, length, my_off, sample, doc, seen};
                            sr.spec_length = cka.y;
                            sr.spec_doc = ckb.z;
                            sr.spec_sample = u64of(ckb.x, ckb.y);
                            b.ch.seams[rd] = sr;
                            met = true;
                        } else {
                            const char* const cp = reinterpret_cast<const char*>(ch_ckpt + ((gi >> CKPT_SHIFT) - 1));
                            cka = *reinterpret_cast<const V16*>(cp);
                            ckb = *reinterpret_cast<const V16*>(cp + 16);
                        }
                    } else if (xi == 0) {
                        // reached the chunk's first character without meeting the speculative walk: fine for a read's first
                        // chunk (the read is done); otherwise k_chunk_scan has the chunk below entered with this state
                        SeamRec sr;
                        sr.t = base;
                        sr.met = b.ch.round << 8;
                        sr.reset_above = seen;
                        sr.ext = WalkState{k, length, my_off, sample, doc, seen};
                        sr.spec_length = 0;
                        sr.spec_doc = 0;
                        sr.spec_sample = 0;
                        b.ch.seams[rd] = sr;
                    }
                }
                if (CHUNK == 1) {
                    const uint64_t gi = base + xi;
                    seen |= rflag;
                    const uint32_t slot = (uint32_t)gi & 7;
                    fb |= (uint64_t)rflag << (slot * 8);
                    if (slot == 0 || xi == 0) {
                        const uint64_t g8 = gi & ~7ull;
                        if (g8 >= base && g8 + 7 < base + m) {
                            *reinterpret_cast<uint64_t*>(ch_flags + g8) = fb;
                        } else {
#pragma unroll
                            for (int t8 = 0; t8 < 8; ++t8)
                                if (g8 + t8 >= gi && g8 + t8 < base + m) ch_flags[g8 + t8] = (uint8_t)(fb >> (t8 * 8));
                        }
                        fb = 0;
                    }
                    // the state before character base + xi - 1: at the chunk's lower end for the walk that enters the chunk
                    // below, every 16 characters for pass 2 to meet
                    if (xi == 0 || ((base + xi) & ((1u << CKPT_SHIFT) - 1)) == 0) {
                        const WalkState ws{k, length, off == OFF_LAST32 ? OFF_END : (uint64_t)off, sample, doc, seen};
                        if (xi == 0)
                            b.ch.ends[rd] = ws;
                        else
                            ch_ckpt[(base + xi) >> CKPT_SHIFT] = ws;
                    }
                }
                if (MODE == SPX_MODE_MS && CHUNK != 2) {
                    // ms_pointers[m - i - 1] = sample   (:618), doc_nums[m - i - 1] = curr_doc_id   (:677; ids < 65536): into
                    // the lane's LDS group, which is complete at the line's lowest position (or the read's)
                    const uint32_t slot = ((uint32_t)base + xi) & (PGRP - 1);
                    const uint64_t pv = (sample & 0xffffffffffffull) | (DOC ? (uint64_t)doc << 48 : 0ull);
                    if (pflush) {  // (the group above has not left yet: its slot PGRP - 1 is still needed)
                        phold = pv;
                        pheld = true;
                        pheld_end = xi == 0;
                    } else {
                        s_ptrs[slot * PROW + tid] = pv;
                        if (slot == 0 || xi == 0) {
                            pflush = true;
                            pfxi = xi;
                        }
                    }
                }
                if (DSTAGE) {  // doc_nums[m - i - 1] = curr_doc_id   (:336); ids < 65536
                    const uint32_t slot = ((uint32_t)base + xi) & (DGRP - 1);
                    if (pflush) {
                        phold = doc;
                        pheld = true;
                        pheld_end = xi == 0;
                    } else {
                        s_docs[tid * DROW + slot] = (uint16_t)doc;
                        if (slot == 0 || xi == 0) {
                            pflush = true;
                            pfxi = xi;
                        }
                    }
                }
                if (PML && CHUNK != 2) {
                    mbits = (mbits << 1) | (length == 0 ? 1u : 0u);
                    if ((xi & 63) == 0) {  // (two consecutive characters: at most one word completes per iteration)
                        if (STAGE && staged) {  // (the read's only word: xi == 0)
                            s_cword[cw0 + cidx] = mbits;
                            s_clen[cw0 + cidx] = (uint8_t)m;
                        } else {
                            fbits = mbits;
                            fxi = xi;
                            flush = true;
                        }
                        mbits = 0;
                    }
                }
                if (want_class) {
                    if (xi < bin_lo) {  // crossed into the previous bin (descending index)
                        const bool ab = bin_max >= b.max_value_thr;
                        above += ab ? 1u : 0u;
                        below += ab ? 0u : 1u;
                        sum_max += bin_max;
                        bin_max = 0;
                        bin_lo -= (uint32_t)b.bin_width;
                    }
                    bin_max = length > bin_max ? length : bin_max;
                }
                if (xi == 0 || (CHUNK == 2 && met)) {
                    if (want_class) {
                        const bool ab = bin_max >= b.max_value_thr;
                        if (STAGE && staged) {
                            s_ccls[2 * (cw0 + cidx)] = sum_max + bin_max;
                            s_ccls[2 * (cw0 + cidx) + 1] = u64of(above + (ab ? 1u : 0u), below + (ab ? 0u : 1u));
                        } else {
                            b.out_class[rd] = spx_class{sum_max + bin_max, above + (ab ? 1u : 0u), below + (ab ? 0u : 1u)};
                        }
                    }
                    rd += DYN ? 0u : nlanes;
                    ph = DYN ? Q_WANT : (rd < nitems ? Q_READ : Q_DONE);
                    addr = DYN ? rows_b : item_b + (uint64_t)rd * ITEM_BYTES;
                    fl = 0;
                    act = 0;
                } else {
                    // where the walk is now, and what it knows about the run it is in: the row that travelled with the
                    // row it stood on (the step ended in run LFrun), the run's head, or nothing
                    const bool stand = fl & F_EMB;
                    const bool head_only = !stand && hd != 0 && rep + 1 < STEP_REPS;  // (no repetition left to look at the next character)
                    const bool ld = !stand && !head_only;
                    q0 = stand ? u64of(gb.x, gb.y) : q0;
                    q1 = stand ? u64of(gb.z, gb.w) : (head_only ? (uint64_t)hd : q1);
                    fl = (fl & ~(F_EMB | F_NOROW)) | (head_only ? F_NOROW : 0u) | (ld ? F_WIDE : 0u);
                    const char* a_land = rows_b + (uint64_t)k * sizeof(Row32);
                    addr = ld ? a_land : addr;
                    ph = ld ? Q_LAND : ph;
                    act = ld ? 0u : A_STEP;
                }
            }
        }
        if (act != 0) {
            ph = Q_STEP;  // still standing: go on in the next iteration (the gather is a dummy)
            addr = rows_b;
            fl &= ~(F_WIDE | F_EMB);
        }
        if (STAGE) {
            // ---- claims whose last read ended in this iteration leave (the bookkeeping on wave-uniform values) ----
            // a lane that ended a read -- staged or not, empty ones too -- stands in Q_WANT with its cidx still set: it is
            // counted once and gives the cidx up
            const bool ended = ph == Q_WANT && cidx != C_NONE;
            if (__builtin_amdgcn_ballot_w64(ended) != 0) {
                uint32_t ready = 0;
#pragma unroll
                for (int s = 0; s < CSLOTS; ++s) {
                    c_left[s] -= (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(ended && (cidx >> 6) == (uint32_t)s));
                    ready |= (c_n[s] != 0 && c_left[s] == 0) ? 1u << s : 0u;
                }
                cidx = ended ? C_NONE : cidx;
                while (ready != 0) {
                    const uint32_t s = (uint32_t)__builtin_ctz(ready);
                    ready &= ready - 1;
                    const uint32_t cn = s == 0 ? c_n[0] : (s == 1 ? c_n[1] : c_n[2]);
                    const uint32_t cf = s == 0 ? c_first[0] : (s == 1 ? c_first[1] : c_first[2]);
                    c_n[0] = s == 0 ? 0u : c_n[0];
                    c_n[1] = s == 1 ? 0u : c_n[1];
                    c_n[2] = s == 2 ? 0u : c_n[2];
                    const uint32_t lane = tid & 63, so = cw0 + s * 64;
                    // the class records: one contiguous, aligned stretch of 16 bytes a read
                    if (want_class && lane < cn && s_clen[so + lane] != 0) {
                        const uint64_t cv = s_ccls[2 * (so + lane) + 1];
                        b.out_class[cf + lane] = spx_class{s_ccls[2 * (so + lane)], (uint32_t)cv, (uint32_t)(cv >> 32)};
                    }
                    if (want_len) {
                        // The lengths: the claim's reads lie one after the other from position lo on.  The wavefront goes over
                        // the aligned lines of 64 values (128 / 256 bytes, by address) that the stretch touches, lane l taking
                        // value l of each line: it finds the read the position belongs to -- through a bit map when the stretch
                        // is short enough for one, else with a cursor that only moves up (positions and bases both
                        // ascend) -- and writes lengths[p] as the store loop below does -- the
                        // distance to the first reset at or after p, the read's end when there is none.  A position whose
                        // read was not staged (clen == 0: empty, or longer than a word and written by that loop), or that
                        // lies outside the stretch (first and last line), fails `p < clen` and is left alone.
                        const int64_t lo = (int64_t)s_cbase[so];
                        const int64_t hi = (int64_t)s_cbase[so + cn - 1] + s_clen[so + cn - 1];
                        const int64_t skew = (int64_t)(((uintptr_t)b.out_lengths >> (NARROW ? 1 : 2)) & 63);
                        const int64_t e00 = ((lo + skew) & ~63ll) - skew;  // the first line's first position
                        uint32_t ci = 0;
                        int64_t cb = lo;
                        if (hi - e00 <= 64 * 64) {
                            // At most 64 lines (always, but for claims with reads longer than a word): the map from position to
                            // read without a search.  The reads that hold positions move to the front of the slot (lane i has
                            // read i in registers; an empty read would share its first position with the next one) and mark
                            // that position in a bit map of the stretch, one word a line, in the slot's class records (which
                            // have left).  Lane l keeps line l's word; per line the word is read from that lane, and position
                            // q of the line belongs to read (marks before the line) + (marks of the line up to q) - 1.
                            const bool mine = lane < cn;
                            const int64_t bi = mine ? (int64_t)s_cbase[so + lane] : hi;
                            const int64_t bn = lane + 1 < cn ? (int64_t)s_cbase[so + lane + 1] : hi;  // (the last read ends at hi, staged or not)
                            const uint32_t li = s_clen[so + lane];
                            const uint64_t wi = s_cword[so + lane];
                            const bool holds = mine && bn > bi;
                            const uint64_t hmask = __builtin_amdgcn_ballot_w64(holds);
                            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(hmask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hmask, 0u));
                            unsigned long long* const bits = reinterpret_cast<unsigned long long*>(&s_ccls[2 * so]);
                            bits[lane] = 0;
                            if (holds) {
                                const uint32_t q = (uint32_t)(bi - e00);  // < 4096: bi < hi
                                atomicOr(&bits[q >> 6], 1ull << (q & 63));
                                s_cbase[so + rank] = (uint64_t)bi;
                                s_clen[so + rank] = (uint8_t)li;
                                s_cword[so + rank] = wi;
                            }
                            const uint64_t mown = atomicOr(&bits[lane], 0ull);
                            const uint32_t nlines = (uint32_t)((hi - e00 + 63) >> 6);
                            uint32_t before = 0;
                            for (uint32_t ln = 0; ln < nlines; ++ln) {
                                const uint64_t mk = u64of((uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mown, (int)ln),
                                                          (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(mown >> 32), (int)ln));
                                const uint32_t upto = before + __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u)) +
                                                      (uint32_t)((mk >> lane) & 1);
                                before += (uint32_t)__popcll(mk);
                                const int64_t e = e00 + (int64_t)ln * 64 + lane;
                                if (upto != 0) {  // (0: in front of the claim's first position)
                                    const uint64_t p = (uint64_t)(e - (int64_t)s_cbase[so + upto - 1]);
                                    const uint32_t cm = s_clen[so + upto - 1];
                                    if (p < cm) {
                                        const uint64_t t = s_cword[so + upto - 1] >> p;
                                        const uint32_t v = t != 0 ? (uint32_t)__builtin_ctzll(t) : cm - (uint32_t)p;
                                        if (NARROW)
                                            reinterpret_cast<uint16_t*>(b.out_lengths)[e] = (uint16_t)v;
                                        else
                                            b.out_lengths[e] = v;
                                    }
                                }
                            }
                        } else
                        for (int64_t e0 = e00; e0 < hi; e0 += 64) {
                            const int64_t e = e0 + lane;
                            while (ci + 1 < cn) {
                                const int64_t nb = (int64_t)s_cbase[so + ci + 1];
                                if (nb > e) break;
                                cb = nb;
                                ++ci;
                            }
                            const uint64_t p = (uint64_t)(e - cb);
                            const uint32_t cm = s_clen[so + ci];
                            if (p < cm) {
                                const uint64_t t = s_cword[so + ci] >> p;
                                const uint32_t v = t != 0 ? (uint32_t)__builtin_ctzll(t) : cm - (uint32_t)p;
                                if (NARROW)
                                    reinterpret_cast<uint16_t*>(b.out_lengths)[e] = (uint16_t)v;
                                else
                                    b.out_lengths[e] = v;
                            }
                        }
                    }
                }
            }
        }
        if (DYN) {
            // ---- the dynamic deal (all of it on wave-uniform values) ----
            if (w_pend) {  // the claim that went out with this iteration's gather: reads [nlanes + claimed, ... + CHUNK_CLAIM)
                const uint64_t c0 = (uint64_t)nlanes + u64of((uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)claimed),
                                                             (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(claimed >> 32)));
                const uint64_t c1 = c0 + CHUNK_CLAIM;
                w_n1 = (uint32_t)(c0 < nitems ? c0 : nitems);  // (a claim past the end is clipped)
                w_e1 = (uint32_t)(c1 < nitems ? c1 : nitems);
                w_dry = c1 >= nitems;  // (the word only grows: a later claim would lie past the end)
                w_pend = false;
                w_cv1 = w_ct1 = false;
            }
            if (w_n0 == w_e0) {  // the first range is used up: the second takes its place
                w_n0 = w_n1;
                w_e0 = w_e1;
                w_n1 = w_e1 = 0;
                w_cb0 = w_cb1;
                w_cv0 = w_cv1;
                w_ct0 = w_ct1;
            }
            const uint64_t wants = __builtin_amdgcn_ballot_w64(ph == Q_WANT);
            if (wants != 0) {
                // the j-th lane that wants a read takes the reservoir's j-th index; a lane that finds it empty parks for an
                // iteration (a dummy gather, like Q_STEP's) while a claim is on its way, and is done when none can come
                const uint32_t j = __builtin_amdgcn_mbcnt_hi((uint32_t)(wants >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)wants, 0u));
                const uint32_t have0 = w_e0 - w_n0, have1 = w_e1 - w_n1, nw = (uint32_t)__popcll(wants);
                const bool over = !w_pend && w_dry;
                if (STAGE) {
                    // a claim takes its slot when its first read is handed out (not when it arrives: it would hold the slot
                    // for the iterations it waits in the reservoir)
                    if (have0 != 0 && !w_ct0) {
                        take_slot(w_n0, have0, w_cb0, w_cv0);
                        w_ct0 = true;
                    }
                    if (nw > have0 && have1 != 0 && !w_ct1) {
                        take_slot(w_n1, have1, w_cb1, w_cv1);
                        w_ct1 = true;
                    }
                }
                if (ph == Q_WANT) {
                    const bool got = j < have0 + have1;
                    rd = j < have0 ? w_n0 + j : w_n1 + (j - have0);
                    ph = got ? Q_READ : (over ? Q_DONE : Q_WANT);
                    addr = got ? item_b + (uint64_t)rd * ITEM_BYTES : rows_b;
                    if (STAGE) cidx = (got && (j < have0 ? w_cv0 : w_cv1)) ? rd + (j < have0 ? w_cb0 : w_cb1) : C_NONE;
                }
                const uint32_t t0 = nw < have0 ? nw : have0, t1 = (nw - t0) < have1 ? (nw - t0) : have1;
                w_n0 += t0;
                w_n1 += t1;
                if (nw > have0 + have1) w_wait = 0;  // (lanes are parked: no reason left to hold the claim back)
                if (w_n0 == w_e0) {
                    w_n0 = w_n1;
                    w_e0 = w_e1;
                    w_n1 = w_e1 = 0;
                    w_cb0 = w_cb1;
                    w_cv0 = w_cv1;
                    w_ct0 = w_ct1;
                }
            }
            // refill ahead of need: the next iteration can take at most 64 reads (a lane ends one read per iteration)
            w_wait -= w_wait != 0 ? 1u : 0u;
            w_pend = !w_dry && w_wait == 0 && w_n1 == w_e1 && (w_e0 - w_n0) < 64u;
        }
        if (EARLY) issue_gather();  // the next iteration's
        if (MODE == SPX_MODE_MS && CHUNK != 2) {
            // Eight finished groups per round: lanes 8j .. 8j + 7 write the j-th of them, two pointers (16 bytes) each -- whole
            // 128-byte lines instead of a lane's 16-byte stores into 64 different lines (which cost the MS walk a third of
            // its time: profiles/r03_ms_pointer_stores.txt), once per iteration (at most one group per lane completes in it)
            const uint32_t lane = tid & 63;
            uint64_t todo = __builtin_amdgcn_ballot_w64(pflush);
            while (todo != 0) {
                while (todo != 0) {
                    uint32_t src = 64;
#pragma unroll
                    for (int kx = 0; kx < PNG; ++kx) {
                        if (todo != 0) {
                            const uint32_t l = (uint32_t)__builtin_ctzll(todo);
                            todo &= todo - 1;
                            src = (lane / PLPG) == (uint32_t)kx ? l : src;
                        }
                    }
                    const bool valid = src < 64;
                    const uint32_t from = valid ? src : lane;
                    const uint32_t sxi = (uint32_t)__shfl((int)pfxi, (int)from);
                    const uint32_t sm = (uint32_t)__shfl((int)m, (int)from);
                    const uint64_t sbase = u64of((uint32_t)__shfl((int)(uint32_t)base, (int)from), (uint32_t)__shfl((int)(uint32_t)(base >> 32), (int)from));
                    const uint32_t e2 = (lane % PLPG) * 2;
                    const uint64_t lo = sbase + sxi, hi = sbase + sm;  // the group's positions that belong to the read: [lo, hi)
                    const uint64_t p0 = (lo & ~(uint64_t)(PGRP - 1)) + e2;
                    const uint64_t v0 = s_ptrs[e2 * PROW + (tid & ~63u) + from];
                    const uint64_t v1 = s_ptrs[(e2 + 1) * PROW + (tid & ~63u) + from];
                    const bool ok0 = valid && p0 >= lo && p0 < hi, ok1 = valid && p0 + 1 >= lo && p0 + 1 < hi;
                    const uint64_t q0p = (uint64_t)((int64_t)(v0 << 16) >> 16), q1p = (uint64_t)((int64_t)(v1 << 16) >> 16);
                    if (ok0 && ok1) {
                        // 16 bytes of a line that the wavefront writes whole: non-temporal stores (the line is complete
                        // and nobody reads it before the kernel ends)
                        __builtin_nontemporal_store(q0p, b.out_pointers + p0);
                        __builtin_nontemporal_store(q1p, b.out_pointers + p0 + 1);
                    } else if (ok0) {
                        b.out_pointers[p0] = q0p;
                    } else if (ok1) {
                        b.out_pointers[p0 + 1] = q1p;
                    }
                    if (DOC) {
                        const uint32_t d0 = (uint32_t)(v0 >> 48), d1 = (uint32_t)(v1 >> 48);
                        if (NARROW) {
                            uint16_t* const dp = reinterpret_cast<uint16_t*>(b.out_docs) + p0;
                            if (ok0 && ok1)
                                *reinterpret_cast<H16x2*>(dp) = H16x2{d0 | (d1 << 16)};
                            else if (ok0)
                                dp[0] = (uint16_t)d0;
                            else if (ok1)
                                dp[1] = (uint16_t)d1;
                        } else {
                            if (ok0 && ok1)
                                *reinterpret_cast<U32x2*>(b.out_docs + p0) = U32x2{d0, d1};
                            else if (ok0)
                                b.out_docs[p0] = d0;
                            else if (ok1)
                                b.out_docs[p0 + 1] = d1;
                        }
                    }
                }
                // the pointer that had to wait takes its place (slot PGRP - 1 of the next group); when it was its read's last,
                // that group is complete as well (rare: a second round)
                pflush = false;
                if (pheld) {
                    s_ptrs[(PGRP - 1) * PROW + tid] = phold;
                    pheld = false;
                    pflush = pheld_end;
                    pfxi = 0;
                }
                todo = __builtin_amdgcn_ballot_w64(pflush);
            }
        }
        if (DSTAGE) {
            // the same for PML's document ids: eight finished groups per round, lane 8j + e writes ids 4e .. 4e + 3 of the
            // j-th of them (64 contiguous bytes of 16-bit ids per group)
            const uint32_t lane = tid & 63;
            uint64_t todo = __builtin_amdgcn_ballot_w64(pflush);
            while (todo != 0) {
                while (todo != 0) {
                    uint32_t src = 64;
#pragma unroll
                    for (int kx = 0; kx < 8; ++kx) {
                        if (todo != 0) {
                            const uint32_t l = (uint32_t)__builtin_ctzll(todo);
                            todo &= todo - 1;
                            src = (lane >> 3) == (uint32_t)kx ? l : src;
                        }
                    }
                    const bool valid = src < 64;
                    const uint32_t from = valid ? src : lane;
                    const uint32_t sxi = (uint32_t)__shfl((int)pfxi, (int)from);
                    const uint32_t sm = (uint32_t)__shfl((int)m, (int)from);
                    const uint64_t sbase = u64of((uint32_t)__shfl((int)(uint32_t)base, (int)from), (uint32_t)__shfl((int)(uint32_t)(base >> 32), (int)from));
                    const uint32_t e4 = (lane & 7) * 4;
                    const uint64_t lo = sbase + sxi, hi = sbase + sm;  // the group's positions that belong to the read: [lo, hi)
                    const uint64_t p0 = (lo & ~(uint64_t)(DGRP - 1)) + e4;
                    const uint16_t* const sp = &s_docs[((tid & ~63u) + from) * DROW + e4];
                    const uint32_t w0 = *reinterpret_cast<const uint32_t*>(sp), w1 = *reinterpret_cast<const uint32_t*>(sp + 2);
                    if (valid && p0 >= lo && p0 + 4 <= hi) {
                        if (NARROW)
                            *reinterpret_cast<H16x4*>(reinterpret_cast<uint16_t*>(b.out_docs) + p0) = H16x4{u64of(w0, w1)};
                        else
                            *reinterpret_cast<U32x4*>(b.out_docs + p0) = U32x4{w0 & 0xffffu, w0 >> 16, w1 & 0xffffu, w1 >> 16};
                    } else if (valid) {
#pragma unroll
                        for (int t4 = 0; t4 < 4; ++t4) {
                            const uint32_t dv = ((t4 & 2 ? w1 : w0) >> ((t4 & 1) * 16)) & 0xffffu;
                            if (p0 + t4 >= lo && p0 + t4 < hi) {
                                if (NARROW)
                                    reinterpret_cast<uint16_t*>(b.out_docs)[p0 + t4] = (uint16_t)dv;
                                else
                                    b.out_docs[p0 + t4] = dv;
                            }
                        }
                    }
                }
                pflush = false;
                if (pheld) {
                    s_docs[tid * DROW + (DGRP - 1)] = (uint16_t)phold;
                    pheld = false;
                    pflush = pheld_end;
                    pfxi = 0;
                }
                todo = __builtin_amdgcn_ballot_w64(pflush);
            }
        }
        if (PML && want_len) {
            // lengths[p] = distance from p to the first reset at or after it (the read's end when there is none):
            // the reference's `length = 0` / `length++` (compute_ms_pml.cpp:249-250, 266-276) read from the other side
            uint64_t todo = __builtin_amdgcn_ballot_w64(flush);
            const uint32_t lane = tid & 63;
            while (todo != 0) {
                const uint32_t l = (uint32_t)__builtin_ctzll(todo);
                todo &= todo - 1;
                const uint64_t wbits = u64of((uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)fbits, l),
                                             (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(fbits >> 32), l));
                const uint32_t wxi = (uint32_t)__builtin_amdgcn_readlane((int)fxi, l);
                const uint32_t wnr = (uint32_t)__builtin_amdgcn_readlane((int)nr, l);
                const uint32_t wm = (uint32_t)__builtin_amdgcn_readlane((int)m, l);
                const uint64_t wbase = u64of((uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)base, l),
                                             (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(base >> 32), l));
                const uint32_t cnt = wm - wxi;  // characters of the read from wxi on: 64 or more but for the read's top word
                const uint64_t t = wbits >> lane;
                const uint32_t v = t != 0 ? (uint32_t)__builtin_ctzll(t) : wnr - (wxi + lane);
                if (lane < cnt) {
                    if (NARROW)
                        reinterpret_cast<uint16_t*>(b.out_lengths)[wbase + wxi + lane] = (uint16_t)v;
                    else
                        b.out_lengths[wbase + wxi + lane] = v;
                }
            }
        }
        if (PML && CHUNK != 2 && flush) nr = fbits != 0 ? fxi + (uint32_t)__builtin_ctzll(fbits) : nr;
    }
#undef WIN_AT
#undef CUR_C
#undef COUNT
    if ((tid & 63) == 0) {
        if (CHUNK == 2) {  // characters walked a second time: not steps (or jumps) of the batch
            atomicAdd(&b.counters->reserved0, (unsigned long long)w_again);
        } else {
            atomicAdd(&b.counters->jumps, (unsigned long long)w_jumps);
            atomicAdd(&b.counters->pred_jumps, (unsigned long long)w_pred);
        }
        atomicAdd(&b.counters->row_loads, (unsigned long long)w_rows);
        atomicAdd(&b.counters->dir_loads, (unsigned long long)w_dir);
    }
    (void)sample;
    (void)doc;
    (void)s_ptrs;
    (void)s_docs;
    (void)seen;
    (void)fb;
    (void)ch_flags;
    (void)ch_ckpt;
    (void)tlimit;
    (void)cka;
    (void)ckb;
    (void)w_again;
    (void)w_n0, (void)w_e0, (void)w_n1, (void)w_e1, (void)w_pend, (void)w_dry, (void)w_wait, (void)claimed;
    (void)cidx, (void)c_first, (void)c_n, (void)c_left, (void)w_cb0, (void)w_cb1, (void)w_cv0, (void)w_cv1, (void)w_ct0, (void)w_ct1;
    (void)take_slot, (void)cw0, (void)s_cbase, (void)s_cword, (void)s_ccls, (void)s_clen;
    // every character of the batch is one step
    if (CHUNK != 2 && blockIdx.x == 0 && tid == 0) atomicAdd(&b.counters->steps, (unsigned long long)(b.offs[b.nreads] - b.offs[0]));
}
