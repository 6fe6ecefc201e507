// spx_internal.h -- private definitions shared by the library's translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/spumoni_gpu.h"
#include "spx_layout.h"

namespace spx {

void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what, const char* file, int line);
// hipSetDevice(device) after checking that it exists and is a gfx950 (SPX_E_NODEVICE: no usable device)
int select_device(int device);

#define SPX_HIP(call)                                                        \
    do {                                                                     \
        hipError_t e_ = (call);                                              \
        if (e_ != hipSuccess) return spx::hip_fail(e_, #call, __FILE__, __LINE__); \
    } while (0)

// The host-buffer entry points enqueue their copies on streams of the handle and leave early on any error after that.  A copy
// that is still reading the caller's inputs (or writing its outputs) when the call has already failed would leave work in
// flight on memory the caller may free: every way out that is not through done(SPX_OK) waits first -- for the stream, or
// (device_wide: the pipelines run on several streams of the handle) for the device.
struct QuietOnError {
    hipStream_t st;
    bool device_wide;
    bool ok = false;
    explicit QuietOnError(hipStream_t s, bool wide = false) : st(s), device_wide(wide) {}
    int done(int rc) {
        ok = rc == SPX_OK;
        return rc;
    }
    ~QuietOnError() {
        if (ok) return;
        if (device_wide)
            (void)hipDeviceSynchronize();
        else
            (void)hipStreamSynchronize(st);
    }
};

// counters written by the walk kernels (one instance per index, device memory)
struct WalkCounters {
    unsigned long long reserved0;
    unsigned long long steps;
    unsigned long long jumps;
    unsigned long long pred_jumps;
    unsigned long long row_loads;
    unsigned long long dir_loads;
    unsigned long long error;      // non-zero: a structural invariant was violated
    unsigned long long pad_;
    // the next read index (less the launch's lanes) that the plain k_walk_fast launch of a batch with more reads than lanes
    // hands out (spx_walk_fast.inc: the dynamic deal).  Zero when that launch starts: zeroed with the rest once per call,
    // and by launch_lanes itself before a call's second such launch (spx_index::claim_used)
    unsigned long long claim;
};

// ---- long reads: exact speculative chunking (spx_walk.hip) -----------------------
// The walk of a read is one dependent chain; a batch with fewer reads than the chip has lanes is
// latency-bound.  Such a batch is cut into chunks -- a read's intersection with an aligned block of
// CHUNK characters of the concatenated input -- and
//   pass 1  every chunk is walked from the default state (pos = n - 1): right for a read's last
//           chunk, speculative for the others;
//   pass 2  for every other chunk, the walk that ended the chunk above it (its recorded end state)
//           is carried on into the chunk, overwriting the speculative results, until its position
//           equals the position the speculative walk recorded at the same character (checkpoints):
//           from there on the two walks are the same walk;
//   pass 3  per read, top down: `length` / `sample` are counters that the walk only adds to until
//           the next jump resets them, so what is left of a wrong start value is a constant
//           offset (a stale value, for the document id) up to the first reset below each seam:
//           patched from the recorded values;
//   What pass 2 wrote is only the truth if the state it entered the chunk with was: true for the
//   chunk below a read's last, and from there down as long as every seam closed (the recorded end
//   state of a chunk whose seam closed IS the true walk's).  A seam left open -- pass 2 reached the
//   chunk's first character still apart from the speculative walk -- breaks the chain: between
//   rounds a scan per read (k_chunk_scan) follows the chain down to the first open seam and has the
//   chunk below it entered again in the next round, now with the state the true walk ended in, down
//   to at least where the earlier, unfounded walk had stopped writing.  After the last round a read
//   whose chain is still broken is walked again the plain way.  Then the bin classifier runs over
//   the finished lengths.
struct ChunkDesc {     // 16 B
    uint64_t gend;     // index (in the concatenated input) one past the chunk's last character
    uint32_t len;      // characters
    uint32_t rd;       // read
};
struct WalkState {     // 32 B: what a walk carries from one character to the next
    uint32_t k0;       // landing target of the last step: run ...
    uint32_t length;   // PML length counter
    uint64_t offp;     // ... and offset (OFF_END: last position of the run)
    uint64_t sample;   // MS pointer counter
    uint32_t doc;      // current document id
    uint32_t flags;    // bit 0: a reset happened since the state's owner started
};
struct SeamRec {       // 64 B, one per chunk that is not its read's last: where and how pass 2 ended
    uint64_t t;        // pass 2 stopped with the results of [t, chunk end) written; t == chunk start: never met
    uint32_t met;      // bit 0: positions met at t (0: ran to the chunk's start); bits 8..: round of pass 2
    uint32_t reset_above;  // pass 2 saw a reset between the chunk's end and t
    WalkState ext;     // pass 2's counters at t
    uint32_t spec_length, spec_doc;
    uint64_t spec_sample;  // the speculative walk's counters at t
};
constexpr uint32_t CKPT_SHIFT = 4;  // a checkpoint every 16 characters

struct ChunkArgs {
    const ChunkDesc* desc;       // chunks, a read's chunks consecutive, last chunk of a read first... no: ascending
    const uint64_t* nchunks;     // device counter
    WalkState* ends;             // per chunk: state after the chunk's first (lowest) character
    WalkState* ckpt;             // per 16 characters of the input: state before character 16 * i - 1
    SeamRec* seams;              // per chunk
    uint8_t* flags;              // per character: bit 0 length / sample were reset, bit 1 doc was set
    uint32_t* read_fail;         // per read: the chain of seams is still broken after the last round
    const uint64_t* chunk_start; // per read: first chunk
    WalkState* reentry;          // per chunk: state to enter it with in a later round (flags: how far down to write)
    uint64_t* vtop;              // per read: chunks from here up hold the truth
    uint32_t* pending;           // per round of pass 2: chunks to enter (round 1: unused)
    uint32_t round;              // pass 2: 1 = every chunk but a read's last, later = the chunks below open seams
    uint32_t last_round;         // pass 2: an open seam now condemns the read to the plain walk
};
constexpr uint32_t CHUNK_TOP = 0x80000000u, CHUNK_BOTTOM = 0x40000000u, CHUNK_ACTIVE = 0x20000000u;  // in ChunkDesc::len
constexpr uint32_t CHUNK_LEN_MASK = 0x1fffffffu;
constexpr int CHUNK_EXTRA_ROUNDS = 3;

struct BatchArgs {
    const uint8_t* seqs;   // readable for round_up(total_chars, 4) + 32 bytes
    const uint64_t* offs;
    uint64_t nreads;
    uint64_t total_chars;
    uint32_t* out_lengths;
    uint64_t* out_pointers;
    uint32_t* out_docs;
    spx_class* out_class;
    uint64_t bin_width;
    uint64_t bin_magic;  // floor(2^64 / bin_width) + 1: division by multiplication in the kernel
    uint64_t max_value_thr;
    WalkCounters* counters;
    uint32_t lanes_per_wave;  // active lanes per wavefront (64 unless the batch is small)
    uint32_t narrow;          // out_lengths / out_docs point to uint16_t arrays (reads < 65536 characters)
    ChunkArgs ch;             // chunked walks only
    const uint32_t* only_flagged;  // plain walk: skip the reads whose flag is 0 (fallback after chunking)
    // reads that were digested on the device a moment ago (spx_digest.hip) and are still where the digestion parked
    // them: read q's characters are seqs[in_starts[q] ..), offs[q + 1] - offs[q] of them, while offs places its results
    // as always (k_walk_fast only; null: seqs[offs[q] ..))
    const uint64_t* in_starts;
    // PML, plain walk: the lengths leave the walk as ONE BIT per character (length == 0, i.e. "reset here":
    // a PML length is the distance to the next reset at or after it, compute_ms_pml.cpp:249-250, 266-276) and
    // k_expand_lengths writes out_lengths from the bits as a stream.  Read q's bits: 16-byte pairs of words
    // [((offs[q] - offs[0]) >> 7) + q, ...) (pairs of different reads never overlap), bit p & 63 of word p >> 6
    // for character p of the read.
    uint64_t* len_mask;
    // k_walk_fast, plain and full launches: the word the wavefronts claim their reads from after the first, strided round
    // (&counters->claim; null: every round is strided).  Set by launch_lanes.
    unsigned long long* claim;
    uint64_t len_mask_pairs;  // 16-byte pairs len_mask holds (sized from total_chars: checked, the caller may be wrong)
};

__device__ inline unsigned long long wave_sum(unsigned long long v) {  // over the wavefront's 64 lanes, in every lane
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

}  // namespace spx

struct spc_params;  // include/spumoni_chain.h
struct spa_params;  // include/spumoni_align.h
struct spe_params;  // include/spumoni_extend.h
struct spn_mapping;  // include/spumoni_map.h

namespace spx {
// The device arrays of an index once more than one handle uses them: spx_index_clone onto the SAME device hands out a
// second query context -- its own counters, scratch, stream and locks -- over the same (read-only) arrays instead of a
// copy; the arrays go when the last handle does.
struct ArrayOwner {
    int device = 0;
    void* p[10] = {};
    ~ArrayOwner() {
        (void)hipSetDevice(device);
        for (void* a : p)
            if (a) (void)hipFree(a);
    }
};
}  // namespace spx

struct spx_index {
    int device = 0;
    uint64_t n = 0, r = 0;
    bool has_samples = false, has_docs = false;
    spx::Row* rows = nullptr;
    uint32_t* q_alloc = nullptr;  // Q = q_alloc + 1
    spx::JumpRow* dirrows = nullptr;
    char* fat = nullptr;  // slots of DevIndex::fat_stride bytes
    uint32_t* fat_js = nullptr;  // fatjs_count(nfat) entries
    spx::Aux* aux = nullptr;
    uint64_t* ss_by_run = nullptr;
    uint32_t* rundocs = nullptr;
    spx::LetterInfo* letters = nullptr;
    uint8_t* text = nullptr;
    uint64_t n_text = 0;
    // bytes of every device array above, in the order of spx::index_arrays() (saved / cloned as they are)
    static constexpr int NARR = 10;
    uint64_t arr_bytes[NARR] = {};
    std::shared_ptr<spx::ArrayOwner> owner;  // set once the arrays are shared with a same-device clone (else: this handle frees them)
    // host-buffer queries (spx_query_batch*, spx_digest_*batch, spx_query_text_*) run on a stream of the handle's own, so
    // that two handles on one device -- the CLI's two workers per device -- overlap one's copies with the other's kernels
    hipStream_t ctx_stream = nullptr;
    // the digestion's scratch slots (digest_scr below), the stream its last call ran on and what that call enqueued
    static constexpr int NDIGSCR = 15;
    hipEvent_t ev_dig = nullptr;
    hipStream_t dig_stream = nullptr;
    bool dig_used = false;
    spx::DevIndex view{};
    spx::WalkCounters* counters = nullptr;
    bool claim_used = false;  // a launch of this call has claimed reads from counters->claim since the counters were zeroed
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_done = nullptr;
    bool have_timing = false;
    hipStream_t last_stream = nullptr;
    uint64_t device_bytes = 0;
    int waves_per_cu = 0; // 0 = default occupancy target
    int occ_blocks[8] = {};  // resident 256-thread blocks per CU, per kernel variant (4..7: k_walk_fast)
    int occ_blocks_dyn[4] = {};  // ... of k_walk_fast's instances that deal on demand (their claim-staged output takes more LDS)
    int num_cus = 0;
    int force_lanes_per_wave = 0;  // experiment knob: 0 = automatic
    int force_digest_kernel = 0;   // test knob: 0 automatic, 1 lane-per-read, 2 wavefront-per-read, 3 lane-per-chunk
    int digest_parked = 0;         // digest + walk: 0 the digested reads stay parked when the batch fills the device, 1 never, 2 whenever the walk can take them
    uint8_t charhash[4] = {0, 0, 0, 0};  // -m digestion: 8-bit character hashes of A, C, G, T
    char source_tag[128] = {0};          // spx_index_set_source_tag(): the caller's fingerprint of the index files
    // host-buffer queries of large batches run as a pipeline over chunks of reads: copy in,
    // walk, copy out on three streams (created on first use)
    static constexpr int PIPE_CHUNKS = 10;  // pieces of a pipelined host batch (growing: run_pipelined)
    hipStream_t pipe_s[3] = {nullptr, nullptr, nullptr};
    hipEvent_t pipe_in[PIPE_CHUNKS] = {}, pipe_k[PIPE_CHUNKS] = {};
    std::mutex mu;       // device-buffer queries / options
    std::mutex host_mu;  // host-buffer queries (taken before mu)
    // Device scratch owned by the index: grow-only, so that no call pays a hipMalloc / hipFree of its own.  A buffer that grows
    // is freed first, which synchronises the whole device: a pipeline sizes its slots for the worst case before it starts.
    struct Scratch {
        void* p = nullptr;
        size_t cap = 0;
        hipError_t grow(size_t bytes, void** out) {  // the one growth rule: a quarter and 256 bytes of head-room
            if (cap < bytes) {
                if (p) (void)hipFree(p);
                p = nullptr;
                cap = 0;
                const size_t want = bytes + bytes / 4 + 256;
                const hipError_t e = hipMalloc(&p, want);
                if (e != hipSuccess) return e;
                cap = want;
            }
            *out = p;
            return hipSuccess;
        }
        int reserve(size_t bytes, void** out) {
            SPX_HIP(grow(bytes, out));
            return SPX_OK;
        }
    };
    // host-buffer queries (under host_mu).  The walk reads S_SEQ; under digestion the caller's reads go to S_RAW and S_SEQ
    // holds what the digestion made of them (reads_slot).  S_GAP .. S_TEXT: text output, + i for the stream
    enum { S_SEQ, S_OFFS, S_LEN, S_PTR, S_DOC, S_CLASS, S_RAW, S_DIG_OFFS, S_GAP, S_SCAN,
           S_LINE_BYTES, S_LINE_START = S_LINE_BYTES + 3, S_TEXT = S_LINE_START + 3, S_COUNT = S_TEXT + 3 };
    static constexpr int reads_slot(int digest_kind) { return digest_kind ? S_RAW : S_SEQ; }
    Scratch scratch[S_COUNT];
    // chunked walks and, C_LEN_BITS, the PML reset bits of every walk (under mu)
    enum { C_DESC, C_ENDS, C_SEAMS, C_CKPT, C_FLAGS, C_FAIL, C_CNT, C_CUB, C_LEN_BITS, C_COUNT };
    Scratch chunk_scr[C_COUNT];
    Scratch digest_scr[NDIGSCR];  // spx_digest.hip (under mu): handed out in the order asked for, the last one to the scans
    // The staged walk (spx_stage.hip, under host_mu) under spv_assign_batch, spm_mems_begin and spp_place_batch: two buffer
    // sets of the seven arrays a piece of reads needs on its way through digestion and walk, G_SET_STRIDE slots each, and
    // the two streams the pieces of a batch alternate between.  One group for the three products: each holds host_mu for
    // its whole call, and what a product keeps beyond its call (spm_mems_fetch: M_OUT, M_OUT_DOCS) is the product's own.
    enum { G_RAW, G_OFFS, G_DIG, G_DIG_OFFS, G_LEN, G_DOC, G_PTR, G_SET_STRIDE, G_COUNT = 2 * G_SET_STRIDE };
    Scratch stage_scr[G_COUNT];
    hipStream_t stage_s[2] = {nullptr, nullptr};
    // What a product's kernels count and how long they take (product_open .. product_collect below, under mu): the device
    // words they count in, zeroed in front of every launch; the events around the kernels enqueued last, the marks between
    // them -- from mark i on the time belongs to step label[i], from ev0 on to step label0, -1: to none -- and the stream
    // they ran on; and what the call has collected so far: acc[i] is the sum of word i (the error word's stays 0), error
    // the OR of the error word, ms the time between ev0 and ev1, step_ms the time of every labelled step.
    struct Product {
        static constexpr int WORDS = 17, MARKS = 6, STEPS = 6;  // (the extended CIGARs' counters, marks and steps)
        Scratch counters;
        hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_mark[MARKS] = {};
        int label0 = -1, label[MARKS] = {}, nmarks = 0;
        hipStream_t stream = nullptr;
        bool have = false, pending = false;
        uint64_t acc[WORDS] = {};
        uint64_t error = 0;
        float ms = 0, step_ms[STEPS] = {};
    };
    // The records of a _begin that wait on the device for its _fetch, or for the product that goes on from them
    // (ready_publish / ready_take / ready_fetch below, under host_mu): n entries of `reads` reads.
    struct Ready {
        bool ok = false;
        uint64_t n = 0, reads = 0;
    };
    // document votes (spx_docvote.hip): read lists and the long reads' tables (under mu), then the records of the staged
    // walk's two buffer sets (under host_mu)
    enum { V_MEDIUM, V_LONG, V_TILES, V_ACC, V_TABLE, V_OUT0, V_COUNT = V_OUT0 + 2 };
    Scratch vote_scr[V_COUNT];
    Product votes;  // acc: reads short, medium, long, empty; voting positions; tiles
    // matches (spx_mems.hip): the bitmap of reported starts, its prefix sums and the scan's space (under mu), then
    // spm_mems_begin's match offsets (under host_mu); the capacity of the last call; and the records that wait for
    // spm_mems_fetch (reads: unused), with or without their document ids
    enum { M_BITS, M_PREFIX, M_CUB, M_MOFFS, M_OUT, M_OUT_DOCS, M_COUNT };
    Scratch mems_scr[M_COUNT];
    Product mems;  // acc: values, matches, longest; steps: count, write -- two intervals, in the host form with a wait between
    uint64_t mems_capacity = 0;
    Ready mems_ready;
    bool mems_ready_docs = false;
    // placements (spx_place.hip): the records of the staged walk's two buffer sets (under host_mu)
    Scratch place_scr[2];
    Product place;  // acc: values, placed, seed values, extended values
    // chains (spx_chain.hip): the records of spc_chain_batch (under host_mu); its matches are spm_mems_begin's, in mems_scr
    enum { H_OUT, H_COUNT };
    Scratch chain_scr[H_COUNT];
    Product chain;  // acc: reads, anchors, chained reads, chain anchors, candidates
    // alignments (spx_align.hip): the gap counts, their offsets, the per-gap table, where each gap's strings start, the list
    // of the gaps that take a wavefront and the scan's space (under mu), then spa_align_batch's chain records, its
    // alignments and pred (under host_mu)
    enum { L_CNT, L_GOFFS, L_GAPS, L_DESC, L_LIST, L_CUB, L_CHAINS, L_OUT, L_PRED, L_COUNT };
    Scratch align_scr[L_COUNT];
    Product align;  // acc: reads, aligned reads, gaps, filled gaps, cells; steps: count and scan, walk, fill, reduce
    // CIGARs (spx_cigar.hip): the scratch of the shared count, walk and reduce in the slots they have above, the list of the
    // gaps that take a wavefront (two kinds, from either end), each gap's words of path and their offsets, the path, the
    // wavefronts' trace buffers and the reads' entry counts (under mu), then spg_cigar_begin's chain records, alignments,
    // pred, op offsets and entries (under host_mu); and the entries that wait for spg_cigar_fetch
    enum { TB_CNT, TB_GOFFS, TB_GAPS, TB_DESC, TB_LIST, TB_CUB, TB_PW, TB_POFFS, TB_PATH, TB_TRACE, TB_OCNT, TB_CHAINS, TB_OUT,
           TB_PRED, TB_OOFFS, TB_OPS, TB_EPW, TB_EPOFFS, TB_ERES, TB_ETRACE, TB_ENDS, TB_COUNT };
    Scratch cigar_scr[TB_COUNT];
    Product cigar;  // acc: the words of CigarCounters; steps: plan, lane fills, wavefront fills, emit, reduce
    Ready cigar_ready;
    // extended CIGARs (spx_extend.hip): the same set once more, the product's own (both drive the code of
    // spx_cigar_kernels.h through a TraceView), with the slots only this product fills: each end's words of path and their
    // offsets, the ends' results, the trace buffers of the ends' wavefronts (under mu) and spe_extend_begin's ends (under
    // host_mu)
    Scratch extend_scr[TB_COUNT];
    Product extend;  // acc: as cigar's; steps: cigar's five, then the ends (which run between plan and lane fills)
    Ready extend_ready;
    // mappings (spx_map.hip): the piece starts P[0 .. map_pieces] on the device beside the index -- this handle's own
    // copy, a clone has another -- and the lengths they came from; each read's plan, entry count and the scan's space
    // (under mu), then spn_map_begin's read offsets, records, op offsets and entries (under host_mu); and the entries that
    // wait for spn_map_fetch
    uint64_t* map_P = nullptr;
    uint64_t map_pieces = 0;
    uint32_t map_strands = 0;
    std::vector<uint64_t> map_seq_lengths;
    enum { N_PLAN, N_OCNT, N_CUB, N_ROFFS, N_OUT, N_OOFFS, N_OPS, N_COUNT };
    Scratch map_scr[N_COUNT];
    Product map;  // acc: reads, mapped, cut, reverse, entries in and out, characters cut; steps: locate and count, write
    Ready map_ready;
    // What the coverage and the pileup keep alike (spx_genome_kernels.h): one Product per step -- add, finish, output --; the
    // shared scratch: the list of the reads that take a wavefront, the scans' space, the output's tile counts and offsets
    // (under mu), its count word and records (under host_mu); from S_OWN on the product's own, first the ARRAYS arrays a
    // reset sizes for the genome.  G: the forward genome they were sized for, 0 without a reset; dropped: spn_set_sequences
    // took them away; dirty: the finished arrays are older than the summed ones; acc: the add's first counters over the adds
    // the stats speak of; n_out: what the last output counted; ready, ready_n: the records that wait for the fetch
    struct GenomeAcc {
        enum { ADD, FIN, OUT };
        enum { S_LONG, S_CUB, S_CUB2, S_TCNT, S_TOFFS, S_NOUT, S_RECORDS, S_OWN, ARRAYS = 5, S_COUNT = S_OWN + 7 };
        Product step[3];  // (acc unused)
        Scratch scr[S_COUNT];
        uint64_t G = 0, acc[8] = {}, n_out = 0, ready_n = 0;
        bool dropped = false, dirty = false, ready = false;
        int sw = 64;  // a read of more entries than this takes a wavefront
        float step_ms[3] = {};
    };
    // coverage (spx_cover.hip): diff, mism, depth, the per-sequence counts, the summary; the output is the runs.  acc: reads,
    // mapped, added, skipped, intervals, atomics.  sw: the "cover_switch" option.  cover_mapped: mapped reads since the reset
    enum { D_DIFF = GenomeAcc::S_OWN, D_MISM, D_DEPTH, D_COUNTS, D_OUT };
    GenomeAcc cover;
    uint64_t cover_mapped = 0;
    // pileup and calls (spx_call.hip): alt, other, ins, ddiff, del, the batch's reads and their offsets (copied on a stream of
    // the product's own, so that the copy overlaps spn_map_begin); the output is the calls.  sw: the "call_switch" option
    enum { PL_ALT = GenomeAcc::S_OWN, PL_OTHER, PL_INS, PL_DDIFF, PL_DEL, PL_READS, PL_ROFFS };
    GenomeAcc call;
    hipStream_t call_copy_s = nullptr;
    hipEvent_t call_copy_ev = nullptr;
    // consensus (spx_consensus.hip): the emitted byte of every position, the tiles' letter counts and their offsets, each
    // sequence's (letters, bytes) and their running sums, the scans' space (under mu), then sps_consensus_begin's records
    // and body (under host_mu), which wait for sps_consensus_fetch: cons_seqs records, cons_bytes bytes.  cons_G: the
    // positions of the last call
    enum { CS_EMIT, CS_TCNT, CS_TOFFS, CS_PAIRS, CS_STARTS, CS_CUB, CS_CUB2, CS_RECORDS, CS_BODY, CS_NOUT, CS_COUNT };
    Scratch cons_scr[CS_COUNT];
    Product cons;  // acc: letters, substituted, deleted, masked, insertion sites, bytes; steps: count, scans, write
    uint64_t cons_G = 0, cons_seqs = 0, cons_bytes = 0;
    bool cons_ready = false;
    // spx_query_text_begin -> spx_query_text_fetch: the streams' sizes and where they wait on the device
    uint64_t text_bytes[3] = {0, 0, 0};
    uint64_t text_nreads = 0;
    bool text_ready = false;
    spx_class* text_cls_host = nullptr;  // the class records travel with the text (spx_query_text_fetch)
    // A few words the host waits for at the end of a step (stream sizes, the digested total, the walk's counters): written by
    // a kernel into page-locked host memory, NOT copied -- a device-to-host copy of 8 bytes queues on the copy engine behind
    // whatever another query context of the same device is copying out (1.4 ms per super-batch of text), which made
    // spx_query_text_begin of one worker wait for spx_query_text_fetch of the other (profiles/r05_cli_overlap.txt).
    int blocking_sync = 0;          // "blocking_sync" option: the host-buffer text queries wait for their stream on an event with
    hipEvent_t ev_wait = nullptr;   // hipEventBlockingSync (the thread sleeps) instead of hipStreamSynchronize (it spins on a core)
    uint64_t* h_pub = nullptr;      // host address
    uint64_t* h_pub_dev = nullptr;  // the same memory as the device sees it
    int chunk_mode = 0;   // "chunk_mode" option: 0 automatic, 1 never, 2 always
    int chunk_shift = 0;  // "chunk_shift" option: log2 of the chunk size (0 = automatic)
    int chunk_len = 0;    // "chunk_len" option: chunk size in characters (rounded up to 16; 0 = automatic)
    uint64_t last_chunk_len = 0, last_chunk_bound = 0;  // last query: chunk size (0 = plain walk), chunk bound
};

namespace spx {
// the device arrays of an index, in a fixed order (cache file / clone)
enum { A_ROWS, A_DIRROWS, A_FAT, A_FATJ, A_Q, A_AUX, A_SSRUN, A_RUNDOCS, A_LETTERS, A_TEXT };
inline void index_arrays(spx_index* ix, void*** out) {
    out[A_ROWS] = (void**)&ix->rows;
    out[A_DIRROWS] = (void**)&ix->dirrows;
    out[A_FAT] = (void**)&ix->fat;
    out[A_FATJ] = (void**)&ix->fat_js;
    out[A_Q] = (void**)&ix->q_alloc;
    out[A_AUX] = (void**)&ix->aux;
    out[A_SSRUN] = (void**)&ix->ss_by_run;
    out[A_RUNDOCS] = (void**)&ix->rundocs;
    out[A_LETTERS] = (void**)&ix->letters;
    out[A_TEXT] = (void**)&ix->text;
}
// points the kernel-visible view at the index's arrays (scalars of the view are kept)
inline void bind_view(spx_index* ix) {
    DevIndex& v = ix->view;
    v.rows = ix->rows;
    v.dirrows = ix->dirrows;
    v.fat = ix->fat;
    v.Q = ix->q_alloc ? ix->q_alloc + 1 : nullptr;
    v.aux = ix->aux;
    v.ss_by_run = ix->ss_by_run;
    v.rundocs = ix->rundocs;
    v.fat_js = ix->fat_js;
    v.letters = ix->letters;
    v.text = ix->text;
    v.n_text = ix->n_text;
}
// spx_api.hip: the stream of the handle's host-buffer queries (created on first use; callers hold host_mu), waiting for it
// (spinning or, "blocking_sync", asleep), and what every index carries however its arrays came to be
int ctx_stream_of(spx_index* ix, hipStream_t* out);
int ctx_wait(spx_index* ix, hipStream_t st);
int init_runtime(spx_index* ix);
// ---- spx_stage.hip: the staged walk.  A batch of reads in host memory is cut into pieces of about 32 Mi characters that
// alternate between two buffer sets and two streams: a piece's reads are copied in while the piece before is digested,
// walked and handed to the product's kernels (queries on one index are serialised; the copies are not).  A piece is
// finished -- its walk's and its product's counters read -- before the kernels of the next are enqueued.
struct StageView {  // a piece behind its walk, on the device
    const uint8_t* reads;  // the characters the values belong to: the digested reads under digestion
    const uint64_t* offs;  // nreads + 1 offsets of the values (and of `reads`)
    const void* lengths;   // value_bits wide
    const uint64_t* pointers;  // MS mode, else null
    const void* docs;          // when asked for, else null
    uint64_t q0, nreads;       // the piece's reads are [q0, q0 + nreads) of the batch
    uint64_t total_values;     // an upper bound: a digestion only shortens the reads
    int value_bits, set;
    hipStream_t stream;
};
struct StageJob {
    int mode = SPX_MODE_MS, digest_kind = 0;
    uint32_t k = 0, w = 0;
    const uint8_t* seqs = nullptr;
    const uint64_t* offsets = nullptr;
    uint64_t nreads = 0;       // at least 1
    uint64_t* out_values = nullptr;  // per read, the values it had (null: not wanted)
    bool want_docs = false;
    // the product's kernels read view.reads at view.offs: the digested reads are never parked while the call runs.  The
    // others keep the index's own digest_parked (parking is a measured tuning of large batches)
    bool reads_characters = false;
    bool one_piece = false;    // the batch is one piece however large, on streams[0] alone
    hipStream_t streams[2] = {nullptr, nullptr};
    std::function<int(hipStream_t)> wait;            // the host waits for a piece's stream
    std::function<int(const StageView&)> enqueue;    // the product's kernels and its copy-out, behind the piece's walk
    std::function<int(const StageView&)> collect;    // after the wait and spx_last_walk_stats
};
struct StagePlan {
    std::vector<uint64_t> cut;  // piece c is reads [cut[c], cut[c + 1])
    uint64_t longest = 0, worst_chars = 0, worst_reads = 0, raw_bytes = 0, dig_bytes = 0;
    bool narrow = true;  // 16-bit values: every read is below 65536 characters
    int sets = 1;        // buffer sets in use: 2 when there is more than one piece
    void* p[2][spx_index::G_SET_STRIDE] = {};  // null: not needed by this job
};
// checks the offsets, cuts the batch and reserves the buffer sets for the worst piece, before anything is enqueued (a
// buffer that grows is freed first: a device-wide wait)
int stage_plan(spx_index* ix, const StageJob& job, StagePlan* plan);
int stage_streams(spx_index* ix, hipStream_t out[2]);  // the two streams of the pieces (created on first use)
int stage_run(spx_index* ix, const StageJob& job, const StagePlan& plan);
void release_stage(spx_index* ix);
// A product's kernels between its two events: open, the launches with a mark wherever the next step begins, close.  The
// caller holds ix->mu and has set the device.  The counters and the events are the index's: a call on another stream
// waits for the one before.  open zeroes the counters (*c) and records ev0; the time from there on belongs to `step`.
int product_open(spx_index::Product& p, size_t words, hipStream_t st, int step, void** c);
// from here on the time belongs to `step`: -1 (to none) .. Product::STEPS - 1
int product_mark(spx_index::Product& p, int step, hipStream_t st);
int product_close(spx_index::Product& p, hipStream_t st);
template <typename Launch>  // `launch` gets the zeroed counters
int product_enqueue(spx_index::Product& p, size_t words, hipStream_t st, Launch&& launch, int step = -1) {
    void* c = nullptr;
    int rc;
    if ((rc = product_open(p, words, st, step, &c)) != SPX_OK || (rc = launch(c)) != SPX_OK) return rc;
    return product_close(p, st);
}
// waits for the kernels enqueued last; adds their first `nacc` words to p.acc but word `error_word` (-1: the last), which
// is ORed into p.error; adds the time between the two events to p.ms and the time of every labelled step to its
// p.step_ms.  Takes ix->mu.
int product_collect(spx_index* ix, spx_index::Product& p, int words, int nacc, int error_word = -1);
void product_reset(spx_index* ix, spx_index::Product& p);
void product_release(spx_index::Product& p);
void release(spx_index::Scratch* scr, int n, spx_index::Product* p);  // frees scr[0 .. n) and, unless null, releases *p
// The fetch slot.  publish and take: the caller holds host_mu.  take: the records `whose` left for `who` are still there
// -- `reads` reads, n entries -- and are `who`'s from here on: nothing waits for the fetch.  fetch TAKES host_mu itself
// (it is the whole body of a _fetch): the op offsets and the entries from their two scratch slots to the caller's arrays.
inline void ready_publish(spx_index::Ready& r, uint64_t n, uint64_t reads) { r = spx_index::Ready{true, n, reads}; }
int ready_take(spx_index::Ready& r, uint64_t reads, uint64_t n, const char* who, const char* whose);
int ready_fetch(spx_index* ix, spx_index::Ready& r, const spx_index::Scratch& op_offsets, const spx_index::Scratch& ops,
                const char* fetch_name, const char* begin_name, uint64_t* out_op_offsets, uint32_t* out_ops);
int check_digest_kind(int digest_kind);  // 0, SPX_DIGEST_PROMOTED or SPX_DIGEST_DNA, else SPX_E_ARG and the message
// The argument checks the host forms share, in the order they report: min_length (BATCH_MIN_LENGTH), digest_kind, the SA
// samples and the text that `what` ("the chains") need (BATCH_TEXT), the document array (want_docs), the caller's own
// pointers (null_pointers: the message when one of them is null, else null) and the one piece (BATCH_ONE_PIECE).
enum { BATCH_MIN_LENGTH = 1, BATCH_TEXT = 2, BATCH_ONE_PIECE = 4 };
int check_batch(const spx_index* ix, const char* what, int flags, uint64_t min_length, int digest_kind, int want_docs,
                const char* null_pointers, const uint64_t* offsets, uint64_t nreads);
// spx_docvote.hip: frees what the document votes hold of the device (spx_index_free)
void release_votes(spx_index* ix);
// spx_mems.hip: the same for the matches
void release_mems(spx_index* ix);
// spx_place.hip: the same for the placements
void release_place(spx_index* ix);
// spx_chain.hip: the same for the chains
void release_chain(spx_index* ix);
// spx_chain.hip: the chain parameters' ranges (SPX_E_ARG with a message beyond them)
int chain_check_params(const spx_index* ix, const struct ::spc_params* p);
// spx_align.hip: the same for the alignments
void release_align(spx_index* ix);
// spx_cigar.hip: the same for the CIGARs
void release_cigar(spx_index* ix);
// spx_extend.hip: the same for the extended CIGARs
void release_extend(spx_index* ix);
// spx_map.hip: the same for the mappings and the sequence table; and the table of `src` copied into a fresh clone
void release_map(spx_index* ix);
int clone_map(spx_index* src, spx_index* ix);
int need_table(const spx_index* ix, const char* who);  // SPX_E_ARG and a message naming `who` unless ix has a sequence table
// spx_cover.hip: the same for the coverage; what spn_set_sequences does to it (the caller holds host_mu and mu): the host
// forms' arrays were sized for the table that goes; and a fresh clone of an index that has the arrays gets its own, empty
void release_cover(spx_index* ix);
void cover_table_changed(spx_index* ix);
int clone_cover(spx_index* src, spx_index* ix);
// ... and what spd_cover_add_batch does behind its first check, for it and for spl_call_add_batch: `also` (may be empty)
// enqueues the caller's work on the batch's records and entries, behind the coverage's add and in front of the one wait
struct CoverBatch {
    const spn_mapping* d_mappings;
    const uint64_t* d_op_offsets;
    const uint32_t* d_ops;
    uint64_t in_entries, nreads;
    hipStream_t stream;
};
int cover_add_batch_with(spx_index* ix, const char* who, int digest_kind, uint32_t k, uint32_t w, const uint8_t* seqs, const uint64_t* offsets,
                         uint64_t nreads, uint64_t min_length, int want_docs, const struct ::spc_params* chain_params,
                         const struct ::spa_params* align_params, const struct ::spe_params* extend_params, spn_mapping* out_mappings,
                         const std::function<int(const CoverBatch&)>& also);
int cover_need_arrays(spx_index* ix, const char* who);  // the host forms' arrays are there (the caller holds host_mu)
int cover_finish_host(spx_index* ix);                   // ... and depth is brought up to date
// spx_call.hip: the same three for the pileup and the calls
void release_call(spx_index* ix);
void call_table_changed(spx_index* ix);
int clone_call(spx_index* src, spx_index* ix);
// ... and for a product that goes on from the pileup's arrays (spx_consensus.hip; the caller holds host_mu): they and the
// coverage's are there, named as `who`'s refusal; and del is brought up to date
int call_arrays_ready(spx_index* ix, const char* who);
int call_finish_arrays(spx_index* ix);
// spx_consensus.hip: frees what the consensus holds of the device; and what spn_set_sequences does to it (the caller holds
// host_mu and mu): the records and the body that wait for the fetch belong to the table that goes
void release_consensus(spx_index* ix);
void consensus_table_changed(spx_index* ix);
// spx_mems.hip: what spm_mems_begin does behind its argument checks -- the staged walk in MS mode with exactly one piece,
// count -> host wait -> records at their exact size -> k_mems_write -- for a product that goes on from the records on the
// device.  `then` (may be empty) is called with the write kernels enqueued and enqueues its own work behind them on
// m.stream; the call returns when that stream has been waited for.  The records stay in mems_scr (M_MOFFS, M_OUT,
// M_OUT_DOCS) as they do for spm_mems_fetch.  The caller holds host_mu, has set the device and passes nreads >= 1.
// reads_characters: `then` reads the piece's characters (MemsOnDevice::reads at read_offsets: the digested reads under
// digestion), so they are not parked while the call runs (StageJob::reads_characters).
struct MemsOnDevice {
    const uint8_t* reads;           // the characters the walk saw
    const uint64_t* read_offsets;   // nreads + 1
    const uint64_t* match_offsets;  // nreads + 1
    const void* records;            // n spm_match
    const uint32_t* docs;           // n ids, null unless asked for
    uint64_t nreads, n;
    hipStream_t stream;
};
int mems_begin_staged(spx_index* ix, int digest_kind, uint32_t k, uint32_t w, const uint8_t* seqs, const uint64_t* offsets,
                      uint64_t nreads, uint64_t min_length, int want_docs, uint64_t* match_offsets, uint64_t* out_values,
                      uint64_t* n_matches, bool reads_characters, const std::function<int(const MemsOnDevice&)>& then);
// spx_flatten.hip: (re)builds fat / fat_js from letters, Q, dirrows and aux (view.r / nfat / fat_stride set)
int build_fat(spx_index* ix);
// spx_walk.hip: MS text against the index: text[samples_start[k]] must be the head of run k
int launch_text_check(spx_index* ix, unsigned long long* d_bad, hipStream_t stream);
// spx_walk.hip: the indexed text from the MS index (LF chains from every run's first position)
int launch_text_from_index(spx_index* ix, uint8_t* d_text, uint64_t n_text, unsigned long long* d_stuck, hipStream_t stream);
// spx_flatten.hip: builds every device array of `ix` from raw per-run arrays
// that already live on the device.
int flatten_on_device(spx_index* ix, const uint8_t* d_heads, const uint64_t* d_lens,
                      const uint64_t* d_thr, const uint64_t* d_ssa, const uint64_t* d_esa,
                      const uint64_t* d_ds, const uint64_t* d_de, const std::function<void()>& release_inputs = {});
// spx_walk.hip
// *wrote_lengths: the walk wrote the PML lengths itself (k_walk_fast): launch_len_expand is not needed
int launch_walk(spx_index* ix, int mode, const BatchArgs& args, uint64_t total_chars,
                hipStream_t stream, bool* wrote_lengths = nullptr);
int launch_ms_extend(spx_index* ix, const BatchArgs& args, hipStream_t stream);
// PML lengths through one bit per character: prepare_len_mask before the walk (sets args.len_mask; nothing
// to do for MS or a classification-only query), launch_len_expand after it
int prepare_len_mask(spx_index* ix, int mode, BatchArgs& args);
inline uint64_t len_mask_pairs(uint64_t chars, uint64_t reads) { return (chars >> 7) + reads + 2; }  // 16-byte pairs of the bits
int launch_len_expand(spx_index* ix, const BatchArgs& args, hipStream_t stream);
// long-read batches: the chunked walk (returns SPX_OK and sets *done = false when the batch does not
// qualify and the plain walk should run)
// geom_chars (0: total_chars): the characters the batch is expected to hold when total_chars is only an upper bound
int launch_walk_chunked(spx_index* ix, int mode, const BatchArgs& args, uint64_t total_chars, hipStream_t stream,
                        bool* done, uint64_t geom_chars = 0);
// spx_text.hip: the values lines of one vector as text (count + scan, then -- the stream's size known -- the digits)
int launch_text_count(const void* d_vals, int value_bytes, const uint64_t* d_offs, const uint32_t* d_gap, uint64_t nreads,
                      uint64_t* d_line_bytes, uint64_t* d_line_start, void* d_cub, size_t cub_bytes, hipStream_t st);
size_t text_scan_bytes(uint64_t nreads);
int launch_text_write(const void* d_vals, int value_bytes, const uint64_t* d_offs, const uint32_t* d_gap, uint64_t nreads,
                      const uint64_t* d_line_start, char* d_text, hipStream_t st);
// spx_digest.hip: d_out_offs gets nreads + 1 offsets, d_out the digested reads (capacity is the
// caller's business: spx_digest_capacity)
int launch_digest(spx_index* ix, int kind, uint32_t k, uint32_t w, const uint8_t* d_seqs, const uint64_t* d_offs,
                  uint64_t nreads, uint64_t total_chars, uint8_t* d_out, uint64_t* d_out_offs, hipStream_t stream,
                  bool* parked = nullptr);
}  // namespace spx
