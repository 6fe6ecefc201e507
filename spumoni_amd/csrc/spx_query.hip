// spx_query.hip -- the query entry points of the C-ABI: digestion, walk and text output over device and host buffers.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <thread>

#include "spx_internal.h"

using namespace spx;

extern "C" {

// Words the host is waiting for, written into page-locked host memory by a kernel (spx_internal.h: h_pub): dst[i] = *src[i]
// (0 for a null source) for i < 4, then nwords words of `more`.
struct PubSrc {
    const uint64_t* one[4];
    const uint64_t* more;
    int nmore;
};
__global__ void k_publish(uint64_t* dst, PubSrc src) {
    const int t = (int)threadIdx.x;
    if (t < 4) dst[t] = src.one[t] ? *src.one[t] : 0;
    if (t >= 4 && t - 4 < src.nmore) dst[t] = src.more[t - 4];
    __threadfence_system();
}
static int publish(spx_index* ix, const PubSrc& src, hipStream_t st) {
    if (!ix->h_pub) {
        SPX_HIP(hipHostMalloc((void**)&ix->h_pub, 64 * sizeof(uint64_t), hipHostMallocMapped | hipHostMallocCoherent));  // (coherent whatever HIP_HOST_COHERENT says)
        SPX_HIP(hipHostGetDevicePointer((void**)&ix->h_pub_dev, ix->h_pub, 0));
    }
    k_publish<<<1, 64, 0, st>>>(ix->h_pub_dev, src);
    SPX_HIP(hipGetLastError());
    return SPX_OK;
}

uint64_t spx_digest_capacity(int kind, uint32_t k, uint64_t total_chars) {
    // every k-mer can be reported once: <= total_chars values of 1 byte (-m) or k bytes (-a);
    // + the padding spx_query_batch_device asks of its d_seqs
    const uint64_t body = (kind == SPX_DIGEST_DNA ? (uint64_t)(k ? k : 1) : 1ull) * total_chars;
    return ((body + 3) / 4) * 4 + 32;
}

int spx_digest_batch_device(spx_index* ix, int kind, uint32_t k, uint32_t w, const uint8_t* d_seqs,
                            const uint64_t* d_offsets, uint64_t nreads, uint64_t total_chars,
                            uint8_t* d_out_seqs, uint64_t out_capacity, uint64_t* d_out_offsets, void* stream) {
    if (!ix || !d_seqs || !d_offsets || !d_out_seqs || !d_out_offsets) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    if (((uintptr_t)d_seqs & 15) != 0) {
        set_error("d_seqs must be 16-byte aligned (and readable for round_up(total_chars, 16) + 16 bytes)");
        return SPX_E_ARG;
    }
    if (out_capacity < spx_digest_capacity(kind, k, total_chars)) {
        set_error("d_out_seqs must hold spx_digest_capacity() = %llu bytes",
                  (unsigned long long)spx_digest_capacity(kind, k, total_chars));
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    return launch_digest(ix, kind, k, w, d_seqs, d_offsets, nreads, total_chars, d_out_seqs, d_out_offsets, st);
}

// Digestion in front of a walk on the same device (run -m / -a, compute_ms_pml.cpp:919-923).  When the walk that follows
// is the plain one over compact rows (k_walk_fast) and needs the reads only as characters, the digested reads stay where the
// digestion parked them -- read q's at d_dig[d_offs[q] ..] -- and *in_starts = d_offs tells the walk so: the pass that would
// concatenate them (0.5 of 2.1 ms per 10^7 x 200 bp) is not made.  d_dig_offs are the offsets of the concatenation either
// way: that is where the results go.
static int digest_for_walk(spx_index* ix, int mode, bool ms_lengths, int kind, uint32_t k, uint32_t w, const uint8_t* d_raw,
                           const uint64_t* d_offs, uint64_t nreads, uint64_t total_in, uint8_t* d_dig, uint64_t cap,
                           uint64_t* d_dig_offs, void* stream, const uint64_t** in_starts) {
    *in_starts = nullptr;
    if (!ix || !d_raw || !d_offs || !d_dig || !d_dig_offs) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    if (((uintptr_t)d_raw & 15) != 0) {
        set_error("d_seqs must be 16-byte aligned (and readable for round_up(total_chars, 16) + 16 bytes)");
        return SPX_E_ARG;
    }
    if (cap < spx_digest_capacity(kind, k, total_in)) {
        set_error("the buffer for the digested reads must hold spx_digest_capacity() = %llu bytes",
                  (unsigned long long)spx_digest_capacity(kind, k, total_in));
        return SPX_E_ARG;
    }
    static const bool old_walk = getenv("SPX_OLD_WALK") != nullptr;
    // (SPX_DIGEST_PARKED: the "digest_parked" option from the environment, for callers that have no handle on it -- the CLI's tests)
    static const int env_parked = getenv("SPX_DIGEST_PARKED") ? atoi(getenv("SPX_DIGEST_PARKED")) : -1;
    const int parked_mode = env_parked >= 0 ? env_parked : ix->digest_parked;
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    if (ix->num_cus == 0) {
        hipDeviceProp_t prop;
        SPX_HIP(hipGetDeviceProperties(&prop, ix->device));
        ix->num_cus = prop.multiProcessorCount;
    }
    // (automatic: only batches that fill the device's lanes with reads -- the others may be long reads that the chunked
    // walk should get, and that one takes its reads by their offsets)
    bool park = parked_mode != 1 && ix->rows != nullptr && ix->view.compact && !old_walk && nreads > 0 && nreads < (1ull << 31) &&
                !(mode == SPX_MODE_MS && ms_lengths) && ix->force_lanes_per_wave == 0 &&
                (parked_mode == 2 || nreads * 2 > (uint64_t)ix->num_cus * 20 * 64);
    const int rc = launch_digest(ix, kind, k, w, d_raw, d_offs, nreads, total_in, d_dig, d_dig_offs, (hipStream_t)stream, &park);
    if (rc == SPX_OK && park) *in_starts = d_offs;
    return rc;
}

// the walk's own verdict on a batch as the error of the call that ran it (SPX_OK: none)
enum { WALK_ERR_PLAIN, WALK_ERR_NARROW, WALK_ERR_STATS };
static int walk_error(const WalkCounters& wc, int hint) {
    if (!wc.error) return SPX_OK;
    set_error("the walk hit %llu undefined steps (%s%s)", wc.error,
              hint == WALK_ERR_STATS ? "inconsistent thresholds; or a read of 65536 characters or more with 16-bit outputs; or a "
                                       "batch that holds more characters than total_chars"
                                     : "predecessor jump without a predecessor run: thresholds are inconsistent with the BWT",
              hint == WALK_ERR_NARROW ? "; or a read of 65536 characters or more with 16-bit outputs" : "");
    return SPX_E_FORMAT;
}

// What a host-buffer query needs of ix->scratch, in the order it is reserved.  take() leaves the pointer of a slot that is
// not in the plan null.
struct ScratchPlan {
    struct Item { int slot; size_t bytes; } item[spx_index::S_COUNT];
    int n = 0;
    void add(int slot, size_t bytes) { item[n++] = Item{slot, bytes}; }
};
static int take(spx_index* ix, const ScratchPlan& plan, int slot, void** out) {
    for (int i = 0; i < plan.n; ++i)
        if (plan.item[i].slot == slot) return ix->scratch[slot].reserve(plan.item[i].bytes, out);
    return SPX_OK;
}

// the four result vectors; pad: values behind the last that lengths and document ids have room for (the text formatter: 8)
static void plan_vectors(ScratchPlan& plan, bool len, bool ptr, bool doc, bool cls, uint64_t chars, uint64_t reads, uint64_t pad) {
    if (len) plan.add(spx_index::S_LEN, (chars + pad) * 4);
    if (ptr) plan.add(spx_index::S_PTR, (chars + 1) * 8);
    if (doc) plan.add(spx_index::S_DOC, (chars + pad) * 4);
    if (cls) plan.add(spx_index::S_CLASS, (reads + 1) * sizeof(spx_class));
}
static int take_vectors(spx_index* ix, const ScratchPlan& plan, void** len, void** ptr, void** doc, void** cls) {
    int rc;
    if ((rc = take(ix, plan, spx_index::S_LEN, len)) != SPX_OK) return rc;
    if ((rc = take(ix, plan, spx_index::S_PTR, ptr)) != SPX_OK) return rc;
    if ((rc = take(ix, plan, spx_index::S_DOC, doc)) != SPX_OK) return rc;
    return take(ix, plan, spx_index::S_CLASS, cls);
}

int spx_digest_batch(spx_index* ix, int kind, uint32_t k, uint32_t w, const uint8_t* seqs, const uint64_t* offsets,
                     uint64_t nreads, uint8_t* out_seqs, uint64_t out_capacity, uint64_t* out_offsets) {
    if (!ix || !seqs || !offsets || !out_offsets) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> hg(ix->host_mu);
    SPX_HIP(hipSetDevice(ix->device));
    const uint64_t total = nreads ? offsets[nreads] : 0;
    const uint64_t cap = spx_digest_capacity(kind, k, total);
    void *dseq = nullptr, *doff = nullptr, *dout = nullptr, *dooff = nullptr;
    int rc;
    if ((rc = ix->scratch[spx_index::S_RAW].reserve(((total + 15) & ~15ull) + 16, &dseq)) != SPX_OK) return rc;
    if ((rc = ix->scratch[spx_index::S_OFFS].reserve((nreads + 1) * 8, &doff)) != SPX_OK) return rc;
    if ((rc = ix->scratch[spx_index::S_SEQ].reserve(cap, &dout)) != SPX_OK) return rc;
    if ((rc = ix->scratch[spx_index::S_DIG_OFFS].reserve((nreads + 1) * 8, &dooff)) != SPX_OK) return rc;
    hipStream_t st = nullptr;
    if ((rc = ctx_stream_of(ix, &st)) != SPX_OK) return rc;
    QuietOnError quiet(st);
    SPX_HIP(hipMemcpyAsync(dseq, seqs, total, hipMemcpyHostToDevice, st));
    SPX_HIP(hipMemcpyAsync(doff, offsets, (nreads + 1) * 8, hipMemcpyHostToDevice, st));
    rc = spx_digest_batch_device(ix, kind, k, w, (const uint8_t*)dseq, (const uint64_t*)doff, nreads, total,
                                 (uint8_t*)dout, cap, (uint64_t*)dooff, st);
    if (rc != SPX_OK) return rc;
    SPX_HIP(hipMemcpyAsync(out_offsets, dooff, (nreads + 1) * 8, hipMemcpyDeviceToHost, st));
    SPX_HIP(hipStreamSynchronize(st));
    const uint64_t dtotal = out_offsets[nreads];
    if (dtotal > out_capacity || (dtotal && !out_seqs)) {
        set_error("out_seqs holds %llu bytes, the digested reads need %llu", (unsigned long long)out_capacity,
                  (unsigned long long)dtotal);
        return SPX_E_ARG;
    }
    if (dtotal) {
        SPX_HIP(hipMemcpyAsync(out_seqs, dout, dtotal, hipMemcpyDeviceToHost, st));
        SPX_HIP(hipStreamSynchronize(st));
    }
    return quiet.done(SPX_OK);
}

static int check_query(spx_index* ix, int mode, const void* seqs, const void* offs,
                       uint32_t* out_lengths, uint64_t* out_pointers, uint32_t* out_docs,
                       spx_class* out_class, uint64_t bin_width) {
    if (!ix || !seqs || !offs) {
        set_error("index, seqs and offsets must be non-null");
        return SPX_E_ARG;
    }
    if (mode != SPX_MODE_PML && mode != SPX_MODE_MS) {
        set_error("mode must be SPX_MODE_PML or SPX_MODE_MS");
        return SPX_E_ARG;
    }
    if (mode == SPX_MODE_PML && !out_lengths && !out_class) {
        set_error("PML mode needs out_lengths (or out_class alone: classification without the per-character values)");
        return SPX_E_ARG;
    }
    if (mode == SPX_MODE_PML && out_pointers) {
        set_error("out_pointers is only produced in MS mode");
        return SPX_E_ARG;
    }
    if (mode == SPX_MODE_MS) {
        if (!ix->has_samples) {
            set_error("MS mode needs an index built with SA samples (.ssa/.esa)");
            return SPX_E_ARG;
        }
        if (!out_pointers) {
            set_error("MS mode needs out_pointers");
            return SPX_E_ARG;
        }
        if (out_lengths && !ix->text) {
            set_error("MS lengths need the text: call spx_index_set_text first");
            return SPX_E_ARG;
        }
        if (out_class && !out_lengths) {
            set_error("MS classification needs out_lengths");
            return SPX_E_ARG;
        }
    }
    if (out_docs && !ix->has_docs) {
        set_error("document ids requested but the index has no document array");
        return SPX_E_ARG;
    }
    if (out_class && bin_width == 0) {
        set_error("bin_width must be > 0");
        return SPX_E_ARG;
    }
    return SPX_OK;
}

// narrow: lengths / docs are uint16_t arrays (the 16-bit entry points).  The class records are enqueue_walk's business.
static BatchArgs make_batch_args(spx_index* ix, const uint8_t* d_seqs, const uint64_t* d_offsets, uint64_t nreads, uint64_t total_chars,
                                 uint32_t* lengths, uint64_t* pointers, uint32_t* docs, uint64_t bin_width, uint64_t max_value_thr,
                                 bool narrow, const uint64_t* d_in_starts) {
    BatchArgs a{};
    a.seqs = d_seqs;
    a.offs = d_offsets;
    a.nreads = nreads;
    a.total_chars = total_chars;
    a.out_lengths = lengths;
    a.out_pointers = pointers;
    a.out_docs = docs;
    // A read has fewer than 2^32 values, so every width from 2^32 - 1 on is "one bin": m / w < 1 for w > m, and
    // m = w = 2^32 - 1 is one bin too.  The walks keep the width in 32 bits (registers of the hot loop); clamped here,
    // before the magic number is derived from it, every kernel sees the same width.
    if (bin_width > 0xffffffffull) bin_width = 0xffffffffull;
    a.bin_width = bin_width;
    a.bin_magic = bin_width > 1 ? (uint64_t)(~0ull / bin_width) + 1 : 0;
    a.max_value_thr = max_value_thr;
    a.counters = ix->counters;
    a.narrow = narrow ? 1 : 0;
    a.in_starts = d_in_starts;
    return a;
}

// The kernels of one query, or of one piece of a pipelined one, on st.  cls goes to the walk (PML) or to the extension (MS).
// Callers hold mu and have zeroed the counters; timed: ev0 / ev1 are recorded around the walk.  geom_chars: what the batch
// is expected to hold when a.total_chars is only an upper bound -- reads digested on the device a moment ago; it shapes
// the chunks, total_chars sizes the scratch.
static int enqueue_walk(spx_index* ix, int mode, BatchArgs& a, spx_class* cls, uint64_t geom_chars, hipStream_t st, bool timed) {
    int rc;
    a.out_class = mode == SPX_MODE_PML ? cls : nullptr;
    if ((rc = prepare_len_mask(ix, mode, a)) != SPX_OK) return rc;
    if (timed) SPX_HIP(hipEventRecord(ix->ev0, st));
    bool chunked = false, wrote = false;
    if (a.nreads > 0) {
        if (!a.in_starts && (rc = launch_walk_chunked(ix, mode, a, a.total_chars, st, &chunked, geom_chars)) != SPX_OK) return rc;
        if (!chunked && (rc = launch_walk(ix, mode, a, a.total_chars, st, &wrote)) != SPX_OK) return rc;
    }
    if (timed) SPX_HIP(hipEventRecord(ix->ev1, st));
    // PML, state-machine walk: it left one bit per character; the lengths are written from them here
    if (a.nreads > 0 && !chunked && !wrote && (rc = launch_len_expand(ix, a, st)) != SPX_OK) return rc;
    if (mode == SPX_MODE_MS && a.out_lengths && a.nreads > 0) {
        a.out_class = cls;
        if ((rc = launch_ms_extend(ix, a, st)) != SPX_OK) return rc;
    }
    return SPX_OK;
}

static int query_device_impl(spx_index* ix, int mode, const uint8_t* d_seqs, const uint64_t* d_offsets,
                             uint64_t nreads, uint64_t total_chars, uint32_t* d_out_lengths,
                             uint64_t* d_out_pointers, uint32_t* d_out_docs, spx_class* d_out_class,
                             uint64_t bin_width, uint64_t max_value_thr, void* stream, bool narrow,
                             const uint64_t* d_in_starts = nullptr, uint64_t geom_chars = 0) {
    int rc = check_query(ix, mode, d_seqs, d_offsets, d_out_lengths, d_out_pointers, d_out_docs,
                         d_out_class, bin_width);
    if (rc != SPX_OK) return rc;
    if (((uintptr_t)d_seqs & 15) != 0) {
        set_error("d_seqs must be 16-byte aligned (and readable for round_up(total_chars, 4) + 32 bytes)");
        return SPX_E_ARG;
    }
    if ((((uintptr_t)d_out_lengths | (uintptr_t)d_out_pointers | (uintptr_t)d_out_docs) & 15) != 0) {
        set_error("output buffers must be 16-byte aligned (results are written as 16-byte vectors)");
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    // the counters / events belong to the index: a query enqueued on another stream waits for
    // the previous one (queries on one index are serialised, as the header promises)
    if (ix->have_timing && ix->last_stream != st) SPX_HIP(hipStreamWaitEvent(st, ix->ev_done, 0));
    SPX_HIP(hipMemsetAsync(ix->counters, 0, sizeof(WalkCounters), st));
    ix->claim_used = false;
    // (d_in_starts: reads parked by the digestion -- digest_for_walk below made sure the plain fast walk takes them)
    BatchArgs a = make_batch_args(ix, d_seqs, d_offsets, nreads, total_chars, d_out_lengths, d_out_pointers, d_out_docs, bin_width,
                                  max_value_thr, narrow, d_in_starts);
    if ((rc = enqueue_walk(ix, mode, a, d_out_class, geom_chars, st, true)) != SPX_OK) return rc;
    SPX_HIP(hipEventRecord(ix->ev_done, st));
    ix->have_timing = true;
    ix->last_stream = st;
    return SPX_OK;
}

int spx_query_batch_device(spx_index* ix, int mode, const uint8_t* d_seqs, const uint64_t* d_offsets,
                           uint64_t nreads, uint64_t total_chars, uint32_t* d_out_lengths,
                           uint64_t* d_out_pointers, uint32_t* d_out_docs, spx_class* d_out_class,
                           uint64_t bin_width, uint64_t max_value_thr, void* stream) {
    return query_device_impl(ix, mode, d_seqs, d_offsets, nreads, total_chars, d_out_lengths, d_out_pointers,
                             d_out_docs, d_out_class, bin_width, max_value_thr, stream, false);
}

int spx_query_batch_device16(spx_index* ix, int mode, const uint8_t* d_seqs, const uint64_t* d_offsets,
                             uint64_t nreads, uint64_t total_chars, uint16_t* d_out_lengths,
                             uint64_t* d_out_pointers, uint16_t* d_out_docs, spx_class* d_out_class,
                             uint64_t bin_width, uint64_t max_value_thr, void* stream) {
    return query_device_impl(ix, mode, d_seqs, d_offsets, nreads, total_chars, (uint32_t*)d_out_lengths,
                             d_out_pointers, (uint32_t*)d_out_docs, d_out_class, bin_width, max_value_thr, stream,
                             true);
}

// device side of the host-buffer queries: d_seq / d_off are resident (scratch), results go
// through the scratch vectors to the host buffers.  Caller holds host_mu.  width: bytes per length /
// doc value in the host buffers (4, or 2 for the 16-bit entry points)
static int run_and_fetch(spx_index* ix, int mode, const uint8_t* d_seq, const uint64_t* d_off, uint64_t nreads,
                         uint64_t total, void* out_lengths, uint64_t* out_pointers, void* out_docs,
                         spx_class* out_class, uint64_t bin_width, uint64_t max_value_thr, size_t width = 4,
                         const uint64_t* d_in_starts = nullptr) {
    void *dlen = nullptr, *dptr = nullptr, *ddoc = nullptr, *dcls = nullptr;
    ScratchPlan plan;
    plan_vectors(plan, out_lengths, out_pointers, out_docs, out_class, total, nreads, 1);
    int rc;
    if ((rc = take_vectors(ix, plan, &dlen, &dptr, &ddoc, &dcls)) != SPX_OK) return rc;
    hipStream_t st = nullptr;
    if ((rc = ctx_stream_of(ix, &st)) != SPX_OK) return rc;
    rc = query_device_impl(ix, mode, d_seq, d_off, nreads, total, (uint32_t*)dlen, (uint64_t*)dptr,
                           (uint32_t*)ddoc, (spx_class*)dcls, bin_width, max_value_thr, st, width == 2, d_in_starts);
    if (rc != SPX_OK) return rc;
    if (out_lengths) SPX_HIP(hipMemcpyAsync(out_lengths, dlen, total * width, hipMemcpyDeviceToHost, st));
    if (out_pointers) SPX_HIP(hipMemcpyAsync(out_pointers, dptr, total * 8, hipMemcpyDeviceToHost, st));
    if (out_docs) SPX_HIP(hipMemcpyAsync(out_docs, ddoc, total * width, hipMemcpyDeviceToHost, st));
    if (out_class) SPX_HIP(hipMemcpyAsync(out_class, dcls, nreads * sizeof(spx_class), hipMemcpyDeviceToHost, st));
    WalkCounters wc;
    SPX_HIP(hipMemcpyAsync(&wc, ix->counters, sizeof wc, hipMemcpyDeviceToHost, st));
    SPX_HIP(hipStreamSynchronize(st));
    return walk_error(wc, width == 2 ? WALK_ERR_NARROW : WALK_ERR_PLAIN);
}

// Large host batches: chunks of reads go through copy-in / walk / copy-out on three streams, so the
// PCIe transfers of one chunk overlap the kernel of another.  Offsets are absolute, so every chunk
// is launched on the same device buffers with the offsets pointer advanced.  Caller holds host_mu.
// 16-bit outputs hold values below 65536: a read that long is refused.  first_long_read: its index, or q1 (the error
// text is thread-local: the caller's thread reports)
static uint64_t first_long_read(const uint64_t* offsets, uint64_t q0, uint64_t q1) {
    for (uint64_t q = q0; q < q1; ++q)
        if (offsets[q + 1] - offsets[q] >= 65536) return q;
    return q1;
}
static int check_narrow_reads(const uint64_t* offsets, uint64_t q0, uint64_t q1) {
    const uint64_t q = first_long_read(offsets, q0, q1);
    if (q == q1) return SPX_OK;
    set_error("read %llu has 65536 characters or more: use the 32-bit entry point", (unsigned long long)q);
    return SPX_E_ARG;
}

static int run_pipelined(spx_index* ix, int mode, const uint8_t* seqs, const uint64_t* offsets, uint64_t nreads,
                         uint8_t* d_seq, uint64_t* d_off, uint64_t padded, void* out_lengths, uint64_t* out_pointers,
                         void* out_docs, spx_class* out_class, uint64_t bin_width, uint64_t max_value_thr,
                         size_t width) {
    const uint64_t total = offsets[nreads];
    void *dlen = nullptr, *dptr = nullptr, *ddoc = nullptr, *dcls = nullptr;
    ScratchPlan plan;
    plan_vectors(plan, out_lengths, out_pointers, out_docs, out_class, total, nreads, 1);
    int rc;
    if ((rc = take_vectors(ix, plan, &dlen, &dptr, &ddoc, &dcls)) != SPX_OK) return rc;
    std::lock_guard<std::mutex> g(ix->mu);
    constexpr int NCH = spx_index::PIPE_CHUNKS;
    if (!ix->pipe_s[0]) {
        for (auto& st : ix->pipe_s) SPX_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        for (int c = 0; c < NCH; ++c) {
            SPX_HIP(hipEventCreateWithFlags(&ix->pipe_in[c], hipEventDisableTiming));
            SPX_HIP(hipEventCreateWithFlags(&ix->pipe_k[c], hipEventDisableTiming));
        }
    }
    hipStream_t s_in = ix->pipe_s[0], s_k = ix->pipe_s[1], s_out = ix->pipe_s[2];
    // The pieces GROW.  The call is as long as its copy-out (the results are twice the bytes of the reads, and the
    // walk is faster than either copy) plus whatever passes before the first result can leave: so the first piece is
    // small (1/64 of the reads: copied in, walked and on its way out after ~0.4 ms instead of the ~3.7 ms an eighth of
    // the batch and the whole offsets array took), and every piece is 1.5 x the one before -- less than the 1.7 x by
    // which the walk outruns the copy-out, so the copy-out stream never waits for a walk.
    uint64_t cut[NCH + 1];
    {
        double acc = 0, piece = 1.0 / 64.0;
        cut[0] = 0;
        for (int c = 0; c < NCH; ++c) {
            acc += piece;
            piece *= 1.5;
            // (the series reaches the whole before the last piece: what is left then is one smaller piece)
            cut[c + 1] = (c + 1 == NCH || acc >= 1.0) ? nreads : (uint64_t)((double)nreads * acc);
        }
    }
    if (mode == SPX_MODE_PML && out_lengths) {
        // the length-bit scratch is sized for the largest piece BEFORE the pipeline starts: growing it between
        // pieces would hipFree (an implicit device synchronisation) in the middle of the copy / compute overlap
        uint64_t worst = 0;
        for (int c = 0; c < NCH; ++c) {
            const uint64_t q0 = cut[c], q1 = cut[c + 1];
            worst = std::max(worst, len_mask_pairs(offsets[q1] - offsets[q0], q1 - q0));
        }
        void* unused = nullptr;
        if ((rc = ix->chunk_scr[spx_index::C_LEN_BITS].reserve(worst * 16, &unused)) != SPX_OK) return rc;
    }
    if (ix->have_timing && ix->last_stream != s_k) SPX_HIP(hipStreamWaitEvent(s_k, ix->ev_done, 0));
    SPX_HIP(hipMemsetAsync(ix->counters, 0, sizeof(WalkCounters), s_k));
    ix->claim_used = false;
    SPX_HIP(hipEventRecord(ix->ev0, s_k));
    // SPX_PIPE_TRACE=1: when every piece's copy-in, walk and copy-out ended, on stderr (timed events of their own)
    static const bool trace = getenv("SPX_PIPE_TRACE") != nullptr;
    const auto h0 = std::chrono::steady_clock::now();
    hipEvent_t tr0 = nullptr, tr[NCH][3] = {};
    if (trace) {
        SPX_HIP(hipEventCreate(&tr0));
        for (auto& row : tr)
            for (auto& e : row) SPX_HIP(hipEventCreate(&e));
        SPX_HIP(hipEventRecord(tr0, s_in));
    }
    // 16-bit outputs: the reads' lengths are checked by a thread of its own while this one enqueues (10^7 offsets are
    // 3-4 ms of one core; in front of the pipeline that is 15 % of the call, and spread between the pieces' enqueues it
    // made the copy-out of the later pieces slow: profiles/r03_host_path_pipeline.txt)
    uint64_t long_read = nreads;
    std::thread narrow_check;
    if (width == 2) narrow_check = std::thread([&] { long_read = first_long_read(offsets, 0, nreads); });
    struct Joiner {
        std::thread& t;
        ~Joiner() {
            if (t.joinable()) t.join();
        }
    } joiner{narrow_check};
    // the read-ahead padding first, on the copy-in stream: every piece's event covers it; a piece's offsets travel
    // with the piece (the whole array up front is 80 MB for 10^7 reads: 1.4 ms before anything else could start)
    SPX_HIP(hipMemsetAsync(d_seq + total, 0, padded - total, s_in));
    for (int c = 0; c < NCH; ++c) {
        const uint64_t q0 = cut[c], q1 = cut[c + 1];
        if (q1 == q0) continue;
        const uint64_t a = offsets[q0], b = offsets[q1];
        SPX_HIP(hipMemcpyAsync(d_off + q0, offsets + q0, (q1 - q0 + 1) * 8, hipMemcpyHostToDevice, s_in));
        SPX_HIP(hipMemcpyAsync(d_seq + a, seqs + a, b - a, hipMemcpyHostToDevice, s_in));
        SPX_HIP(hipEventRecord(ix->pipe_in[c], s_in));
        if (trace) SPX_HIP(hipEventRecord(tr[c][0], s_in));
        SPX_HIP(hipStreamWaitEvent(s_k, ix->pipe_in[c], 0));
        // (a piece of few, long reads is cut further and walked chunk-wise: spx_walk.hip)
        BatchArgs args = make_batch_args(ix, d_seq, d_off + q0, q1 - q0, b - a, (uint32_t*)dlen, (uint64_t*)dptr, (uint32_t*)ddoc,
                                         bin_width, max_value_thr, width == 2, nullptr);
        if ((rc = enqueue_walk(ix, mode, args, dcls ? (spx_class*)dcls + q0 : nullptr, 0, s_k, false)) != SPX_OK) return rc;
        SPX_HIP(hipEventRecord(ix->pipe_k[c], s_k));
        if (trace) SPX_HIP(hipEventRecord(tr[c][1], s_k));
        SPX_HIP(hipStreamWaitEvent(s_out, ix->pipe_k[c], 0));
        if (out_lengths)
            SPX_HIP(hipMemcpyAsync((char*)out_lengths + a * width, (char*)dlen + a * width, (b - a) * width,
                                   hipMemcpyDeviceToHost, s_out));
        if (out_pointers)
            SPX_HIP(hipMemcpyAsync(out_pointers + a, (uint64_t*)dptr + a, (b - a) * 8, hipMemcpyDeviceToHost, s_out));
        if (out_docs)
            SPX_HIP(hipMemcpyAsync((char*)out_docs + a * width, (char*)ddoc + a * width, (b - a) * width,
                                   hipMemcpyDeviceToHost, s_out));
        if (out_class)
            SPX_HIP(hipMemcpyAsync(out_class + q0, (spx_class*)dcls + q0, (q1 - q0) * sizeof(spx_class),
                                   hipMemcpyDeviceToHost, s_out));
        if (trace) SPX_HIP(hipEventRecord(tr[c][2], s_out));
    }
    SPX_HIP(hipEventRecord(ix->ev1, s_k));
    SPX_HIP(hipEventRecord(ix->ev_done, s_k));
    ix->have_timing = true;
    ix->last_stream = s_k;
    const double h_enq = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count();
    SPX_HIP(hipStreamSynchronize(s_out));
    SPX_HIP(hipStreamSynchronize(s_k));
    if (narrow_check.joinable()) narrow_check.join();
    if (long_read != nreads) return check_narrow_reads(offsets, long_read, nreads);  // (the walk counted it as an error, too)
    if (trace) {
        std::fprintf(stderr, "spx pipeline: host: all pieces enqueued after %.2f ms, streams drained after %.2f ms\n", h_enq, 
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count());
        std::fprintf(stderr, "spx pipeline: piece reads | copy-in done, walk done, copy-out done (ms after the first copy was enqueued)\n");
        for (int c = 0; c < NCH; ++c) {
            float t[3] = {0, 0, 0};
            if (cut[c + 1] > cut[c])
                for (int j = 0; j < 3; ++j) (void)hipEventElapsedTime(&t[j], tr0, tr[c][j]);
            std::fprintf(stderr, "  %2d %9llu | %7.2f %7.2f %7.2f\n", c, (unsigned long long)(cut[c + 1] - cut[c]), t[0], t[1], t[2]);
            for (auto& e : tr[c]) (void)hipEventDestroy(e);
        }
        (void)hipEventDestroy(tr0);
    }
    WalkCounters wc;
    SPX_HIP(hipMemcpy(&wc, ix->counters, sizeof wc, hipMemcpyDeviceToHost));
    return walk_error(wc, width == 2 ? WALK_ERR_NARROW : WALK_ERR_PLAIN);
}

static int query_host_impl(spx_index* ix, int mode, const uint8_t* seqs, const uint64_t* offsets, uint64_t nreads,
                           void* out_lengths, uint64_t* out_pointers, void* out_docs, spx_class* out_class,
                           uint64_t bin_width, uint64_t max_value_thr, size_t width) {
    int rc = check_query(ix, mode, seqs, offsets, (uint32_t*)out_lengths, out_pointers, (uint32_t*)out_docs,
                         out_class, bin_width);
    if (rc != SPX_OK) return rc;
    // (a pipelined batch checks its pieces as it enqueues them: 10^7 offsets are 3 ms of one core, spent beside the
    // device's work there instead of in front of it)
    const bool pipelined = nreads >= (1ull << 18) && nreads && offsets[nreads] >= (64u << 20);
    if (width == 2 && !pipelined && (rc = check_narrow_reads(offsets, 0, nreads)) != SPX_OK) return rc;
    std::lock_guard<std::mutex> hg(ix->host_mu);  // one host-buffer query at a time per index
    SPX_HIP(hipSetDevice(ix->device));
    const uint64_t total = nreads ? offsets[nreads] : 0;
    void *dseq = nullptr, *doff = nullptr;
    const uint64_t padded = ((total + 3) / 4) * 4 + 32;
    if ((rc = ix->scratch[spx_index::S_SEQ].reserve(padded, &dseq)) != SPX_OK) return rc;
    if ((rc = ix->scratch[spx_index::S_OFFS].reserve((nreads + 1) * 8, &doff)) != SPX_OK) return rc;
    if (pipelined) {
        QuietOnError quiet(nullptr, true);
        return quiet.done(run_pipelined(ix, mode, seqs, offsets, nreads, (uint8_t*)dseq, (uint64_t*)doff, padded, out_lengths,
                                        out_pointers, out_docs, out_class, bin_width, max_value_thr, width));
    }
    hipStream_t st = nullptr;
    if ((rc = ctx_stream_of(ix, &st)) != SPX_OK) return rc;
    QuietOnError quiet(st);
    SPX_HIP(hipMemcpyAsync(doff, offsets, (nreads + 1) * 8, hipMemcpyHostToDevice, st));
    SPX_HIP(hipMemsetAsync((char*)dseq + total, 0, padded - total, st));
    SPX_HIP(hipMemcpyAsync(dseq, seqs, total, hipMemcpyHostToDevice, st));
    return quiet.done(run_and_fetch(ix, mode, (const uint8_t*)dseq, (const uint64_t*)doff, nreads, total, out_lengths,
                                    out_pointers, out_docs, out_class, bin_width, max_value_thr, width));
}

int spx_query_batch(spx_index* ix, int mode, const uint8_t* seqs, const uint64_t* offsets,
                    uint64_t nreads, uint32_t* out_lengths, uint64_t* out_pointers,
                    uint32_t* out_docs, spx_class* out_class, uint64_t bin_width,
                    uint64_t max_value_thr) {
    return query_host_impl(ix, mode, seqs, offsets, nreads, out_lengths, out_pointers, out_docs, out_class,
                           bin_width, max_value_thr, 4);
}

int spx_query_batch16(spx_index* ix, int mode, const uint8_t* seqs, const uint64_t* offsets,
                      uint64_t nreads, uint16_t* out_lengths, uint64_t* out_pointers,
                      uint16_t* out_docs, spx_class* out_class, uint64_t bin_width,
                      uint64_t max_value_thr) {
    return query_host_impl(ix, mode, seqs, offsets, nreads, out_lengths, out_pointers, out_docs, out_class,
                           bin_width, max_value_thr, 2);
}

int spx_digest_query_batch(spx_index* ix, int mode, int kind, uint32_t k, uint32_t w, const uint8_t* seqs,
                           const uint64_t* offsets, uint64_t nreads, uint64_t* out_offsets, uint64_t out_capacity,
                           uint32_t* out_lengths, uint64_t* out_pointers, uint32_t* out_docs, spx_class* out_class,
                           uint64_t bin_width, uint64_t max_value_thr) {
    int rc = check_query(ix, mode, seqs, offsets, out_lengths, out_pointers, out_docs, out_class, bin_width);
    if (rc != SPX_OK) return rc;
    if (!out_offsets) {
        set_error("out_offsets must be non-null");
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> hg(ix->host_mu);
    SPX_HIP(hipSetDevice(ix->device));
    const uint64_t total = nreads ? offsets[nreads] : 0;
    const uint64_t cap = spx_digest_capacity(kind, k, total);
    void *draw = nullptr, *doff = nullptr, *dseq = nullptr, *dooff = nullptr;
    if ((rc = ix->scratch[spx_index::S_RAW].reserve(((total + 15) & ~15ull) + 16, &draw)) != SPX_OK) return rc;
    if ((rc = ix->scratch[spx_index::S_OFFS].reserve((nreads + 1) * 8, &doff)) != SPX_OK) return rc;
    if ((rc = ix->scratch[spx_index::S_SEQ].reserve(cap, &dseq)) != SPX_OK) return rc;
    if ((rc = ix->scratch[spx_index::S_DIG_OFFS].reserve((nreads + 1) * 8, &dooff)) != SPX_OK) return rc;
    hipStream_t st = nullptr;
    if ((rc = ctx_stream_of(ix, &st)) != SPX_OK) return rc;
    QuietOnError quiet(st);
    SPX_HIP(hipMemcpyAsync(draw, seqs, total, hipMemcpyHostToDevice, st));
    SPX_HIP(hipMemcpyAsync(doff, offsets, (nreads + 1) * 8, hipMemcpyHostToDevice, st));
    const uint64_t* in_starts = nullptr;
    rc = digest_for_walk(ix, mode, out_lengths != nullptr, kind, k, w, (const uint8_t*)draw, (const uint64_t*)doff, nreads, total,
                         (uint8_t*)dseq, cap, (uint64_t*)dooff, st, &in_starts);
    if (rc != SPX_OK) return rc;
    SPX_HIP(hipMemcpyAsync(out_offsets, dooff, (nreads + 1) * 8, hipMemcpyDeviceToHost, st));
    SPX_HIP(hipStreamSynchronize(st));
    const uint64_t dtotal = out_offsets[nreads];
    if (dtotal > out_capacity) {
        set_error("output buffers hold %llu entries, the digested reads have %llu characters",
                  (unsigned long long)out_capacity, (unsigned long long)dtotal);
        return SPX_E_ARG;
    }
    // the digested reads never leave the device: the walk starts from the scratch buffers
    return quiet.done(run_and_fetch(ix, mode, (const uint8_t*)dseq, (const uint64_t*)dooff, nreads, dtotal, out_lengths,
                                    out_pointers, out_docs, out_class, bin_width, max_value_thr, 4, in_starts));
}

// The same with everything resident in HBM and asynchronous on `stream`: DNA reads in, results at the digested reads'
// offsets (d_out_offsets) out.  What `run -m / -a` does to a read before matching_statistics (compute_ms_pml.cpp:919-923)
// and the query itself, one call.
static int digest_query_device_impl(spx_index* ix, int mode, int kind, uint32_t k, uint32_t w, const uint8_t* d_seqs,
                                    const uint64_t* d_offsets, uint64_t nreads, uint64_t total_chars, uint8_t* d_digested,
                                    uint64_t digested_capacity, uint64_t* d_out_offsets, uint32_t* d_out_lengths,
                                    uint64_t* d_out_pointers, uint32_t* d_out_docs, spx_class* d_out_class, uint64_t bin_width,
                                    uint64_t max_value_thr, void* stream, bool narrow) {
    const uint64_t* in_starts = nullptr;
    // everything the walk would refuse is refused BEFORE the digestion is enqueued (a misaligned d_digested
    // used to take the digestion's dword stores first and the error afterwards)
    int rc = check_query(ix, mode, d_seqs, d_offsets, d_out_lengths, d_out_pointers, d_out_docs, d_out_class, bin_width);
    if (rc != SPX_OK) return rc;
    if ((((uintptr_t)d_digested | (uintptr_t)d_out_lengths | (uintptr_t)d_out_pointers | (uintptr_t)d_out_docs) & 15) != 0) {
        set_error("d_digested and the output buffers must be 16-byte aligned");
        return SPX_E_ARG;
    }
    rc = digest_for_walk(ix, mode, d_out_lengths != nullptr, kind, k, w, d_seqs, d_offsets, nreads, total_chars, d_digested,
                         digested_capacity, d_out_offsets, stream, &in_starts);
    if (rc != SPX_OK) return rc;
    // total_chars bounds the digested characters and sizes the walk's scratch; the chunked walk's geometry (is the batch
    // long reads at all, how long is a chunk) goes by what a digestion leaves: about two minimizers per window of
    // w - k + 1 k-mers, k letters each with -a
    const uint64_t per = (kind == SPX_DIGEST_DNA ? (uint64_t)k : 1ull) * 2;
    const uint64_t est = std::min<uint64_t>(total_chars, total_chars * per / (uint64_t)(w - k + 2) + nreads);
    return query_device_impl(ix, mode, d_digested, d_out_offsets, nreads, total_chars, d_out_lengths, d_out_pointers, d_out_docs,
                             d_out_class, bin_width, max_value_thr, stream, narrow, in_starts, est);
}

int spx_digest_query_batch_device(spx_index* ix, int mode, int kind, uint32_t k, uint32_t w, const uint8_t* d_seqs,
                                  const uint64_t* d_offsets, uint64_t nreads, uint64_t total_chars, uint8_t* d_digested,
                                  uint64_t digested_capacity, uint64_t* d_out_offsets, uint32_t* d_out_lengths,
                                  uint64_t* d_out_pointers, uint32_t* d_out_docs, spx_class* d_out_class, uint64_t bin_width,
                                  uint64_t max_value_thr, void* stream) {
    return digest_query_device_impl(ix, mode, kind, k, w, d_seqs, d_offsets, nreads, total_chars, d_digested, digested_capacity,
                                    d_out_offsets, d_out_lengths, d_out_pointers, d_out_docs, d_out_class, bin_width, max_value_thr,
                                    stream, false);
}

int spx_digest_query_batch_device16(spx_index* ix, int mode, int kind, uint32_t k, uint32_t w, const uint8_t* d_seqs,
                                    const uint64_t* d_offsets, uint64_t nreads, uint64_t total_chars, uint8_t* d_digested,
                                    uint64_t digested_capacity, uint64_t* d_out_offsets, uint16_t* d_out_lengths,
                                    uint64_t* d_out_pointers, uint16_t* d_out_docs, spx_class* d_out_class, uint64_t bin_width,
                                    uint64_t max_value_thr, void* stream) {
    return digest_query_device_impl(ix, mode, kind, k, w, d_seqs, d_offsets, nreads, total_chars, d_digested, digested_capacity,
                                    d_out_offsets, (uint32_t*)d_out_lengths, d_out_pointers, (uint32_t*)d_out_docs, d_out_class,
                                    bin_width, max_value_thr, stream, true);
}

// ---------------------------------------------------------------------------------------------
// The vectors as the text the reference writes (compute_ms_pml.cpp:1001-1010, 1182-1205), produced on the device
// (spx_text.hip): spx_query_text_begin runs [digestion +] the walk [+ the MS extension] and formats; the sizes of
// the streams come back, the caller sizes its (page-locked) buffers, spx_query_text_fetch copies the text.
// ---------------------------------------------------------------------------------------------
// The scratch of one text query, for spx_query_text_begin to take and for spx_query_text_reserve to allocate ahead.  The
// vectors hold value_chars values: under digestion the digested total, which _begin learns on the way and _reserve bounds by
// in_chars.  text_bytes (or null): the three streams' bytes; hint: 0 is "not known" and plans nothing (else: a buffer of no bytes).
static ScratchPlan text_plan(int mode, int digest_kind, uint32_t k, uint64_t in_chars, uint64_t value_chars, uint64_t reads,
                             uint32_t streams, bool with_class, const uint64_t* text_bytes, bool hint) {
    const bool want_len = streams & SPX_TEXT_LENGTHS, want_doc = streams & SPX_TEXT_DOCS;
    const bool ms = mode == SPX_MODE_MS, want_ptr = (streams & SPX_TEXT_POINTERS) && ms;
    ScratchPlan plan;
    plan.add(spx_index::reads_slot(digest_kind), ((in_chars + 3) / 4) * 4 + 32);
    plan.add(spx_index::S_OFFS, (reads + 1) * 8);
    plan.add(spx_index::S_GAP, (reads + 1) * 4);
    if (digest_kind) {
        plan.add(spx_index::S_SEQ, spx_digest_capacity(digest_kind, k, in_chars));
        plan.add(spx_index::S_DIG_OFFS, (reads + 1) * 8);
    }
    plan_vectors(plan, want_len || (ms && with_class), ms, want_doc, with_class, value_chars, reads, 8);
    plan.add(spx_index::S_SCAN, text_scan_bytes(reads) + 256);
    const bool on[3] = {want_len, want_ptr, want_doc};
    for (int i = 0; i < 3; ++i) {
        if (!on[i]) continue;
        plan.add(spx_index::S_LINE_BYTES + i, (reads + 2) * 8);
        plan.add(spx_index::S_LINE_START + i, (reads + 2) * 8);
        if (text_bytes && (text_bytes[i] || !hint)) plan.add(spx_index::S_TEXT + i, text_bytes[i] + 64);
    }
    return plan;
}

int spx_query_text_begin(spx_index* ix, int mode, int digest_kind, uint32_t k, uint32_t w, const uint8_t* seqs,
                         const uint64_t* offsets, uint64_t nreads, const uint32_t* gap, uint32_t streams,
                         spx_class* out_class, uint64_t bin_width, uint64_t max_value_thr, uint64_t out_bytes[3]) {
    if (!ix || !seqs || !offsets || !out_bytes) {
        set_error("index, seqs, offsets and out_bytes must be non-null");
        return SPX_E_ARG;
    }
    const bool want_len = streams & SPX_TEXT_LENGTHS, want_ptr = streams & SPX_TEXT_POINTERS, want_doc = streams & SPX_TEXT_DOCS;
    // (check_query looks at which outputs are asked for, not at the pointers' targets)
    int rc = check_query(ix, mode, seqs, offsets, (want_len || (mode == SPX_MODE_MS && out_class)) ? (uint32_t*)1 : nullptr, (mode == SPX_MODE_MS) ? (uint64_t*)1 : nullptr,
                         want_doc ? (uint32_t*)1 : nullptr, out_class, bin_width);
    if (rc != SPX_OK) return rc;
    if (want_ptr && mode != SPX_MODE_MS) {
        set_error("the pointers stream is only produced in MS mode");
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> hg(ix->host_mu);
    ix->text_ready = false;
    SPX_HIP(hipSetDevice(ix->device));
    static const bool timing = getenv("SPX_TIMING") != nullptr;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t_mark = now();
    hipStream_t st = nullptr;
    if ((rc = ctx_stream_of(ix, &st)) != SPX_OK) return rc;
    auto lap = [&](const char* what) {
        if (!timing) return;
        (void)hipStreamSynchronize(st);
        const double t = now();
        fprintf(stderr, "[spx] text_begin: %-28s %.2f ms\n", what, (t - t_mark) * 1e3);
        t_mark = t;
    };
    // SPX_PHASE_TRACE=1: the device's own times of a call's phases (events on the handle's stream, read after the call's one
    // synchronisation: nothing is added to the stream's work) -- how long the copy in / the kernels / the copy out of one
    // query context take while another context of the same device is at work (profiles/r05_cli_overlap.txt)
    static const bool phase_trace = getenv("SPX_PHASE_TRACE") != nullptr;
    static thread_local hipEvent_t pe[4] = {nullptr, nullptr, nullptr, nullptr};
    auto mark = [&](int i) {
        if (!phase_trace) return;
        if (!pe[i]) (void)hipEventCreate(&pe[i]);
        (void)hipEventRecord(pe[i], st);
    };
    mark(0);
    const uint64_t total_in = nreads ? offsets[nreads] : 0;
    void *dseq = nullptr, *doff = nullptr, *dgap = nullptr;
    const uint64_t padded = ((total_in + 3) / 4) * 4 + 32;
    // (the plan is made again as more is known: the digested total sizes the vectors, out_bytes the digits)
    auto plan_for = [&](uint64_t value_chars, const uint64_t* text_bytes) {
        return text_plan(mode, digest_kind, k, total_in, value_chars, nreads, streams, out_class != nullptr, text_bytes, false);
    };
    ScratchPlan plan = plan_for(total_in, nullptr);
    if ((rc = take(ix, plan, spx_index::reads_slot(digest_kind), &dseq)) != SPX_OK) return rc;
    if ((rc = take(ix, plan, spx_index::S_OFFS, &doff)) != SPX_OK) return rc;
    if ((rc = take(ix, plan, spx_index::S_GAP, &dgap)) != SPX_OK) return rc;
    QuietOnError quiet(st);  // (a failed call leaves nothing reading seqs / offsets / gap)
    SPX_HIP(hipMemcpyAsync(dseq, seqs, total_in, hipMemcpyHostToDevice, st));
    SPX_HIP(hipMemsetAsync((char*)dseq + total_in, 0, padded - total_in, st));
    SPX_HIP(hipMemcpyAsync(doff, offsets, (nreads + 1) * 8, hipMemcpyHostToDevice, st));
    if (gap) SPX_HIP(hipMemcpyAsync(dgap, gap, nreads * 4, hipMemcpyHostToDevice, st));
    mark(1);
    lap("copy in");
    const uint8_t* wseq = (const uint8_t*)dseq;
    const uint64_t* woff = (const uint64_t*)doff;
    uint64_t total = total_in;
    const bool narrow = first_long_read(offsets, 0, nreads) == nreads;
    const uint64_t* in_starts = nullptr;  // set when the digested reads stay where the digestion parked them
    if (digest_kind) {
        // perform_minimizer_digestion / perform_dna_minimizer_digestion (compute_ms_pml.cpp:919-923): the digested
        // reads never leave the device; the vectors are laid out at the digested offsets
        const uint64_t cap = spx_digest_capacity(digest_kind, k, total_in);
        void *dd = nullptr, *ddo = nullptr;
        if ((rc = take(ix, plan, spx_index::S_SEQ, &dd)) != SPX_OK) return rc;
        if ((rc = take(ix, plan, spx_index::S_DIG_OFFS, &ddo)) != SPX_OK) return rc;
        rc = digest_for_walk(ix, mode, want_len || out_class != nullptr, digest_kind, k, w, (const uint8_t*)dseq, (const uint64_t*)doff,
                             nreads, total_in, (uint8_t*)dd, cap, (uint64_t*)ddo, st, &in_starts);
        if (rc != SPX_OK) return rc;
        {
            PubSrc ps{{(const uint64_t*)ddo + nreads, nullptr, nullptr, nullptr}, nullptr, 0};
            if ((rc = publish(ix, ps, st)) != SPX_OK) return rc;
            if ((rc = ctx_wait(ix, st)) != SPX_OK) return rc;
            total = ix->h_pub[0];
        }
        wseq = (const uint8_t*)dd;
        woff = (const uint64_t*)ddo;
    }
    void *dlen = nullptr, *dptr = nullptr, *ddoc = nullptr, *dcls = nullptr;
    plan = plan_for(total, nullptr);
    if ((rc = take_vectors(ix, plan, &dlen, &dptr, &ddoc, &dcls)) != SPX_OK) return rc;
    rc = query_device_impl(ix, mode, wseq, woff, nreads, total, (uint32_t*)dlen, (uint64_t*)dptr, (uint32_t*)ddoc,
                           (spx_class*)dcls, bin_width, max_value_thr, st, narrow, in_starts);
    if (rc != SPX_OK) return rc;
    mark(2);
    lap("[digest +] walk");
    // count + scan per stream, then ONE read-back of the three sizes
    const size_t cub = text_scan_bytes(nreads);
    void* dcub = nullptr;
    if ((rc = take(ix, plan, spx_index::S_SCAN, &dcub)) != SPX_OK) return rc;
    const void* vals[3] = {want_len ? dlen : nullptr, want_ptr ? dptr : nullptr, want_doc ? ddoc : nullptr};
    const int vbytes[3] = {narrow ? 2 : 4, 8, narrow ? 2 : 4};
    void *lb[3] = {nullptr, nullptr, nullptr}, *ls[3] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < 3; ++i) {
        out_bytes[i] = 0;
        ix->text_bytes[i] = 0;
        if (!vals[i]) continue;
        if ((rc = take(ix, plan, spx_index::S_LINE_BYTES + i, &lb[i])) != SPX_OK) return rc;
        if ((rc = take(ix, plan, spx_index::S_LINE_START + i, &ls[i])) != SPX_OK) return rc;
        if ((rc = launch_text_count(vals[i], vbytes[i], woff, gap ? (const uint32_t*)dgap : nullptr, nreads, (uint64_t*)lb[i],
                                    (uint64_t*)ls[i], dcub, cub, st)) != SPX_OK)
            return rc;
    }
    // the three sizes and the walk's counters: published, not copied (h_pub); the class records travel with the text
    WalkCounters wc;
    {
        PubSrc ps{{nullptr, nullptr, nullptr, nullptr}, (const uint64_t*)ix->counters, (int)(sizeof wc / 8)};
        for (int i = 0; i < 3; ++i)
            if (vals[i]) ps.one[i] = (const uint64_t*)ls[i] + nreads;
        if ((rc = publish(ix, ps, st)) != SPX_OK) return rc;
        mark(3);
        if ((rc = ctx_wait(ix, st)) != SPX_OK) return rc;
        if (phase_trace) {
            float a = 0, b = 0, c = 0;
            (void)hipEventElapsedTime(&a, pe[0], pe[1]);
            (void)hipEventElapsedTime(&b, pe[1], pe[2]);
            (void)hipEventElapsedTime(&c, pe[2], pe[3]);
            fprintf(stderr, "[phases] %p begin: copy in %.3f  walk %.3f  sizes %.3f ms\n", (void*)ix, a, b, c);
        }
        for (int i = 0; i < 3; ++i) out_bytes[i] = vals[i] ? ix->h_pub[i] : 0;
        std::memcpy(&wc, ix->h_pub + 4, sizeof wc);
    }
    ix->text_cls_host = out_class;
    lap("count + scan");
    plan = plan_for(total, out_bytes);
    for (int i = 0; i < 3; ++i) {
        if (!vals[i]) continue;
        void* dtext = nullptr;
        if ((rc = take(ix, plan, spx_index::S_TEXT + i, &dtext)) != SPX_OK) return rc;
        if ((rc = launch_text_write(vals[i], vbytes[i], woff, gap ? (const uint32_t*)dgap : nullptr, nreads,
                                    (const uint64_t*)ls[i], (char*)dtext, st)) != SPX_OK)
            return rc;
        ix->text_bytes[i] = out_bytes[i];
    }
    // (not waited for: spx_query_text_fetch copies on the same stream, behind the digits)
    lap("digits");
    if ((rc = walk_error(wc, WALK_ERR_PLAIN)) != SPX_OK) return rc;
    ix->text_nreads = nreads;
    ix->text_ready = true;
    return quiet.done(SPX_OK);
}

int spx_query_text_fetch(spx_index* ix, char* text[3], uint64_t* line_start[3]) {
    if (!ix || !text) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> hg(ix->host_mu);
    if (!ix->text_ready) {
        set_error("spx_query_text_fetch without a successful spx_query_text_begin");
        return SPX_E_ARG;
    }
    SPX_HIP(hipSetDevice(ix->device));
    hipStream_t st = nullptr;
    int rc;
    if ((rc = ctx_stream_of(ix, &st)) != SPX_OK) return rc;
    static const bool timing = getenv("SPX_TIMING") != nullptr;
    static const bool phase_trace = getenv("SPX_PHASE_TRACE") != nullptr;
    static thread_local hipEvent_t fe[2] = {nullptr, nullptr};
    if (phase_trace) {
        if (!fe[0]) (void)hipEventCreate(&fe[0]), (void)hipEventCreate(&fe[1]);
        (void)hipEventRecord(fe[0], st);
    }
    const double t0 = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    for (int i = 0; i < 3; ++i) {
        if (ix->text_bytes[i] == 0) continue;
        if (text[i]) SPX_HIP(hipMemcpyAsync(text[i], ix->scratch[spx_index::S_TEXT + i].p, ix->text_bytes[i], hipMemcpyDeviceToHost, st));
        if (line_start && line_start[i])
            SPX_HIP(hipMemcpyAsync(line_start[i], ix->scratch[spx_index::S_LINE_START + i].p, (ix->text_nreads + 1) * 8, hipMemcpyDeviceToHost, st));
    }
    if (ix->text_cls_host)
        SPX_HIP(hipMemcpyAsync(ix->text_cls_host, ix->scratch[spx_index::S_CLASS].p, ix->text_nreads * sizeof(spx_class), hipMemcpyDeviceToHost, st));
    if (phase_trace) (void)hipEventRecord(fe[1], st);
    if ((rc = ctx_wait(ix, st)) != SPX_OK) return rc;
    if (phase_trace) {
        float a = 0;
        (void)hipEventElapsedTime(&a, fe[0], fe[1]);
        fprintf(stderr, "[phases] %p fetch: copy out %.3f ms (behind the digits' kernels)\n", (void*)ix, a);
    }
    ix->text_cls_host = nullptr;
    ix->text_ready = false;
    if (timing)
        fprintf(stderr, "[spx] text_fetch: %.2f ms for %.1f MB\n",
                (std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() - t0) * 1e3,
                (ix->text_bytes[0] + ix->text_bytes[1] + ix->text_bytes[2]) / 1e6);
    return SPX_OK;
}

// The scratch a spx_query_text_begin / _fetch pair of up to max_chars characters in max_reads reads will ask for, allocated now:
// the first super-batch of a run otherwise pays for it (~300 MB of hipMalloc at ~30 ms / GB: 10 ms of a 1.5 ms call, and the
// workers of one device queue behind each other for it), and a scratch buffer that has to GROW mid-run is freed first -- a
// device-wide synchronisation under every other worker's feet.  A hint: whatever turns out larger still grows on demand.
int spx_query_text_reserve(spx_index* ix, int mode, int digest_kind, uint32_t k, uint64_t max_chars, uint64_t max_reads,
                           uint32_t streams, int with_class, const uint64_t text_bytes[3]) {
    if (!ix || (mode != SPX_MODE_PML && mode != SPX_MODE_MS)) {
        set_error("spx_query_text_reserve: index and a mode");
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> hg(ix->host_mu);  // (the order every host-buffer query takes them in: host_mu, then mu)
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    hipStream_t st = nullptr;
    int rc;
    if ((rc = ctx_stream_of(ix, &st)) != SPX_OK) return rc;
    // (under digestion the vectors are sized from the digested total, known only per batch: what an undigested batch would
    // need is the bound)
    const ScratchPlan plan = text_plan(mode, digest_kind, k, max_chars, max_chars, max_reads, streams, with_class != 0, text_bytes, true);
    void* p = nullptr;
    for (int i = 0; i < plan.n; ++i)
        if ((rc = ix->scratch[plan.item[i].slot].reserve(plan.item[i].bytes, &p)) != SPX_OK) return rc;
    const bool need_len = (streams & SPX_TEXT_LENGTHS) || (mode == SPX_MODE_MS && with_class);
    if (mode == SPX_MODE_PML && need_len &&  // the walk's reset bits (prepare_len_mask)
        (rc = ix->chunk_scr[spx_index::C_LEN_BITS].reserve(len_mask_pairs(max_chars, max_reads) * 16, &p)) != SPX_OK)
        return rc;
    if (!ix->h_pub) {
        PubSrc none{{nullptr, nullptr, nullptr, nullptr}, nullptr, 0};
        if ((rc = publish(ix, none, st)) != SPX_OK) return rc;
    }
    SPX_HIP(hipStreamSynchronize(st));
    return SPX_OK;
}

// the counters of the last query, once it has ended (callers hold mu; after_ev1: waits for that event first)
static int last_counters(spx_index* ix, bool after_ev1, WalkCounters& wc) {
    if (!ix->have_timing) {
        set_error("no query has run on this index yet");
        return SPX_E_ARG;
    }
    SPX_HIP(hipSetDevice(ix->device));
    if (after_ev1) SPX_HIP(hipEventSynchronize(ix->ev1));
    SPX_HIP(hipStreamSynchronize(ix->last_stream));
    SPX_HIP(hipMemcpy(&wc, ix->counters, sizeof wc, hipMemcpyDeviceToHost));
    return SPX_OK;
}

int spx_last_chunk_stats(spx_index* ix, uint64_t out[4]) {
    if (!ix || !out) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> g(ix->mu);
    WalkCounters wc;
    const int rc = last_counters(ix, false, wc);
    if (rc != SPX_OK) return rc;
    out[0] = ix->last_chunk_len;
    out[1] = ix->last_chunk_bound;
    out[2] = wc.reserved0;
    out[3] = wc.pad_;
    return SPX_OK;
}

int spx_last_walk_stats(spx_index* ix, spx_walk_stats* out) {
    if (!ix || !out) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> g(ix->mu);
    WalkCounters wc;
    const int rc = last_counters(ix, true, wc);
    if (rc != SPX_OK) return rc;
    float ms = 0;
    SPX_HIP(hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
    out->steps = wc.steps;
    out->jumps = wc.jumps;
    out->pred_jumps = wc.pred_jumps;
    out->row_loads = wc.row_loads;
    out->dir_loads = wc.dir_loads;
    out->kernel_ms = ms;
    return walk_error(wc, WALK_ERR_STATS);
}

}  // extern "C"
