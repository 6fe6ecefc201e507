// spx_stage.hip -- the staged walk under the products over a batch of reads in host memory (spv_assign_batch,
// spm_mems_begin, spp_place_batch; spx_internal.h has the interface), and what every product does alike on the host: the
// counters, events and step times of its kernels (Product), the records that wait for its _fetch (Ready), the argument
// checks of the host forms and the release of its scratch.
//
// What the products share is here once: the checks of the offsets, the cuts, the width of the values, the buffer sets, the
// rebased offsets and the zeroed tail of a piece, the four-way dispatch of digestion and walk, the digested offsets on
// their way back for out_values, and the loop copy_in(c), finish(c - 1), walk(c).  What a product adds -- its kernels on a
// piece's view, what it reads when the piece's stream has been waited for -- it passes in; its streams and its way of
// waiting are its own too (two streams of the pipeline and hipStreamSynchronize, or the handle's stream and ctx_wait).
#include <algorithm>
#include <cstring>

#include "spx_internal.h"

namespace spx {

int stage_streams(spx_index* ix, hipStream_t out[2]) {
    for (int b = 0; b < 2; ++b) {
        if (!ix->stage_s[b]) SPX_HIP(hipStreamCreateWithFlags(&ix->stage_s[b], hipStreamNonBlocking));
        out[b] = ix->stage_s[b];
    }
    return SPX_OK;
}

int stage_plan(spx_index* ix, const StageJob& job, StagePlan* plan) {
    constexpr uint64_t PIECE_CHARS = 32ull << 20, PIECE_READS = 4ull << 20;
    const uint64_t* offsets = job.offsets;
    StagePlan& pl = *plan;
    pl.cut.assign(1, 0);
    for (uint64_t q = 0; q < job.nreads; ++q) {
        if (offsets[q + 1] < offsets[q]) {
            set_error("offsets must not decrease (read %llu)", (unsigned long long)q);
            return SPX_E_ARG;
        }
        pl.longest = std::max(pl.longest, offsets[q + 1] - offsets[q]);
        const uint64_t q0 = pl.cut.back();
        if (q + 1 == job.nreads || (!job.one_piece && (offsets[q + 1] - offsets[q0] >= PIECE_CHARS || q + 1 - q0 >= PIECE_READS))) {
            pl.worst_chars = std::max(pl.worst_chars, offsets[q + 1] - offsets[q0]);
            pl.worst_reads = std::max(pl.worst_reads, q + 1 - q0);
            pl.cut.push_back(q + 1);
        }
    }
    if (pl.longest >= (1ull << 32)) {
        set_error("a read has 2^32 characters or more");
        return SPX_E_ARG;
    }
    pl.narrow = pl.longest < 65536;
    pl.sets = pl.cut.size() > 2 ? 2 : 1;
    const size_t width = pl.narrow ? 2 : 4;
    pl.raw_bytes = ((pl.worst_chars + 15) & ~15ull) + 64;
    pl.dig_bytes = job.digest_kind ? spx_digest_capacity(job.digest_kind, job.k, pl.worst_chars) + 32 : 0;
    size_t sizes[spx_index::G_SET_STRIDE] = {};
    sizes[spx_index::G_RAW] = pl.raw_bytes;
    sizes[spx_index::G_OFFS] = (pl.worst_reads + 1) * 8;
    sizes[spx_index::G_DIG] = pl.dig_bytes;
    sizes[spx_index::G_DIG_OFFS] = job.digest_kind ? (pl.worst_reads + 1) * 8 : 0;
    sizes[spx_index::G_LEN] = (pl.worst_chars + 16) * width;
    sizes[spx_index::G_DOC] = job.want_docs ? (pl.worst_chars + 16) * width : 0;
    sizes[spx_index::G_PTR] = job.mode == SPX_MODE_MS ? (pl.worst_chars + 2) * 8 : 0;
    int rc;
    for (int b = 0; b < pl.sets; ++b)
        for (int i = 0; i < spx_index::G_SET_STRIDE; ++i)
            if (sizes[i] && (rc = ix->stage_scr[b * spx_index::G_SET_STRIDE + i].reserve(sizes[i], &pl.p[b][i])) != SPX_OK) return rc;
    return SPX_OK;
}

int stage_run(spx_index* ix, const StageJob& job, const StagePlan& plan) {
    struct Unparked {
        spx_index* ix;
        int before;
        Unparked(spx_index* i, bool never) : ix(i), before(i->digest_parked) {
            if (never) ix->digest_parked = 1;
        }
        ~Unparked() { ix->digest_parked = before; }
    } unparked(ix, job.reads_characters);
    const uint64_t* offsets = job.offsets;
    const int kind = job.digest_kind;
    struct Set {
        std::vector<uint64_t> h_off, h_dig_off;
        StageView view;
    } set[2];
    const size_t npieces = plan.cut.size() - 1;
    auto copy_in = [&](size_t c) -> int {
        Set& s = set[c & 1];
        void* const* p = plan.p[c & 1];
        hipStream_t st = job.streams[c & 1];
        const uint64_t q0 = plan.cut[c], q1 = plan.cut[c + 1], a0 = offsets[q0], tc = offsets[q1] - a0;
        const uint64_t* src = offsets + q0;
        if (a0) {
            s.h_off.resize(q1 - q0 + 1);
            for (uint64_t q = q0; q <= q1; ++q) s.h_off[q - q0] = offsets[q] - a0;
            src = s.h_off.data();
        }
        uint8_t* raw = (uint8_t*)p[spx_index::G_RAW];
        SPX_HIP(hipMemcpyAsync(p[spx_index::G_OFFS], src, (q1 - q0 + 1) * 8, hipMemcpyHostToDevice, st));
        SPX_HIP(hipMemsetAsync(raw + tc, 0, plan.raw_bytes - tc, st));
        if (tc) SPX_HIP(hipMemcpyAsync(raw, job.seqs + a0, tc, hipMemcpyHostToDevice, st));
        return SPX_OK;
    };
    auto walk = [&](size_t c) -> int {
        Set& s = set[c & 1];
        void* const* p = plan.p[c & 1];
        hipStream_t st = job.streams[c & 1];
        const uint64_t q0 = plan.cut[c], q1 = plan.cut[c + 1], nr = q1 - q0, tc = offsets[q1] - offsets[q0];
        const uint8_t* raw = (const uint8_t*)p[spx_index::G_RAW];
        const uint64_t* off = (const uint64_t*)p[spx_index::G_OFFS];
        uint8_t* dig = (uint8_t*)p[spx_index::G_DIG];
        uint64_t *dig_off = (uint64_t*)p[spx_index::G_DIG_OFFS], *ptr = (uint64_t*)p[spx_index::G_PTR];
        void *len = p[spx_index::G_LEN], *doc = p[spx_index::G_DOC];
        int r;
        if (kind)
            r = plan.narrow ? spx_digest_query_batch_device16(ix, job.mode, kind, job.k, job.w, raw, off, nr, tc, dig, plan.dig_bytes, dig_off,
                                                              (uint16_t*)len, ptr, (uint16_t*)doc, nullptr, 0, 0, st)
                            : spx_digest_query_batch_device(ix, job.mode, kind, job.k, job.w, raw, off, nr, tc, dig, plan.dig_bytes, dig_off,
                                                            (uint32_t*)len, ptr, (uint32_t*)doc, nullptr, 0, 0, st);
        else
            r = plan.narrow ? spx_query_batch_device16(ix, job.mode, raw, off, nr, tc, (uint16_t*)len, ptr, (uint16_t*)doc, nullptr, 0, 0, st)
                            : spx_query_batch_device(ix, job.mode, raw, off, nr, tc, (uint32_t*)len, ptr, (uint32_t*)doc, nullptr, 0, 0, st);
        if (r != SPX_OK) return r;
        s.view = StageView{kind ? dig : raw, kind ? dig_off : off, len, ptr, doc, q0, nr, tc, plan.narrow ? 16 : 32, (int)(c & 1), st};
        if ((r = job.enqueue(s.view)) != SPX_OK) return r;
        if (job.out_values && kind) {
            s.h_dig_off.resize(nr + 1);
            SPX_HIP(hipMemcpyAsync(s.h_dig_off.data(), dig_off, (nr + 1) * 8, hipMemcpyDeviceToHost, st));
        }
        return SPX_OK;
    };
    auto finish = [&](size_t c) -> int {
        Set& s = set[c & 1];
        const uint64_t q0 = plan.cut[c], q1 = plan.cut[c + 1];
        int r = job.wait(job.streams[c & 1]);
        if (r != SPX_OK) return r;
        spx_walk_stats ws;
        if ((r = spx_last_walk_stats(ix, &ws)) != SPX_OK) return r;
        if ((r = job.collect(s.view)) != SPX_OK) return r;
        if (job.out_values)
            for (uint64_t q = q0; q < q1; ++q)
                job.out_values[q] = kind ? s.h_dig_off[q - q0 + 1] - s.h_dig_off[q - q0] : offsets[q + 1] - offsets[q];
        return SPX_OK;
    };
    int rc;
    for (size_t c = 0; c < npieces; ++c) {
        if ((rc = copy_in(c)) != SPX_OK) return rc;
        if (c && (rc = finish(c - 1)) != SPX_OK) return rc;
        if ((rc = walk(c)) != SPX_OK) return rc;
    }
    return finish(npieces - 1);
}

void release_stage(spx_index* ix) {
    release(ix->stage_scr, spx_index::G_COUNT, nullptr);
    for (auto& st : ix->stage_s)
        if (st) (void)hipStreamDestroy(st);
}

int product_open(spx_index::Product& p, size_t words, hipStream_t st, int step, void** c) {
    if (!p.ev0) SPX_HIP(hipEventCreate(&p.ev0));
    if (!p.ev1) SPX_HIP(hipEventCreate(&p.ev1));
    int rc;
    if ((rc = p.counters.reserve(words * 8, c)) != SPX_OK) return rc;
    if (p.have && p.stream != st) SPX_HIP(hipStreamWaitEvent(st, p.ev1, 0));
    SPX_HIP(hipMemsetAsync(*c, 0, words * 8, st));
    SPX_HIP(hipEventRecord(p.ev0, st));
    p.label0 = step < spx_index::Product::STEPS ? step : -1;  // (product_mark refuses such a label; here it is a constant)
    p.nmarks = 0;
    return SPX_OK;
}
int product_mark(spx_index::Product& p, int step, hipStream_t st) {
    if (p.nmarks == spx_index::Product::MARKS || step >= spx_index::Product::STEPS) {
        set_error("internal: more marks, or a later step, than a product holds");
        return SPX_E_ARG;
    }
    hipEvent_t& e = p.ev_mark[p.nmarks];
    if (!e) SPX_HIP(hipEventCreate(&e));
    SPX_HIP(hipEventRecord(e, st));
    p.label[p.nmarks++] = step;
    return SPX_OK;
}
int product_close(spx_index::Product& p, hipStream_t st) {
    SPX_HIP(hipEventRecord(p.ev1, st));
    p.have = p.pending = true;
    p.stream = st;
    return SPX_OK;
}
int product_collect(spx_index* ix, spx_index::Product& p, int words, int nacc, int error_word) {
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    SPX_HIP(hipEventSynchronize(p.ev1));
    unsigned long long c[spx_index::Product::WORDS];
    SPX_HIP(hipMemcpy(c, p.counters.p, (size_t)words * 8, hipMemcpyDeviceToHost));
    if (error_word < 0) error_word = words - 1;
    for (int i = 0; i < nacc; ++i)
        if (i != error_word) p.acc[i] += c[i];
    p.error |= c[error_word];
    float ms = 0;
    SPX_HIP(hipEventElapsedTime(&ms, p.ev0, p.ev1));
    p.ms += ms;
    // the boundaries ev0, the marks, ev1: what lies between two of them is the step's that the first one names
    hipEvent_t from = p.ev0;
    int step = p.label0;
    for (int i = 0; i <= p.nmarks; ++i) {
        hipEvent_t to = i < p.nmarks ? p.ev_mark[i] : p.ev1;
        if (step >= 0) {
            SPX_HIP(hipEventElapsedTime(&ms, from, to));
            p.step_ms[step] += ms;
        }
        from = to;
        step = i < p.nmarks ? p.label[i] : -1;
    }
    p.pending = false;
    return SPX_OK;
}
void product_reset(spx_index* ix, spx_index::Product& p) {
    std::lock_guard<std::mutex> g(ix->mu);
    std::memset(p.acc, 0, sizeof p.acc);
    std::memset(p.step_ms, 0, sizeof p.step_ms);
    p.ms = 0;
    p.error = 0;
    p.pending = false;
}
void product_release(spx_index::Product& p) {
    if (p.counters.p) (void)hipFree(p.counters.p);
    if (p.ev0) (void)hipEventDestroy(p.ev0);
    if (p.ev1) (void)hipEventDestroy(p.ev1);
    for (hipEvent_t e : p.ev_mark)
        if (e) (void)hipEventDestroy(e);
}
void release(spx_index::Scratch* scr, int n, spx_index::Product* p) {
    for (int i = 0; i < n; ++i)
        if (scr[i].p) (void)hipFree(scr[i].p);
    if (p) product_release(*p);
}

int ready_take(spx_index::Ready& r, uint64_t reads, uint64_t n, const char* who, const char* whose) {
    // (another host thread on this handle between the two locks would have taken the entries or replaced them)
    if (!r.ok || r.reads != reads || r.n != n) {
        set_error("%s: another call on this index took %s: calls on one handle must not overlap", who, whose);
        return SPX_E_ARG;
    }
    r.ok = false;
    return SPX_OK;
}
int ready_fetch(spx_index* ix, spx_index::Ready& r, const spx_index::Scratch& op_offsets, const spx_index::Scratch& ops,
                const char* fetch_name, const char* begin_name, uint64_t* out_op_offsets, uint32_t* out_ops) {
    std::lock_guard<std::mutex> hg(ix->host_mu);
    if (!r.ok) {
        set_error("%s without a successful %s before it", fetch_name, begin_name);
        return SPX_E_ARG;
    }
    if (!out_op_offsets || (r.n && !out_ops)) {
        set_error("out_op_offsets and out_ops must be non-null");
        return SPX_E_ARG;
    }
    r.ok = false;
    if (r.reads == 0) {
        out_op_offsets[0] = 0;
        return SPX_OK;
    }
    SPX_HIP(hipSetDevice(ix->device));
    SPX_HIP(hipMemcpy(out_op_offsets, op_offsets.p, (r.reads + 1) * 8, hipMemcpyDeviceToHost));
    if (r.n) SPX_HIP(hipMemcpy(out_ops, ops.p, r.n * 4, hipMemcpyDeviceToHost));
    return SPX_OK;
}

int check_digest_kind(int digest_kind) {
    if (digest_kind != 0 && digest_kind != SPX_DIGEST_PROMOTED && digest_kind != SPX_DIGEST_DNA) {
        set_error("digest_kind must be 0, SPX_DIGEST_PROMOTED or SPX_DIGEST_DNA");
        return SPX_E_ARG;
    }
    return SPX_OK;
}
int check_batch(const spx_index* ix, const char* what, int flags, uint64_t min_length, int digest_kind, int want_docs,
                const char* null_pointers, const uint64_t* offsets, uint64_t nreads) {
    constexpr uint64_t PIECE_CHARS = 32ull << 20, PIECE_READS = 4ull << 20;
    if ((flags & BATCH_MIN_LENGTH) && min_length == 0) {
        set_error("min_length must be at least 1: a position of length 0 matches nothing");
        return SPX_E_ARG;
    }
    int rc;
    if ((rc = check_digest_kind(digest_kind)) != SPX_OK) return rc;
    if ((flags & BATCH_TEXT) && (!ix->has_samples || !ix->text)) {
        set_error("%s need an index built with SA samples and the text (spx_index_set_text / spx_index_rebuild_text)", what);
        return SPX_E_ARG;
    }
    if (want_docs && !ix->has_docs) {
        set_error("document ids requested but the index has no document array");
        return SPX_E_ARG;
    }
    if (null_pointers) {
        set_error("%s", null_pointers);
        return SPX_E_ARG;
    }
    if ((flags & BATCH_ONE_PIECE) &&
        (nreads > PIECE_READS || (nreads && offsets[nreads] >= offsets[0] && offsets[nreads] - offsets[0] > PIECE_CHARS))) {
        set_error("one piece per call: at most 32 Mi characters and 4 Mi reads");
        return SPX_E_ARG;
    }
    return SPX_OK;
}

}  // namespace spx
