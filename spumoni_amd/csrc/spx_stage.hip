// spx_stage.hip -- the staged walk under the products over a batch of reads in host memory (spv_assign_batch,
// spm_mems_begin, spp_place_batch; spx_internal.h has the interface), and the counters of a product's kernels.
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
    for (auto& sc : ix->stage_scr)
        if (sc.p) (void)hipFree(sc.p);
    for (auto& st : ix->stage_s)
        if (st) (void)hipStreamDestroy(st);
}

int product_collect(spx_index* ix, spx_index::Product& p, int words, int nacc) {
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    SPX_HIP(hipEventSynchronize(p.ev1));
    unsigned long long c[16];
    SPX_HIP(hipMemcpy(c, p.counters.p, (size_t)words * 8, hipMemcpyDeviceToHost));
    float ms = 0;
    SPX_HIP(hipEventElapsedTime(&ms, p.ev0, p.ev1));
    for (int i = 0; i < nacc; ++i) p.acc[i] += c[i];
    p.ms += ms;
    p.error |= c[words - 1];
    p.pending = false;
    return SPX_OK;
}
void product_reset(spx_index* ix, spx_index::Product& p) {
    std::lock_guard<std::mutex> g(ix->mu);
    std::memset(p.acc, 0, sizeof p.acc);
    p.ms = 0;
    p.error = 0;
    p.pending = false;
}
void product_release(spx_index::Product& p) {
    if (p.counters.p) (void)hipFree(p.counters.p);
    if (p.ev0) (void)hipEventDestroy(p.ev0);
    if (p.ev1) (void)hipEventDestroy(p.ev1);
}

}  // namespace spx
