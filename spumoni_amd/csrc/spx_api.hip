// spx_api.hip -- the C-ABI of libspumoni_gpu.so (include/spumoni_gpu.h).
// No CPU fallback exists anywhere in this library: without a gfx950 device every
// entry point that needs one returns SPX_E_NODEVICE.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "spx_internal.h"

namespace spx {

static thread_local std::string g_err;

void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}

int hip_fail(hipError_t e, const char* what, const char* file, int line) {
    set_error("HIP error %d (%s) at %s:%d: %s", (int)e, hipGetErrorString(e), file, line, what);
    return SPX_E_HIP;
}

static int usable_devices() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int select_device(int device) {
    const int n = usable_devices();
    if (n <= 0) {
        set_error("no HIP device visible: libspumoni_gpu has no CPU fallback");
        return SPX_E_NODEVICE;
    }
    if (device < 0 || device >= n) {
        set_error("device %d out of range (0..%d)", device, n - 1);
        return SPX_E_ARG;
    }
    SPX_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    SPX_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s; this library is built for gfx950 (MI355X) only", device,
                  prop.gcnArchName);
        return SPX_E_NODEVICE;
    }
    return SPX_OK;
}

static bool read_file(const std::string& path, std::vector<uint8_t>& out) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    out.resize((size_t)sz);
    bool ok = sz == 0 || fread(out.data(), 1, (size_t)sz, f) == (size_t)sz;
    fclose(f);
    return ok;
}

// 5-byte little-endian records (THRBYTES / SSABYTES, include/common.hpp:59-60)
static void unpack5(const std::vector<uint8_t>& raw, size_t stride, size_t pick, std::vector<uint64_t>& out) {
    // 10^9 records take seconds on one thread (and so does first touching 8 GB of output): eight threads
    const size_t n = raw.size() / (5 * stride);
    out.resize(n);
    const unsigned nt = n >= (1u << 22) ? 8 : 1;
    auto work = [&](unsigned t) {
        for (size_t i = n * t / nt, e = n * (t + 1) / nt; i < e; ++i) {
            uint64_t v = 0;
            std::memcpy(&v, raw.data() + (i * stride + pick) * 5, 5);
            out[i] = v;
        }
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; ++t) th.emplace_back(work, t);
    work(0);
    for (auto& x : th) x.join();
}

// bonsai's RollingHasher draws its character table from a Mersenne twister seeded with 1337
// and keeps 8 bits (our reading of CharacterHash): entry c = c-th output
static void default_charhash(uint8_t out[4]) {
    std::mt19937 gen(1337u);
    uint8_t table[256];
    for (int c = 0; c < 256; ++c) table[c] = (uint8_t)(gen() & 0xffu);
    out[0] = table['A'];
    out[1] = table['C'];
    out[2] = table['G'];
    out[3] = table['T'];
}

// the stream of the handle's host-buffer queries (created on first use; callers hold host_mu)
int ctx_stream_of(spx_index* ix, hipStream_t* out) {
    if (!ix->ctx_stream) SPX_HIP(hipStreamCreateWithFlags(&ix->ctx_stream, hipStreamNonBlocking));
    *out = ix->ctx_stream;
    return SPX_OK;
}

// Waiting for the handle's stream: spinning (hipStreamSynchronize: lowest latency) or, "blocking_sync", asleep on an event.
int ctx_wait(spx_index* ix, hipStream_t st) {
    if (!ix->blocking_sync) {
        SPX_HIP(hipStreamSynchronize(st));
        return SPX_OK;
    }
    if (!ix->ev_wait) SPX_HIP(hipEventCreateWithFlags(&ix->ev_wait, hipEventBlockingSync | hipEventDisableTiming));
    SPX_HIP(hipEventRecord(ix->ev_wait, st));
    SPX_HIP(hipEventSynchronize(ix->ev_wait));
    return SPX_OK;
}

// counters, events and knobs every index carries, however its arrays came to be
int init_runtime(spx_index* ix) {
    default_charhash(ix->charhash);
    SPX_HIP(hipMalloc((void**)&ix->counters, sizeof(WalkCounters)));
    SPX_HIP(hipMemset(ix->counters, 0, sizeof(WalkCounters)));
    SPX_HIP(hipEventCreate(&ix->ev0));
    SPX_HIP(hipEventCreate(&ix->ev1));
    SPX_HIP(hipEventCreateWithFlags(&ix->ev_done, hipEventDisableTiming));
    SPX_HIP(hipEventCreateWithFlags(&ix->ev_dig, hipEventDisableTiming));
    SPX_HIP(hipDeviceSynchronize());
    return SPX_OK;
}

}  // namespace spx

using namespace spx;

extern "C" {

const char* spx_last_error(void) { return g_err.c_str(); }

int spx_device_count(void) { return usable_devices(); }

void spx_index_free(spx_index* ix) {
    if (!ix) return;
    static const bool trace = getenv("SPX_FREE_TRACE") != nullptr;
#define SPX_FT(what) do { if (trace) fprintf(stderr, "[spx] free %p: %s\n", (void*)ix, what); } while (0)
    SPX_FT("begin");
    (void)hipSetDevice(ix->device);
    if (ix->owner) {
        ix->owner.reset();  // shared with same-device clones: the last handle frees the arrays
    } else {
        void** arr[spx_index::NARR];
        index_arrays(ix, arr);
        for (void** a : arr)
            if (*a) (void)hipFree(*a);
    }
    SPX_FT("arrays released");
    if (ix->counters) (void)hipFree(ix->counters);
    if (ix->ctx_stream) (void)hipStreamDestroy(ix->ctx_stream);
    if (ix->h_pub) (void)hipHostFree(ix->h_pub);
    if (ix->ev_wait) (void)hipEventDestroy(ix->ev_wait);
    SPX_FT("stream destroyed");
    for (auto& st : ix->pipe_s)
        if (st) (void)hipStreamDestroy(st);
    for (int c = 0; c < spx_index::PIPE_CHUNKS; ++c) {
        if (ix->pipe_in[c]) (void)hipEventDestroy(ix->pipe_in[c]);
        if (ix->pipe_k[c]) (void)hipEventDestroy(ix->pipe_k[c]);
    }
    for (auto& sc : ix->scratch)
        if (sc.p) (void)hipFree(sc.p);
    for (auto& sc : ix->chunk_scr)
        if (sc.p) (void)hipFree(sc.p);
    for (auto& sc : ix->digest_scr)
        if (sc.p) (void)hipFree(sc.p);
    release_stage(ix);
    release_votes(ix);
    release_mems(ix);
    release_place(ix);
    release_chain(ix);
    release_align(ix);
    release_cigar(ix);
    release_extend(ix);
    release_map(ix);
    release_cover(ix);
    release_call(ix);
    release_consensus(ix);
    if (ix->ev_dig) (void)hipEventDestroy(ix->ev_dig);
    if (ix->ev0) (void)hipEventDestroy(ix->ev0);
    if (ix->ev1) (void)hipEventDestroy(ix->ev1);
    if (ix->ev_done) (void)hipEventDestroy(ix->ev_done);
    SPX_FT("done");
#undef SPX_FT
    delete ix;
}

// The text is one of the shared arrays: it can only be replaced while no same-device clone reads it (callers hold mu).
static int own_arrays_alone(spx_index* ix) {
    if (!ix->owner) return SPX_OK;
    if (ix->owner.use_count() > 1) {
        set_error("the index shares its arrays with a clone on the same device: set or rebuild the text before cloning");
        return SPX_E_ARG;
    }
    for (void*& a : ix->owner->p) a = nullptr;  // back to plain ownership by this handle
    ix->owner.reset();
    return SPX_OK;
}

static int from_runs_impl(spx_index* ix, const uint8_t* heads, const uint64_t* lens,
                          const uint64_t* thr, uint64_t r, const uint64_t* ssa, const uint64_t* esa,
                          const uint64_t* ds, const uint64_t* de, int where) {
    if (!heads || !lens || !thr || r == 0) {
        set_error("heads, lens and thr must be non-null and r > 0");
        return SPX_E_ARG;
    }
    if ((ssa == nullptr) != (esa == nullptr) || (ds == nullptr) != (de == nullptr)) {
        set_error("ssa/esa and doc_start/doc_end must be given in pairs");
        return SPX_E_ARG;
    }
    ix->r = r;
    struct Tmp {
        void* p = nullptr;
        ~Tmp() {
            if (p) (void)hipFree(p);
        }
    } t[7];
    const void* src[7] = {heads, lens, thr, ssa, esa, ds, de};
    const void* dev[7];
    for (int i = 0; i < 7; ++i) {
        dev[i] = src[i];
        if (where == 0 && src[i]) {
            const size_t bytes = (i == 0 ? 1 : 8) * r;
            SPX_HIP(hipMalloc(&t[i].p, bytes));
            SPX_HIP(hipMemcpy(t[i].p, src[i], bytes, hipMemcpyHostToDevice));
            dev[i] = t[i].p;
        }
    }
    // (host arrays: the device copies are this function's own and are given back before the fat table is sized)
    int rc = flatten_on_device(ix, (const uint8_t*)dev[0], (const uint64_t*)dev[1],
                               (const uint64_t*)dev[2], (const uint64_t*)dev[3],
                               (const uint64_t*)dev[4], (const uint64_t*)dev[5],
                               (const uint64_t*)dev[6], [&] {
                                   for (Tmp& x : t) {
                                       if (x.p) (void)hipFree(x.p);
                                       x.p = nullptr;
                                   }
                               });
    if (rc != SPX_OK) return rc;
    return init_runtime(ix);
}

spx_index* spx_index_from_runs(const uint8_t* heads, const uint64_t* lens, const uint64_t* thr,
                               uint64_t r, const uint64_t* ssa, const uint64_t* esa,
                               const uint64_t* doc_start, const uint64_t* doc_end, int where,
                               int device) {
    if (select_device(device) != SPX_OK) return nullptr;
    if (where != 0 && where != 1) {
        set_error("where must be 0 (host) or 1 (device)");
        return nullptr;
    }
    spx_index* ix = new spx_index();
    ix->device = device;
    if (from_runs_impl(ix, heads, lens, thr, r, ssa, esa, doc_start, doc_end, where) != SPX_OK) {
        spx_index_free(ix);
        return nullptr;
    }
    return ix;
}

spx_index* spx_index_load_raw(const char* prefix, int mode, int device) {
    if (!prefix) {
        set_error("prefix is null");
        return nullptr;
    }
    const std::string p(prefix);
    std::vector<uint8_t> heads, raw;
    std::vector<uint64_t> lens, thr, ssa, esa;
    if (!read_file(p + ".bwt.heads", heads) || heads.empty()) {
        set_error("cannot read %s.bwt.heads", prefix);
        return nullptr;
    }
    const uint64_t r = heads.size();
    if (!read_file(p + ".bwt.len", raw) || raw.size() != r * 5) {
        set_error("%s.bwt.len missing or not %llu 5-byte records", prefix, (unsigned long long)r);
        return nullptr;
    }
    unpack5(raw, 1, 0, lens);
    if (!read_file(p + ".thr_pos", raw) || raw.size() != r * 5) {
        set_error("%s.thr_pos missing or not %llu 5-byte records", prefix, (unsigned long long)r);
        return nullptr;
    }
    unpack5(raw, 1, 0, thr);
    if (mode == SPX_MODE_MS) {
        uint64_t n = 0;
        for (uint64_t v : lens) n += v;
        for (int which = 0; which < 2; ++which) {
            const std::string path = p + (which ? ".esa" : ".ssa");
            if (!read_file(path, raw) || raw.size() != r * 10) {
                set_error("%s missing or not %llu (left,right) 5-byte pairs", path.c_str(),
                          (unsigned long long)r);
                return nullptr;
            }
            std::vector<uint64_t>& dst = which ? esa : ssa;
            unpack5(raw, 2, 1, dst);
            for (auto& v : dst) v = v ? v - 1 : n - 1;  // compute_ms_pml.cpp:433
        }
    }
    return spx_index_from_runs(heads.data(), lens.data(), thr.data(), r,
                               ssa.empty() ? nullptr : ssa.data(), esa.empty() ? nullptr : esa.data(),
                               nullptr, nullptr, 0, device);
}

int spx_index_stats(const spx_index* ix, uint64_t* n, uint64_t* r) {
    if (!ix) {
        set_error("index is null");
        return SPX_E_ARG;
    }
    if (n) *n = ix->n;
    if (r) *r = ix->r;
    return SPX_OK;
}

int spx_index_device_bytes(const spx_index* ix, uint64_t* bytes) {
    if (!ix || !bytes) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    *bytes = ix->device_bytes + ix->n_text;
    return SPX_OK;
}

int spx_index_set_text(spx_index* ix, const uint8_t* text, uint64_t n_text, int where) {
    if (!ix || !text) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    const bool unchecked = (where & SPX_TEXT_UNCHECKED) != 0;
    where &= ~SPX_TEXT_UNCHECKED;
    if (!unchecked && n_text + 1 != ix->n) {
        // the BWT of a text of n_text characters plus its terminator has n_text + 1 positions
        set_error("text has %llu characters but the index was built over %llu (+ terminator): not the indexed text",
                  (unsigned long long)n_text, (unsigned long long)(ix->n - 1));
        return SPX_E_FORMAT;
    }
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    if (const int rc_own = own_arrays_alone(ix); rc_own != SPX_OK) return rc_own;
    if (ix->text) (void)hipFree(ix->text);
    ix->text = nullptr;
    ix->n_text = 0;
    bind_view(ix);
    SPX_HIP(hipMalloc((void**)&ix->text, n_text + 16));
    SPX_HIP(hipMemcpy(ix->text, text, n_text, where ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    SPX_HIP(hipMemset(ix->text + n_text, 0, 16));
    ix->n_text = n_text;
    ix->arr_bytes[A_TEXT] = n_text + 16;
    bind_view(ix);
    if (!unchecked && ix->has_samples) {
        // every run's first BWT character is the text character in front of its suffix:
        // text[samples_start[k]] == head of run k, for all r runs (one pass over the samples)
        // (whatever fails from here on, an UNCHECKED text must not stay bound to the index)
        auto drop_text = [&] {
            (void)hipFree(ix->text);
            ix->text = nullptr;
            ix->n_text = 0;
            ix->arr_bytes[A_TEXT] = 0;
            bind_view(ix);
        };
        unsigned long long* d_bad = nullptr;
        int rc = SPX_OK;
        if (hipMalloc((void**)&d_bad, 8) != hipSuccess || hipMemset(d_bad, 0, 8) != hipSuccess) {
            set_error("hipMalloc / hipMemset failed while checking the text");
            rc = SPX_E_HIP;
        }
        if (rc == SPX_OK) rc = launch_text_check(ix, d_bad, nullptr);
        unsigned long long bad = 0;
        if (rc == SPX_OK && hipMemcpy(&bad, d_bad, 8, hipMemcpyDeviceToHost) != hipSuccess) {
            set_error("hipMemcpy failed while checking the text");
            rc = SPX_E_HIP;
        }
        if (d_bad) (void)hipFree(d_bad);
        if (rc != SPX_OK) {
            drop_text();
            return rc;
        }
        if (bad) {
            drop_text();
            set_error("text disagrees with the index at %llu of %llu runs (text[samples_start[k]] must be the head "
                      "of run k): not the text this index was built from", bad, (unsigned long long)ix->r);
            return SPX_E_FORMAT;
        }
    }
    return SPX_OK;
}

// A caller's fingerprint of what the index was built from (the host harness: names, sizes and modification times of
// the index files): saved with the flat-layout cache and handed back after spx_index_load_flat, so that a cache left
// over from an index that has since been rebuilt under the same prefix is recognised and not used.
int spx_index_set_source_tag(spx_index* ix, const char* tag) {
    if (!ix || !tag) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> g(ix->mu);
    snprintf(ix->source_tag, sizeof ix->source_tag, "%s", tag);
    return SPX_OK;
}

const char* spx_index_source_tag(const spx_index* ix) { return ix ? ix->source_tag : ""; }

int spx_index_rebuild_text(spx_index* ix) {
    if (!ix) {
        set_error("index is null");
        return SPX_E_ARG;
    }
    if (!ix->has_samples) {
        set_error("the text can only be rebuilt from an index with SA samples (an MS index)");
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    const uint64_t n_text = ix->n - 1;
    if (const int rc_own = own_arrays_alone(ix); rc_own != SPX_OK) return rc_own;
    if (ix->text) (void)hipFree(ix->text);
    ix->text = nullptr;
    ix->n_text = 0;
    ix->arr_bytes[A_TEXT] = 0;
    bind_view(ix);
    uint8_t* d_text = nullptr;
    unsigned long long* d_cnt = nullptr;
    SPX_HIP(hipMalloc((void**)&d_text, n_text + 16));
    SPX_HIP(hipMemset(d_text, 0, n_text + 16));
    SPX_HIP(hipMalloc((void**)&d_cnt, 16));
    SPX_HIP(hipMemset(d_cnt, 0, 16));
    int rc = launch_text_from_index(ix, d_text, n_text, d_cnt, nullptr);
    unsigned long long stuck = 0;
    if (rc == SPX_OK && hipMemcpy(&stuck, d_cnt, 8, hipMemcpyDeviceToHost) != hipSuccess) rc = SPX_E_HIP;
    if (rc == SPX_OK && stuck) {
        set_error("the run structure is not a permutation (%llu LF chains did not end): corrupt index", stuck);
        rc = SPX_E_FORMAT;
    }
    if (rc == SPX_OK) {
        ix->text = d_text;
        ix->n_text = n_text;
        ix->arr_bytes[A_TEXT] = n_text + 16;
        bind_view(ix);
        // (the chains partition the BWT positions of a consistent run structure; the check below confirms the
        // samples' positions, which is what spx_index_set_text checks of a text handed in)
        SPX_HIP(hipMemset(d_cnt, 0, 8));
        rc = launch_text_check(ix, d_cnt, nullptr);
        unsigned long long bad = 0;
        if (rc == SPX_OK && hipMemcpy(&bad, d_cnt, 8, hipMemcpyDeviceToHost) != hipSuccess) rc = SPX_E_HIP;
        if (rc == SPX_OK && bad) {
            set_error("the rebuilt text disagrees with the index at %llu runs: SA samples and run structure do not belong together", bad);
            rc = SPX_E_FORMAT;
        }
    } else {
        (void)hipFree(d_text);
    }
    (void)hipFree(d_cnt);
    return rc;
}

int spx_index_copy_text(spx_index* ix, uint8_t* out, uint64_t capacity, int where, uint64_t* n_text) {
    if (!ix) {
        set_error("index is null");
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> g(ix->mu);
    if (n_text) *n_text = ix->n_text;
    if (!out) return SPX_OK;  // size query
    if (!ix->text || capacity < ix->n_text) {
        set_error(ix->text ? "buffer too small for the text" : "the index has no text");
        return SPX_E_ARG;
    }
    SPX_HIP(hipSetDevice(ix->device));
    SPX_HIP(hipMemcpy(out, ix->text, ix->n_text, where ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return SPX_OK;
}

void* spx_host_alloc(size_t bytes) {
    if (usable_devices() <= 0) {
        set_error("no HIP device visible: libspumoni_gpu has no CPU fallback");
        return nullptr;
    }
    void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) {
        (void)hip_fail(e, "hipHostMalloc", __FILE__, __LINE__);
        return nullptr;
    }
    return p;
}

void spx_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

int spx_host_register(void* p, size_t bytes) {
    if (!p || bytes == 0) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    if (usable_devices() <= 0) {
        set_error("no HIP device visible: libspumoni_gpu has no CPU fallback");
        return SPX_E_NODEVICE;
    }
    const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterPortable);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return hip_fail(e, "hipHostRegister", __FILE__, __LINE__);
    }
    return SPX_OK;
}

int spx_host_unregister(void* p) {
    if (!p) return SPX_OK;
    const hipError_t e = hipHostUnregister(p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return hip_fail(e, "hipHostUnregister", __FILE__, __LINE__);
    }
    return SPX_OK;
}

int spx_set_option(spx_index* ix, const char* key, int64_t value) {
    if (!ix || !key) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> g(ix->mu);
    if (!strcmp(key, "blocking_sync")) {  // 1: spx_query_text_begin / _fetch sleep while they wait for the device (several
        ix->blocking_sync = value != 0;    // query contexts of one process: a core per spinning waiter is a core less for the host's work)
        return SPX_OK;
    }
    if (!strcmp(key, "waves_per_cu")) {
        ix->waves_per_cu = (int)value;
        return SPX_OK;
    }
    if (!strcmp(key, "lanes_per_wave")) {
        ix->force_lanes_per_wave = (int)value;
        return SPX_OK;
    }
    if (!strcmp(key, "chunk_mode")) {  // long-read chunking: 0 automatic, 1 never, 2 always
        ix->chunk_mode = (int)value;
        return SPX_OK;
    }
    if (!strcmp(key, "chunk_len")) {  // chunk size in characters (0 = automatic)
        ix->chunk_len = (int)value;
        return SPX_OK;
    }
    if (!strcmp(key, "chunk_shift")) {  // log2 of the chunk size (0 = automatic)
        ix->chunk_shift = (int)value;
        return SPX_OK;
    }
    if (!strcmp(key, "digest_parked")) {  // 0 automatic, 1 never, 2 whenever the walk can (tests, A/B)
        ix->digest_parked = (int)value;
        return SPX_OK;
    }
    if (!strcmp(key, "digest_kernel")) {
        ix->force_digest_kernel = (int)value;
        return SPX_OK;
    }
    if (!strcmp(key, "cover_switch")) {  // spx_cover.hip: a read of more entries than this takes a wavefront (measurement, tests)
        if (value < 0 || value > 0x7fffffff) {
            set_error("cover_switch must be between 0 and 2^31 - 1");
            return SPX_E_ARG;
        }
        ix->cover.sw = (int)value;
        return SPX_OK;
    }
    if (!strcmp(key, "call_switch")) {  // spx_call.hip: the same for the pileup's add
        if (value < 0 || value > 0x7fffffff) {
            set_error("call_switch must be between 0 and 2^31 - 1");
            return SPX_E_ARG;
        }
        ix->call.sw = (int)value;
        return SPX_OK;
    }
    if (!strcmp(key, "minimizer_charhash")) {
        for (int c = 0; c < 4; ++c) ix->charhash[c] = (uint8_t)((uint64_t)value >> (8 * c));
        return SPX_OK;
    }
    set_error("unknown option '%s'", key);
    return SPX_E_ARG;
}

}  // extern "C"
