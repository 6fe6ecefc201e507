// spx_cache.hip -- the C-ABI's flat-layout cache (.spx) and the replication of an index.
#include <sys/stat.h>
#include <unistd.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "spx_internal.h"

using namespace spx;

extern "C" {

// ---------------------------------------------------------------------------------------------
// flat-layout cache (.spx) and replication: the device arrays of an index as they are
// ---------------------------------------------------------------------------------------------
namespace {

struct SpxFileHeader {
    char magic[8];        // "SPXFLAT\0"
    char layout[56];      // spx_version(): a cache written by another layout is refused
    uint64_t header_bytes;
    uint64_t n, r;
    uint32_t has_samples, has_docs;
    uint64_t n_text;
    uint64_t arr_bytes[spx_index::NARR];
    uint64_t arr_offset[spx_index::NARR];  // file offsets, 4096-aligned
    spx::DevIndex view;   // scalars; the pointers inside are rebound on load
    uint64_t device_bytes;
    char source_tag[128]; // spx_index_set_source_tag(): what the index was built from, as the caller names it
};

constexpr size_t STAGE = 16u << 20;

// file -> device through two page-locked staging buffers (read of chunk i+1 overlaps copy of chunk i)
int read_to_device(FILE* f, uint64_t off, void* dst, uint64_t bytes, void* stage[2], hipStream_t st, hipEvent_t ev[2]) {
    if (fseeko(f, (off_t)off, SEEK_SET) != 0) {
        set_error("seek failed");
        return SPX_E_IO;
    }
    int b = 0;
    for (uint64_t done = 0; done < bytes; b ^= 1) {
        const size_t take = (size_t)std::min<uint64_t>(STAGE, bytes - done);
        SPX_HIP(hipEventSynchronize(ev[b]));  // the copy that last used this buffer
        if (fread(stage[b], 1, take, f) != take) {
            set_error("cache file is truncated");
            return SPX_E_IO;
        }
        SPX_HIP(hipMemcpyAsync((char*)dst + done, stage[b], take, hipMemcpyHostToDevice, st));
        SPX_HIP(hipEventRecord(ev[b], st));
        done += take;
    }
    return SPX_OK;
}

int write_from_device(FILE* f, const void* src, uint64_t bytes, void* stage[2], hipStream_t st, hipEvent_t ev[2]) {
    // device -> host copy of chunk i+1 overlaps the fwrite of chunk i
    uint64_t issued = 0, written = 0;
    size_t len[2] = {0, 0};
    int b = 0;
    auto issue = [&](int buf) -> int {
        len[buf] = (size_t)std::min<uint64_t>(STAGE, bytes - issued);
        SPX_HIP(hipMemcpyAsync(stage[buf], (const char*)src + issued, len[buf], hipMemcpyDeviceToHost, st));
        SPX_HIP(hipEventRecord(ev[buf], st));
        issued += len[buf];
        return SPX_OK;
    };
    if (bytes == 0) return SPX_OK;
    int rc = issue(0);
    if (rc != SPX_OK) return rc;
    while (written < bytes) {
        if (issued < bytes && (rc = issue(b ^ 1)) != SPX_OK) return rc;
        SPX_HIP(hipEventSynchronize(ev[b]));
        if (fwrite(stage[b], 1, len[b], f) != len[b]) {
            set_error("write failed (disk full?)");
            return SPX_E_IO;
        }
        written += len[b];
        b ^= 1;
    }
    return SPX_OK;
}

struct Staging {  // two pinned buffers + a stream + two events, released on scope exit
    void* stage[2] = {nullptr, nullptr};
    hipStream_t st = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    int init() {
        for (int i = 0; i < 2; ++i) {
            SPX_HIP(hipHostMalloc(&stage[i], STAGE, hipHostMallocDefault));
            SPX_HIP(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
        }
        SPX_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        return SPX_OK;
    }
    ~Staging() {
        for (int i = 0; i < 2; ++i) {
            if (stage[i]) (void)hipHostFree(stage[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
        }
        if (st) (void)hipStreamDestroy(st);
    }
};

// One array between a file and the device, in up to IO_THREADS slices: every slice has its own descriptor position,
// staging buffers and stream (a single reader does 6-7 GB/s from tmpfs, PCIe takes several times that).
constexpr int IO_THREADS = 4;
// Page-locked staging is expensive to allocate and more so to release (seconds for a few hundred MB): the pool
// (8 x 16 MB) is made once per process and kept; one save / load at a time uses it.
struct IoPool {
    Staging sg[IO_THREADS];
    bool ready = false;
    std::mutex mu;
    int init() {
        if (ready) return SPX_OK;
        for (auto& g : sg) {
            const int rc = g.init();
            if (rc != SPX_OK) return rc;
        }
        ready = true;
        return SPX_OK;
    }
};
static IoPool& io_pool() {
    static IoPool* p = new IoPool();  // never destroyed: the HIP runtime may be gone by the time statics are
    return *p;
}
int transfer_array(IoPool& pool, const std::string& path, uint64_t off, void* dev, uint64_t bytes, bool to_device,
                   int device) {
    if (bytes == 0) return SPX_OK;
    const int nt = bytes >= (256ull << 20) ? IO_THREADS : 1;
    std::vector<int> rc(nt, SPX_OK);
    std::vector<std::string> msg(nt);
    auto work = [&](int t) {
        const uint64_t lo = (bytes * t / nt) & ~4095ull, hi = t + 1 == nt ? bytes : (bytes * (t + 1) / nt) & ~4095ull;
        auto run = [&]() -> int {
            SPX_HIP(hipSetDevice(device));
            Staging& sg = pool.sg[t];
            int r = SPX_OK;
            FILE* f = fopen(path.c_str(), to_device ? "rb" : "r+b");
            if (!f) {
                set_error("cannot open %s", path.c_str());
                return SPX_E_IO;
            }
            if (to_device) {
                r = read_to_device(f, off + lo, (char*)dev + lo, hi - lo, sg.stage, sg.st, sg.ev);
                if (r == SPX_OK && hipStreamSynchronize(sg.st) != hipSuccess) r = SPX_E_HIP;
            } else {
                r = fseeko(f, (off_t)(off + lo), SEEK_SET) == 0 ? SPX_OK : SPX_E_IO;
                if (r == SPX_OK) r = write_from_device(f, (const char*)dev + lo, hi - lo, sg.stage, sg.st, sg.ev);
            }
            if (fclose(f) != 0 && r == SPX_OK && !to_device) {
                set_error("write failed (disk full?)");
                r = SPX_E_IO;
            }
            return r;
        };
        rc[t] = run();
        if (rc[t] != SPX_OK) msg[t] = spx_last_error();  // the error text is thread-local: carry it over
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back(work, t);
    work(0);
    for (auto& x : th) x.join();
    for (int t = 0; t < nt; ++t)
        if (rc[t] != SPX_OK) {
            set_error("%s", msg[t].c_str());
            return rc[t];
        }
    return SPX_OK;
}

}  // namespace

const char* spx_version(void) { return SPX_LAYOUT_VERSION; }

int spx_index_save(spx_index* ix, const char* path) {
    if (!ix || !path) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    std::lock_guard<std::mutex> g(ix->mu);
    SPX_HIP(hipSetDevice(ix->device));
    SPX_HIP(hipDeviceSynchronize());
    SpxFileHeader h;
    memset(&h, 0, sizeof h);
    memcpy(h.magic, "SPXFLAT", 8);
    snprintf(h.layout, sizeof h.layout, "%s", SPX_LAYOUT_VERSION);
    h.header_bytes = sizeof h;
    h.n = ix->n;
    h.r = ix->r;
    h.has_samples = ix->has_samples;
    h.has_docs = ix->has_docs;
    h.n_text = ix->n_text;
    h.view = ix->view;
    {  // the file holds no addresses: the pointers are rebound on load (bind_view)
        spx_index blank;
        blank.view = h.view;
        blank.n_text = ix->n_text;
        bind_view(&blank);
        h.view = blank.view;
    }
    h.device_bytes = ix->device_bytes;
    memcpy(h.source_tag, ix->source_tag, sizeof h.source_tag);
    // the fat table and fat_js are not written: spx_index_load_flat rebuilds them from the other arrays (build_fat)
    uint64_t off = (sizeof h + 4095) & ~4095ull;
    for (int i = 0; i < spx_index::NARR; ++i) {
        const bool skip = i == A_FAT || i == A_FATJ;
        h.arr_bytes[i] = ix->arr_bytes[i];
        h.arr_offset[i] = skip ? 0 : off;
        if (!skip) off = (off + ix->arr_bytes[i] + 4095) & ~4095ull;
    }
    const std::string tmp = std::string(path) + ".tmp";
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) {
        set_error("cannot create %s", tmp.c_str());
        return SPX_E_IO;
    }
    IoPool& pool = io_pool();
    std::lock_guard<std::mutex> pg(pool.mu);
    int rc = pool.init();
    if (rc == SPX_OK && (fwrite(&h, sizeof h, 1, f) != 1 || ftruncate(fileno(f), (off_t)off) != 0)) {
        set_error("write failed");
        rc = SPX_E_IO;
    }
    if (fclose(f) != 0 && rc == SPX_OK) {
        set_error("write failed (disk full?)");
        rc = SPX_E_IO;
    }
    void** arr[spx_index::NARR];
    index_arrays(ix, arr);
    for (int i = 0; i < spx_index::NARR && rc == SPX_OK; ++i)
        if (h.arr_offset[i]) rc = transfer_array(pool, tmp, h.arr_offset[i], *arr[i], h.arr_bytes[i], false, ix->device);
    if (rc == SPX_OK && rename(tmp.c_str(), path) != 0) {
        set_error("cannot rename %s to %s", tmp.c_str(), path);
        rc = SPX_E_IO;
    }
    if (rc != SPX_OK) remove(tmp.c_str());
    return rc;
}

spx_index* spx_index_load_flat(const char* path, int device) {
    if (!path) {
        set_error("path is null");
        return nullptr;
    }
    if (select_device(device) != SPX_OK) return nullptr;
    FILE* f = fopen(path, "rb");
    if (!f) {
        set_error("cannot open %s", path);
        return nullptr;
    }
    SpxFileHeader h;
    if (fread(&h, sizeof h, 1, f) != 1 || memcmp(h.magic, "SPXFLAT", 8) != 0 || h.header_bytes != sizeof h) {
        set_error("%s is not a flat-layout cache of this library", path);
        fclose(f);
        return nullptr;
    }
    h.layout[sizeof h.layout - 1] = 0;
    if (strcmp(h.layout, SPX_LAYOUT_VERSION) != 0) {
        set_error("%s was written by layout '%s', this library is '%s': rebuild the cache", path, h.layout,
                  SPX_LAYOUT_VERSION);
        fclose(f);
        return nullptr;
    }
    {   // the header's fields against each other and against the file: a damaged cache must not size device
        // arrays the kernels then run past
        struct stat stf;
        const uint64_t fsize = fstat(fileno(f), &stf) == 0 ? (uint64_t)stf.st_size : 0;
        const uint64_t r = h.view.r;  // runs of the flat layout (pieces of long runs count); h.r is the file's r
        const uint64_t row_bytes = h.view.compact ? sizeof(spx::Row32) : sizeof(spx::Row);
        const bool aux = h.has_samples || h.has_docs;
        uint64_t want[spx_index::NARR] = {};
        want[A_ROWS] = (r + ROW_PAD) * row_bytes;
        want[A_DIRROWS] = (r + ROW_PAD) * sizeof(spx::JumpRow);
        want[A_FAT] = (h.view.nfat + 2) * (uint64_t)h.view.fat_stride;
        want[A_FATJ] = spx::fatjs_count(h.view.nfat) * 4 + 64;
        want[A_Q] = (r + 1 + Q_PAD) * 4;
        want[A_AUX] = aux ? (r + 2) * sizeof(spx::Aux) : 0;
        want[A_SSRUN] = h.has_samples ? (r + 4) * 8 : 0;
        want[A_RUNDOCS] = h.has_docs ? (r + ROW_PAD) * 4 : 0;
        want[A_LETTERS] = 256 * sizeof(spx::LetterInfo);
        want[A_TEXT] = h.n_text ? h.n_text + 16 : 0;
        bool ok = r > 0 && r < 0xfffffff0ull && h.r > 0 && h.r <= r && h.n > 0 && h.view.n == h.n &&
                  (h.view.fat_stride == 32u || (!aux && h.view.fat_stride == 16u)) && (h.view.fat_stride == 16u || aux || h.view.compact) &&
                  (h.n_text == 0 || h.n_text + 1 == h.n || h.n_text < h.n);
        for (int i = 0; ok && i < spx_index::NARR; ++i) {
            ok = h.arr_bytes[i] == want[i];
            const bool stored = i != A_FAT && i != A_FATJ && h.arr_bytes[i] != 0;
            if (ok && stored) ok = h.arr_offset[i] >= sizeof h && h.arr_offset[i] + h.arr_bytes[i] <= fsize;
        }
        if (!ok) {
            set_error("%s: the header does not describe a consistent index (array sizes / offsets against r = %llu and the "
                      "file's %llu bytes): rebuild the cache", path, (unsigned long long)r, (unsigned long long)fsize);
            fclose(f);
            return nullptr;
        }
    }
    spx_index* ix = new spx_index();
    ix->device = device;
    h.source_tag[sizeof h.source_tag - 1] = 0;
    memcpy(ix->source_tag, h.source_tag, sizeof ix->source_tag);
    ix->n = h.n;
    ix->r = h.r;
    ix->has_samples = h.has_samples != 0;
    ix->has_docs = h.has_docs != 0;
    ix->n_text = h.n_text;
    ix->view = h.view;
    ix->device_bytes = h.device_bytes;
    const bool timing = getenv("SPX_TIMING") != nullptr;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    auto body = [&]() -> int {
        double t0 = now();
        IoPool& pool = io_pool();
        std::lock_guard<std::mutex> pg(pool.mu);
        int rc = pool.init();
        if (rc != SPX_OK) return rc;
        if (timing) fprintf(stderr, "[spx] load_flat: staging pool %.3f s\n", now() - t0);
        void** arr[spx_index::NARR];
        index_arrays(ix, arr);
        for (int i = 0; i < spx_index::NARR; ++i) {
            ix->arr_bytes[i] = h.arr_bytes[i];
            if (h.arr_bytes[i] == 0 || h.arr_offset[i] == 0) continue;  // absent, or rebuilt below
            SPX_HIP(hipMalloc(arr[i], h.arr_bytes[i]));
            t0 = now();
            if ((rc = transfer_array(pool, path, h.arr_offset[i], *arr[i], h.arr_bytes[i], true, device)) != SPX_OK) return rc;
            if (timing) fprintf(stderr, "[spx] load_flat: array %d, %.2f GB in %.3f s\n", i, h.arr_bytes[i] / 1e9, now() - t0);
        }
        bind_view(ix);
        t0 = now();
        if ((rc = build_fat(ix)) != SPX_OK) return rc;
        if (timing) fprintf(stderr, "[spx] load_flat: fat table rebuilt in %.3f s\n", now() - t0);
        return init_runtime(ix);
    };
    const int rc = body();
    fclose(f);
    if (rc != SPX_OK) {
        spx_index_free(ix);
        return nullptr;
    }
    return ix;
}

spx_index* spx_index_clone(spx_index* src, int device) {
    if (!src) {
        set_error("index is null");
        return nullptr;
    }
    if (select_device(device) != SPX_OK) return nullptr;
    spx_index* ix = new spx_index();
    ix->device = device;
    auto body = [&]() -> int {
        std::lock_guard<std::mutex> g(src->mu);
        ix->n = src->n;
        ix->r = src->r;
        ix->has_samples = src->has_samples;
        ix->has_docs = src->has_docs;
        ix->n_text = src->n_text;
        ix->view = src->view;
        ix->device_bytes = src->device_bytes;
        if (device != src->device) {  // xGMI peer copies when the devices can reach each other
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, device, src->device) == hipSuccess && can)
                (void)hipDeviceEnablePeerAccess(src->device, 0);
            (void)hipGetLastError();  // "already enabled" is fine
        }
        void** from[spx_index::NARR];
        void** to[spx_index::NARR];
        index_arrays(src, from);
        index_arrays(ix, to);
        if (device == src->device) {
            // the same device: a second query context over the same arrays (nothing is copied; the arrays are read-only
            // once built and go when the last handle is freed) -- what lets two host threads keep one device's copy engines
            // and compute units busy at the same time without a second 200 GB replica
            if (!src->owner) {
                src->owner = std::make_shared<ArrayOwner>();
                src->owner->device = src->device;
                for (int i = 0; i < spx_index::NARR; ++i) src->owner->p[i] = *from[i];
            }
            ix->owner = src->owner;
            for (int i = 0; i < spx_index::NARR; ++i) {
                ix->arr_bytes[i] = src->arr_bytes[i];
                *to[i] = *from[i];
            }
        } else {
            for (int i = 0; i < spx_index::NARR; ++i) {
                ix->arr_bytes[i] = src->arr_bytes[i];
                if (src->arr_bytes[i] == 0) continue;
                SPX_HIP(hipMalloc(to[i], src->arr_bytes[i]));
                SPX_HIP(hipMemcpyPeerAsync(*to[i], device, *from[i], src->device, src->arr_bytes[i], nullptr));
            }
            SPX_HIP(hipDeviceSynchronize());
        }
        bind_view(ix);
        const int rc = init_runtime(ix);
        memcpy(ix->charhash, src->charhash, sizeof ix->charhash);
        memcpy(ix->source_tag, src->source_tag, sizeof ix->source_tag);
        ix->waves_per_cu = src->waves_per_cu;
        ix->chunk_mode = src->chunk_mode;
        ix->chunk_shift = src->chunk_shift;
        ix->chunk_len = src->chunk_len;
        ix->force_lanes_per_wave = src->force_lanes_per_wave;
        ix->force_digest_kernel = src->force_digest_kernel;
        ix->digest_parked = src->digest_parked;
        if (rc != SPX_OK) return rc;
        return clone_map(src, ix);  // (the sequence table is the handle's own, not one of the shared arrays)
    };
    if (body() != SPX_OK) {
        spx_index_free(ix);
        return nullptr;
    }
    return ix;
}

int spx_index_describe(const spx_index* ix, char* buf, size_t cap) {
    if (!ix || !buf || cap == 0) {
        set_error("null argument");
        return SPX_E_ARG;
    }
    const DevIndex& v = ix->view;
    // (SPX_DESCRIBE_ADDRESSES: also where the three big arrays lie -- tools/c5_regimes.py; not part of the description proper,
    // which is equal for an index and its copy)
    char where[160] = "";
    if (getenv("SPX_DESCRIBE_ADDRESSES"))
        snprintf(where, sizeof where, ", \"rows_at\": \"%p\", \"dirrows_at\": \"%p\", \"fat_at\": \"%p\"", (void*)ix->rows, (void*)ix->dirrows, (void*)ix->fat);
    snprintf(buf, cap,
             "{\"layout\": \"%s\", \"n\": %llu, \"r\": %llu, \"flat_runs\": %u, \"letters\": %u, \"compact_rows\": %u, "
             "\"fat_slots\": %llu, \"fat_slots_per_run\": %.4f, \"fat_stride\": %u, \"has_samples\": %d, "
             "\"has_docs\": %d, \"n_text\": %llu, \"device_bytes\": %llu%s}",
             SPX_LAYOUT_VERSION, (unsigned long long)ix->n, (unsigned long long)ix->r, v.r, v.nletters, v.compact,
             (unsigned long long)v.nfat, (double)v.nfat / (double)(v.r ? v.r : 1), v.fat_stride,
             (int)ix->has_samples, (int)ix->has_docs, (unsigned long long)ix->n_text,
             (unsigned long long)(ix->device_bytes + ix->n_text), where);
    return SPX_OK;
}

}  // extern "C"
