// build_main.cpp -- `spumoni build` on MI355X: the reference's command line (src/spumoni.cpp:62-160), option
// validation (include/spumoni_main.hpp:161-225) and log lines (src/spumoni.cpp:555-731), over the device text
// preparation (include/spumoni_reftext.h) and the device index builder (include/spumoni_build.h).  The files it
// writes are byte for byte those of `python -m spumoni_amd.build_index` with the mapped options (-i = -l, -t = -a,
// -c = --no-rev-comp, -d = --doc), except:
//   - the complement is the reference's seqtk table (IUPAC codes accepted; build_index refuses them);
//   - a single -r file with -d takes its document lengths from an existing <prefix>.fa.fdi, as the reference does.
// Not supported here: -g (general text).  -k is accepted and does nothing (the raw files are the index and are always
// kept); -p is accepted and has no effect (there is no PFP).
//
// The binary must also load against libraries without the builder (a CPU test double of the query boundary): the
// spb_* / spr_* entry points are looked up at run time, never linked.
#include <dlfcn.h>
#include <getopt.h>
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <set>
#include <string>
#include <vector>

#include "../../../include/spumoni_build.h"
#include "../../../include/spumoni_gpu.h"
#include "../../../include/spumoni_reftext.h"
#include "read_command.hpp"
#include "reads.hpp"

using namespace spumoni_host;

#define FORCE_LOG(func, ...)                                \
    do {                                                    \
        std::fprintf(stderr, "\033[32m[%s] \033[0m", func); \
        std::fprintf(stderr, __VA_ARGS__);                  \
        std::fprintf(stderr, "\n");                         \
    } while (0)
#define STATUS_LOG(x, ...)                                  \
    do {                                                    \
        std::fprintf(stderr, "\033[32m[%s] \033[0m", x);    \
        std::fprintf(stderr, __VA_ARGS__);                  \
        std::fprintf(stderr, " ... ");                      \
    } while (0)
#define DONE_LOG(x)                                               \
    do {                                                          \
        auto sec = std::chrono::duration<double>(x);              \
        std::fprintf(stderr, "done.  (%.3f sec)\n", sec.count()); \
    } while (0)

namespace {

constexpr size_t NULL_READ_CHUNK = 150, NUM_NULL_READS = 800, NULL_READ_BOUND = 1000;  // spumoni_main.hpp:65-67

bool is_dir(const std::string& p) {
    struct stat st;
    return ::stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}
bool fasta_name(const std::string& p) {  // the reference's extensions, gzip-compressed or not
    const std::string q = ends_with(p, ".gz") ? p.substr(0, p.size() - 3) : p;
    return ends_with(q, ".fa") || ends_with(q, ".fasta") || ends_with(q, ".fna");
}
std::string parent_path(const std::string& p) {
    const size_t s = p.rfind('/');
    return s == std::string::npos ? std::string() : (s == 0 ? std::string("/") : p.substr(0, s));
}

int spumoni_build_usage() {
    std::fprintf(stderr, "spumoni build - builds the ms/pml index for a specified reference file.\n");
    std::fprintf(stderr, "Usage: spumoni build [options]\n");
    std::fprintf(stderr, "Options:\n");
    std::fprintf(stderr, "\tGeneral options:\n");
    std::fprintf(stderr, "\t%-35sprints this usage message\n", "-h, --help");
    std::fprintf(stderr, "\t%-35sturn on verbose logging\n\n", "-v, --verbose");
    std::fprintf(stderr, "\tInput data options:\n");
    std::fprintf(stderr, "\t%-25s%-10spath to reference file to be indexed (default: FASTA)\n", "-r, --ref", "[FILE]");
    std::fprintf(stderr, "\t%-25s%-10sfile with a list of FASTA files to index\n", "-i, --filelist", "[FILE]");
    std::fprintf(stderr, "\t%-25s%-10suse with -r option if input file is general text (default: false)\n",
                 "-g, --general-text", "");
    std::fprintf(stderr, "\t%-25s%-10sdo not add reverse complement, only applies to FASTA (default: true)\n\n",
                 "-c, --no-rev-comp", "");
    std::fprintf(stderr, "\tMinimizer options:\n");
    std::fprintf(stderr, "\t%-25s%-10sturn off minimizer digestion of sequence (default: on)\n", "-n, --no-digest", "");
    std::fprintf(stderr, "\t%-25s%-10suse alphabet-promoted minimizers\n", "-m, --minimizer-alphabet", "");
    std::fprintf(stderr, "\t%-25s%-10suse DNA-letter based minimizers\n", "-t, --dna-minimizer", "");
    std::fprintf(stderr, "\t%-25s%-10ssmall window size (k) for finding minimizers (default: 4)\n", "-K, --small-window",
                 "[INT]");
    std::fprintf(stderr, "\t%-25s%-10slarge window size (w) for finding minimizers (default: 11)\n\n",
                 "-W, --large-window", "[INT]");
    std::fprintf(stderr, "\tIndex file(s) options:\n");
    std::fprintf(stderr, "\t%-25s%-10soutput prefix for index file(s)\n", "-o, --prefix", "[PATH]");
    std::fprintf(stderr, "\t%-25s%-10sbuild an index that can be used to compute MSs\n", "-M, --MS", "");
    std::fprintf(stderr, "\t%-25s%-10sbuild an index that can be used to compute PMLs\n", "-P, --PML", "");
    std::fprintf(stderr, "\t%-25s%-10skeep the temporary files (default: false)\n", "-k, --keep", "");
    std::fprintf(stderr, "\t%-25s%-10sbuild the document array (default: false)\n", "-d, --doc-array", "");
    std::fprintf(stderr, "\t%-25s%-10swrite the sequence table <prefix>.fa.seqs that `spumoni map` needs: name, length,\n"
                         "\t%-35stext start and strands per sequence; only with -n (default: false)\n", "-s, --seq-table", "", "");
    std::fprintf(stderr, "\t%-25s%-10ssize of windows in bp for classification (default: 150)\n\n", "-w, --window",
                 "[INT]");
    std::fprintf(stderr, "\tPFP-related options:\n");
    std::fprintf(stderr, "\t%-25s%-10shash-modulus used for PFP (default: 100)\n\n", "-p, --hash-mod", "[INT]");
    return 0;
}

struct BuildOptions {  // SpumoniBuildOptions (include/spumoni_main.hpp:130-225)
    std::string output_prefix, ref_file, input_list, output_dir;
    size_t hash_mod = 100;
    bool keep_files = false, ms_index = false, pml_index = false, verbose = false, is_fasta = false;
    bool build_doc = false, use_minimizers = true, use_promotions = false, use_dna_letters = false;
    bool is_general_text = false, use_rev_comp = true, seq_table = false;
    size_t k = 4, w = 11, bin_size = 150;

    void validate() {
        if (is_general_text) is_fasta = false;
        if (ref_file.length()) {
            if (!is_file(ref_file)) fatal_error("The following path is not valid: %s", ref_file.data());
            if (output_dir.length()) fatal_error("The -b option should not be set when using a single file.");
            if (is_fasta && !fasta_name(ref_file))
                fatal_error("The reference file provided does not appear to be a FASTA\n"
                            "       file, please convert to FASTA and re-run.");
        } else {
            if (!is_file(input_list)) fatal_error("The following path is not valid: %s", input_list.data());
        }
        if (build_doc && ref_file.length() && !is_file(output_prefix + std::string(".fa.fdi"))) {
            fatal_error("Cannot build a document array if you are indexing a single\n"
                        " file. If so, you need to provide a *.fdi file for that file.");
        } else if (build_doc && ref_file.length() && is_file(output_prefix + std::string(".fa.fdi"))) {
            std::fprintf(stderr, "\n\033[33mWarning: \033[0m");
            std::fprintf(stderr, "proceeding with document array construction, make sure your *.fdi is correct. \U0001F64F");
            std::fprintf(stderr, "\n\n");
        }
        if (use_minimizers) {
            if (use_promotions && use_dna_letters) fatal_error("Only one type of minimizer can be specified.");
            if (!use_promotions && !use_dna_letters) fatal_error("A minimizer type must be specified.");
        } else {
            if (use_promotions || use_dna_letters)
                fatal_error("A minimizer type should not be specified if intending not to use minimizer digestion.");
        }
        if (is_general_text) {
            if (use_promotions || use_dna_letters)
                fatal_error("No minimizer type should be chosen when using general text input.");
        }
        if (!output_prefix.length()) fatal_error("Need to specify an output prefix for the index files.");
        if (!ms_index && !pml_index) fatal_error("At least one index type (-M or -P) must be specified for build.");
        if (k > 4) fatal_warning("small window size (k) cannot be larger than 4 characters.");
        if (w < k) fatal_warning("large window size (w) should be larger than the small window size (k)");
        if (bin_size < 50 || bin_size > 400)
            fatal_warning("the bin size provided is not optimal, re-run using a value between 50 and 400.");
    }
};

void parse_build_options(int argc, char** argv, BuildOptions* opts) {
    static struct option long_options[] = {{"help", no_argument, NULL, 'h'},
                                           {"prefix", required_argument, NULL, 'o'},
                                           {"verbose", no_argument, NULL, 'v'},
                                           {"ref", required_argument, NULL, 'r'},
                                           {"filelist", required_argument, NULL, 'i'},
                                           {"build-dir", required_argument, NULL, 'b'},
                                           {"general-text", no_argument, NULL, 'g'},
                                           {"no-rev-comp", no_argument, NULL, 'c'},
                                           {"no-digest", no_argument, NULL, 'n'},
                                           {"minimizer-alphabet", no_argument, NULL, 'm'},
                                           {"dna-minimizer", no_argument, NULL, 't'},
                                           {"small-window", required_argument, NULL, 'K'},
                                           {"large-window", required_argument, NULL, 'W'},
                                           {"MS", no_argument, NULL, 'M'},
                                           {"PML", no_argument, NULL, 'P'},
                                           {"keep", no_argument, NULL, 'k'},
                                           {"doc-array", no_argument, NULL, 'd'},
                                           {"seq-table", no_argument, NULL, 's'},
                                           {"window", required_argument, NULL, 'w'},
                                           {"hash-mod", required_argument, NULL, 'p'},
                                           {0, 0, 0, 0}};
    int long_index = 0;
    for (int c; (c = getopt_long(argc, argv, "ho:r:MPw:kdi:b:nvmK:W:tgcp:s", long_options, &long_index)) >= 0;) {
        switch (c) {
            case 'h': spumoni_build_usage(); std::exit(1);
            case 'o': opts->output_prefix.assign(optarg); break;
            case 'r': opts->ref_file.assign(optarg); break;
            case 'i': opts->input_list.assign(optarg); break;
            case 'b': opts->output_dir.assign(optarg); break;
            case 'c': opts->use_rev_comp = false; break;
            case 'M': opts->ms_index = true; break;
            case 'P': opts->pml_index = true; break;
            case 'v': opts->verbose = true; break;
            case 'n': opts->use_minimizers = false; opts->is_fasta = true; break;
            case 'm': opts->use_promotions = true; break;
            case 't': opts->use_dna_letters = true; opts->is_fasta = true; break;
            case 'g': opts->is_general_text = true; opts->is_fasta = false; break;
            case 'K': opts->k = std::max(std::atoi(optarg), 1); break;
            case 'W': opts->w = std::max(std::atoi(optarg), 1); break;
            case 'w': opts->bin_size = std::max(std::atoi(optarg), 1); break;
            case 'p': opts->hash_mod = std::max(std::atoi(optarg), 1); break;
            case 'k': opts->keep_files = true; break;
            case 'd': opts->build_doc = true; break;
            case 's': opts->seq_table = true; break;
            default: spumoni_build_usage(); std::exit(1);
        }
    }
}

// ---- the device entry points, resolved at run time ------------------------------------------------------------------
struct DeviceBuilder {
    decltype(&spr_text_from_fasta) text_from_fasta;
    decltype(&spr_text_stats) text_stats;
    decltype(&spr_text_copy) text_copy;
    decltype(&spr_text_free) text_free;
    decltype(&spr_text_names) text_names = nullptr;  // -s alone asks for it
    decltype(&spb_build_from_text) build_from_text;
    decltype(&spb_build_stats) build_stats;
    decltype(&spb_build_copy) build_copy;
    decltype(&spb_build_free) build_free;
};
template <class F>
void resolve(F& fn, const char* name) {
    fn = reinterpret_cast<F>(dlsym(RTLD_DEFAULT, name));
    if (!fn)
        fatal_error("the loaded libspumoni_gpu.so has no %s: `spumoni build` needs the device index builder and text "
                    "preparation, and there is no CPU fallback.",
                    name);
}
DeviceBuilder resolve_builder() {
    DeviceBuilder d;
    resolve(d.text_from_fasta, "spr_text_from_fasta");
    resolve(d.text_stats, "spr_text_stats");
    resolve(d.text_copy, "spr_text_copy");
    resolve(d.text_free, "spr_text_free");
    resolve(d.build_from_text, "spb_build_from_text");
    resolve(d.build_stats, "spb_build_stats");
    resolve(d.build_copy, "spb_build_copy");
    resolve(d.build_free, "spb_build_free");
    return d;
}

// ---- input files: plain, or gzip inflated with the system's zlib (loaded at run time) -----------------------------
struct Zlib {
    void* (*gzopen)(const char*, const char*) = nullptr;
    int (*gzread)(void*, void*, unsigned) = nullptr;
    int (*gzclose)(void*) = nullptr;
    bool load() {
        if (gzopen) return true;
        void* h = dlopen("libz.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) return false;
        gzopen = reinterpret_cast<void* (*)(const char*, const char*)>(dlsym(h, "gzopen"));
        gzread = reinterpret_cast<int (*)(void*, void*, unsigned)>(dlsym(h, "gzread"));
        gzclose = reinterpret_cast<int (*)(void*)>(dlsym(h, "gzclose"));
        return gzopen && gzread && gzclose;
    }
};

bool is_gzip(const std::string& path) {
    unsigned char m[2] = {0, 0};
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    const size_t got = std::fread(m, 1, 2, f);
    std::fclose(f);
    return got == 2 && m[0] == 0x1f && m[1] == 0x8b;
}

std::vector<uint8_t> inflate_file(const std::string& path) {
    static Zlib z;
    if (!z.load())
        fatal_error("%s is gzip-compressed and zlib (libz.so.1) could not be loaded: decompress it and re-run.",
                    path.c_str());
    void* g = z.gzopen(path.c_str(), "rb");
    if (!g) fatal_error("cannot open %s", path.c_str());
    std::vector<uint8_t> out;
    std::vector<uint8_t> buf(1 << 22);
    for (;;) {
        const int got = z.gzread(g, buf.data(), (unsigned)buf.size());
        if (got < 0) fatal_error("%s: gzip stream is corrupt", path.c_str());
        if (got == 0) break;
        out.insert(out.end(), buf.begin(), buf.begin() + got);
    }
    z.gzclose(g);
    return out;
}

struct HostBytes {  // page-locked when the library can, else plain
    uint8_t* p = nullptr;
    bool pinned = false;
    explicit HostBytes(size_t n) {
        p = static_cast<uint8_t*>(spx_host_alloc(n ? n : 1));
        pinned = p != nullptr;
        if (!p) p = static_cast<uint8_t*>(std::malloc(n ? n : 1));
        if (!p) fatal_error("out of host memory (%zu bytes for the input files)", n);
    }
    ~HostBytes() {
        if (pinned) spx_host_free(p);
        else std::free(p);
    }
};

// ---- null reads, KS statistics (spumoni_amd/build_index.py) ---------------------------------------------------------
struct GlibcRand {  // rand() of glibc after srand(seed): TYPE_3, r[i] = r[i-3] + r[i-31], 310 values discarded
    uint32_t r[34];
    int head = 0;  // r[head] is the oldest of the last 34 values
    explicit GlibcRand(uint32_t seed) {
        if (seed == 0) seed = 1;
        std::vector<uint32_t> v{seed};
        for (int i = 1; i < 31; ++i) {
            const int32_t word = (int32_t)v.back();
            const int32_t hi = word / 127773;
            const int32_t lo = word - hi * 127773;
            int64_t x = 16807ll * lo - 2836ll * hi;
            if (x < 0) x += 2147483647;
            v.push_back((uint32_t)x);
        }
        for (int i = 0; i < 3; ++i) v.push_back(v[i]);
        for (int i = 0; i < 34; ++i) r[i] = v[i];
        for (int i = 0; i < 310; ++i) next();
    }
    uint32_t next() {  // append r[-31] + r[-3], drop the oldest
        const uint32_t a = r[(head + 3) % 34], b = r[(head + 31) % 34];
        const uint32_t x = a + b;
        r[head] = x;
        head = (head + 1) % 34;
        return x;
    }
    uint32_t rand() { return next() >> 1; }
};

using Piece = std::pair<const uint8_t*, size_t>;

std::vector<Piece> null_reads_from_list(const std::vector<Piece>& seqs, GlibcRand& rng) {
    std::vector<Piece> reads;
    for (const Piece& s : seqs) {
        const size_t grab = reads.size() >= NUM_NULL_READS ? 25 : 100;
        bool go = reads.size() < NULL_READ_BOUND;
        for (size_t i = 0; i < grab && go && s.second > NULL_READ_CHUNK; ++i) {
            const size_t at = rng.rand() % (s.second - NULL_READ_CHUNK);
            reads.push_back({s.first + at, NULL_READ_CHUNK});
            go = reads.size() < NULL_READ_BOUND;
        }
        if (s.second <= NULL_READ_CHUNK) reads.push_back(s);
    }
    return reads;
}

std::vector<Piece> null_reads_from_fasta(const std::vector<Piece>& seqs, GlibcRand& rng) {
    std::vector<Piece> reads;
    bool go = true;
    for (const Piece& s : seqs) {
        if (!go) break;
        const size_t grab = reads.size() >= NUM_NULL_READS ? 25 : 100;
        for (size_t i = 0; i < grab && go && s.second > NULL_READ_CHUNK; ++i) {
            const size_t at = rng.rand() % (s.second - NULL_READ_CHUNK);
            if (!std::memchr(s.first + at, 'N', NULL_READ_CHUNK)) {
                reads.push_back({s.first + at, NULL_READ_CHUNK});
                go = reads.size() < NULL_READ_BOUND;
            }
        }
        if (s.second <= NULL_READ_CHUNK) reads.push_back(s);
    }
    return reads;
}

double ks_statistic(const uint64_t* pos, size_t npos, const uint64_t* nul, size_t nnul) {
    uint64_t top = 0;
    for (size_t i = 0; i < npos; ++i) top = std::max(top, pos[i]);
    for (size_t i = 0; i < nnul; ++i) top = std::max(top, nul[i]);
    std::vector<uint64_t> cp(top + 1, 0), cn(top + 1, 0);
    for (size_t i = 0; i < npos; ++i) cp[pos[i]]++;
    for (size_t i = 0; i < nnul; ++i) cn[nul[i]]++;
    double best = -INFINITY;
    uint64_t sp = 0, sn = 0;
    for (uint64_t v = 0; v <= top; ++v) {
        sp += cp[v];
        sn += cn[v];
        const double pc = (double)sp / ((double)npos + 0.0), nc = (double)sn / ((double)nnul + 0.0);
        best = std::max(best, nc - pc);
        if (pc >= 1.0 || nc >= 1.0) break;
    }
    return std::max(0.0, best);
}

void run_kstest(const uint64_t* lengths, size_t n, const std::vector<uint64_t>& null_stats, size_t bin,
                GlibcRand& rng, std::vector<double>& out) {
    const size_t nv = null_stats.size();
    if (nv == 2 * bin)
        fatal_error("the null database holds exactly two windows of statistics (%zu values for -w %zu): the reference "
                    "divides by zero here; re-run with another -w.",
                    nv, bin);
    size_t start = 0;
    while (start < n) {
        const uint32_t draw = rng.rand();
        const size_t null_pos = nv < 2 * bin ? 0 : draw % (nv - 2 * bin);
        size_t end;
        if (n < bin) end = n;
        else end = start + bin <= n - bin ? start + bin : n;
        const size_t region = end - start;
        const size_t stop = std::min(nv, null_pos + region);
        out.push_back(ks_statistic(lengths + start, region, null_stats.data() + null_pos, stop - null_pos));
        start += region;
    }
}

int width_of(const std::vector<uint64_t>& vals) {  // _width
    uint64_t mx = 0;
    for (uint64_t v : vals) mx = std::max(mx, v);
    return mx > 0 ? std::max((int)std::ceil(std::log2((double)mx)), 1) : 1;
}

double percentile_value(const std::vector<uint64_t>& stats) {
    std::map<uint64_t, uint64_t> cnt;
    for (uint64_t v : stats) cnt[v]++;
    double best = 0.0;
    bool any = false;
    for (const auto& kv : cnt)
        if (kv.second >= 5) {
            best = (double)kv.first;
            any = true;
        }
    return any ? best : 0.0;
}

void put(std::string& b, const void* p, size_t n) { b.append(static_cast<const char*>(p), n); }

void append_int_vector(std::string& b, const std::vector<uint64_t>& vals, int width) {  // _int_vector
    const uint64_t bits = (uint64_t)vals.size() * width;
    const uint8_t w8 = (uint8_t)width;
    put(b, &bits, 8);
    put(b, &w8, 1);
    std::vector<uint64_t> words((bits + 63) / 64, 0);
    const uint64_t mask = width >= 64 ? ~0ull : ((1ull << width) - 1);
    for (size_t i = 0; i < vals.size(); ++i) {
        const uint64_t v = vals[i] & mask, bit = (uint64_t)i * width;
        const uint64_t wi = bit >> 6, sh = bit & 63;
        words[wi] |= v << sh;
        if (sh + width > 64) words[wi + 1] |= v >> (64 - sh);
    }
    put(b, words.data(), 8 * words.size());
}

void write_bytes(const std::string& path, const void* p, size_t n) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) fatal_error("cannot write %s", path.c_str());
    if (n && std::fwrite(p, 1, n, f) != n) fatal_error("cannot write %s", path.c_str());
    if (std::fclose(f) != 0) fatal_error("cannot write %s", path.c_str());
}

void write_null_db(const std::string& path, const std::vector<uint64_t>& stats, double ks) {
    std::string b;
    const uint64_t nv = stats.size();
    uint64_t sum = 0;
    for (uint64_t v : stats) sum += v;
    const double mean = nv ? (double)sum / (double)nv : 0.0, pv = percentile_value(stats);
    put(b, &nv, 8);
    put(b, &ks, 8);
    put(b, &mean, 8);
    put(b, &pv, 8);
    append_int_vector(b, stats, width_of(stats));
    write_bytes(path, b.data(), b.size());
}

void write_five(const std::string& path, const std::vector<uint64_t>& v) {  // 5-byte little-endian records
    std::vector<uint8_t> b(v.size() * 5);
    for (size_t i = 0; i < v.size(); ++i) std::memcpy(&b[5 * i], &v[i], 5);
    write_bytes(path, b.data(), b.size());
}

constexpr uint64_t MAX_TEXT = 0xfffffffeull;  // the index builder's limit: n_text < 2^32 - 1 (32-bit positions)

[[noreturn]] void refuse_long_text(unsigned long long n_text) {
    fatal_error("the text to index has %llu characters: the index builder takes fewer than 2^32 - 1 (4294967295) "
                "(32-bit positions). Digest it with -m (or -t) to make it shorter.",
                n_text);
}

}  // namespace

int build_main(int argc, char** argv) {
    if (argc == 1) {
        spumoni_build_usage();
        return 1;
    }
    BuildOptions opts;
    parse_build_options(argc, argv, &opts);
    if (opts.is_general_text)
        fatal_error("general-text input (-g) is not supported by this build: index FASTA files (-r / -i).");
    if (opts.seq_table && opts.use_minimizers)
        fatal_error("the sequence table (-s) cannot be written for a digested text (-m, -t or the default digestion):\n"
                    "       digested coordinates cannot be turned back into bases. Build with -n.");
    opts.validate();
    if (opts.use_promotions) opts.use_dna_letters = false;
    const int digest_kind = !opts.use_minimizers ? 0 : opts.use_promotions ? SPX_DIGEST_PROMOTED : SPX_DIGEST_DNA;

    const std::string prefix_dir = parent_path(opts.output_prefix);
    if (!is_dir(prefix_dir))
        fatal_error("Output prefix path is not valid. If you would like store index in current directory, use './' "
                    "prior to name.");
    const std::string prefix = opts.output_prefix + (opts.use_promotions ? ".bin" : ".fa");  // src/spumoni.cpp:744-747
    const std::string null_read_file = prefix_dir + "/spumoni_null_reads.fa";

    // everything the build needs of the library, before any file is written
    DeviceBuilder dev = resolve_builder();
    if (opts.seq_table) resolve(dev.text_names, "spr_text_names");
    if (spx_device_count() <= 0)
        fatal_error("no usable gfx950 device: `spumoni build` runs on the GPU and has no CPU fallback.");
    int device = 0;
    if (const char* g = std::getenv("SPUMONI_GPUS")) device = std::atoi(g);

    // the input files: "<path> [<document id>]" per line of the list (src/refbuilder.cpp:52-70)
    std::vector<std::string> files;
    std::vector<long> doc_ids;
    if (opts.ref_file.length()) {
        files.push_back(opts.ref_file);
    } else {
        std::ifstream in(opts.input_list);
        std::string line;
        while (std::getline(in, line)) {
            std::istringstream ss(line);
            std::string path, id;
            if (!(ss >> path)) continue;
            if (!is_file(path)) fatal_error("The following path in the input list is not valid: %s", path.data());
            if (!fasta_name(path)) fatal_error("The following input-file is not a FASTA file: %s", path.data());
            files.push_back(path);
            if (opts.build_doc) {
                if (!(ss >> id)) {
                    doc_ids.push_back((long)files.size());
                } else if (id.empty() || id.find_first_not_of("0123456789") != std::string::npos) {
                    fatal_error("A document ID in the file_list is not an integer: %s", id.data());
                } else {
                    doc_ids.push_back(std::atol(id.c_str()));
                }
            }
        }
        if (files.empty()) fatal_error("The file list %s names no file.", opts.input_list.data());
        if (!doc_ids.empty()) {
            if (doc_ids[0] != 1) fatal_error("The first ID in file_list must be 1");
            for (size_t i = 1; i < doc_ids.size(); ++i)
                if (doc_ids[i] != doc_ids[i - 1] && doc_ids[i] != doc_ids[i - 1] + 1)
                    fatal_error("The IDs in the file_list must be staying constant or increasing by 1.");
        }
    }
    if (opts.hash_mod != 100 || opts.verbose)
        FORCE_LOG("build_main", "the PFP hash modulus (-p) has no effect here: the index is built by suffix sorting on "
                                "the device, not by PFP");

    auto total_start = std::chrono::system_clock::now();
    if (!opts.input_list.length())
        FORCE_LOG("build_main", "input: single reference file (%s)\n", opts.ref_file.data());
    else
        FORCE_LOG("build_main", "input: list of files (%s)\n", opts.input_list.data());
    STATUS_LOG("build_main", "reference file is being generated (%s)", prefix.data());
    auto task_start = std::chrono::system_clock::now();

    // read every file into one page-locked buffer
    std::vector<std::vector<uint8_t>> inflated(files.size());
    std::vector<uint64_t> sizes(files.size()), file_ends(files.size());
    uint64_t total = 0;
    for (size_t i = 0; i < files.size(); ++i) {
        if (is_gzip(files[i])) {
            inflated[i] = inflate_file(files[i]);
            sizes[i] = inflated[i].size();
        } else {
            struct stat st;
            if (::stat(files[i].c_str(), &st) != 0) fatal_error("cannot read %s", files[i].c_str());
            sizes[i] = (uint64_t)st.st_size;
        }
        total += sizes[i];
        file_ends[i] = total;
    }
    uint64_t n_text = 0, n_seqs = 0, n_fwd = 0;
    std::vector<uint8_t> text, fwd;
    std::vector<uint64_t> file_len(files.size()), seq_ends;
    std::vector<uint32_t> seq_file;
    std::vector<uint8_t> names;
    std::vector<uint64_t> name_ends;
    {
        HostBytes buf(total);
        for (size_t i = 0; i < files.size(); ++i) {
            uint8_t* dst = buf.p + (file_ends[i] - sizes[i]);
            if (!inflated[i].empty() || sizes[i] == 0) {
                if (sizes[i]) std::memcpy(dst, inflated[i].data(), sizes[i]);
                std::vector<uint8_t>().swap(inflated[i]);
                continue;
            }
            FILE* f = std::fopen(files[i].c_str(), "rb");
            if (!f || std::fread(dst, 1, sizes[i], f) != sizes[i]) fatal_error("cannot read %s", files[i].c_str());
            std::fclose(f);
        }
        spr_text* t = dev.text_from_fasta(buf.p, total, file_ends.data(), (uint32_t)files.size(),
                                          opts.use_rev_comp ? 1 : 0, digest_kind, (uint32_t)opts.k, (uint32_t)opts.w,
                                          MAX_TEXT, device);
        if (!t) {
            const char* e = spx_last_error();
            unsigned long long long_text = 0;
            if (std::sscanf(e, "the text has %llu characters", &long_text) == 1) refuse_long_text(long_text);
            unsigned fi = 0;
            if (std::sscanf(e, "file #%u", &fi) == 1 && fi < files.size())
                fatal_error("%s (file #%u is %s)", e, fi, files[fi].c_str());
            fatal_error("preparing the reference text on the device failed: %s", e);
        }
        dev.text_stats(t, &n_text, &n_seqs, &n_fwd);
        text.resize(n_text);
        fwd.resize(n_fwd);
        seq_ends.resize(n_seqs);
        seq_file.resize(n_seqs);
        dev.text_copy(t, text.data(), file_len.data(), fwd.data(), seq_ends.data(), seq_file.data());
        if (opts.seq_table) {
            uint64_t n_name_bytes = 0;
            dev.text_names(t, nullptr, nullptr, &n_name_bytes);
            names.resize(n_name_bytes);
            name_ends.resize(n_seqs);
            dev.text_names(t, names.data(), name_ends.data(), nullptr);
        }
        dev.text_free(t);
    }
    if (n_text == 0) {
        std::printf("\n\n");
        fatal_warning("After sequence digestion, there is no sequence left. "
                      "Note minimizer digestion can only be used with FASTA files.");
    }
    if (n_text > MAX_TEXT) refuse_long_text(n_text);

    // documents: one per file, files with the same id merged; a single file with -d: the lengths of <prefix>.fa.fdi
    std::vector<uint64_t> doc_lengths;
    bool fdi_given = false;
    if (opts.ref_file.length() && opts.build_doc) {
        const std::string fdi = opts.output_prefix + ".fa.fdi";
        std::ifstream in(fdi);
        std::string line;
        uint64_t sum = 0;
        while (std::getline(in, line)) {
            std::istringstream ss(line);
            std::string name;
            unsigned long long len = 0;
            if (!(ss >> name)) continue;
            if (!(ss >> len)) fatal_error("%s: every line must be <name><TAB><length>: %s", fdi.c_str(), line.c_str());
            doc_lengths.push_back(len);
            sum += len;
        }
        if (doc_lengths.empty() || sum != n_text)
            fatal_error("the document lengths in %s sum to %llu, the text has %llu characters.", fdi.c_str(),
                        (unsigned long long)sum, (unsigned long long)n_text);
        fdi_given = true;
    } else {
        for (size_t i = 0; i < files.size(); ++i) {
            if (!doc_ids.empty() && i > 0 && doc_ids[i] == doc_ids[i - 1]) doc_lengths.back() += file_len[i];
            else doc_lengths.push_back(file_len[i]);
        }
    }
    DONE_LOG((std::chrono::system_clock::now() - task_start));

    // the index
    STATUS_LOG("build_main", "building the run-length BWT, thresholds and SA samples on the device");
    task_start = std::chrono::system_clock::now();
    spb_build* b = dev.build_from_text(text.data(), n_text, doc_lengths.data(), (uint32_t)doc_lengths.size(), 1, device);
    if (!b) fatal_error("building the index on the device failed: %s", spx_last_error());
    uint64_t n = 0, r = 0;
    dev.build_stats(b, &n, &r);
    std::vector<uint8_t> heads(r);
    std::vector<uint64_t> lens(r), thr(r), ssa(r), esa(r), ds(r), de(r);
    dev.build_copy(b, heads.data(), lens.data(), thr.data(), ssa.data(), esa.data(), ds.data(), de.data());
    dev.build_free(b);
    DONE_LOG((std::chrono::system_clock::now() - task_start));

    STATUS_LOG("build_main", "writing the index files (%s.*)", prefix.data());
    task_start = std::chrono::system_clock::now();
    {
        std::string fa = ">concatenated\n";
        fa.append(reinterpret_cast<const char*>(text.data()), text.size());
        fa.push_back('\n');
        write_bytes(prefix, fa.data(), fa.size());
    }
    write_bytes(prefix + ".bwt.heads", heads.data(), heads.size());
    write_five(prefix + ".bwt.len", lens);
    write_five(prefix + ".thr_pos", thr);
    {
        std::vector<uint64_t> sp(2 * r), ep(2 * r);
        uint64_t start = 0;
        for (uint64_t i = 0; i < r; ++i) {
            sp[2 * i] = start;
            sp[2 * i + 1] = (ssa[i] + 1) % n;
            ep[2 * i] = start + lens[i] - 1;
            ep[2 * i + 1] = (esa[i] + 1) % n;
            start += lens[i];
        }
        write_five(prefix + ".ssa", sp);
        write_five(prefix + ".esa", ep);
    }
    write_bytes(prefix + ".rawtext", text.data(), text.size());
    if (!(fdi_given && prefix + ".fdi" == opts.output_prefix + ".fa.fdi")) {
        std::string f;
        for (size_t i = 0; i < doc_lengths.size(); ++i)
            f += "group_" + std::to_string(i + 1) + "\t" + std::to_string(doc_lengths[i]) + "\n";
        write_bytes(prefix + ".fdi", f.data(), f.size());
    }
    if (opts.seq_table) {
        // spumoni_amd/map.py: seq_table_bytes.  Without digestion the text is every sequence followed at once by its
        // reverse complement (unless -c): a sequence's forward piece starts where the pieces before it end
        const uint64_t strands = opts.use_rev_comp ? 2 : 1;
        std::string f;
        std::set<std::string> seen;
        uint64_t start = 0, dup = 0;
        for (uint64_t q = 0; q < n_seqs; ++q) {
            const uint64_t len = seq_ends[q] - (q ? seq_ends[q - 1] : 0), n0 = q ? name_ends[q - 1] : 0;
            const std::string name(reinterpret_cast<const char*>(names.data()) + n0, name_ends[q] - n0);
            dup += !seen.insert(name).second;
            f += name + "\t" + std::to_string(len) + "\t" + std::to_string(start) + "\t" + std::to_string(strands) + "\n";
            start += len * strands;
        }
        if (start != n_text)
            fatal_error("internal: the sequences of the table add up to %llu characters, the text has %llu.",
                        (unsigned long long)start, (unsigned long long)n_text);
        write_bytes(prefix + ".seqs", f.data(), f.size());
        if (dup)
            std::fprintf(stderr, "\nwarning: %llu sequence name(s) occur more than once in the sequence table\n",
                         (unsigned long long)dup);
    }
    DONE_LOG((std::chrono::system_clock::now() - task_start));

    // the empirical null: reads drawn from the sequences, reversed, upper-cased and digested like the text; their
    // statistics are the databases and their own KS statistics give the thresholds.  One generator, MS then PML
    // (both databases are always written, as build_index writes them).
    GlibcRand rng(0);
    std::vector<Piece> seqs(n_seqs);
    for (uint64_t q = 0; q < n_seqs; ++q) {
        const uint64_t s = q ? seq_ends[q - 1] : 0;
        seqs[q] = {fwd.data() + s, (size_t)(seq_ends[q] - s)};
    }
    std::vector<uint8_t> upper_fwd;
    std::vector<Piece> reads;
    if (opts.ref_file.length()) {
        reads = null_reads_from_fasta(seqs, rng);
    } else {
        upper_fwd = fwd;
        for (uint8_t& c : upper_fwd)
            if (c >= 'a' && c <= 'z') c -= 32;
        for (Piece& p : seqs) p.first = upper_fwd.data() + (p.first - fwd.data());
        reads = null_reads_from_list(seqs, rng);
    }
    {
        std::string f;
        for (size_t i = 0; i < reads.size(); ++i) {
            f += ">read_" + std::to_string(i) + "\n";
            f.append(reinterpret_cast<const char*>(reads[i].first), reads[i].second);
            f += "\n";
        }
        write_bytes(null_read_file, f.data(), f.size());
    }
    std::vector<uint64_t> stats_ms{0}, stats_pml{0};
    double ks_ms = 0.0, ks_pml = 0.0;
    std::vector<uint8_t> q;
    std::vector<uint64_t> offs{0};
    spx_index* ix = nullptr;
    if (!reads.empty()) {
        for (const Piece& p : reads) {
            for (size_t i = p.second; i-- > 0;) {
                uint8_t c = p.first[i];
                q.push_back(c >= 'a' && c <= 'z' ? (uint8_t)(c - 32) : c);
            }
            offs.push_back(q.size());
        }
        const uint64_t nreads = reads.size();
        ix = spx_index_from_runs(heads.data(), lens.data(), thr.data(), r, ssa.data(), esa.data(), ds.data(),
                                            de.data(), 0, device);
        if (!ix) fatal_error("loading the index on the device failed: %s", spx_last_error());
        if (spx_index_set_text(ix, text.data(), n_text, 0) != SPX_OK)
            fatal_error("loading the index text on the device failed: %s", spx_last_error());
        if (digest_kind) {
            const uint64_t cap = spx_digest_capacity(digest_kind, (uint32_t)opts.k, q.size());
            std::vector<uint8_t> dq(cap);
            std::vector<uint64_t> doffs(nreads + 1);
            if (spx_digest_batch(ix, digest_kind, (uint32_t)opts.k, (uint32_t)opts.w, q.data(), offs.data(), nreads,
                                 dq.data(), cap, doffs.data()) != SPX_OK)
                fatal_error("digesting the null reads failed: %s", spx_last_error());
            dq.resize(doffs[nreads]);
            q.swap(dq);
            offs.swap(doffs);
        }
    }
    const uint64_t nreads = reads.size(), tot = offs.back();
    for (int mode : {SPX_MODE_MS, SPX_MODE_PML}) {
        STATUS_LOG("build_main", "building the empirical null statistic database for %s",
                   mode == SPX_MODE_MS ? "MS" : "PML");
        task_start = std::chrono::system_clock::now();
        std::vector<uint32_t> lengths;
        if (ix) {
            lengths.resize(std::max<uint64_t>(tot, 1) + 8);
            std::vector<uint64_t> ptrs(mode == SPX_MODE_MS ? std::max<uint64_t>(tot, 1) : 0);
            if (spx_query_batch(ix, mode, q.data(), offs.data(), nreads, lengths.data(),
                                mode == SPX_MODE_MS ? ptrs.data() : nullptr, nullptr, nullptr, 0, 0) != SPX_OK)
                fatal_error("computing the null statistics failed: %s", spx_last_error());
        }
        if (ix && tot) {
            std::vector<uint64_t> st(lengths.begin(), lengths.begin() + tot);
            const int wd = width_of(st);
            const uint64_t mask = wd >= 64 ? ~0ull : ((1ull << wd) - 1);
            std::vector<uint64_t> stored(st);
            for (uint64_t& v : stored) v &= mask;
            std::vector<double> ks;
            for (uint64_t i = 0; i < nreads; ++i)
                if (offs[i + 1] > offs[i])
                    run_kstest(st.data() + offs[i], offs[i + 1] - offs[i], stored, opts.bin_size, rng, ks);
            double sum = 0.0;
            for (double x : ks) sum += x;
            const double mean = sum / (double)ks.size();
            double sq = 0.0;
            for (double x : ks) sq += std::pow(x - mean, 2.0);
            const double thr_ks = mean + 3 * std::pow(sq / (double)ks.size(), 0.5);
            if (mode == SPX_MODE_MS) {
                stats_ms.swap(st);
                ks_ms = thr_ks;
            } else {
                stats_pml.swap(st);
                ks_pml = thr_ks;
            }
        }
        if (mode == SPX_MODE_MS) write_null_db(prefix + ".msnulldb", stats_ms, ks_ms);
        else write_null_db(prefix + ".pmlnulldb", stats_pml, ks_pml);
        DONE_LOG((std::chrono::system_clock::now() - task_start));
    }
    if (ix) spx_index_free(ix);
    if (opts.build_doc) {
        STATUS_LOG("build_main", "building the document array");
        task_start = std::chrono::system_clock::now();
        const uint64_t nd = std::max<uint64_t>(doc_lengths.size(), 2);
        const int w = std::max(1, (int)std::ceil(std::log2((double)nd)));
        std::string d;
        put(d, &r, 8);
        append_int_vector(d, ds, w);
        append_int_vector(d, de, w);
        write_bytes(prefix + ".doc", d.data(), d.size());
        DONE_LOG((std::chrono::system_clock::now() - task_start));
    }
    std::fprintf(stderr, "\n");

    const auto total_time = std::chrono::duration<double>(std::chrono::system_clock::now() - total_start);
    FORCE_LOG("build_main", "n = %llu, r = %llu, documents = %zu, null reads = %zu, KS threshold PML = %.4f MS = %.4f",
              (unsigned long long)n, (unsigned long long)r, doc_lengths.size(), reads.size(), ks_pml, ks_ms);
    FORCE_LOG("build_main", "\033[1m\033[32mtotal elapsed time for build process (s): %.3f\033[0m", total_time.count());
    FORCE_LOG("build_main", "\033[1m\033[32mindex files are saved in the %s.* files.\033[0m\n", prefix.data());
    return 0;
}
