// place_main.cpp -- `spumoni place`: one line per read -- where its longest match with the text, extended to both sides
// without gaps, sits on the reference and how many characters agree there (include/spumoni_place.h has the rule).  The
// reads come from reads.cpp (same ids, same FASTA / FASTQ quirks as `run`), the MS index through the loaders `run` uses,
// and super-batches of SPUMONI_SUPER_BATCH characters go through spp_place_batch: digestion, walk, extension and the
// placement stay on the device and 32 bytes per read come back.  A lean driver of its own: one device (the first of
// SPUMONI_GPUS), lines written in input order with plain buffered writes; a run that fails leaves no file.
//
// The binary must also load against libraries without the placements (a CPU test double of the query boundary): the
// spp_* entry points are looked up at run time, never linked.
#include <dlfcn.h>
#include <getopt.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "../../../include/spumoni_place.h"
#include "classify.hpp"
#include "index_files.hpp"
#include "reads.hpp"

using namespace spumoni_host;

namespace {

bool is_file(const std::string& p) {
    struct stat st;
    return ::stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}
bool ends_with(const std::string& s, const std::string& suf) {
    return s.size() >= suf.size() && s.compare(s.size() - suf.size(), suf.size(), suf) == 0;
}

int spumoni_place_usage() {
    std::fprintf(stderr, "spumoni place - Uses a spumoni MS index to place each read on the reference: its longest match, extended without gaps.\n");
    std::fprintf(stderr, "Usage: spumoni place [options]\n\n");
    std::fprintf(stderr, "Options:\n");
    std::fprintf(stderr, "\t%-35sprints this usage message\n", "-h, --help");
    std::fprintf(stderr, "\t%-25s%-10soutput prefix used for index\n", "-r, --ref", "[FILE]");
    std::fprintf(stderr, "\t%-25s%-10spath to patterns file that will be used.\n", "-p, --pattern", "[FILE]");
    std::fprintf(stderr, "\t%-25s%-10sturn off minimizer digestion of reads (default: on)\n", "-n, --no-digest", "");
    std::fprintf(stderr, "\t%-25s%-10suse alphabet-promoted minimizers\n", "-m, --minimizer-alphabet", "");
    std::fprintf(stderr, "\t%-25s%-10suse DNA-letter based minimizers\n", "-a, --dna-minimizer", "");
    std::fprintf(stderr, "\t%-25s%-10ssmall window size (k) for finding minimizers (default: 4)\n", "-K, --small-window", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10slarge window size (w) for finding minimizers (default: 11)\n", "-W, --large-window", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10suse document array to name the document of each read's seed\n", "-d, --doc-array", "");
    std::fprintf(stderr, "\t%-25s%-10sa read is placed when its longest match is at least this long (default: the\n", "-L, --min-seed", "[INT]");
    std::fprintf(stderr, "\t%-35sMS threshold `run -c` classifies with, from the null database)\n", "");
    std::fprintf(stderr, "\t%-25s%-10swhat a mismatch costs in the extension, a match scoring 1 (default: 4)\n", "-B, --mismatch-penalty", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10sthe extension stops when its score falls more than this below its best (default: 16)\n\n", "-X, --x-drop", "[INT]");
    std::fprintf(stderr, "Matching statistics (-M) are implied. Writes <pattern>.placements: id, values, read_start, read_end, ref_start,\n");
    std::fprintf(stderr, "matches, seed_pos, seed_len[, doc] per read, positions in the (digested) read and text; an unplaced read has -1\n");
    std::fprintf(stderr, "for ref_start (and doc) and zeros elsewhere.\n\n");
    return 1;
}

struct PlaceOptions : RunOptions {
    bool pml_requested = false;
    bool have_min_seed = false;
    uint64_t min_seed = 0;
    unsigned long long penalty = 4, x_drop = 16;
};

void parse(int argc, char** argv, PlaceOptions& o) {
    static struct option long_options[] = {{"help", no_argument, NULL, 'h'},
                                           {"ref", required_argument, NULL, 'r'},
                                           {"pattern", required_argument, NULL, 'p'},
                                           {"MS", no_argument, NULL, 'M'},
                                           {"PML", no_argument, NULL, 'P'},
                                           {"no-digest", no_argument, NULL, 'n'},
                                           {"minimizer-alphabet", no_argument, NULL, 'm'},
                                           {"dna-minimizer", no_argument, NULL, 'a'},
                                           {"small-window", required_argument, NULL, 'K'},
                                           {"large-window", required_argument, NULL, 'W'},
                                           {"doc-array", no_argument, NULL, 'd'},
                                           {"min-seed", required_argument, NULL, 'L'},
                                           {"mismatch-penalty", required_argument, NULL, 'B'},
                                           {"x-drop", required_argument, NULL, 'X'},
                                           {0, 0, 0, 0}};
    int long_index = 0;
    for (int c; (c = getopt_long(argc, argv, "hr:p:MPnmaK:W:dL:B:X:", long_options, &long_index)) >= 0;) {
        switch (c) {
            case 'r': o.ref_file.assign(optarg); break;
            case 'p': o.pattern_file.assign(optarg); break;
            case 'M': break;  // implied
            case 'P': o.pml_requested = true; break;
            case 'm': o.use_promotions = true; break;
            case 'a': o.use_dna_letters = true; break;
            case 'n': o.min_digest = false; break;
            case 'K': o.k = std::max(std::atoi(optarg), 1); break;
            case 'W': o.w = std::max(std::atoi(optarg), 1); break;
            case 'd': o.use_doc = true; break;
            case 'L':
                o.have_min_seed = true;
                o.min_seed = std::strtoull(optarg, nullptr, 10);
                break;
            case 'B': o.penalty = optarg[0] == '-' ? ~0ull : std::strtoull(optarg, nullptr, 10); break;
            case 'X': o.x_drop = optarg[0] == '-' ? ~0ull : std::strtoull(optarg, nullptr, 10); break;
            default: spumoni_place_usage(); std::exit(1);
        }
    }
}

// `run`'s rules and messages where the rule is the same (spumoni_main.cpp: validate)
void validate(const PlaceOptions& o) {
    if (o.ref_file == "" || o.pattern_file == "") fatal_warning("Both a reference file (-r) and pattern file (-p) must be provided.");
    if (o.pml_requested)
        fatal_warning("-P cannot be used with `spumoni place`: reads are placed by their matching statistics (-M is implied); "
                      "PMLs have no pointers.");
    const std::string base = o.ref_file + (o.use_promotions ? ".bin" : ".fa");
    if (!is_file(base)) fatal_error("The following path is not valid: %s (remember to only specify output prefix)", base.data());
    if (!is_file(o.pattern_file)) fatal_error("The following path is not valid: %s", o.pattern_file.data());
    if (!ends_with(o.pattern_file, ".fa") && !ends_with(o.pattern_file, ".fasta") && !ends_with(o.pattern_file, ".fna"))
        fatal_error("The pattern file provided does not appear to be a FASTA\n"
                    "       file, please convert to FASTA and re-run.");
    if (o.use_doc && !is_file(base + ".doc"))
        fatal_warning("document array file (%s) is not present, so it cannot be used.", (base + ".doc").data());
    const bool have_raw = is_file(base + ".bwt.heads") && is_file(base + ".bwt.len") && is_file(base + ".thr_pos") &&
                          is_file(base + ".ssa") && is_file(base + ".esa");
    if (!have_raw && !is_file(base + ".thrbv.ms"))
        fatal_warning("The index required for this computation is not available, please use spumoni build.");
    if (o.k > 4) fatal_warning("small window size (k) cannot be larger than 4 characters.");
    if (o.w < o.k) fatal_warning("large window size (w) should be larger than the small window size (k)");
    if (o.min_digest) {
        if (o.use_promotions && o.use_dna_letters) fatal_error("Only one type of minimizer can be specified from either -m or -a.");
        if (!o.use_promotions && !o.use_dna_letters) fatal_error("A minimizer type must be specified using -m or -a.");
    } else if (o.use_promotions || o.use_dna_letters) {
        fatal_error("A minimizer type should not be specified if intending not to use minimizer digestion.");
    }
    if (o.have_min_seed && o.min_seed == 0) fatal_warning("the minimum seed length (-L) must be at least 1.");
    if (o.penalty > 65535) fatal_warning("the mismatch penalty (-B) must be between 0 and 65535.");
    if (o.x_drop > 2147483647ull) fatal_warning("the x-drop (-X) must be between 0 and 2147483647.");
}

// the output of a run that fails does not stay (every way out through fatal_error / fatal_warning comes here)
std::string g_partial;
void drop_partial() {
    if (!g_partial.empty()) ::unlink(g_partial.c_str());
    g_partial.clear();
}

}  // namespace

int place_main(int argc, char** argv) {
    if (argc == 1) return spumoni_place_usage();
    PlaceOptions o;
    parse(argc, argv, o);
    validate(o);
    o.ref_file += o.use_promotions ? ".bin" : ".fa";
    o.ms = true;
    // everything the command needs of the library, before any file is written
    auto place_batch = reinterpret_cast<decltype(&spp_place_batch)>(dlsym(RTLD_DEFAULT, "spp_place_batch"));
    if (!place_batch)
        fatal_error("the loaded libspumoni_gpu.so has no spp_place_batch: `spumoni place` needs the placement kernels of "
                    "the device library, and there is no CPU fallback.");
    if (spx_device_count() <= 0) fatal_error("no usable gfx950 device: `spumoni place` runs on the GPU and has no CPU fallback.");
    int device = 0;
    if (const char* g = std::getenv("SPUMONI_GPUS")) device = std::atoi(g);
    if (const char* t = std::getenv("SPUMONI_TEXT")) o.text_file = t;
    size_t super_batch = 8u << 20;
    if (const char* t = std::getenv("SPUMONI_SUPER_BATCH")) super_batch = std::max<size_t>(1000, std::strtoull(t, nullptr, 10));

    const auto t_start = std::chrono::steady_clock::now();
    std::unique_ptr<ReadFile> reads;
    try {
        reads.reset(new ReadFile(o.pattern_file));
    } catch (const std::exception& e) {
        fatal_error("%s", e.what());
    }
    IndexSet set;
    {
        RunOptions lo = o;
        lo.devices = {device};
        lo.pattern_file.clear();  // (nothing of `run`'s text output is reserved)
        set.load(lo);
    }
    spx_index* ix = set.ix[0];
    if (o.use_promotions)
        if (const char* pin = std::getenv("SPUMONI_CHARHASH")) {
            unsigned v[4] = {0, 0, 0, 0};
            if (std::sscanf(pin, "%u,%u,%u,%u", &v[0], &v[1], &v[2], &v[3]) != 4)
                fatal_error("SPUMONI_CHARHASH must be four comma-separated byte values (A,C,G,T)");
            const int64_t packed = (int64_t)((v[0] & 255) | ((v[1] & 255) << 8) | ((v[2] & 255) << 16) | ((uint64_t)(v[3] & 255) << 24));
            if (spx_set_option(ix, "minimizer_charhash", packed) != SPX_OK) fatal_error("%s", spx_last_error());
        }
    uint64_t min_seed = o.min_seed;
    if (!o.have_min_seed) {  // what `run -M -c` classifies with (classify.cpp)
        double percentile = 0.0;
        std::string err;
        (void)load_null_db(o.ref_file + ".msnulldb", percentile, err);
        min_seed = std::max<uint64_t>(1, max_value_threshold(percentile, false, o.use_promotions, o.use_dna_letters));
    }
    const int kind = o.use_promotions ? SPX_DIGEST_PROMOTED : (o.use_dna_letters ? SPX_DIGEST_DNA : 0);
    std::fprintf(stderr, "[place] index loaded (n = %llu, r = %llu); a read is placed from a seed of length %llu on (penalty %llu, x-drop %llu)\n",
                 (unsigned long long)set.n, (unsigned long long)set.r, (unsigned long long)min_seed, o.penalty, o.x_drop);

    set_exit_hook(drop_partial);
    const std::string out_path = o.pattern_file + ".placements";
    FILE* out = std::fopen(out_path.c_str(), "wb");
    if (!out) fatal_error("cannot create %s", out_path.c_str());
    g_partial = out_path;
    std::setvbuf(out, nullptr, _IOFBF, 1 << 20);
    uint64_t num_reads = 0, num_placed = 0;
    std::vector<ReadRec> recs;
    std::vector<uint8_t> seqs;
    std::vector<uint64_t> offs, values;
    std::vector<spp_placement> placed;
    // 0 none, 1 a malformed record, 2 a read that is empty: fatal, as in `run`
    int deferred = 0;
    std::string deferred_msg;
    auto flush = [&](size_t take) {
        if (!take) return;
        offs.assign(1, 0);
        size_t chars = 0;
        for (size_t i = 0; i < take; ++i) offs.push_back(chars += recs[i].seq_len);
        seqs.resize(chars + 1);
        for (size_t i = 0; i < take; ++i) reads->copy_seq_upper(recs[i], seqs.data() + offs[i]);
        values.resize(take + 1);
        placed.resize(take + 1);
        if (place_batch(ix, kind, (uint32_t)o.k, (uint32_t)o.w, seqs.data(), offs.data(), take, min_seed, (uint32_t)o.penalty, o.x_drop,
                        o.use_doc ? 1 : 0, placed.data(), values.data()) != SPX_OK)
            fatal_error("%s", spx_last_error());
        for (size_t i = 0; i < take; ++i) {
            if (values[i] == 0) {  // compute_ms_pml.cpp:926-931
                deferred = 2;
                deferred_msg.assign(recs[i].id, recs[i].id_len);
                return;
            }
            const spp_placement& p = placed[i];
            const bool is_placed = p.ref_start != SPP_UNPLACED;
            std::fwrite(recs[i].id, 1, recs[i].id_len, out);
            std::fprintf(out, "\t%llu\t%u\t%u\t", (unsigned long long)values[i], p.read_start, p.read_end);
            if (is_placed)
                std::fprintf(out, "%llu", (unsigned long long)p.ref_start);
            else
                std::fputs("-1", out);
            std::fprintf(out, "\t%u\t%u\t%u", p.matches, p.seed_pos, p.seed_len);
            if (o.use_doc) std::fprintf(out, "\t%lld", p.doc == SPP_NO_DOC ? -1ll : (long long)p.doc);
            std::fputc('\n', out);
            num_placed += is_placed;
            num_reads++;
        }
    };
    reads->precompute_ranges(1000);
    ReadFile::Range range;
    size_t pending_chars = 0;
    while (!deferred && reads->next_range(1000, range)) {
        ReadFile::ParseError err;
        const size_t before = recs.size();
        reads->scan_range(range, recs, err);
        size_t take = recs.size();
        for (size_t i = before; i < recs.size(); ++i) {
            if (recs[i].seq_len == 0) {
                deferred = 2;
                deferred_msg.assign(recs[i].id, recs[i].id_len);
                take = i;
                break;
            }
            pending_chars += recs[i].seq_len;
        }
        if (!deferred && err.fatal) {
            deferred = 1;
            deferred_msg = err.message;
        }
        if (deferred) break;
        if (pending_chars >= super_batch) {
            flush(take);
            recs.clear();
            pending_chars = 0;
        }
    }
    if (!deferred) flush(recs.size());
    if (deferred == 1) fatal_error("%s", deferred_msg.c_str());
    if (deferred == 2) {
        std::cout << "\n\n";
        fatal_warning("%s was empty after digestion, commonly due to reads "
                      "consisting of mostly non-ACGT characters. Please remove "
                      "read or run SPUMONI without minimizer digestion.", deferred_msg.data());
    }
    if (std::fclose(out) != 0) fatal_error("write failed (disk full?): %s", out_path.c_str());
    g_partial.clear();
    std::fprintf(stderr, "[place] %llu reads, %llu placed, %llu unplaced (%.3f sec). results are saved in *.placements\n",
                 (unsigned long long)num_reads, (unsigned long long)num_placed, (unsigned long long)(num_reads - num_placed),
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count());
    return 0;
}
