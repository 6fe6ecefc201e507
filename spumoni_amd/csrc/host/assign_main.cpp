// assign_main.cpp -- `spumoni assign`: one line per read that names the document most of the read's positions point
// to (include/spumoni_docvote.h has the rule).  The reads come from reads.cpp (same ids, same FASTA / FASTQ quirks as
// `run`), the index through the loaders `run` uses, and super-batches of SPUMONI_SUPER_BATCH characters go through
// spv_assign_batch: digestion, walk and votes stay on the device and 16 bytes per read come back.  A lean driver of its
// own: one device (the first of SPUMONI_GPUS), lines written in input order with plain buffered writes.
//
// The binary must also load against libraries without the votes (a CPU test double of the query boundary): the spv_*
// entry point is looked up at run time, never linked.
#include <dlfcn.h>
#include <getopt.h>
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../../include/spumoni_docvote.h"
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

int spumoni_assign_usage() {
    std::fprintf(stderr, "spumoni assign - Uses a spumoni index with a document array to assign each read to a document.\n");
    std::fprintf(stderr, "Usage: spumoni assign [options]\n\n");
    std::fprintf(stderr, "Options:\n");
    std::fprintf(stderr, "\t%-35sprints this usage message\n", "-h, --help");
    std::fprintf(stderr, "\t%-25s%-10soutput prefix used for index\n", "-r, --ref", "[FILE]");
    std::fprintf(stderr, "\t%-25s%-10spath to patterns file that will be used.\n", "-p, --pattern", "[FILE]");
    std::fprintf(stderr, "\t%-25s%-10suse index to compute MSs\n", "-M, --MS", "");
    std::fprintf(stderr, "\t%-25s%-10suse index to compute PMLs\n", "-P, --PML", "");
    std::fprintf(stderr, "\t%-25s%-10sturn off minimizer digestion of reads (default: on)\n", "-n, --no-digest", "");
    std::fprintf(stderr, "\t%-25s%-10suse alphabet-promoted minimizers\n", "-m, --minimizer-alphabet", "");
    std::fprintf(stderr, "\t%-25s%-10suse DNA-letter based minimizers\n", "-a, --dna-minimizer", "");
    std::fprintf(stderr, "\t%-25s%-10ssmall window size (k) for finding minimizers (default: 4)\n", "-K, --small-window", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10slarge window size (w) for finding minimizers (default: 11)\n", "-W, --large-window", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10sa position votes when its value is at least this (default: the\n", "-T, --min-length", "[INT]");
    std::fprintf(stderr, "\t%-35sthreshold `run -c` classifies with, from the null database)\n\n", "");
    std::fprintf(stderr, "Writes <pattern>.assignments (id, top_doc, top_votes, second_votes, voters, values per read)\n");
    std::fprintf(stderr, "and <pattern>.assignments.by_doc (reads per document).\n\n");
    return 1;
}

struct AssignOptions : RunOptions {
    bool ms_requested = false, pml_requested = false;
    bool have_min_length = false;
    uint64_t min_length = 0;
};

void parse(int argc, char** argv, AssignOptions& o) {
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
                                           {"min-length", required_argument, NULL, 'T'},
                                           {0, 0, 0, 0}};
    int long_index = 0;
    for (int c; (c = getopt_long(argc, argv, "hr:p:MPnmaK:W:T:", long_options, &long_index)) >= 0;) {
        switch (c) {
            case 'r': o.ref_file.assign(optarg); break;
            case 'p': o.pattern_file.assign(optarg); break;
            case 'M': o.ms_requested = true; break;
            case 'P': o.pml_requested = true; break;
            case 'm': o.use_promotions = true; break;
            case 'a': o.use_dna_letters = true; break;
            case 'n': o.min_digest = false; break;
            case 'K': o.k = std::max(std::atoi(optarg), 1); break;
            case 'W': o.w = std::max(std::atoi(optarg), 1); break;
            case 'T':
                o.have_min_length = true;
                o.min_length = std::strtoull(optarg, nullptr, 10);
                break;
            default: spumoni_assign_usage(); std::exit(1);
        }
    }
}

// `run`'s rules and messages where the rule is the same (spumoni_main.cpp: validate)
void validate(const AssignOptions& o) {
    if (o.ref_file == "" || o.pattern_file == "") fatal_warning("Both a reference file (-r) and pattern file (-p) must be provided.");
    if (o.ms_requested == o.pml_requested)
        fatal_warning("An output type with -M or -P must be specified, only one can be used at a time.");
    const std::string base = o.ref_file + (o.use_promotions ? ".bin" : ".fa");
    if (!is_file(base)) fatal_error("The following path is not valid: %s (remember to only specify output prefix)", base.data());
    if (!is_file(o.pattern_file)) fatal_error("The following path is not valid: %s", o.pattern_file.data());
    if (!ends_with(o.pattern_file, ".fa") && !ends_with(o.pattern_file, ".fasta") && !ends_with(o.pattern_file, ".fna"))
        fatal_error("The pattern file provided does not appear to be a FASTA\n"
                    "       file, please convert to FASTA and re-run.");
    if (!is_file(base + ".doc")) fatal_warning("document array file (%s) is not present, so it cannot be used.", (base + ".doc").data());
    const bool ms = o.ms_requested;
    const bool have_raw = is_file(base + ".bwt.heads") && is_file(base + ".bwt.len") && is_file(base + ".thr_pos") &&
                          (!ms || (is_file(base + ".ssa") && is_file(base + ".esa")));
    if (!have_raw && !is_file(base + (ms ? ".thrbv.ms" : ".thrbv.spumoni")))
        fatal_warning("The index required for this computation is not available, please use spumoni build.");
    if (o.k > 4) fatal_warning("small window size (k) cannot be larger than 4 characters.");
    if (o.w < o.k) fatal_warning("large window size (w) should be larger than the small window size (k)");
    if (o.min_digest) {
        if (o.use_promotions && o.use_dna_letters) fatal_error("Only one type of minimizer can be specified from either -m or -a.");
        if (!o.use_promotions && !o.use_dna_letters) fatal_error("A minimizer type must be specified using -m or -a.");
    } else if (o.use_promotions || o.use_dna_letters) {
        fatal_error("A minimizer type should not be specified if intending not to use minimizer digestion.");
    }
}

struct OutFile {
    std::string path;
    FILE* f = nullptr;
    void open(const std::string& p) {
        path = p;
        f = std::fopen(p.c_str(), "wb");
        if (!f) fatal_error("cannot create %s", p.c_str());
        std::setvbuf(f, nullptr, _IOFBF, 1 << 20);
    }
    void close() {
        if (f && std::fclose(f) != 0) fatal_error("write failed (disk full?): %s", path.c_str());
        f = nullptr;
    }
};

}  // namespace

int assign_main(int argc, char** argv) {
    if (argc == 1) return spumoni_assign_usage();
    AssignOptions o;
    parse(argc, argv, o);
    validate(o);
    o.ref_file += o.use_promotions ? ".bin" : ".fa";
    o.ms = o.ms_requested;
    o.use_doc = true;
    // everything the command needs of the library, before any file is written
    auto assign_batch = reinterpret_cast<decltype(&spv_assign_batch)>(dlsym(RTLD_DEFAULT, "spv_assign_batch"));
    if (!assign_batch)
        fatal_error("the loaded libspumoni_gpu.so has no spv_assign_batch: `spumoni assign` needs the document votes of "
                    "the device library, and there is no CPU fallback.");
    if (spx_device_count() <= 0) fatal_error("no usable gfx950 device: `spumoni assign` runs on the GPU and has no CPU fallback.");
    int device = 0;
    if (const char* g = std::getenv("SPUMONI_GPUS")) device = std::atoi(g);
    if (const char* t = std::getenv("SPUMONI_TEXT")) o.text_file = t;
    size_t super_batch = o.ms ? 8u << 20 : 32u << 20;
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
    uint64_t min_length = o.min_length;
    if (!o.have_min_length) {  // what `run -c` classifies with (classify.cpp)
        double percentile = 0.0;
        std::string err;
        (void)load_null_db(o.ref_file + (o.ms ? ".msnulldb" : ".pmlnulldb"), percentile, err);
        min_length = max_value_threshold(percentile, !o.ms, o.use_promotions, o.use_dna_letters);
    }
    const int kind = o.use_promotions ? SPX_DIGEST_PROMOTED : (o.use_dna_letters ? SPX_DIGEST_DNA : 0);
    std::fprintf(stderr, "[assign] index loaded (n = %llu, r = %llu); a position votes from %llu on\n", (unsigned long long)set.n,
                 (unsigned long long)set.r, (unsigned long long)min_length);

    OutFile lines;
    lines.open(o.pattern_file + ".assignments");
    std::map<uint32_t, uint64_t> by_doc;
    uint64_t unassigned = 0, num_reads = 0;
    std::vector<ReadRec> recs;
    std::vector<uint8_t> seqs;
    std::vector<uint64_t> offs, values;
    std::vector<spv_vote> votes;
    // 0 none, 1 a malformed record, 2 a read that is empty: fatal once everything in front of it is written, as in `run`
    int deferred = 0;
    std::string deferred_msg;
    auto flush = [&](size_t take) {
        offs.assign(1, 0);
        size_t chars = 0;
        for (size_t i = 0; i < take; ++i) offs.push_back(chars += recs[i].seq_len);
        seqs.resize(chars + 1);
        for (size_t i = 0; i < take; ++i) reads->copy_seq_upper(recs[i], seqs.data() + offs[i]);
        votes.resize(take + 1);
        values.resize(take + 1);
        if (take && assign_batch(ix, o.ms ? SPX_MODE_MS : SPX_MODE_PML, kind, (uint32_t)o.k, (uint32_t)o.w, seqs.data(), offs.data(), take,
                                 min_length, votes.data(), values.data()) != SPX_OK)
            fatal_error("%s", spx_last_error());
        for (size_t i = 0; i < take; ++i) {
            if (values[i] == 0) {  // compute_ms_pml.cpp:926-931
                deferred = 2;
                deferred_msg.assign(recs[i].id, recs[i].id_len);
                return;
            }
            const spv_vote& v = votes[i];
            std::fwrite(recs[i].id, 1, recs[i].id_len, lines.f);
            if (v.top_votes) {
                std::fprintf(lines.f, "\t%u\t%u\t%u\t%u\t%llu\n", v.top_doc, v.top_votes, v.second_votes, v.voters, (unsigned long long)values[i]);
                by_doc[v.top_doc]++;
            } else {
                std::fprintf(lines.f, "\t-1\t0\t0\t0\t%llu\n", (unsigned long long)values[i]);
                unassigned++;
            }
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
        if (deferred || pending_chars >= super_batch) {
            const int d = deferred;
            const std::string msg = deferred_msg;
            deferred = 0;
            flush(take);
            if (!deferred) {
                deferred = d;
                deferred_msg = msg;
            }
            recs.clear();
            pending_chars = 0;
        }
    }
    if (!deferred) flush(recs.size());
    lines.close();
    if (deferred == 1) fatal_error("%s", deferred_msg.c_str());
    if (deferred == 2) {
        std::cout << "\n\n";
        fatal_warning("%s was empty after digestion, commonly due to reads "
                      "consisting of mostly non-ACGT characters. Please remove "
                      "read or run SPUMONI without minimizer digestion.", deferred_msg.data());
    }
    OutFile summary;
    summary.open(o.pattern_file + ".assignments.by_doc");
    for (const auto& kv : by_doc) std::fprintf(summary.f, "%u\t%llu\n", kv.first, (unsigned long long)kv.second);
    if (unassigned) std::fprintf(summary.f, "-1\t%llu\n", (unsigned long long)unassigned);
    summary.close();
    std::fprintf(stderr, "[assign] %llu reads assigned to %zu documents, %llu unassigned (%.3f sec). results are saved in *.assignments\n",
                 (unsigned long long)(num_reads - unassigned), by_doc.size(), (unsigned long long)unassigned,
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count());
    return 0;
}
