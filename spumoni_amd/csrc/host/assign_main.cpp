// assign_main.cpp -- `spumoni assign`: one line per read that names the document most of the read's positions point
// to (include/spumoni_docvote.h has the rule).  The reads come from reads.cpp (same ids, same FASTA / FASTQ quirks as
// `run`), the index through the loaders `run` uses, and super-batches of SPUMONI_SUPER_BATCH characters go through
// spv_assign_batch: digestion, walk and votes stay on the device and 16 bytes per read come back.  The driver is
// read_command.cpp; the reads in front of one that fails are assigned and stay in <pattern>.assignments.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../../../include/spumoni_docvote.h"
#include "read_command.hpp"

using namespace spumoni_host;

namespace {

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

}  // namespace

int assign_main(int argc, char** argv) {
    if (argc == 1) return spumoni_assign_usage();
    ReadOptions o;
    parse_read_options(argc, argv, o, spumoni_assign_usage, false, "T:", {{"min-length", required_argument, NULL, 'T'}},
                       [&](int, const char* arg) {
                           o.have_threshold = true;
                           o.threshold = std::strtoull(arg, nullptr, 10);
                       });
    require_ref_and_pattern(o);
    if (o.ms_requested == o.pml_requested)
        fatal_warning("An output type with -M or -P must be specified, only one can be used at a time.");
    o.ms = o.ms_requested;
    o.use_doc = true;
    validate_read_options(o);
    o.ref_file += o.use_promotions ? ".bin" : ".fa";
    auto assign_batch = reinterpret_cast<decltype(&spv_assign_batch)>(
        device_entry_points("assign", {"spv_assign_batch"}, "the document votes")[0]);
    ReadRun run;
    open_read_run(o, o.ms ? 8u << 20 : 32u << 20, run);
    const uint64_t min_length = o.have_threshold ? o.threshold : null_db_threshold(o);
    std::fprintf(stderr, "[assign] index loaded (n = %llu, r = %llu); a position votes from %llu on\n", (unsigned long long)run.set.n,
                 (unsigned long long)run.set.r, (unsigned long long)min_length);

    LinesFile lines;
    lines.open(o.pattern_file + ".assignments", true);
    std::map<uint32_t, uint64_t> by_doc;
    uint64_t unassigned = 0, num_reads = 0;
    std::vector<spv_vote> votes;
    scan_reads(
        run, lines,
        [&](ReadBatch& b) {
            votes.resize(b.take + 1);
            if (assign_batch(run.ix, o.ms ? SPX_MODE_MS : SPX_MODE_PML, run.digest_kind, (uint32_t)o.k, (uint32_t)o.w, b.seqs.data(),
                             b.offs.data(), b.take, min_length, votes.data(), b.values.data()) != SPX_OK)
                fatal_error("%s", spx_last_error());
        },
        [&](const ReadBatch& b, size_t i) {
            const spv_vote& v = votes[i];
            std::fwrite(b.recs[i].id, 1, b.recs[i].id_len, lines.f);
            if (v.top_votes) {
                std::fprintf(lines.f, "\t%u\t%u\t%u\t%u\t%llu\n", v.top_doc, v.top_votes, v.second_votes, v.voters, (unsigned long long)b.values[i]);
                by_doc[v.top_doc]++;
            } else {
                std::fprintf(lines.f, "\t-1\t0\t0\t0\t%llu\n", (unsigned long long)b.values[i]);
                unassigned++;
            }
            num_reads++;
        });
    LinesFile summary;
    summary.open(o.pattern_file + ".assignments.by_doc", true);
    for (const auto& kv : by_doc) std::fprintf(summary.f, "%u\t%llu\n", kv.first, (unsigned long long)kv.second);
    if (unassigned) std::fprintf(summary.f, "-1\t%llu\n", (unsigned long long)unassigned);
    summary.close();
    std::fprintf(stderr, "[assign] %llu reads assigned to %zu documents, %llu unassigned (%.3f sec). results are saved in *.assignments\n",
                 (unsigned long long)(num_reads - unassigned), by_doc.size(), (unsigned long long)unassigned,
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - run.t_start).count());
    return 0;
}
