// cover_main.cpp -- `spumoni cover`: per sequence of the index, how many reads map to it, how much of it they cover and how
// deep -- `spumoni map`'s mappings accumulated on the device into per-base depth and mismatch counts
// (include/spumoni_cover.h has the rule), and one line per sequence in place of one line per read.  The options, the
// sequence table, the reads and the index are `map`'s; super-batches of SPUMONI_SUPER_BATCH characters go through
// spd_cover_add_batch in calls of one piece each and add up.  The driver is read_command.cpp; both files are written when
// everything has been fetched, so a run that fails leaves none.
#include <unistd.h>

#include <cstdio>
#include <string>
#include <vector>

#include "../../../include/spumoni_cover.h"
#include "read_command.hpp"

using namespace spumoni_host;

namespace {

int spumoni_cover_usage() {
    std::fprintf(stderr, "spumoni cover - Uses a spumoni MS index and its sequence table to map each read as `spumoni map` does, and reports per sequence how many reads map to it, how much of it they cover and how deep.\n");
    std::fprintf(stderr, "Usage: spumoni cover [options]\n\n");
    std::fprintf(stderr, "Options:\n");
    std::fprintf(stderr, "\t%-35sprints this usage message\n", "-h, --help");
    std::fprintf(stderr, "\t%-25s%-10soutput prefix used for index; <prefix>.fa.seqs must exist (spumoni build -n -s)\n", "-r, --ref", "[FILE]");
    std::fprintf(stderr, "\t%-25s%-10spath to patterns file that will be used.\n", "-p, --pattern", "[FILE]");
    std::fprintf(stderr, "\t%-25s%-10sno minimizer digestion of reads: required, digested coordinates cannot be turned back into bases\n", "-n, --no-digest", "");
    std::fprintf(stderr, "\t%-25s%-10srefused by `spumoni cover`\n", "-m, --minimizer-alphabet", "");
    std::fprintf(stderr, "\t%-25s%-10srefused by `spumoni cover`\n", "-a, --dna-minimizer", "");
    std::fprintf(stderr, "\t%-25s%-10ssmall window size (k) for finding minimizers (default: 4)\n", "-K, --small-window", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10slarge window size (w) for finding minimizers (default: 11)\n", "-W, --large-window", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10suse document array: matches chain within one document\n", "-d, --doc-array", "");
    std::fprintf(stderr, "\t%-25s%-10salso writes <pattern>.bedgraph: the runs of equal depth\n", "-b, --bedgraph", "");
    std::fprintf(stderr, "\t%-25s%-10sthe smallest depth of a run in the bedgraph, 0 .. 4294967295 (default: 1)\n", "-D, --min-depth", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10s`spumoni map`'s options with its defaults: the anchors' minimum length, the chain\n", "-L -S -G -B -H", "[INT]");
    std::fprintf(stderr, "\t%-35s(max-dist, max-gap, gap-penalty, lookback)\n", "");
    std::fprintf(stderr, "\t%-25s%-10s... the filled gaps (max-fill) and the extension (max-extend, band, mismatch, indel)\n\n", "-F -E -O -N -I", "[INT]");
    std::fprintf(stderr, "Matching statistics (-M) are implied. Writes <pattern>.cover, one line per sequence in the table's order: name,\n");
    std::fprintf(stderr, "length, reads mapped to it, covered bases, breadth (covered / length), bases (the sum of the depth), mean depth\n");
    std::fprintf(stderr, "(bases / length), the largest depth, mismatches (X columns) and indels (I + D lengths). A deleted base is not\n");
    std::fprintf(stderr, "covered. The bedgraph has name, start, end and depth per run, in the sequences' forward coordinates.\n\n");
    return 1;
}

// six decimals of num / den from the integers, rounded half up: no floating point, the same digits everywhere
std::string ratio6(uint64_t num, uint64_t den) {
    const unsigned __int128 scaled = ((unsigned __int128)num * 2000000u + den) / ((unsigned __int128)den * 2);
    char buf[64];
    std::snprintf(buf, sizeof buf, "%llu.%06llu", (unsigned long long)(scaled / 1000000u), (unsigned long long)(scaled % 1000000u));
    return buf;
}

}  // namespace

int cover_main(int argc, char** argv) {
    if (argc == 1) return spumoni_cover_usage();
    ReadOptions o;
    MapOptions m(MapOptions::EXTEND);
    unsigned long long min_depth = 1;
    bool bedgraph = false;
    parse_read_options(argc, argv, o, spumoni_cover_usage, true, m.shorts("D:b").c_str(),
                       m.longs({{"min-depth", required_argument, NULL, 'D'}, {"bedgraph", no_argument, NULL, 'b'}}),
                       [&](int c, const char* arg) {
                           if (m.set(o, c, arg)) return;
                           if (c == 'b')
                               bedgraph = true;
                           else
                               min_depth = count_argument(arg);
                       });
    require_ref_and_pattern(o);
    imply_ms(o, "cover");
    require_bases(o, "cover");
    validate_read_options(o);
    m.validate(o);
    if (min_depth > 4294967295ull) fatal_warning("the smallest depth (-D) must be between 0 and 4294967295.");
    TableRun run;
    open_table_run(o, m, "cover", {"spd_cover_add_batch", "spn_set_sequences", "spd_cover_reset", "spd_cover_summary", "spd_cover_runs_begin",
                                   "spd_cover_runs_fetch"}, "the coverage kernels", "spd_cover_reset", run);
    const SeqTable& table = run.table;
    std::fprintf(stderr, "%s\n", run.loaded.c_str());

    const ReadCounts counts = accumulate_reads(run, o, m, run.entry<decltype(&spd_cover_add_batch)>("spd_cover_add_batch"));
    // everything that can fail on the device comes before the first file
    std::vector<spd_seq_cover> cover(table.names.size());
    if (run.entry<decltype(&spd_cover_summary)>("spd_cover_summary")(run.ix, cover.data(), cover.size()) != SPX_OK)
        fatal_error("%s", spx_last_error());
    std::vector<spd_run> runs;
    if (bedgraph) {
        uint64_t n = 0;
        if (run.entry<decltype(&spd_cover_runs_begin)>("spd_cover_runs_begin")(run.ix, (uint32_t)min_depth, &n) != SPX_OK)
            fatal_error("%s", spx_last_error());
        runs.resize(n + 1);
        if (run.entry<decltype(&spd_cover_runs_fetch)>("spd_cover_runs_fetch")(run.ix, runs.data()) != SPX_OK) fatal_error("%s", spx_last_error());
        runs.resize(n);
    }
    uint64_t added = 0;
    for (const spd_seq_cover& c : cover) added += c.reads;
    const std::string bed_path = o.pattern_file + ".bedgraph";
    if (bedgraph) {
        LinesFile bed;
        bed.open(bed_path, false);
        for (const spd_run& r : runs)
            std::fprintf(bed.f, "%s\t%llu\t%llu\t%u\n", table.names[r.seq].c_str(), (unsigned long long)r.start, (unsigned long long)r.end,
                         r.depth);
        bed.close();
    }
    LinesFile out;
    out.open(o.pattern_file + ".cover", false);
    for (size_t s = 0; s < cover.size(); ++s) {
        const spd_seq_cover& c = cover[s];
        const uint64_t len = table.lengths[s];
        std::fprintf(out.f, "%s\t%llu\t%llu\t%llu\t%s\t%llu\t%s\t%u\t%llu\t%llu\n", table.names[s].c_str(), (unsigned long long)len,
                     (unsigned long long)c.reads, (unsigned long long)c.covered, ratio6(c.covered, len).c_str(), (unsigned long long)c.bases,
                     ratio6(c.bases, len).c_str(), c.max_depth, (unsigned long long)c.mismatches, (unsigned long long)c.indels);
    }
    if (std::fflush(out.f) != 0 || std::ferror(out.f)) {
        if (bedgraph) ::unlink(bed_path.c_str());  // (a run that fails leaves no file: this one was complete already)
        fatal_error("write failed (disk full?): %s", out.path.c_str());
    }
    out.close();
    std::fprintf(stderr, "[cover] %llu reads, %llu mapped, %llu added to the coverage, %llu without a mapping (%.3f sec). results are saved in "
                 "*.cover%s\n",
                 (unsigned long long)counts.reads, (unsigned long long)counts.mapped, (unsigned long long)added,
                 (unsigned long long)(counts.reads - counts.mapped),
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - run.t_start).count(), bedgraph ? " and *.bedgraph" : "");
    return 0;
}
