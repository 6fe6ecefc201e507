// call_main.cpp -- `spumoni call`: the single-nucleotide calls of a read set against the index -- `spumoni map`'s mappings
// accumulated on the device into the coverage and, beside it, per-base counts of the letters the reads carried where they
// disagreed with the reference (include/spumoni_call.h has the rule), and one VCF line per call in place of one line per
// read.  The options, the sequence table, the reads and the index are `map`'s; super-batches of SPUMONI_SUPER_BATCH
// characters go through spl_call_add_batch in calls of one piece each and add up.  The driver is read_command.cpp; the
// lines are call_vcf.hpp's; the file is written when everything has been fetched, so a run that fails leaves none.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "../../../include/spumoni_call.h"
#include "call_vcf.hpp"
#include "read_command.hpp"

using namespace spumoni_host;

namespace {

int spumoni_call_usage() {
    std::fprintf(stderr, "spumoni call - Uses a spumoni MS index and its sequence table to map each read as `spumoni map` does, and reports the positions where the reads support a letter other than the reference's.\n");
    std::fprintf(stderr, "Usage: spumoni call [options]\n\n");
    std::fprintf(stderr, "Options:\n");
    std::fprintf(stderr, "\t%-35sprints this usage message\n", "-h, --help");
    std::fprintf(stderr, "\t%-25s%-10soutput prefix used for index; <prefix>.fa.seqs must exist (spumoni build -n -s)\n", "-r, --ref", "[FILE]");
    std::fprintf(stderr, "\t%-25s%-10spath to patterns file that will be used.\n", "-p, --pattern", "[FILE]");
    std::fprintf(stderr, "\t%-25s%-10sno minimizer digestion of reads: required, digested coordinates cannot be turned back into bases\n", "-n, --no-digest", "");
    std::fprintf(stderr, "\t%-25s%-10srefused by `spumoni call`\n", "-m, --minimizer-alphabet", "");
    std::fprintf(stderr, "\t%-25s%-10srefused by `spumoni call`\n", "-a, --dna-minimizer", "");
    std::fprintf(stderr, "\t%-25s%-10ssmall window size (k) for finding minimizers (default: 4)\n", "-K, --small-window", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10slarge window size (w) for finding minimizers (default: 11)\n", "-W, --large-window", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10suse document array: matches chain within one document\n", "-d, --doc-array", "");
    std::fprintf(stderr, "\t%-25s%-10sthe smallest depth of a call, 1 .. 4294967295 (default: 2)\n", "-D, --min-depth", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10sthe fewest reads that carry the called letter, 1 .. 4294967295 (default: 2)\n", "-A, --min-alt", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10sthe smallest share of the depth that carries it, in thousandths, 0 .. 1000 (default: 500)\n", "-Q, --min-permille", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10s`spumoni map`'s options with its defaults: the anchors' minimum length, the chain\n", "-L -S -G -B -H", "[INT]");
    std::fprintf(stderr, "\t%-35s(max-dist, max-gap, gap-penalty, lookback)\n", "");
    std::fprintf(stderr, "\t%-25s%-10s... the filled gaps (max-fill) and the extension (max-extend, band, mismatch, indel)\n\n", "-F -E -O -N -I", "[INT]");
    std::fprintf(stderr, "Matching statistics (-M) are implied. Writes <pattern>.vcf (VCFv4.2): one line per position where the letter that\n");
    std::fprintf(stderr, "most mismatching reads carry passes the three thresholds, with DP (depth), AD (reads that match the reference,\n");
    std::fprintf(stderr, "reads with the called letter), BC (mismatching reads by letter A, C, G, T), OT (with another byte), DL (reads that\n");
    std::fprintf(stderr, "delete the base) and IN (insertions in front of it). Insertions and deletions are counted, not called.\n\n");
    return 1;
}

}  // namespace

int call_main(int argc, char** argv) {
    if (argc == 1) return spumoni_call_usage();
    ReadOptions o;
    MapOptions m(MapOptions::EXTEND);
    CallThresholds t;
    parse_read_options(argc, argv, o, spumoni_call_usage, true, m.shorts(t.shorts().c_str()).c_str(), m.longs(t.longs()),
                       [&](int c, const char* arg) {
                           if (!m.set(o, c, arg)) t.set(c, arg);
                       });
    require_ref_and_pattern(o);
    imply_ms(o, "call");
    require_bases(o, "call");
    validate_read_options(o);
    m.validate(o);
    t.validate("the fewest reads with the called letter");
    TableRun run;
    open_table_run(o, m, "call", {"spl_call_add_batch", "spn_set_sequences", "spl_call_reset", "spl_calls_begin", "spl_calls_fetch",
                                  "spd_cover_depth"}, "the pileup kernels", "spl_call_reset", run);
    const SeqTable& table = run.table;
    std::fprintf(stderr, "%s; a call needs depth %llu, %llu reads and %llu thousandths of the depth\n", run.loaded.c_str(), t.min_depth,
                 t.min_alt, t.min_permille);

    const ReadCounts counts = accumulate_reads(run, o, m, run.entry<decltype(&spl_call_add_batch)>("spl_call_add_batch"));
    // everything that can fail on the device comes before the file
    uint64_t n = 0;
    if (run.entry<decltype(&spl_calls_begin)>("spl_calls_begin")(run.ix, (uint32_t)t.min_depth, (uint32_t)t.min_alt,
                                                                 (uint32_t)t.min_permille, &n) != SPX_OK)
        fatal_error("%s", spx_last_error());
    std::vector<spl_call> calls(n + 1);
    if (run.entry<decltype(&spl_calls_fetch)>("spl_calls_fetch")(run.ix, calls.data()) != SPX_OK) fatal_error("%s", spx_last_error());
    calls.resize(n);
    // ref_count is depth - mism: the mismatch counts of the calls' bases, from slices of 16 Mi positions that hold a call
    std::vector<uint64_t> starts(table.lengths.size() + 1, 0);
    for (size_t s = 0; s < table.lengths.size(); ++s) starts[s + 1] = starts[s] + table.lengths[s];
    std::vector<uint32_t> mism(n + 1), slice;
    auto cover_depth = run.entry<decltype(&spd_cover_depth)>("spd_cover_depth");
    for (uint64_t i = 0; i < n;) {
        if (calls[i].seq >= table.lengths.size() || calls[i].pos >= table.lengths[calls[i].seq])
            fatal_error("a call lies outside the sequence table (sequence %u, position %llu)", calls[i].seq, (unsigned long long)calls[i].pos);
        const uint64_t first = starts[calls[i].seq] + calls[i].pos, count = std::min<uint64_t>(16u << 20, starts.back() - first);
        slice.resize(count);
        if (cover_depth(run.ix, first, count, nullptr, slice.data()) != SPX_OK) fatal_error("%s", spx_last_error());
        for (; i < n && calls[i].seq < table.lengths.size() && calls[i].pos < table.lengths[calls[i].seq] &&
               starts[calls[i].seq] + calls[i].pos >= first && starts[calls[i].seq] + calls[i].pos - first < count; ++i)
            mism[i] = slice[starts[calls[i].seq] + calls[i].pos - first];
    }
    LinesFile out;
    out.open(o.pattern_file + ".vcf", false);
    write_vcf_header(out.f, table.names, table.lengths);
    if (!write_vcf_calls(out.f, table.names, calls.data(), mism.data(), n)) fatal_error("a call names a sequence or a letter that does not exist");
    if (std::fflush(out.f) != 0 || std::ferror(out.f)) fatal_error("write failed (disk full?): %s", out.path.c_str());
    out.close();
    std::fprintf(stderr, "[call] %llu reads, %llu mapped, %llu without a mapping, %llu calls (%.3f sec). results are saved in *.vcf\n",
                 (unsigned long long)counts.reads, (unsigned long long)counts.mapped, (unsigned long long)(counts.reads - counts.mapped),
                 (unsigned long long)n, std::chrono::duration<double>(std::chrono::steady_clock::now() - run.t_start).count());
    return 0;
}
