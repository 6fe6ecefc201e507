// consensus_main.cpp -- `spumoni consensus`: the sequences a read set implies for the index's reference -- `spumoni call`'s
// coverage and pileup accumulated on the device, then per base the reference's letter kept, substituted, deleted or masked
// (include/spumoni_consensus.h has the rule) and the text of a FASTA file laid out on the device.  The options, the
// sequence table, the reads and the index are `call`'s; super-batches of SPUMONI_SUPER_BATCH characters go through
// spl_call_add_batch in calls of one piece each and add up.  The driver is read_command.cpp; the files are
// consensus_fasta.hpp's; both are written when everything has been fetched, so a run that fails leaves neither.
#include <unistd.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/spumoni_consensus.h"
#include "consensus_fasta.hpp"
#include "read_command.hpp"

using namespace spumoni_host;

namespace {

int spumoni_consensus_usage() {
    std::fprintf(stderr, "spumoni consensus - Uses a spumoni MS index and its sequence table to map each read as `spumoni map` does, and writes the reference's sequences as the reads imply them.\n");
    std::fprintf(stderr, "Usage: spumoni consensus [options]\n\n");
    std::fprintf(stderr, "Options:\n");
    std::fprintf(stderr, "\t%-35sprints this usage message\n", "-h, --help");
    std::fprintf(stderr, "\t%-25s%-10soutput prefix used for index; <prefix>.fa.seqs must exist (spumoni build -n -s)\n", "-r, --ref", "[FILE]");
    std::fprintf(stderr, "\t%-25s%-10spath to patterns file that will be used.\n", "-p, --pattern", "[FILE]");
    std::fprintf(stderr, "\t%-25s%-10sno minimizer digestion of reads: required, digested coordinates cannot be turned back into bases\n", "-n, --no-digest", "");
    std::fprintf(stderr, "\t%-25s%-10srefused by `spumoni consensus`\n", "-m, --minimizer-alphabet", "");
    std::fprintf(stderr, "\t%-25s%-10srefused by `spumoni consensus`\n", "-a, --dna-minimizer", "");
    std::fprintf(stderr, "\t%-25s%-10ssmall window size (k) for finding minimizers (default: 4)\n", "-K, --small-window", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10slarge window size (w) for finding minimizers (default: 11)\n", "-W, --large-window", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10suse document array: matches chain within one document\n", "-d, --doc-array", "");
    std::fprintf(stderr, "\t%-25s%-10sthe smallest depth of a base that is not masked, 1 .. 4294967295 (default: 2)\n", "-D, --min-depth", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10sthe fewest reads that carry a substituted letter or delete a base, 1 .. 4294967295 (default: 2)\n", "-A, --min-alt", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10sthe smallest share of the reads that do, in thousandths, 0 .. 1000 (default: 500)\n", "-Q, --min-permille", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10sthe byte written for a masked base (default: N)\n", "-U, --mask", "[CHAR]");
    std::fprintf(stderr, "\t%-25s%-10swrite the reference's letter for a masked base instead\n", "-u, --keep-low", "");
    std::fprintf(stderr, "\t%-25s%-10sletters per line, 0 .. 2147483647; 0: one line per sequence (default: 60)\n", "-J, --line-width", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10s`spumoni map`'s options with its defaults: the anchors' minimum length, the chain\n", "-L -S -G -B -H", "[INT]");
    std::fprintf(stderr, "\t%-35s(max-dist, max-gap, gap-penalty, lookback)\n", "");
    std::fprintf(stderr, "\t%-25s%-10s... the filled gaps (max-fill) and the extension (max-extend, band, mismatch, indel)\n\n", "-F -E -O -N -I", "[INT]");
    std::fprintf(stderr, "Matching statistics (-M) are implied. Writes <pattern>.consensus.fa: per sequence of the table `>name` and its letters --\n");
    std::fprintf(stderr, "the reference's, a substituted letter where `spumoni call` would call one, nothing where enough reads delete the base, the\n");
    std::fprintf(stderr, "mask where fewer than min-depth reads cover it -- and <pattern>.consensus.tsv: name, length, letters, substituted, deleted,\n");
    std::fprintf(stderr, "masked and insertion sites per sequence. Insertion sites are counted, not applied.\n\n");
    return 1;
}

}  // namespace

int consensus_main(int argc, char** argv) {
    if (argc == 1) return spumoni_consensus_usage();
    ReadOptions o;
    MapOptions m(MapOptions::EXTEND);
    CallThresholds t;
    unsigned long long line_width = 60;
    std::string mask = "N";
    bool keep_low = false;
    parse_read_options(argc, argv, o, spumoni_consensus_usage, true, m.shorts(t.shorts("U:uJ:").c_str()).c_str(),
                       m.longs(t.longs({{"mask", required_argument, NULL, 'U'},
                                        {"keep-low", no_argument, NULL, 'u'},
                                        {"line-width", required_argument, NULL, 'J'}})),
                       [&](int c, const char* arg) {
                           if (m.set(o, c, arg) || t.set(c, arg)) return;
                           if (c == 'U')
                               mask = arg;
                           else if (c == 'u')
                               keep_low = true;
                           else
                               line_width = count_argument(arg);
                       });
    require_ref_and_pattern(o);
    imply_ms(o, "consensus");
    require_bases(o, "consensus");
    validate_read_options(o);
    m.validate(o);
    t.validate("the fewest reads with a substituted letter or a deletion");
    if (mask.size() != 1 || mask[0] == '\n' || mask[0] == '>') fatal_warning("the mask (-U) must be one byte other than a newline and '>'.");
    if (line_width > 2147483647ull) fatal_warning("the line width (-J) must be between 0 and 2147483647.");
    TableRun run;
    open_table_run(o, m, "consensus", {"spl_call_add_batch", "spn_set_sequences", "spl_call_reset", "sps_consensus_begin",
                                       "sps_consensus_fetch"}, "the consensus kernels", "spl_call_reset", run);
    const SeqTable& table = run.table;
    std::fprintf(stderr, "%s; a base needs depth %llu, a substitution or a deletion %llu reads and %llu thousandths; %s for a masked base, "
                 "%llu letters a line\n",
                 run.loaded.c_str(), t.min_depth, t.min_alt, t.min_permille, keep_low ? "the reference's letter" : mask.c_str(), line_width);

    const ReadCounts counts = accumulate_reads(run, o, m, run.entry<decltype(&spl_call_add_batch)>("spl_call_add_batch"));
    // everything that can fail on the device comes before the first file
    sps_params cp;
    std::memset(&cp, 0, sizeof cp);
    cp.min_depth = (uint32_t)t.min_depth;
    cp.min_alt = (uint32_t)t.min_alt;
    cp.min_permille = (uint32_t)t.min_permille;
    cp.line_width = (uint32_t)line_width;
    cp.mask = keep_low ? 0 : (uint8_t)mask[0];
    uint64_t n_bytes = 0;
    if (run.entry<decltype(&sps_consensus_begin)>("sps_consensus_begin")(run.ix, &cp, &n_bytes) != SPX_OK) fatal_error("%s", spx_last_error());
    std::vector<sps_seq> records(table.names.size());
    std::vector<uint8_t> body(n_bytes + 1);
    if (run.entry<decltype(&sps_consensus_fetch)>("sps_consensus_fetch")(run.ix, records.data(), body.data()) != SPX_OK)
        fatal_error("%s", spx_last_error());
    if (!consensus_records_fit(records.data(), records.size(), n_bytes)) fatal_error("the consensus records do not describe the body");
    const std::string fa_path = o.pattern_file + ".consensus.fa";
    {
        LinesFile fa;
        fa.open(fa_path, false);
        write_consensus_fasta(fa.f, table.names, records.data(), body.data(), n_bytes);
        if (std::fflush(fa.f) != 0 || std::ferror(fa.f)) fatal_error("write failed (disk full?): %s", fa.path.c_str());
        fa.close();
    }
    LinesFile out;
    out.open(o.pattern_file + ".consensus.tsv", false);
    write_consensus_tsv(out.f, table.names, table.lengths, records.data());
    if (std::fflush(out.f) != 0 || std::ferror(out.f)) {
        ::unlink(fa_path.c_str());  // (a run that fails leaves no file: this one was complete already)
        fatal_error("write failed (disk full?): %s", out.path.c_str());
    }
    out.close();
    sps_seq sum;
    std::memset(&sum, 0, sizeof sum);
    for (const sps_seq& r : records) {
        sum.letters += r.letters;
        sum.substituted += r.substituted;
        sum.deleted += r.deleted;
        sum.masked += r.masked;
        sum.ins_sites += r.ins_sites;
    }
    std::fprintf(stderr, "[consensus] %llu reads, %llu mapped, %llu without a mapping; %llu letters, %llu substituted, %llu deleted, %llu masked",
                 (unsigned long long)counts.reads, (unsigned long long)counts.mapped, (unsigned long long)(counts.reads - counts.mapped),
                 (unsigned long long)sum.letters, (unsigned long long)sum.substituted, (unsigned long long)sum.deleted,
                 (unsigned long long)sum.masked);
    if (sum.ins_sites) std::fprintf(stderr, "; %llu insertion sites were not applied", (unsigned long long)sum.ins_sites);
    std::fprintf(stderr, " (%.3f sec). results are saved in *.consensus.fa and *.consensus.tsv\n",
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - run.t_start).count());
    return 0;
}
