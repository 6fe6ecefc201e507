// consensus_main.cpp -- `spumoni consensus`: the sequences a read set implies for the index's reference -- `spumoni call`'s
// coverage and pileup accumulated on the device, then per base the reference's letter kept, substituted, deleted or masked
// (include/spumoni_consensus.h has the rule) and the text of a FASTA file laid out on the device.  The options, the
// sequence table, the reads and the index are `call`'s; super-batches of SPUMONI_SUPER_BATCH characters go through
// spl_call_add_batch in calls of one piece each and add up.  The driver is read_command.cpp; the files are
// consensus_fasta.hpp's; both are written when everything has been fetched, so a run that fails leaves neither.
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
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
    unsigned long long min_depth = 2, min_alt = 2, min_permille = 500, line_width = 60;
    std::string mask = "N";
    bool keep_low = false;
    parse_read_options(argc, argv, o, spumoni_consensus_usage, true, m.shorts("D:A:Q:U:uJ:").c_str(),
                       m.longs({{"min-depth", required_argument, NULL, 'D'},
                                {"min-alt", required_argument, NULL, 'A'},
                                {"min-permille", required_argument, NULL, 'Q'},
                                {"mask", required_argument, NULL, 'U'},
                                {"keep-low", no_argument, NULL, 'u'},
                                {"line-width", required_argument, NULL, 'J'}}),
                       [&](int c, const char* arg) {
                           if (m.set(o, c, arg)) return;
                           if (c == 'U')
                               mask = arg;
                           else if (c == 'u')
                               keep_low = true;
                           else
                               (c == 'D' ? min_depth : c == 'A' ? min_alt : c == 'Q' ? min_permille : line_width) = count_argument(arg);
                       });
    require_ref_and_pattern(o);
    if (o.pml_requested)
        fatal_warning("-P cannot be used with `spumoni consensus`: the anchors are read off matching statistics (-M is implied); "
                      "PMLs have no pointers.");
    if (o.use_promotions || o.use_dna_letters)
        fatal_warning("-m / -a cannot be used with `spumoni consensus`: digested coordinates cannot be turned back into bases. "
                      "Map against an index built with -n -s.");
    if (o.min_digest)
        fatal_warning("`spumoni consensus` needs -n: digested coordinates cannot be turned back into bases (index built with -n -s).");
    o.ms = true;
    validate_read_options(o);
    m.validate(o);
    if (min_depth < 1 || min_depth > 4294967295ull) fatal_warning("the smallest depth (-D) must be between 1 and 4294967295.");
    if (min_alt < 1 || min_alt > 4294967295ull)
        fatal_warning("the fewest reads with a substituted letter or a deletion (-A) must be between 1 and 4294967295.");
    if (min_permille > 1000) fatal_warning("the smallest share (-Q) must be between 0 and 1000 thousandths.");
    if (mask.size() != 1 || mask[0] == '\n' || mask[0] == '>') fatal_warning("the mask (-U) must be one byte other than a newline and '>'.");
    if (line_width > 2147483647ull) fatal_warning("the line width (-J) must be between 0 and 2147483647.");
    o.ref_file += ".fa";
    const std::string table_path = o.ref_file + ".seqs";
    if (!is_file(table_path))
        fatal_warning("the index has no sequence table (%s): build it with -s (spumoni build -n -s).", table_path.c_str());
    const SeqTable table = read_seq_table(table_path);
    const std::vector<void*> entry =
        device_entry_points("consensus", {"spl_call_add_batch", "spn_set_sequences", "spl_call_reset", "sps_consensus_begin",
                                          "sps_consensus_fetch"}, "the consensus kernels");
    auto add_batch = reinterpret_cast<decltype(&spl_call_add_batch)>(entry[0]);
    auto set_sequences = reinterpret_cast<decltype(&spn_set_sequences)>(entry[1]);
    auto reset = reinterpret_cast<decltype(&spl_call_reset)>(entry[2]);
    auto consensus_begin = reinterpret_cast<decltype(&sps_consensus_begin)>(entry[3]);
    auto consensus_fetch = reinterpret_cast<decltype(&sps_consensus_fetch)>(entry[4]);
    ReadRun run;
    open_read_run(o, 8u << 20, run);
    run.super_batch = std::min<size_t>(run.super_batch, 32u << 20);  // (one piece per spl_call_add_batch)
    if (set_sequences(run.ix, table.lengths.data(), table.lengths.size(), table.strands) != SPX_OK)
        fatal_error("%s: %s", table_path.c_str(), spx_last_error());
    if (reset(run.ix) != SPX_OK) fatal_error("%s", spx_last_error());
    const uint64_t min_length = m.min_length(o);
    const spc_params params = m.chain();
    const spa_params fill = m.fill();
    const spe_params ends = m.ends();
    std::fprintf(stderr, "[consensus] index loaded (n = %llu, r = %llu), %llu sequences on %u strand(s); %s; a base needs depth %llu, a "
                 "substitution or a deletion %llu reads and %llu thousandths; %s for a masked base, %llu letters a line\n",
                 (unsigned long long)run.set.n, (unsigned long long)run.set.r, (unsigned long long)table.names.size(), table.strands,
                 m.describe(min_length).c_str(), min_depth, min_alt, min_permille, keep_low ? "the reference's letter" : mask.c_str(),
                 line_width);

    LinesFile none;  // (nothing is written per read)
    none.keep_partial = false;
    uint64_t num_reads = 0, num_mapped = 0;
    std::vector<spn_mapping> maps;
    scan_reads(
        run, none,
        [&](ReadBatch& b) {
            maps.resize(b.take + 1);
            for_each_piece(b, [&](size_t q0, size_t q1) {
                if (add_batch(run.ix, 0, (uint32_t)o.k, (uint32_t)o.w, b.seqs.data(), b.offs.data() + q0, q1 - q0, min_length,
                              o.use_doc ? 1 : 0, &params, &fill, &ends, maps.data() + q0) != SPX_OK)
                    fatal_error("%s", spx_last_error());
                // (without digestion a read's values are its characters)
                for (size_t q = q0; q < q1; ++q) b.values[q] = b.offs[q + 1] - b.offs[q];
            });
        },
        [&](const ReadBatch&, size_t i) {
            num_reads++;
            num_mapped += maps[i].seq != SPN_UNMAPPED;
        });
    // everything that can fail on the device comes before the first file
    sps_params cp;
    std::memset(&cp, 0, sizeof cp);
    cp.min_depth = (uint32_t)min_depth;
    cp.min_alt = (uint32_t)min_alt;
    cp.min_permille = (uint32_t)min_permille;
    cp.line_width = (uint32_t)line_width;
    cp.mask = keep_low ? 0 : (uint8_t)mask[0];
    uint64_t n_bytes = 0;
    if (consensus_begin(run.ix, &cp, &n_bytes) != SPX_OK) fatal_error("%s", spx_last_error());
    std::vector<sps_seq> records(table.names.size());
    std::vector<uint8_t> body(n_bytes + 1);
    if (consensus_fetch(run.ix, records.data(), body.data()) != SPX_OK) fatal_error("%s", spx_last_error());
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
                 (unsigned long long)num_reads, (unsigned long long)num_mapped, (unsigned long long)(num_reads - num_mapped),
                 (unsigned long long)sum.letters, (unsigned long long)sum.substituted, (unsigned long long)sum.deleted,
                 (unsigned long long)sum.masked);
    if (sum.ins_sites) std::fprintf(stderr, "; %llu insertion sites were not applied", (unsigned long long)sum.ins_sites);
    std::fprintf(stderr, " (%.3f sec). results are saved in *.consensus.fa and *.consensus.tsv\n",
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - run.t_start).count());
    return 0;
}
