// call_main.cpp -- `spumoni call`: the single-nucleotide calls of a read set against the index -- `spumoni map`'s mappings
// accumulated on the device into the coverage and, beside it, per-base counts of the letters the reads carried where they
// disagreed with the reference (include/spumoni_call.h has the rule), and one VCF line per call in place of one line per
// read.  The options, the sequence table, the reads and the index are `map`'s; super-batches of SPUMONI_SUPER_BATCH
// characters go through spl_call_add_batch in calls of one piece each and add up.  The driver is read_command.cpp; the
// lines are call_vcf.hpp's; the file is written when everything has been fetched, so a run that fails leaves none.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
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
    unsigned long long min_depth = 2, min_alt = 2, min_permille = 500;
    parse_read_options(argc, argv, o, spumoni_call_usage, true, m.shorts("D:A:Q:").c_str(),
                       m.longs({{"min-depth", required_argument, NULL, 'D'},
                                {"min-alt", required_argument, NULL, 'A'},
                                {"min-permille", required_argument, NULL, 'Q'}}),
                       [&](int c, const char* arg) {
                           if (!m.set(o, c, arg)) (c == 'D' ? min_depth : c == 'A' ? min_alt : min_permille) = count_argument(arg);
                       });
    require_ref_and_pattern(o);
    if (o.pml_requested)
        fatal_warning("-P cannot be used with `spumoni call`: the anchors are read off matching statistics (-M is implied); "
                      "PMLs have no pointers.");
    if (o.use_promotions || o.use_dna_letters)
        fatal_warning("-m / -a cannot be used with `spumoni call`: digested coordinates cannot be turned back into bases. "
                      "Map against an index built with -n -s.");
    if (o.min_digest)
        fatal_warning("`spumoni call` needs -n: digested coordinates cannot be turned back into bases (index built with -n -s).");
    o.ms = true;
    validate_read_options(o);
    m.validate(o);
    if (min_depth < 1 || min_depth > 4294967295ull) fatal_warning("the smallest depth (-D) must be between 1 and 4294967295.");
    if (min_alt < 1 || min_alt > 4294967295ull) fatal_warning("the fewest reads with the called letter (-A) must be between 1 and 4294967295.");
    if (min_permille > 1000) fatal_warning("the smallest share (-Q) must be between 0 and 1000 thousandths.");
    o.ref_file += ".fa";
    const std::string table_path = o.ref_file + ".seqs";
    if (!is_file(table_path))
        fatal_warning("the index has no sequence table (%s): build it with -s (spumoni build -n -s).", table_path.c_str());
    const SeqTable table = read_seq_table(table_path);
    const std::vector<void*> entry =
        device_entry_points("call", {"spl_call_add_batch", "spn_set_sequences", "spl_call_reset", "spl_calls_begin", "spl_calls_fetch",
                                     "spd_cover_depth"}, "the pileup kernels");
    auto add_batch = reinterpret_cast<decltype(&spl_call_add_batch)>(entry[0]);
    auto set_sequences = reinterpret_cast<decltype(&spn_set_sequences)>(entry[1]);
    auto reset = reinterpret_cast<decltype(&spl_call_reset)>(entry[2]);
    auto calls_begin = reinterpret_cast<decltype(&spl_calls_begin)>(entry[3]);
    auto calls_fetch = reinterpret_cast<decltype(&spl_calls_fetch)>(entry[4]);
    auto cover_depth = reinterpret_cast<decltype(&spd_cover_depth)>(entry[5]);
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
    std::fprintf(stderr, "[call] index loaded (n = %llu, r = %llu), %llu sequences on %u strand(s); %s; a call needs depth %llu, %llu reads and "
                 "%llu thousandths of the depth\n",
                 (unsigned long long)run.set.n, (unsigned long long)run.set.r, (unsigned long long)table.names.size(), table.strands,
                 m.describe(min_length).c_str(), min_depth, min_alt, min_permille);

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
    // everything that can fail on the device comes before the file
    uint64_t n = 0;
    if (calls_begin(run.ix, (uint32_t)min_depth, (uint32_t)min_alt, (uint32_t)min_permille, &n) != SPX_OK) fatal_error("%s", spx_last_error());
    std::vector<spl_call> calls(n + 1);
    if (calls_fetch(run.ix, calls.data()) != SPX_OK) fatal_error("%s", spx_last_error());
    calls.resize(n);
    // ref_count is depth - mism: the mismatch counts of the calls' bases, from slices of 16 Mi positions that hold a call
    std::vector<uint64_t> starts(table.lengths.size() + 1, 0);
    for (size_t s = 0; s < table.lengths.size(); ++s) starts[s + 1] = starts[s] + table.lengths[s];
    std::vector<uint32_t> mism(n + 1), slice;
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
                 (unsigned long long)num_reads, (unsigned long long)num_mapped, (unsigned long long)(num_reads - num_mapped),
                 (unsigned long long)n, std::chrono::duration<double>(std::chrono::steady_clock::now() - run.t_start).count());
    return 0;
}
