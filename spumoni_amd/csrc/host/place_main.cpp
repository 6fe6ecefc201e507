// place_main.cpp -- `spumoni place`: one line per read -- where its longest match with the text, extended to both sides
// without gaps, sits on the reference and how many characters agree there (include/spumoni_place.h has the rule).  The
// reads come from reads.cpp (same ids, same FASTA / FASTQ quirks as `run`), the MS index through the loaders `run` uses,
// and super-batches of SPUMONI_SUPER_BATCH characters go through spp_place_batch: digestion, walk, extension and the
// placement stay on the device and 32 bytes per read come back.  The driver is read_command.cpp; a run that fails leaves
// no file.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../../include/spumoni_place.h"
#include "read_command.hpp"

using namespace spumoni_host;

namespace {

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

}  // namespace

int place_main(int argc, char** argv) {
    if (argc == 1) return spumoni_place_usage();
    ReadOptions o;
    unsigned long long penalty = 4, x_drop = 16;
    parse_read_options(argc, argv, o, spumoni_place_usage, true, "L:B:X:",
                       {{"min-seed", required_argument, NULL, 'L'},
                        {"mismatch-penalty", required_argument, NULL, 'B'},
                        {"x-drop", required_argument, NULL, 'X'}},
                       [&](int c, const char* arg) {
                           if (c == 'L') {
                               o.have_threshold = true;
                               o.threshold = std::strtoull(arg, nullptr, 10);
                           } else {
                               (c == 'B' ? penalty : x_drop) = arg[0] == '-' ? ~0ull : std::strtoull(arg, nullptr, 10);
                           }
                       });
    require_ref_and_pattern(o);
    if (o.pml_requested)
        fatal_warning("-P cannot be used with `spumoni place`: reads are placed by their matching statistics (-M is implied); "
                      "PMLs have no pointers.");
    o.ms = true;
    validate_read_options(o);
    if (o.have_threshold && o.threshold == 0) fatal_warning("the minimum seed length (-L) must be at least 1.");
    if (penalty > 65535) fatal_warning("the mismatch penalty (-B) must be between 0 and 65535.");
    if (x_drop > 2147483647ull) fatal_warning("the x-drop (-X) must be between 0 and 2147483647.");
    o.ref_file += o.use_promotions ? ".bin" : ".fa";
    auto place_batch = reinterpret_cast<decltype(&spp_place_batch)>(
        device_entry_points("place", {"spp_place_batch"}, "the placement kernels")[0]);
    ReadRun run;
    open_read_run(o, 8u << 20, run);
    const uint64_t min_seed = o.have_threshold ? o.threshold : std::max<uint64_t>(1, null_db_threshold(o));
    std::fprintf(stderr, "[place] index loaded (n = %llu, r = %llu); a read is placed from a seed of length %llu on (penalty %llu, x-drop %llu)\n",
                 (unsigned long long)run.set.n, (unsigned long long)run.set.r, (unsigned long long)min_seed, penalty, x_drop);

    LinesFile out;
    out.open(o.pattern_file + ".placements", false);
    uint64_t num_reads = 0, num_placed = 0;
    std::vector<spp_placement> placed;
    scan_reads(
        run, out,
        [&](ReadBatch& b) {
            placed.resize(b.take + 1);
            if (place_batch(run.ix, run.digest_kind, (uint32_t)o.k, (uint32_t)o.w, b.seqs.data(), b.offs.data(), b.take, min_seed,
                            (uint32_t)penalty, x_drop, o.use_doc ? 1 : 0, placed.data(), b.values.data()) != SPX_OK)
                fatal_error("%s", spx_last_error());
        },
        [&](const ReadBatch& b, size_t i) {
            const spp_placement& p = placed[i];
            const bool is_placed = p.ref_start != SPP_UNPLACED;
            std::fwrite(b.recs[i].id, 1, b.recs[i].id_len, out.f);
            std::fprintf(out.f, "\t%llu\t%u\t%u\t", (unsigned long long)b.values[i], p.read_start, p.read_end);
            if (is_placed)
                std::fprintf(out.f, "%llu", (unsigned long long)p.ref_start);
            else
                std::fputs("-1", out.f);
            std::fprintf(out.f, "\t%u\t%u\t%u", p.matches, p.seed_pos, p.seed_len);
            if (o.use_doc) std::fprintf(out.f, "\t%lld", p.doc == SPP_NO_DOC ? -1ll : (long long)p.doc);
            std::fputc('\n', out.f);
            num_placed += is_placed;
            num_reads++;
        });
    std::fprintf(stderr, "[place] %llu reads, %llu placed, %llu unplaced (%.3f sec). results are saved in *.placements\n",
                 (unsigned long long)num_reads, (unsigned long long)num_placed, (unsigned long long)(num_reads - num_placed),
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - run.t_start).count());
    return 0;
}
