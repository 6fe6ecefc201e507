// mems_main.cpp -- `spumoni mems`: one line per match of a read with the text -- where a new exact match starts and is
// at least -L long (include/spumoni_mems.h has the rule).  The reads come from reads.cpp (same ids, same FASTA / FASTQ
// quirks as `run`), the MS index through the loaders `run` uses, and super-batches of SPUMONI_SUPER_BATCH characters go
// through spm_mems_begin / spm_mems_fetch: digestion, walk, extension and the reduction stay on the device and 16 bytes
// per match come back.  The driver is read_command.cpp; a run that fails leaves no file.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../../include/spumoni_mems.h"
#include "read_command.hpp"

using namespace spumoni_host;

namespace {

int spumoni_mems_usage() {
    std::fprintf(stderr, "spumoni mems - Uses a spumoni MS index to report each read's maximal exact matches with the reference.\n");
    std::fprintf(stderr, "Usage: spumoni mems [options]\n\n");
    std::fprintf(stderr, "Options:\n");
    std::fprintf(stderr, "\t%-35sprints this usage message\n", "-h, --help");
    std::fprintf(stderr, "\t%-25s%-10soutput prefix used for index\n", "-r, --ref", "[FILE]");
    std::fprintf(stderr, "\t%-25s%-10spath to patterns file that will be used.\n", "-p, --pattern", "[FILE]");
    std::fprintf(stderr, "\t%-25s%-10sturn off minimizer digestion of reads (default: on)\n", "-n, --no-digest", "");
    std::fprintf(stderr, "\t%-25s%-10suse alphabet-promoted minimizers\n", "-m, --minimizer-alphabet", "");
    std::fprintf(stderr, "\t%-25s%-10suse DNA-letter based minimizers\n", "-a, --dna-minimizer", "");
    std::fprintf(stderr, "\t%-25s%-10ssmall window size (k) for finding minimizers (default: 4)\n", "-K, --small-window", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10slarge window size (w) for finding minimizers (default: 11)\n", "-W, --large-window", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10suse document array to name each match's document\n", "-d, --doc-array", "");
    std::fprintf(stderr, "\t%-25s%-10sa match is reported when it is at least this long (default: the\n", "-L, --min-length", "[INT]");
    std::fprintf(stderr, "\t%-35sMS threshold `run -c` classifies with, from the null database)\n\n", "");
    std::fprintf(stderr, "Matching statistics (-M) are implied. Writes <pattern>.mems: id, read_pos, length, ref_pos[, doc]\n");
    std::fprintf(stderr, "per match, positions in the (digested) read and text; reads without a match write nothing.\n\n");
    return 1;
}

}  // namespace

int mems_main(int argc, char** argv) {
    if (argc == 1) return spumoni_mems_usage();
    ReadOptions o;
    parse_read_options(argc, argv, o, spumoni_mems_usage, true, "L:", {{"min-length", required_argument, NULL, 'L'}},
                       [&](int, const char* arg) {
                           o.have_threshold = true;
                           o.threshold = std::strtoull(arg, nullptr, 10);
                       });
    require_ref_and_pattern(o);
    if (o.pml_requested)
        fatal_warning("-P cannot be used with `spumoni mems`: matches are read off matching statistics (-M is implied); "
                      "PMLs have no pointers.");
    o.ms = true;
    validate_read_options(o);
    if (o.have_threshold && o.threshold == 0) fatal_warning("the minimum match length (-L) must be at least 1.");
    o.ref_file += o.use_promotions ? ".bin" : ".fa";
    const std::vector<void*> fn = device_entry_points("mems", {"spm_mems_begin", "spm_mems_fetch"}, "the match kernels");
    auto mems_begin = reinterpret_cast<decltype(&spm_mems_begin)>(fn[0]);
    auto mems_fetch = reinterpret_cast<decltype(&spm_mems_fetch)>(fn[1]);
    ReadRun run;
    open_read_run(o, 8u << 20, run);
    run.super_batch = std::min<size_t>(run.super_batch, 32u << 20);  // (one piece per spm_mems_begin)
    const uint64_t min_length = o.have_threshold ? o.threshold : std::max<uint64_t>(1, null_db_threshold(o));
    std::fprintf(stderr, "[mems] index loaded (n = %llu, r = %llu); a match is reported from length %llu on\n", (unsigned long long)run.set.n,
                 (unsigned long long)run.set.r, (unsigned long long)min_length);

    LinesFile out;
    out.open(o.pattern_file + ".mems", false);
    uint64_t num_reads = 0, num_matches = 0, without = 0;
    std::vector<uint64_t> moffs;
    std::vector<spm_match> matches;
    std::vector<uint32_t> docs;
    scan_reads(
        run, out,
        [&](ReadBatch& b) {
            moffs.resize(b.take + 1);
            uint64_t n = 0;
            if (mems_begin(run.ix, run.digest_kind, (uint32_t)o.k, (uint32_t)o.w, b.seqs.data(), b.offs.data(), b.take, min_length,
                           o.use_doc ? 1 : 0, moffs.data(), b.values.data(), &n) != SPX_OK)
                fatal_error("%s", spx_last_error());
            matches.resize(n + 1);
            docs.resize(n + 1);
            if (mems_fetch(run.ix, matches.data(), o.use_doc ? docs.data() : nullptr) != SPX_OK) fatal_error("%s", spx_last_error());
        },
        [&](const ReadBatch& b, size_t i) {
            for (uint64_t j = moffs[i]; j < moffs[i + 1]; ++j) {
                const spm_match& m = matches[j];
                std::fwrite(b.recs[i].id, 1, b.recs[i].id_len, out.f);
                if (o.use_doc)
                    std::fprintf(out.f, "\t%u\t%u\t%llu\t%u\n", m.read_pos, m.length, (unsigned long long)m.ref_pos, docs[j]);
                else
                    std::fprintf(out.f, "\t%u\t%u\t%llu\n", m.read_pos, m.length, (unsigned long long)m.ref_pos);
            }
            num_matches += moffs[i + 1] - moffs[i];
            without += moffs[i + 1] == moffs[i];
            num_reads++;
        });
    std::fprintf(stderr, "[mems] %llu reads, %llu matches, %llu reads without a match (%.3f sec). results are saved in *.mems\n",
                 (unsigned long long)num_reads, (unsigned long long)num_matches, (unsigned long long)without,
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - run.t_start).count());
    return 0;
}
