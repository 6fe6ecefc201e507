// chain_main.cpp -- `spumoni chain`: one line per read -- the best collinear chain of its matches with the text, where it
// starts and ends in the read and on the reference, its score and the gaps it bridges (include/spumoni_chain.h has the
// rule).  The reads come from reads.cpp (same ids, same FASTA / FASTQ quirks as `run`), the MS index through the loaders
// `run` uses, and super-batches of SPUMONI_SUPER_BATCH characters go through spc_chain_batch: digestion, walk, extension,
// the matches and the chaining stay on the device and 48 bytes per read come back.  The driver is read_command.cpp; a
// run that fails leaves no file.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../../include/spumoni_chain.h"
#include "read_command.hpp"

using namespace spumoni_host;

namespace {

int spumoni_chain_usage() {
    std::fprintf(stderr, "spumoni chain - Uses a spumoni MS index to chain each read's matches with the reference: the best collinear chain per read.\n");
    std::fprintf(stderr, "Usage: spumoni chain [options]\n\n");
    std::fprintf(stderr, "Options:\n");
    std::fprintf(stderr, "\t%-35sprints this usage message\n", "-h, --help");
    std::fprintf(stderr, "\t%-25s%-10soutput prefix used for index\n", "-r, --ref", "[FILE]");
    std::fprintf(stderr, "\t%-25s%-10spath to patterns file that will be used.\n", "-p, --pattern", "[FILE]");
    std::fprintf(stderr, "\t%-25s%-10sturn off minimizer digestion of reads (default: on)\n", "-n, --no-digest", "");
    std::fprintf(stderr, "\t%-25s%-10suse alphabet-promoted minimizers\n", "-m, --minimizer-alphabet", "");
    std::fprintf(stderr, "\t%-25s%-10suse DNA-letter based minimizers\n", "-a, --dna-minimizer", "");
    std::fprintf(stderr, "\t%-25s%-10ssmall window size (k) for finding minimizers (default: 4)\n", "-K, --small-window", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10slarge window size (w) for finding minimizers (default: 11)\n", "-W, --large-window", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10suse document array: matches chain within one document, and the chain names it\n", "-d, --doc-array", "");
    std::fprintf(stderr, "\t%-25s%-10sa match is an anchor when it is at least this long, 1 or more (default: the\n", "-L, --min-length", "[INT]");
    std::fprintf(stderr, "\t%-35sMS threshold `run -c` classifies with, from the null database)\n", "");
    std::fprintf(stderr, "\t%-25s%-10slargest distance between two chained anchors in the read and in the text,\n", "-S, --max-dist", "[INT]");
    std::fprintf(stderr, "\t%-35s1 .. 2147483647 (default: 5000)\n", "");
    std::fprintf(stderr, "\t%-25s%-10slargest difference of those two distances, 0 .. 2147483647 (default: 500)\n", "-G, --max-gap", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10swhat a unit of that difference costs, 0 .. 65535 (default: 1)\n", "-B, --gap-penalty", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10spredecessors an anchor looks back at, 1 .. 64 (default: 64)\n\n", "-H, --lookback", "[INT]");
    std::fprintf(stderr, "Matching statistics (-M) are implied. Writes <pattern>.chains: id, values, score, anchors, read_start, read_end,\n");
    std::fprintf(stderr, "ref_start, ref_end, gap[, doc] per read, positions in the (digested) read and text; a read without a match has -1\n");
    std::fprintf(stderr, "for ref_start (and doc) and zeros elsewhere.\n\n");
    return 1;
}

}  // namespace

int chain_main(int argc, char** argv) {
    if (argc == 1) return spumoni_chain_usage();
    ReadOptions o;
    MapOptions m(MapOptions::CHAIN);
    parse_read_options(argc, argv, o, spumoni_chain_usage, true, m.shorts().c_str(), m.longs(),
                       [&](int c, const char* arg) { m.set(o, c, arg); });
    require_ref_and_pattern(o);
    imply_ms(o, "chain");
    validate_read_options(o);
    m.validate(o);
    o.ref_file += o.use_promotions ? ".bin" : ".fa";
    auto chain_batch = reinterpret_cast<decltype(&spc_chain_batch)>(
        device_entry_points("chain", {"spc_chain_batch"}, "the chain kernel")[0]);
    ReadRun run;
    open_read_run(o, 8u << 20, run);
    run.super_batch = std::min<size_t>(run.super_batch, 32u << 20);  // (one piece per spc_chain_batch)
    const uint64_t min_length = m.min_length(o);
    const spc_params params = m.chain();
    std::fprintf(stderr, "[chain] index loaded (n = %llu, r = %llu); %s\n",
                 (unsigned long long)run.set.n, (unsigned long long)run.set.r, m.describe(min_length).c_str());

    LinesFile out;
    out.open(o.pattern_file + ".chains", false);
    uint64_t num_reads = 0, num_chained = 0;
    std::vector<spc_chain> chains;
    scan_reads(
        run, out,
        [&](ReadBatch& b) {
            chains.resize(b.take + 1);
            for_each_piece(b, [&](size_t q0, size_t q1) {
                if (chain_batch(run.ix, run.digest_kind, (uint32_t)o.k, (uint32_t)o.w, b.seqs.data(), b.offs.data() + q0, q1 - q0,
                                min_length, o.use_doc ? 1 : 0, &params, chains.data() + q0, b.values.data() + q0) != SPX_OK)
                    fatal_error("%s", spx_last_error());
            });
        },
        [&](const ReadBatch& b, size_t i) {
            const spc_chain& c = chains[i];
            const bool chained = c.ref_start != SPC_UNCHAINED;
            std::fwrite(b.recs[i].id, 1, b.recs[i].id_len, out.f);
            std::fprintf(out.f, "\t%llu\t%u\t%u\t%u\t%u\t", (unsigned long long)b.values[i], c.score, c.anchors, c.read_start, c.read_end);
            if (chained)
                std::fprintf(out.f, "%llu", (unsigned long long)c.ref_start);
            else
                std::fputs("-1", out.f);
            std::fprintf(out.f, "\t%llu\t%u", (unsigned long long)c.ref_end, c.gap);
            if (o.use_doc) std::fprintf(out.f, "\t%lld", c.doc == SPC_NO_DOC ? -1ll : (long long)c.doc);
            std::fputc('\n', out.f);
            num_chained += chained;
            num_reads++;
        });
    std::fprintf(stderr, "[chain] %llu reads, %llu chained, %llu without a match (%.3f sec). results are saved in *.chains\n",
                 (unsigned long long)num_reads, (unsigned long long)num_chained, (unsigned long long)(num_reads - num_chained),
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - run.t_start).count());
    return 0;
}
