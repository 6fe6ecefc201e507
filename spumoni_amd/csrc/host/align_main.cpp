// align_main.cpp -- `spumoni align`: one line per read -- the read aligned along the best collinear chain of its matches
// with the text, every gap between two anchors filled by an exact edit-distance table: where the alignment starts and
// ends in the read and on the reference, its matches and edits (include/spumoni_align.h has the rule).  The reads come
// from reads.cpp (same ids, same FASTA / FASTQ quirks as `run`), the MS index through the loaders `run` uses, and
// super-batches of SPUMONI_SUPER_BATCH characters go through spa_align_batch: digestion, walk, extension, the matches,
// the chaining and the gaps stay on the device and 48 bytes per read come back.  The driver is read_command.cpp; a run
// that fails leaves no file.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../../include/spumoni_align.h"
#include "read_command.hpp"

using namespace spumoni_host;

namespace {

int spumoni_align_usage() {
    std::fprintf(stderr, "spumoni align - Uses a spumoni MS index to align each read along the best chain of its matches with the reference.\n");
    std::fprintf(stderr, "Usage: spumoni align [options]\n\n");
    std::fprintf(stderr, "Options:\n");
    std::fprintf(stderr, "\t%-35sprints this usage message\n", "-h, --help");
    std::fprintf(stderr, "\t%-25s%-10soutput prefix used for index\n", "-r, --ref", "[FILE]");
    std::fprintf(stderr, "\t%-25s%-10spath to patterns file that will be used.\n", "-p, --pattern", "[FILE]");
    std::fprintf(stderr, "\t%-25s%-10sturn off minimizer digestion of reads (default: on)\n", "-n, --no-digest", "");
    std::fprintf(stderr, "\t%-25s%-10suse alphabet-promoted minimizers\n", "-m, --minimizer-alphabet", "");
    std::fprintf(stderr, "\t%-25s%-10suse DNA-letter based minimizers\n", "-a, --dna-minimizer", "");
    std::fprintf(stderr, "\t%-25s%-10ssmall window size (k) for finding minimizers (default: 4)\n", "-K, --small-window", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10slarge window size (w) for finding minimizers (default: 11)\n", "-W, --large-window", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10suse document array: matches chain within one document, and the alignment names it\n", "-d, --doc-array", "");
    std::fprintf(stderr, "\t%-25s%-10sa match is an anchor when it is at least this long, 1 or more (default: the\n", "-L, --min-length", "[INT]");
    std::fprintf(stderr, "\t%-35sMS threshold `run -c` classifies with, from the null database)\n", "");
    std::fprintf(stderr, "\t%-25s%-10slargest distance between two chained anchors in the read and in the text,\n", "-S, --max-dist", "[INT]");
    std::fprintf(stderr, "\t%-35s1 .. 2147483647 (default: 5000)\n", "");
    std::fprintf(stderr, "\t%-25s%-10slargest difference of those two distances, 0 .. 2147483647 (default: 500)\n", "-G, --max-gap", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10swhat a unit of that difference costs, 0 .. 65535 (default: 1)\n", "-B, --gap-penalty", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10spredecessors an anchor looks back at, 1 .. 64 (default: 64)\n", "-H, --lookback", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10sa gap between two anchors is filled when neither side is longer, 1 .. 4096\n", "-F, --max-fill", "[INT]");
    std::fprintf(stderr, "\t%-35s(default: 512)\n\n", "");
    std::fprintf(stderr, "Matching statistics (-M) are implied. Writes <pattern>.alignments: id, values, read_start, read_end, ref_start,\n");
    std::fprintf(stderr, "ref_end, matches, edits, anchors, unfilled, skipped[, doc] per read, positions in the (digested) read and text; a\n");
    std::fprintf(stderr, "read without a match has -1 for ref_start (and doc) and zeros elsewhere.\n\n");
    return 1;
}

}  // namespace

int align_main(int argc, char** argv) {
    if (argc == 1) return spumoni_align_usage();
    ReadOptions o;
    MapOptions m(MapOptions::FILL);
    parse_read_options(argc, argv, o, spumoni_align_usage, true, m.shorts().c_str(), m.longs(),
                       [&](int c, const char* arg) { m.set(o, c, arg); });
    require_ref_and_pattern(o);
    imply_ms(o, "align");
    validate_read_options(o);
    m.validate(o);
    o.ref_file += o.use_promotions ? ".bin" : ".fa";
    auto align_batch = reinterpret_cast<decltype(&spa_align_batch)>(
        device_entry_points("align", {"spa_align_batch"}, "the align kernels")[0]);
    ReadRun run;
    open_read_run(o, 8u << 20, run);
    run.super_batch = std::min<size_t>(run.super_batch, 32u << 20);  // (one piece per spa_align_batch)
    const uint64_t min_length = m.min_length(o);
    const spc_params params = m.chain();
    const spa_params fill = m.fill();
    std::fprintf(stderr, "[align] index loaded (n = %llu, r = %llu); %s\n",
                 (unsigned long long)run.set.n, (unsigned long long)run.set.r, m.describe(min_length).c_str());

    LinesFile out;
    out.open(o.pattern_file + ".alignments", false);
    uint64_t num_reads = 0, num_aligned = 0;
    std::vector<spa_alignment> recs;
    scan_reads(
        run, out,
        [&](ReadBatch& b) {
            recs.resize(b.take + 1);
            for_each_piece(b, [&](size_t q0, size_t q1) {
                if (align_batch(run.ix, run.digest_kind, (uint32_t)o.k, (uint32_t)o.w, b.seqs.data(), b.offs.data() + q0, q1 - q0,
                                min_length, o.use_doc ? 1 : 0, &params, &fill, recs.data() + q0, nullptr,
                                b.values.data() + q0) != SPX_OK)
                    fatal_error("%s", spx_last_error());
            });
        },
        [&](const ReadBatch& b, size_t i) {
            const spa_alignment& c = recs[i];
            const bool aligned = c.ref_start != SPA_UNALIGNED;
            std::fwrite(b.recs[i].id, 1, b.recs[i].id_len, out.f);
            std::fprintf(out.f, "\t%llu\t%u\t%u\t", (unsigned long long)b.values[i], c.read_start, c.read_end);
            if (aligned)
                std::fprintf(out.f, "%llu", (unsigned long long)c.ref_start);
            else
                std::fputs("-1", out.f);
            std::fprintf(out.f, "\t%llu\t%u\t%u\t%u\t%u\t%u", (unsigned long long)c.ref_end, c.matches, c.edits, c.anchors, c.unfilled,
                         c.skipped);
            if (o.use_doc) std::fprintf(out.f, "\t%lld", c.doc == SPC_NO_DOC ? -1ll : (long long)c.doc);
            std::fputc('\n', out.f);
            num_aligned += aligned;
            num_reads++;
        });
    std::fprintf(stderr, "[align] %llu reads, %llu aligned, %llu without a match (%.3f sec). results are saved in *.alignments\n",
                 (unsigned long long)num_reads, (unsigned long long)num_aligned, (unsigned long long)(num_reads - num_aligned),
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - run.t_start).count());
    return 0;
}
