// extend_main.cpp -- `spumoni extend`: one line per read -- `spumoni cigar`'s columns with the alignment taken to the
// read's ends: both ends of the chain extended by a banded dynamic programme, the spans, matches and edits with the
// extensions in them, and what is left of the read on either side as soft clips (S), so that the CIGAR accounts for every
// read character (include/spumoni_extend.h has the rule).  The reads come from reads.cpp (same ids, same FASTA / FASTQ
// quirks as `run`), the MS index through the loaders `run` uses, and super-batches of SPUMONI_SUPER_BATCH characters go
// through spe_extend_begin / spe_extend_fetch in calls of one piece each.  The driver is read_command.cpp; a run that
// fails leaves no file.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../../include/spumoni_extend.h"
#include "cigar_text.hpp"
#include "read_command.hpp"

using namespace spumoni_host;

namespace {

int spumoni_extend_usage() {
    std::fprintf(stderr, "spumoni extend - Uses a spumoni MS index to align each read along the best chain of its matches with the reference, extends the alignment to the read's ends and reports it as a CIGAR with soft clips.\n");
    std::fprintf(stderr, "Usage: spumoni extend [options]\n\n");
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
    std::fprintf(stderr, "\t%-35s(default: 512)\n", "");
    std::fprintf(stderr, "\t%-25s%-10slargest end side that is extended, 1 .. 4096 (default: 512)\n", "-E, --max-extend", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10show far an extension may drift off the diagonal, 0 .. 63 (default: 16)\n", "-O, --band", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10swhat an unequal column of an extension costs, 0 .. 65535 (default: 4)\n", "-N, --mismatch", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10swhat an inserted or deleted character of an extension costs, 0 .. 65535\n", "-I, --indel", "[INT]");
    std::fprintf(stderr, "\t%-35s(default: 6); an equal column scores 1\n\n", "");
    std::fprintf(stderr, "Matching statistics (-M) are implied. Writes <pattern>.extended: id, values, read_start, read_end, ref_start,\n");
    std::fprintf(stderr, "ref_end, matches, edits, anchors, unfilled, skipped[, doc], length and the CIGAR per read, positions in the\n");
    std::fprintf(stderr, "(digested) read and text; length is the read's length in values, so that a line can be checked on its own: the\n");
    std::fprintf(stderr, "CIGAR's = X I and S add up to it. The operations are = X I D, N for the text side of a gap that is not filled, and\n");
    std::fprintf(stderr, "S for the read characters outside the alignment; a run is at most 268435455 long and a longer one is printed as\n");
    std::fprintf(stderr, "several. A read without a match has -1 for ref_start (and doc), zeros elsewhere and * for the CIGAR.\n\n");
    return 1;
}

}  // namespace

int extend_main(int argc, char** argv) {
    if (argc == 1) return spumoni_extend_usage();
    ReadOptions o;
    MapOptions m(MapOptions::EXTEND);
    parse_read_options(argc, argv, o, spumoni_extend_usage, true, m.shorts().c_str(), m.longs(),
                       [&](int c, const char* arg) { m.set(o, c, arg); });
    require_ref_and_pattern(o);
    imply_ms(o, "extend");
    validate_read_options(o);
    m.validate(o);
    o.ref_file += o.use_promotions ? ".bin" : ".fa";
    const std::vector<void*> entry = device_entry_points("extend", {"spe_extend_begin", "spe_extend_fetch"}, "the extend kernels");
    auto extend_begin = reinterpret_cast<decltype(&spe_extend_begin)>(entry[0]);
    auto extend_fetch = reinterpret_cast<decltype(&spe_extend_fetch)>(entry[1]);
    ReadRun run;
    open_read_run(o, 8u << 20, run);
    run.super_batch = std::min<size_t>(run.super_batch, 32u << 20);  // (one piece per spe_extend_begin)
    const uint64_t min_length = m.min_length(o);
    const spc_params params = m.chain();
    const spa_params fill = m.fill();
    const spe_params ends = m.ends();
    std::fprintf(stderr, "[extend] index loaded (n = %llu, r = %llu); %s\n",
                 (unsigned long long)run.set.n, (unsigned long long)run.set.r, m.describe(min_length).c_str());

    LinesFile out;
    out.open(o.pattern_file + ".extended", false);
    uint64_t num_reads = 0, num_aligned = 0, num_entries = 0, num_clipped = 0;
    std::vector<spa_alignment> recs;
    BatchEntries entries;
    scan_reads(
        run, out,
        [&](ReadBatch& b) {
            recs.resize(b.take + 1);
            entries.start(b.take);
            for_each_piece(b, [&](size_t q0, size_t q1) {
                if (!entries.piece(
                        q0, q1,
                        [&](uint64_t* n) {
                            return extend_begin(run.ix, run.digest_kind, (uint32_t)o.k, (uint32_t)o.w, b.seqs.data(), b.offs.data() + q0,
                                                q1 - q0, min_length, o.use_doc ? 1 : 0, &params, &fill, &ends, recs.data() + q0, nullptr,
                                                b.values.data() + q0, nullptr, n);
                        },
                        [&](uint64_t* offs, uint32_t* ops) { return extend_fetch(run.ix, offs, ops); }))
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
            std::fprintf(out.f, "\t%llu\t", (unsigned long long)b.values[i]);
            write_cigar(out.f, entries, i, false, true);
            std::fputc('\n', out.f);
            for (uint64_t e = entries.op_offs[i]; e < entries.op_offs[i + 1]; ++e)
                if ((entries.ops[e] & 15) == SPE_OP_S) num_clipped += entries.ops[e] >> 4;
            num_entries += entries.op_offs[i + 1] - entries.op_offs[i];
            num_aligned += aligned;
            num_reads++;
        });
    std::fprintf(stderr, "[extend] %llu reads, %llu aligned, %llu without a match, %llu CIGAR entries, %llu characters clipped (%.3f sec). "
                 "results are saved in *.extended\n",
                 (unsigned long long)num_reads, (unsigned long long)num_aligned, (unsigned long long)(num_reads - num_aligned),
                 (unsigned long long)num_entries, (unsigned long long)num_clipped,
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - run.t_start).count());
    return 0;
}
