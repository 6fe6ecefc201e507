// map_main.cpp -- `spumoni map`: one line of PAF per mapped read -- `spumoni extend`'s alignment in the coordinates of the
// sequence it lies on: which sequence, which strand, where in it, cut at the sequence's borders, and on the reverse strand
// turned round so that the CIGAR runs along the forward sequence (include/spumoni_map.h has the rule).  The sequences'
// names, lengths and strands come from <prefix>.fa.seqs, the table `spumoni build -s` writes; the reads from reads.cpp
// (same ids, same FASTA / FASTQ quirks as `run`), the MS index through the loaders `run` uses, and super-batches of
// SPUMONI_SUPER_BATCH characters go through spn_map_begin / spn_map_fetch in calls of one piece each.  The driver is
// read_command.cpp; a run that fails leaves no file.
#include <cstdio>
#include <vector>

#include "../../../include/spumoni_map.h"
#include "cigar_text.hpp"
#include "read_command.hpp"

using namespace spumoni_host;

namespace {

int spumoni_map_usage() {
    std::fprintf(stderr, "spumoni map - Uses a spumoni MS index and its sequence table to map each read: the extended alignment of `spumoni extend` by sequence name, strand and position in the sequence, as PAF.\n");
    std::fprintf(stderr, "Usage: spumoni map [options]\n\n");
    std::fprintf(stderr, "Options:\n");
    std::fprintf(stderr, "\t%-35sprints this usage message\n", "-h, --help");
    std::fprintf(stderr, "\t%-25s%-10soutput prefix used for index; <prefix>.fa.seqs must exist (spumoni build -n -s)\n", "-r, --ref", "[FILE]");
    std::fprintf(stderr, "\t%-25s%-10spath to patterns file that will be used.\n", "-p, --pattern", "[FILE]");
    std::fprintf(stderr, "\t%-25s%-10sno minimizer digestion of reads: required, digested coordinates cannot be turned back into bases\n", "-n, --no-digest", "");
    std::fprintf(stderr, "\t%-25s%-10srefused by `spumoni map`\n", "-m, --minimizer-alphabet", "");
    std::fprintf(stderr, "\t%-25s%-10srefused by `spumoni map`\n", "-a, --dna-minimizer", "");
    std::fprintf(stderr, "\t%-25s%-10ssmall window size (k) for finding minimizers (default: 4)\n", "-K, --small-window", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10slarge window size (w) for finding minimizers (default: 11)\n", "-W, --large-window", "[INT]");
    std::fprintf(stderr, "\t%-25s%-10suse document array: matches chain within one document, and the dc tag names it\n", "-d, --doc-array", "");
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
    std::fprintf(stderr, "Matching statistics (-M) are implied. Writes <pattern>.paf, one line per mapped read (a read without a mapping has\n");
    std::fprintf(stderr, "no line; their number is printed): id, length, read_start, read_end, strand (+ or -), sequence name, sequence\n");
    std::fprintf(stderr, "length, target_start, target_end, matches, block length and 255 for the mapping quality (one chain per read: none\n");
    std::fprintf(stderr, "is estimated), then NM:i: the edits (X + I + D), an:i: the anchors, ct:i: 1 when the alignment was cut at a sequence\n");
    std::fprintf(stderr, "border on the left in text order, 2 on the right, 3 both, dc:i: the document under -d, and cg:Z: the CIGAR\n");
    std::fprintf(stderr, "(= X I D N) along the sequence's forward strand. read_start and read_end are in the read as given, on either strand.\n\n");
    return 1;
}

}  // namespace

int map_main(int argc, char** argv) {
    if (argc == 1) return spumoni_map_usage();
    ReadOptions o;
    MapOptions m(MapOptions::EXTEND);
    parse_read_options(argc, argv, o, spumoni_map_usage, true, m.shorts().c_str(), m.longs(),
                       [&](int c, const char* arg) { m.set(o, c, arg); });
    require_ref_and_pattern(o);
    imply_ms(o, "map");
    require_bases(o, "map");
    validate_read_options(o);
    m.validate(o);
    TableRun run;
    open_table_run(o, m, "map", {"spn_set_sequences", "spn_map_begin", "spn_map_fetch"}, "the map kernels", nullptr, run);
    const SeqTable& table = run.table;
    auto map_begin = run.entry<decltype(&spn_map_begin)>("spn_map_begin");
    auto map_fetch = run.entry<decltype(&spn_map_fetch)>("spn_map_fetch");
    const spc_params params = m.chain();
    const spa_params fill = m.fill();
    const spe_params ends = m.ends();
    std::fprintf(stderr, "%s\n", run.loaded.c_str());

    LinesFile out;
    out.open(o.pattern_file + ".paf", false);
    uint64_t num_reads = 0, num_mapped = 0, num_cut = 0, num_reverse = 0;
    std::vector<spn_mapping> maps;
    std::vector<spa_alignment> recs;
    BatchEntries entries;
    scan_reads(
        run, out,
        [&](ReadBatch& b) {
            maps.resize(b.take + 1);
            recs.resize(b.take + 1);
            entries.start(b.take);
            for_each_piece(b, [&](size_t q0, size_t q1) {
                if (!entries.piece(
                        q0, q1,
                        [&](uint64_t* n) {
                            return map_begin(run.ix, 0, (uint32_t)o.k, (uint32_t)o.w, b.seqs.data(), b.offs.data() + q0, q1 - q0,
                                             run.min_length, o.use_doc ? 1 : 0, &params, &fill, &ends, maps.data() + q0, recs.data() + q0, n);
                        },
                        [&](uint64_t* offs, uint32_t* ops) { return map_fetch(run.ix, offs, ops); }))
                    fatal_error("%s", spx_last_error());
                // (without digestion a read's values are its characters)
                for (size_t q = q0; q < q1; ++q) b.values[q] = b.offs[q + 1] - b.offs[q];
            });
        },
        [&](const ReadBatch& b, size_t i) {
            num_reads++;
            const spn_mapping& m = maps[i];
            if (m.seq == SPN_UNMAPPED) return;
            const spa_alignment& c = recs[i];
            std::fwrite(b.recs[i].id, 1, b.recs[i].id_len, out.f);
            std::fprintf(out.f, "\t%llu\t%u\t%u\t%c\t%s\t%llu\t%llu\t%llu\t%u\t%u\t255\tNM:i:%u\tan:i:%u\tct:i:%u",
                         (unsigned long long)b.values[i], m.read_start, m.read_end, m.strand ? '-' : '+', table.names[m.seq].c_str(),
                         (unsigned long long)table.lengths[m.seq], (unsigned long long)m.target_start, (unsigned long long)m.target_end,
                         m.matches, m.block, m.edits, c.anchors, m.cut);
            if (o.use_doc) std::fprintf(out.f, "\tdc:i:%lld", c.doc == SPC_NO_DOC ? -1ll : (long long)c.doc);
            std::fputs("\tcg:Z:", out.f);
            write_cigar(out.f, entries, i, true, false);
            std::fputc('\n', out.f);
            num_mapped++;
            num_cut += m.cut != 0;
            num_reverse += m.strand;
        });
    std::fprintf(stderr, "[map] %llu reads, %llu mapped, %llu without a mapping, %llu cut at a sequence border, %llu on the reverse strand "
                 "(%.3f sec). results are saved in *.paf\n",
                 (unsigned long long)num_reads, (unsigned long long)num_mapped, (unsigned long long)(num_reads - num_mapped),
                 (unsigned long long)num_cut, (unsigned long long)num_reverse,
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - run.t_start).count());
    return 0;
}
