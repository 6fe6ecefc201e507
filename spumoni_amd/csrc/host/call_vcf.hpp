// call_vcf.hpp -- the lines of `spumoni call`'s <reads>.vcf from the call records: plain host code with no device behind
// it, so that it can be built into a stand-alone program and run under a sanitizer (tools/README.md).
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../../include/spumoni_call.h"

namespace spumoni_host {

// The header: the format, one contig line per sequence in table order, one INFO line per key, the column names.
inline void write_vcf_header(FILE* f, const std::vector<std::string>& names, const std::vector<uint64_t>& lengths) {
    std::fprintf(f, "##fileformat=VCFv4.2\n");
    for (size_t s = 0; s < names.size(); ++s)
        std::fprintf(f, "##contig=<ID=%s,length=%llu>\n", names[s].c_str(), (unsigned long long)lengths[s]);
    std::fprintf(f, "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Reads that cover the base with an = or X column\">\n");
    std::fprintf(f, "##INFO=<ID=AD,Number=2,Type=Integer,Description=\"Reads that match the reference, reads that carry the called allele\">\n");
    std::fprintf(f, "##INFO=<ID=BC,Number=4,Type=Integer,Description=\"Mismatching reads by letter: A, C, G, T\">\n");
    std::fprintf(f, "##INFO=<ID=OT,Number=1,Type=Integer,Description=\"Mismatching reads with a byte outside ACGT\">\n");
    std::fprintf(f, "##INFO=<ID=DL,Number=1,Type=Integer,Description=\"Reads that delete the base\">\n");
    std::fprintf(f, "##INFO=<ID=IN,Number=1,Type=Integer,Description=\"Insertions in front of the base\">\n");
    std::fprintf(f, "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n");
}

// One line per call; mism[i] is the coverage's mismatch count at call i's base (ref_count = depth - mism, modulo 2^32 as
// the arrays are).  False, with nothing more written, when a record names a sequence outside the table or an allele
// outside 0 .. 3.
inline bool write_vcf_calls(FILE* f, const std::vector<std::string>& names, const spl_call* calls, const uint32_t* mism, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) {
        const spl_call& c = calls[i];
        if (c.seq >= names.size() || c.allele > 3) return false;
        std::fprintf(f, "%s\t%llu\t.\t%c\t%c\t.\t.\tDP=%u;AD=%u,%u;BC=%u,%u,%u,%u;OT=%u;DL=%u;IN=%u\n", names[c.seq].c_str(),
                     (unsigned long long)c.pos + 1, (char)c.ref, "ACGT"[c.allele], c.depth, (uint32_t)(c.depth - mism[i]), c.alt[c.allele],
                     c.alt[0], c.alt[1], c.alt[2], c.alt[3], c.other, c.del, c.ins);
    }
    return true;
}

}  // namespace spumoni_host
