// call_vcf_check.cpp -- the host code that formats `spumoni call`'s file (spumoni_amd/csrc/host/call_vcf.hpp) as a
// stand-alone program: a handful of records through write_vcf_header and write_vcf_calls into the file named on the
// command line.  tests/test_call_cpu.py builds it with the address and undefined-behaviour sanitizers and compares the file.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../spumoni_amd/csrc/host/call_vcf.hpp"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 2;
    const std::vector<std::string> names = {"one", "a name with spaces", "three"};
    const std::vector<uint64_t> lengths = {5, 1, 18446744073709551615ull};
    std::vector<spl_call> calls(5);
    std::memset(calls.data(), 0, calls.size() * sizeof(spl_call));
    auto set = [&](size_t i, uint64_t pos, uint32_t seq, uint32_t depth, uint32_t a, uint32_t c, uint32_t g, uint32_t t, uint32_t other,
                   uint32_t del, uint32_t ins, char ref, uint8_t allele) {
        spl_call& r = calls[i];
        r.pos = pos;
        r.seq = seq;
        r.depth = depth;
        r.alt[0] = a;
        r.alt[1] = c;
        r.alt[2] = g;
        r.alt[3] = t;
        r.other = other;
        r.del = del;
        r.ins = ins;
        r.ref = (uint8_t)ref;
        r.allele = allele;
    };
    set(0, 0, 0, 7, 0, 4, 1, 0, 1, 2, 3, 'A', 1);
    set(1, 4, 0, 2, 0, 0, 0, 2, 0, 0, 0, 'c', 3);
    set(2, 0, 1, 4294967295u, 4294967295u, 0, 0, 0, 0, 0, 0, 'N', 0);                         // every count at its largest
    set(3, 18446744073709551614ull, 2, 9, 1, 2, 3, 0, 4294967295u, 4294967295u, 4294967295u, 'T', 2);  // the last position there is
    set(4, 10, 2, 3, 3, 0, 0, 0, 0, 0, 0, 'G', 0);
    const std::vector<uint32_t> mism = {6, 2, 4294967295u, 6, 5};  // (the last one above its depth: the difference wraps as the arrays do)
    spumoni_host::write_vcf_header(f, names, lengths);
    if (!spumoni_host::write_vcf_calls(f, names, calls.data(), mism.data(), calls.size())) return 1;
    if (!spumoni_host::write_vcf_calls(f, names, calls.data(), mism.data(), 0)) return 1;  // no records: nothing is read
    // a record outside the table, and a letter outside 0 .. 3, stop the writer in front of the line
    calls[1].seq = 3;
    if (spumoni_host::write_vcf_calls(f, names, calls.data() + 1, mism.data() + 1, 1)) return 1;
    calls[1].seq = 0;
    calls[1].allele = 4;
    if (spumoni_host::write_vcf_calls(f, names, calls.data() + 1, mism.data() + 1, 1)) return 1;
    if (std::fclose(f) != 0) return 2;
    std::printf("call vcf ok\n");
    return 0;
}
