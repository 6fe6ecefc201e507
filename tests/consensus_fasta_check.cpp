// consensus_fasta_check.cpp -- the host code that writes `spumoni consensus`'s two files
// (spumoni_amd/csrc/host/consensus_fasta.hpp) as a stand-alone program: three sequences, the middle one without letters,
// through write_consensus_fasta and write_consensus_tsv into the files named on the command line.
// tests/test_consensus_cpu.py builds it with the address and undefined-behaviour sanitizers and compares the files.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../spumoni_amd/csrc/host/consensus_fasta.hpp"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fa = std::fopen(argv[1], "wb");
    FILE* tsv = std::fopen(argv[2], "wb");
    if (!fa || !tsv) return 2;
    const std::vector<std::string> names = {"one", "a name with spaces", "three"};
    const std::vector<uint64_t> lengths = {5, 1, 18446744073709551615ull};
    const uint64_t top = 18446744073709551615ull;
    // exactly the body's bytes on the heap: a read beyond them is the sanitizer's to report
    const char text[] = "ACG\nT\nnn\n";
    std::vector<uint8_t> body(text, text + 9);
    std::vector<sps_seq> records(3);
    std::memset(records.data(), 0, records.size() * sizeof(sps_seq));
    auto set = [&](size_t i, uint64_t start, uint64_t letters, uint64_t sub, uint64_t del, uint64_t masked, uint64_t ins) {
        records[i].body_start = start;
        records[i].letters = letters;
        records[i].substituted = sub;
        records[i].deleted = del;
        records[i].masked = masked;
        records[i].ins_sites = ins;
    };
    set(0, 0, 4, 1, 1, 0, 2);
    set(1, 6, 0, 0, 1, 0, 0);
    set(2, 6, 2, top, top, 2, top);  // every count that the body does not bound at its largest
    if (!spumoni_host::write_consensus_fasta(fa, names, records.data(), body.data(), body.size())) return 1;
    spumoni_host::write_consensus_tsv(tsv, names, lengths, records.data());
    // records that do not describe the body stop the writer in front of the first byte: a start that is not where the
    // sequence before ended, a start beyond the body, more letters than bytes, letters without bytes, bytes without
    // letters, a body longer than the records say
    auto refused = [&](size_t i, uint64_t start, uint64_t letters, uint64_t bytes) {
        const sps_seq keep = records[i];
        records[i].body_start = start;
        records[i].letters = letters;
        const bool ok = spumoni_host::write_consensus_fasta(fa, names, records.data(), body.data(), bytes);
        records[i] = keep;
        return !ok;
    };
    if (!refused(1, 5, 0, 9) || !refused(2, 10, 2, 9) || !refused(2, top, 2, 9) || !refused(0, 0, 6, 9) || !refused(1, 6, 1, 9) ||
        !refused(0, 0, 0, 9) || !refused(0, 0, 4, 8) || !refused(0, 1, 4, 9))
        return 1;
    // no sequences and no bytes: nothing is read
    if (!spumoni_host::write_consensus_fasta(fa, {}, nullptr, nullptr, 0)) return 1;
    if (spumoni_host::write_consensus_fasta(fa, {}, nullptr, nullptr, 1)) return 1;
    if (std::fclose(fa) != 0 || std::fclose(tsv) != 0) return 2;
    std::printf("consensus fasta ok\n");
    return 0;
}
