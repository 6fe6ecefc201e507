// consensus_fasta.hpp -- the two files of `spumoni consensus` from the records and the body: plain host code with no device
// behind it, so that it can be built into a stand-alone program and run under a sanitizer (tools/README.md).
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../../include/spumoni_consensus.h"

namespace spumoni_host {

// The records describe the body: every sequence's bytes start where the one before ended, hold its letters and at least
// one newline when there are letters, and the last one ends the body.  Checked before anything is written.
inline bool consensus_records_fit(const sps_seq* records, size_t n_seqs, uint64_t body_bytes) {
    uint64_t at = 0;
    for (size_t s = 0; s < n_seqs; ++s) {
        if (records[s].body_start != at) return false;
        const uint64_t end = s + 1 < n_seqs ? records[s + 1].body_start : body_bytes;
        if (end < at || end > body_bytes) return false;
        if (records[s].letters ? end - at <= records[s].letters : end != at) return false;
        at = end;
    }
    return at == body_bytes;
}

// <reads>.consensus.fa: `>name` and the sequence's slice of the body; a sequence with no letters gets its header only.
// False, with nothing written, when the records do not fit the body.
inline bool write_consensus_fasta(FILE* f, const std::vector<std::string>& names, const sps_seq* records, const uint8_t* body,
                                  uint64_t body_bytes) {
    if (!consensus_records_fit(records, names.size(), body_bytes)) return false;
    for (size_t s = 0; s < names.size(); ++s) {
        const uint64_t at = records[s].body_start, end = s + 1 < names.size() ? records[s + 1].body_start : body_bytes;
        std::fprintf(f, ">%s\n", names[s].c_str());
        if (end > at) std::fwrite(body + at, 1, end - at, f);
    }
    return true;
}

// <reads>.consensus.tsv: name, length, letters, substituted, deleted, masked, insertion sites per sequence
inline void write_consensus_tsv(FILE* f, const std::vector<std::string>& names, const std::vector<uint64_t>& lengths, const sps_seq* records) {
    for (size_t s = 0; s < names.size(); ++s)
        std::fprintf(f, "%s\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\n", names[s].c_str(), (unsigned long long)lengths[s],
                     (unsigned long long)records[s].letters, (unsigned long long)records[s].substituted,
                     (unsigned long long)records[s].deleted, (unsigned long long)records[s].masked,
                     (unsigned long long)records[s].ins_sites);
}

}  // namespace spumoni_host
