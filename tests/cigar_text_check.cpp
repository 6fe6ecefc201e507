// cigar_text_check.cpp -- the host code that gathers a super-batch's CIGAR entries and writes their text
// (spumoni_amd/csrc/host/cigar_text.hpp) as a stand-alone program: BatchEntries fed by begin / fetch callables that play the
// library, write_cigar into the file named on the command line, one CIGAR per line.  tests/test_cigar_cpu.py builds it with
// the address and undefined-behaviour sanitizers and compares the file.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../spumoni_amd/csrc/host/cigar_text.hpp"

namespace {

uint32_t E(uint32_t length, uint32_t op) { return length << 4 | op; }

// One piece as the library hands it over: per read its entries; the offsets count from the piece's first entry.
struct Piece {
    std::vector<std::vector<uint32_t>> reads;
    bool add_to(spumoni_host::BatchEntries& e, size_t q0, int begin_status = 0, int fetch_status = 0) const {
        uint64_t total = 0;
        for (const auto& r : reads) total += r.size();
        return e.piece(
            q0, q0 + reads.size(),
            [&](uint64_t* n) {
                *n = total;
                return begin_status;
            },
            [&](uint64_t* offs, uint32_t* ops) {
                uint64_t at = 0;
                for (size_t q = 0; q < reads.size(); ++q) {
                    offs[q] = at;
                    if (!reads[q].empty()) std::memcpy(ops + at, reads[q].data(), reads[q].size() * sizeof(uint32_t));
                    at += reads[q].size();
                }
                offs[reads.size()] = at;
                ops[at] = 0xdeadbeefu;  // (the slot behind the last entry is the fetch's to write)
                return fetch_status;
            });
    }
};

void lines(FILE* f, const spumoni_host::BatchEntries& e, size_t take, bool skip_clips, bool star_for_none) {
    for (size_t i = 0; i < take; ++i) {
        spumoni_host::write_cigar(f, e, i, skip_clips, star_for_none);
        std::fputc('\n', f);
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 2;
    spumoni_host::BatchEntries e;
    // five reads in two pieces, reads 0-2 and 3-4: the second piece's offsets land behind the first's entries; read 1 has
    // no entries between two that have
    const Piece first = {{{E(3, 4), E(10, 7), E(1, 8), E(2, 1)}, {}, {E(5, 7), E(4, 2), E(6, 3), E(7, 7)}}};
    const Piece second = {{{E(2, 4), E(9, 7), E(1, 4)}, {E(268435455u, 7), E(1, 7)}}};
    e.start(5);
    if (!first.add_to(e, 0) || !second.add_to(e, 3)) return 1;
    if (e.op_offs != std::vector<uint64_t>{0, 4, 4, 8, 11, 13} || e.ops.size() != 13) return 1;
    lines(f, e, 5, false, true);   // `cigar`, `extend`
    lines(f, e, 5, true, false);   // `map`: leading and trailing S left out, nothing for a read without entries
    // a piece with no entries at all between two that have some
    const Piece none = {{{}, {}}};
    e.start(4);
    if (!Piece{{{E(1, 7)}}}.add_to(e, 0) || !none.add_to(e, 1) || !Piece{{{E(2, 8)}}}.add_to(e, 3)) return 1;
    if (e.op_offs != std::vector<uint64_t>{0, 1, 1, 1, 2} || e.ops.size() != 2) return 1;
    lines(f, e, 4, false, true);
    // a super-batch of pieces without entries only
    e.start(2);
    if (!none.add_to(e, 0) || !e.ops.empty() || e.op_offs != std::vector<uint64_t>{0, 0, 0}) return 1;
    lines(f, e, 2, false, true);
    // every op code once
    Piece all = {{{}}};
    for (uint32_t op = 0; op < 16; ++op) all.reads[0].push_back(E(op + 1, op));
    e.start(1);
    if (!all.add_to(e, 0)) return 1;
    lines(f, e, 1, false, true);
    lines(f, e, 1, true, true);
    // a read of clips only: `map` writes nothing, and no `*` either where it was not asked for
    e.start(1);
    if (!Piece{{{E(4, 4)}}}.add_to(e, 0)) return 1;
    lines(f, e, 1, true, false);
    // a failing begin or fetch is passed on
    e.start(1);
    if (first.add_to(e, 0, -1, 0) || first.add_to(e, 0, 0, -1)) return 1;
    if (std::fclose(f) != 0) return 2;
    std::printf("cigar text ok\n");
    return 0;
}
