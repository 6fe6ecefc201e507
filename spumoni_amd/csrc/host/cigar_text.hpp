// cigar_text.hpp -- a super-batch's CIGAR entries as `spumoni cigar`, `extend` and `map` gather them from the library, and
// their text: plain host code with no device behind it, so that it can be built into a stand-alone program and run under a
// sanitizer (tests/cigar_text_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../../include/spumoni_extend.h"

namespace spumoni_host {

// The entries of a super-batch's reads, piece by piece: read i's are ops[op_offs[i]] .. ops[op_offs[i + 1]].
struct BatchEntries {
    std::vector<uint64_t> op_offs;  // per read of the super-batch: where its entries start in `ops`
    std::vector<uint32_t> ops;
    void start(size_t take) {
        op_offs.assign(take + 1, 0);
        ops.clear();
    }
    // Reads [q0, q1): begin(&n) is the product's _begin and says how many entries the piece has, fetch(offsets, entries)
    // its _fetch with room for q1 - q0 + 1 offsets, counted from the piece's first entry, and n + 1 entries.  Both give the
    // library's status; false when one of them is not 0 (the library has the message).
    template <class Begin, class Fetch>
    bool piece(size_t q0, size_t q1, Begin&& begin, Fetch&& fetch) {
        uint64_t n = 0;
        if (begin(&n) != 0) return false;
        const size_t at = ops.size();
        ops.resize(at + n + 1);
        piece_offs.resize(q1 - q0 + 1);
        if (fetch(piece_offs.data(), ops.data() + at) != 0) return false;
        ops.resize(at + n);
        for (size_t q = q0; q <= q1; ++q) op_offs[q] = at + piece_offs[q - q0];
        return true;
    }

private:
    std::vector<uint64_t> piece_offs;
};

// One table for the three commands (include/spumoni_cigar.h: 1 I, 2 D, 3 N, 7 =, 8 X; include/spumoni_extend.h: 4 S).  The
// CIGAR product cannot emit op 4 -- spx_cigar_kernels.h: emit_read pushes OP_S under ENDS only, and the CIGARs instantiate
// it without -- so `spumoni cigar` never reaches the 'S' here.
inline constexpr char CIGAR_OP_CHAR[16] = {'?', 'I', 'D', 'N', 'S', '?', '?', '=', 'X', '?', '?', '?', '?', '?', '?', '?'};

// Read i's entries as <length><op>...: without its soft clips under skip_clips (`map`: the PAF's cg tag has none), and `*`
// for a read without entries where star_for_none asks for it.
inline void write_cigar(FILE* f, const BatchEntries& e, size_t i, bool skip_clips, bool star_for_none) {
    if (star_for_none && e.op_offs[i] == e.op_offs[i + 1]) std::fputc('*', f);
    for (uint64_t at = e.op_offs[i]; at < e.op_offs[i + 1]; ++at)
        if (!skip_clips || (e.ops[at] & 15) != SPE_OP_S) std::fprintf(f, "%u%c", e.ops[at] >> 4, CIGAR_OP_CHAR[e.ops[at] & 15]);
}

}  // namespace spumoni_host
