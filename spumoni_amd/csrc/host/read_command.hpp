// read_command.hpp -- what `spumoni assign`, `mems`, `place` and the chain family (`chain` .. `consensus`) share: a command
// that walks the reads of a FASTA / FASTQ file through one product of the device library and writes lines in input order.
// The shared options and their rules (`run`'s messages where the rule is the same, spumoni_main.cpp: validate), the look-up
// of the product's entry points, the run's set-up -- one device (the first of SPUMONI_GPUS), the reads from reads.cpp, the
// index through the loaders `run` uses --, the loop over super-batches of SPUMONI_SUPER_BATCH characters, and the output
// file; for `map`, `cover`, `call` and `consensus` the run bound to the sequence table, and for the last three the loop that
// adds every super-batch to the genome's arrays.  A command keeps its usage text, its own options and checks, its call into
// the library, its lines and its closing line on stderr.
#pragma once
#include <getopt.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../../include/spumoni_cover.h"
#include "classify.hpp"
#include "reads.hpp"

namespace spumoni_host {

bool is_file(const std::string& path);
bool ends_with(const std::string& s, const std::string& suffix);
// SPUMONI_CHARHASH=<A>,<C>,<G>,<T>: pins the 8-bit character hashes of the -m digestion on every handle (nothing without it)
void pin_charhash(const std::vector<spx_index*>& handles);

struct ReadOptions : RunOptions {
    bool ms_requested = false, pml_requested = false;
    bool have_threshold = false;  // the command's own -T / -L
    uint64_t threshold = 0;
};

// -h -r -p -M -P -n -m -a -K -W [-d] and the command's own: `extra` gets every other option of extra_short / extra_long;
// an unknown one prints the usage and ends the process with status 1
void parse_read_options(int argc, char** argv, ReadOptions& o, int (*usage)(), bool doc_option, const char* extra_short,
                        const std::vector<struct option>& extra_long, const std::function<void(int, const char*)>& extra);
// the rules that do not depend on the command, in two parts: a command's own -M / -P rule stands between them and sets o.ms
void require_ref_and_pattern(const ReadOptions& o);
// `chain` .. `consensus` read their anchors off matching statistics: -P is refused, -M implied (o.ms set)
void imply_ms(ReadOptions& o, const char* command);
// `map` .. `consensus` report bases, not digested coordinates: -m / -a and a missing -n are refused
void require_bases(const ReadOptions& o, const char* command);
void validate_read_options(const ReadOptions& o);  // the paths, .doc with o.use_doc, the index files by o.ms, k, w, -m / -a
// The command's entry points, looked up at run time and never linked: the binary must also load against libraries without
// them (a CPU test double of the query boundary).  `what`: "the document votes".  Ends the process when one is missing or
// no device is usable -- before any file is written.
std::vector<void*> device_entry_points(const char* command, const std::vector<const char*>& names, const char* what);

struct ReadRun {
    std::chrono::steady_clock::time_point t_start;
    std::unique_ptr<ReadFile> reads;
    IndexSet set;
    spx_index* ix = nullptr;
    size_t super_batch = 0;
    int digest_kind = 0;
};
// o.ref_file with its extension, o.ms set.  SPUMONI_GPUS, SPUMONI_TEXT, SPUMONI_SUPER_BATCH, SPUMONI_CHARHASH.
void open_read_run(ReadOptions& o, size_t default_super_batch, ReadRun& run);
// the default of -T / -L: what `run -c` classifies with, from the null database (classify.cpp)
uint64_t null_db_threshold(const ReadOptions& o);

// Lines in input order, plain buffered writes.  keep_partial false: a run that fails leaves no file (every way out through
// fatal_error / fatal_warning unlinks it).
struct LinesFile {
    std::string path;
    FILE* f = nullptr;
    bool keep_partial = true;
    void open(const std::string& p, bool keep_partial_file);
    void close();
};

// The mapping options of `chain` (-L -S -G -B -H), of `align` and `cigar` (FILL: -F on top) and of `extend`, `map`, `cover`,
// `call` and `consensus` (EXTEND: -E -O -N -I on top of those), with their defaults: the option tables for parse_read_options, the setter
// for its `extra` (false: not one of these), the range checks in the order of the options, the parameters for the library
// and the "index loaded" line from "a match is an anchor" to the closing parenthesis.
struct MapOptions {
    enum Level { CHAIN, FILL, EXTEND };
    explicit MapOptions(Level l) : level(l) {}
    Level level;
    unsigned long long max_dist = 5000, max_gap = 500, gap_penalty = 1, lookback = 64, max_fill = 512;
    unsigned long long max_extend = 512, band = 16, mismatch = 4, indel = 6;
    std::string shorts(const char* own = "") const;  // ... with the command's own behind them
    std::vector<struct option> longs(const std::vector<struct option>& own = {}) const;
    bool set(ReadOptions& o, int c, const char* arg);
    void validate(const ReadOptions& o) const;
    uint64_t min_length(const ReadOptions& o) const;  // -L, or the null database's threshold (o.ms set, the index's prefix known)
    spc_params chain() const { return {(uint32_t)lookback, (uint32_t)max_dist, (uint32_t)max_gap, (uint32_t)gap_penalty}; }
    spa_params fill() const { return {(uint32_t)max_fill}; }
    spe_params ends() const { return {(uint32_t)max_extend, (uint32_t)band, (uint32_t)mismatch, (uint32_t)indel}; }
    std::string describe(uint64_t min_length) const;
};
// an option's count: a leading '-' is out of every range
unsigned long long count_argument(const char* arg);

// The thresholds of `call` and `consensus` (-D -A -Q) in MapOptions' manner: the tables behind a command's own, the setter
// (false: not one of these) and the range checks; `alt_what` is the command's wording of -A.
struct CallThresholds {
    unsigned long long min_depth = 2, min_alt = 2, min_permille = 500;
    std::string shorts(const char* own = "") const { return std::string("D:A:Q:") + own; }
    std::vector<struct option> longs(const std::vector<struct option>& own = {}) const;
    bool set(int c, const char* arg);
    void validate(const char* alt_what) const;
};

// <prefix>.fa.seqs, the table `spumoni build -s` writes (`map` .. `consensus`): ends the process on a malformed table
struct SeqTable {
    std::vector<std::string> names;
    std::vector<uint64_t> lengths;
    uint32_t strands = 0;
};
SeqTable read_seq_table(const std::string& path);

// The run of `map`, `cover`, `call` and `consensus`: bound to the index's sequence table, with the command's entry points
// by name.  open_table_run puts .fa onto o.ref_file, refuses an index without a table and reads it -- both before the
// entry points, so that they are reported on a machine without a device too --, looks the entry points up (`names` holds
// spn_set_sequences; the first one is the one a library without them is said to lack), opens the run with super-batches of
// one piece at the most, hands the table to the library and, where the command has one, calls `reset_name`'s entry point
// on the handle (nullptr: none).  It leaves the anchors' minimum length and the head of the "index loaded" line:
// "[command] index loaded (n = .., r = ..), N sequences on S strand(s); <m.describe>" -- the command appends its own clause.
struct TableRun : ReadRun {
    std::string table_path;
    SeqTable table;
    std::vector<const char*> names;
    std::vector<void*> found;
    uint64_t min_length = 0;
    std::string loaded;
    template <class F>
    F entry(const char* name) const {
        for (size_t i = 0; i < names.size(); ++i)
            if (std::strcmp(names[i], name) == 0) return reinterpret_cast<F>(found[i]);
        fatal_error("%s is not among the entry points this command looked up", name);
    }
};
void open_table_run(ReadOptions& o, const MapOptions& m, const char* command, const std::vector<const char*>& names, const char* what,
                    const char* reset_name, TableRun& run);

struct ReadBatch {
    std::vector<ReadRec> recs;  // the first `take` are the batch
    size_t take = 0;
    std::vector<uint8_t> seqs;
    std::vector<uint64_t> offs, values;  // values: per read, what the library says it had after digestion
};
// Scans the reads; per super-batch `query` calls the library (it fills values) and `line` writes read i's lines.  A
// malformed record or a read that is empty (before or after digestion) is fatal as in `run`: with out.keep_partial the
// reads in front of it are flushed and the file is closed first, else nothing more is flushed.  Closes `out`.
void scan_reads(ReadRun& run, LinesFile& out, const std::function<void(ReadBatch&)>& query,
                const std::function<void(const ReadBatch&, size_t)>& line);

// A super-batch ends with the read that fills it, and short reads are many: `call(q0, q1)` for pieces [q0, q1) of at most
// 4 Mi reads and 32 Mi characters, one piece of the staged walk each
void for_each_piece(const ReadBatch& b, const std::function<void(size_t, size_t)>& call);

// `cover`, `call` and `consensus`: every super-batch goes through `add` (spd_cover_add_batch or spl_call_add_batch, one
// signature) in calls of one piece each, and nothing is written per read
struct ReadCounts {
    uint64_t reads = 0, mapped = 0;
};
ReadCounts accumulate_reads(TableRun& run, const ReadOptions& o, const MapOptions& m, decltype(&spd_cover_add_batch) add);

}  // namespace spumoni_host
