// read_command.cpp -- the driver under `spumoni assign`, `mems`, `place` and the chain family (read_command.hpp).
#include "read_command.hpp"

#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>

#include "index_files.hpp"

namespace spumoni_host {

bool is_file(const std::string& path) {
    struct stat st;
    return ::stat(path.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}
bool ends_with(const std::string& s, const std::string& suffix) {
    return s.size() >= suffix.size() && s.compare(s.size() - suffix.size(), suffix.size(), suffix) == 0;
}

void pin_charhash(const std::vector<spx_index*>& handles) {
    const char* pin = std::getenv("SPUMONI_CHARHASH");
    if (!pin) return;
    unsigned v[4] = {0, 0, 0, 0};
    if (std::sscanf(pin, "%u,%u,%u,%u", &v[0], &v[1], &v[2], &v[3]) != 4)
        fatal_error("SPUMONI_CHARHASH must be four comma-separated byte values (A,C,G,T)");
    const int64_t packed = (int64_t)((v[0] & 255) | ((v[1] & 255) << 8) | ((v[2] & 255) << 16) | ((uint64_t)(v[3] & 255) << 24));
    for (spx_index* ix : handles)
        if (spx_set_option(ix, "minimizer_charhash", packed) != SPX_OK) fatal_error("%s", spx_last_error());
}

void parse_read_options(int argc, char** argv, ReadOptions& o, int (*usage)(), bool doc_option, const char* extra_short,
                        const std::vector<struct option>& extra_long, const std::function<void(int, const char*)>& extra) {
    std::vector<struct option> table = {{"help", no_argument, NULL, 'h'},
                                        {"ref", required_argument, NULL, 'r'},
                                        {"pattern", required_argument, NULL, 'p'},
                                        {"MS", no_argument, NULL, 'M'},
                                        {"PML", no_argument, NULL, 'P'},
                                        {"no-digest", no_argument, NULL, 'n'},
                                        {"minimizer-alphabet", no_argument, NULL, 'm'},
                                        {"dna-minimizer", no_argument, NULL, 'a'},
                                        {"small-window", required_argument, NULL, 'K'},
                                        {"large-window", required_argument, NULL, 'W'}};
    std::string shorts = "hr:p:MPnmaK:W:";
    if (doc_option) {
        table.push_back({"doc-array", no_argument, NULL, 'd'});
        shorts += "d";
    }
    table.insert(table.end(), extra_long.begin(), extra_long.end());
    shorts += extra_short;
    table.push_back({0, 0, 0, 0});
    int long_index = 0;
    for (int c; (c = getopt_long(argc, argv, shorts.c_str(), table.data(), &long_index)) >= 0;) {
        switch (c) {
            case 'r': o.ref_file.assign(optarg); break;
            case 'p': o.pattern_file.assign(optarg); break;
            case 'M': o.ms_requested = true; break;
            case 'P': o.pml_requested = true; break;
            case 'm': o.use_promotions = true; break;
            case 'a': o.use_dna_letters = true; break;
            case 'n': o.min_digest = false; break;
            case 'K': o.k = std::max(std::atoi(optarg), 1); break;
            case 'W': o.w = std::max(std::atoi(optarg), 1); break;
            case 'd': o.use_doc = true; break;
            case 'h':
            case '?':
            case ':': usage(); std::exit(1);
            default: extra(c, optarg);
        }
    }
}

void require_ref_and_pattern(const ReadOptions& o) {
    if (o.ref_file == "" || o.pattern_file == "") fatal_warning("Both a reference file (-r) and pattern file (-p) must be provided.");
}

void imply_ms(ReadOptions& o, const char* command) {
    if (o.pml_requested)
        fatal_warning("-P cannot be used with `spumoni %s`: the anchors are read off matching statistics (-M is implied); "
                      "PMLs have no pointers.", command);
    o.ms = true;
}

void require_bases(const ReadOptions& o, const char* command) {
    if (o.use_promotions || o.use_dna_letters)
        fatal_warning("-m / -a cannot be used with `spumoni %s`: digested coordinates cannot be turned back into bases. "
                      "Map against an index built with -n -s.", command);
    if (o.min_digest)
        fatal_warning("`spumoni %s` needs -n: digested coordinates cannot be turned back into bases (index built with -n -s).", command);
}

void validate_read_options(const ReadOptions& o) {
    const std::string base = o.ref_file + (o.use_promotions ? ".bin" : ".fa");
    if (!is_file(base)) fatal_error("The following path is not valid: %s (remember to only specify output prefix)", base.data());
    if (!is_file(o.pattern_file)) fatal_error("The following path is not valid: %s", o.pattern_file.data());
    if (!ends_with(o.pattern_file, ".fa") && !ends_with(o.pattern_file, ".fasta") && !ends_with(o.pattern_file, ".fna"))
        fatal_error("The pattern file provided does not appear to be a FASTA\n"
                    "       file, please convert to FASTA and re-run.");
    if (o.use_doc && !is_file(base + ".doc"))
        fatal_warning("document array file (%s) is not present, so it cannot be used.", (base + ".doc").data());
    const bool have_raw = is_file(base + ".bwt.heads") && is_file(base + ".bwt.len") && is_file(base + ".thr_pos") &&
                          (!o.ms || (is_file(base + ".ssa") && is_file(base + ".esa")));
    if (!have_raw && !is_file(base + (o.ms ? ".thrbv.ms" : ".thrbv.spumoni")))
        fatal_warning("The index required for this computation is not available, please use spumoni build.");
    if (o.k > 4) fatal_warning("small window size (k) cannot be larger than 4 characters.");
    if (o.w < o.k) fatal_warning("large window size (w) should be larger than the small window size (k)");
    if (o.min_digest) {
        if (o.use_promotions && o.use_dna_letters) fatal_error("Only one type of minimizer can be specified from either -m or -a.");
        if (!o.use_promotions && !o.use_dna_letters) fatal_error("A minimizer type must be specified using -m or -a.");
    } else if (o.use_promotions || o.use_dna_letters) {
        fatal_error("A minimizer type should not be specified if intending not to use minimizer digestion.");
    }
}

std::vector<void*> device_entry_points(const char* command, const std::vector<const char*>& names, const char* what) {
    std::vector<void*> found;
    for (const char* name : names) found.push_back(dlsym(RTLD_DEFAULT, name));
    if (std::find(found.begin(), found.end(), nullptr) != found.end())
        fatal_error("the loaded libspumoni_gpu.so has no %s: `spumoni %s` needs %s of "
                    "the device library, and there is no CPU fallback.", names[0], command, what);
    if (spx_device_count() <= 0) fatal_error("no usable gfx950 device: `spumoni %s` runs on the GPU and has no CPU fallback.", command);
    return found;
}

void open_read_run(ReadOptions& o, size_t default_super_batch, ReadRun& run) {
    int device = 0;
    if (const char* g = std::getenv("SPUMONI_GPUS")) device = std::atoi(g);
    if (const char* t = std::getenv("SPUMONI_TEXT")) o.text_file = t;
    run.super_batch = default_super_batch;
    if (const char* t = std::getenv("SPUMONI_SUPER_BATCH")) run.super_batch = std::max<size_t>(1000, std::strtoull(t, nullptr, 10));
    run.t_start = std::chrono::steady_clock::now();
    try {
        run.reads.reset(new ReadFile(o.pattern_file));
    } catch (const std::exception& e) {
        fatal_error("%s", e.what());
    }
    {
        RunOptions lo = o;
        lo.devices = {device};
        lo.pattern_file.clear();  // (nothing of `run`'s text output is reserved)
        run.set.load(lo);
    }
    run.ix = run.set.ix[0];
    if (o.use_promotions) pin_charhash({run.ix});
    run.digest_kind = o.use_promotions ? SPX_DIGEST_PROMOTED : (o.use_dna_letters ? SPX_DIGEST_DNA : 0);
}

uint64_t null_db_threshold(const ReadOptions& o) {
    double percentile = 0.0;
    std::string err;
    (void)load_null_db(o.ref_file + (o.ms ? ".msnulldb" : ".pmlnulldb"), percentile, err);
    return max_value_threshold(percentile, !o.ms, o.use_promotions, o.use_dna_letters);
}

unsigned long long count_argument(const char* arg) { return arg[0] == '-' ? ~0ull : std::strtoull(arg, nullptr, 10); }

namespace {
struct MapOption {
    char c;
    const char* name;
    MapOptions::Level level;
    unsigned long long MapOptions::*value;
    unsigned long long lo, hi;
    const char* what;
};
const MapOption MAP_OPTIONS[] = {
    {'S', "max-dist", MapOptions::CHAIN, &MapOptions::max_dist, 1, 2147483647ull, "largest distance"},
    {'G', "max-gap", MapOptions::CHAIN, &MapOptions::max_gap, 0, 2147483647ull, "largest gap"},
    {'B', "gap-penalty", MapOptions::CHAIN, &MapOptions::gap_penalty, 0, 65535, "gap penalty"},
    {'H', "lookback", MapOptions::CHAIN, &MapOptions::lookback, 1, 64, "lookback"},
    {'F', "max-fill", MapOptions::FILL, &MapOptions::max_fill, 1, 4096, "largest filled gap"},
    {'E', "max-extend", MapOptions::EXTEND, &MapOptions::max_extend, 1, 4096, "largest extended end"},
    {'O', "band", MapOptions::EXTEND, &MapOptions::band, 0, 63, "band"},
    {'N', "mismatch", MapOptions::EXTEND, &MapOptions::mismatch, 0, 65535, "mismatch cost"},
    {'I', "indel", MapOptions::EXTEND, &MapOptions::indel, 0, 65535, "indel cost"},
};
}  // namespace

std::string MapOptions::shorts(const char* own) const {
    std::string s = "L:";
    for (const MapOption& m : MAP_OPTIONS)
        if (m.level <= level) s += std::string(1, m.c) + ":";
    return s + own;
}
std::vector<struct option> MapOptions::longs(const std::vector<struct option>& own) const {
    std::vector<struct option> t = {{"min-length", required_argument, NULL, 'L'}};
    for (const MapOption& m : MAP_OPTIONS)
        if (m.level <= level) t.push_back({m.name, required_argument, NULL, m.c});
    t.insert(t.end(), own.begin(), own.end());
    return t;
}
bool MapOptions::set(ReadOptions& o, int c, const char* arg) {
    if (c == 'L') {
        o.have_threshold = true;
        o.threshold = std::strtoull(arg, nullptr, 10);
        return true;
    }
    for (const MapOption& m : MAP_OPTIONS)
        if (m.level <= level && m.c == c) {
            this->*m.value = count_argument(arg);
            return true;
        }
    return false;
}
void MapOptions::validate(const ReadOptions& o) const {
    if (o.have_threshold && o.threshold == 0) fatal_warning("the minimum match length (-L) must be at least 1.");
    for (const MapOption& m : MAP_OPTIONS)
        if (m.level <= level && (this->*m.value < m.lo || this->*m.value > m.hi))
            fatal_warning("the %s (-%c) must be between %llu and %llu.", m.what, m.c, m.lo, m.hi);
}
uint64_t MapOptions::min_length(const ReadOptions& o) const {
    return o.have_threshold ? o.threshold : std::max<uint64_t>(1, null_db_threshold(o));
}
std::string MapOptions::describe(uint64_t min_length) const {
    std::string s = "a match is an anchor from length " + std::to_string(min_length) + " on (max-dist " + std::to_string(max_dist) +
                    ", max-gap " + std::to_string(max_gap) + ", gap penalty " + std::to_string(gap_penalty) + ", lookback " +
                    std::to_string(lookback);
    if (level >= FILL) s += ", max-fill " + std::to_string(max_fill);
    if (level >= EXTEND)
        s += ", max-extend " + std::to_string(max_extend) + ", band " + std::to_string(band) + ", mismatch " + std::to_string(mismatch) +
             ", indel " + std::to_string(indel);
    return s + ")";
}

std::vector<struct option> CallThresholds::longs(const std::vector<struct option>& own) const {
    std::vector<struct option> t = {{"min-depth", required_argument, NULL, 'D'},
                                    {"min-alt", required_argument, NULL, 'A'},
                                    {"min-permille", required_argument, NULL, 'Q'}};
    t.insert(t.end(), own.begin(), own.end());
    return t;
}
bool CallThresholds::set(int c, const char* arg) {
    if (c != 'D' && c != 'A' && c != 'Q') return false;
    (c == 'D' ? min_depth : c == 'A' ? min_alt : min_permille) = count_argument(arg);
    return true;
}
void CallThresholds::validate(const char* alt_what) const {
    if (min_depth < 1 || min_depth > 4294967295ull) fatal_warning("the smallest depth (-D) must be between 1 and 4294967295.");
    if (min_alt < 1 || min_alt > 4294967295ull) fatal_warning("%s (-A) must be between 1 and 4294967295.", alt_what);
    if (min_permille > 1000) fatal_warning("the smallest share (-Q) must be between 0 and 1000 thousandths.");
}

// name<TAB>length<TAB>text_start<TAB>strands per line (spumoni_amd/map.py: read_seq_table)
SeqTable read_seq_table(const std::string& path) {
    std::ifstream in(path, std::ios::binary);
    if (!in) fatal_error("cannot read %s", path.c_str());
    SeqTable t;
    std::string line;
    uint64_t start = 0, lineno = 0;
    while (std::getline(in, line)) {
        ++lineno;
        if (line.empty()) continue;
        std::vector<std::string> f;
        for (size_t at = 0;;) {
            const size_t tab = line.find('\t', at);
            f.push_back(line.substr(at, tab == std::string::npos ? tab : tab - at));
            if (tab == std::string::npos) break;
            at = tab + 1;
        }
        bool ok = f.size() == 4 && !f[0].empty();
        unsigned long long v[3] = {0, 0, 0};
        for (int i = 0; ok && i < 3; ++i) {
            const std::string& s = f[i + 1];
            ok = !s.empty() && s.size() <= 19 && s.find_first_not_of("0123456789") == std::string::npos;
            if (ok) v[i] = std::strtoull(s.c_str(), nullptr, 10);
        }
        if (!ok) fatal_error("%s: line %llu is not name<TAB>length<TAB>text_start<TAB>strands", path.c_str(), (unsigned long long)lineno);
        if (v[2] < 1 || v[2] > 2 || (t.strands && v[2] != t.strands) || v[0] == 0 || v[1] != start)
            fatal_error("%s: line %llu: strands, length or text_start do not fit the lines before it", path.c_str(),
                        (unsigned long long)lineno);
        t.strands = (uint32_t)v[2];
        t.names.push_back(f[0]);
        t.lengths.push_back(v[0]);
        start += v[0] * v[2];
    }
    if (t.names.empty()) fatal_error("%s: no sequences", path.c_str());
    return t;
}

void open_table_run(ReadOptions& o, const MapOptions& m, const char* command, const std::vector<const char*>& names, const char* what,
                    const char* reset_name, TableRun& run) {
    o.ref_file += ".fa";
    run.table_path = o.ref_file + ".seqs";
    if (!is_file(run.table_path))
        fatal_warning("the index has no sequence table (%s): build it with -s (spumoni build -n -s).", run.table_path.c_str());
    run.table = read_seq_table(run.table_path);
    run.names = names;
    run.found = device_entry_points(command, names, what);
    open_read_run(o, 8u << 20, run);
    run.super_batch = std::min<size_t>(run.super_batch, 32u << 20);  // (one piece per call into the library)
    const SeqTable& t = run.table;
    if (run.entry<decltype(&spn_set_sequences)>("spn_set_sequences")(run.ix, t.lengths.data(), t.lengths.size(), t.strands) != SPX_OK)
        fatal_error("%s: %s", run.table_path.c_str(), spx_last_error());
    if (reset_name && run.entry<decltype(&spd_cover_reset)>(reset_name)(run.ix) != SPX_OK) fatal_error("%s", spx_last_error());
    run.min_length = m.min_length(o);
    run.loaded = "[" + std::string(command) + "] index loaded (n = " + std::to_string(run.set.n) + ", r = " + std::to_string(run.set.r) +
                 "), " + std::to_string(t.names.size()) + " sequences on " + std::to_string(t.strands) + " strand(s); " +
                 m.describe(run.min_length);
}

namespace {
std::string g_partial;
void drop_partial() {
    if (!g_partial.empty()) ::unlink(g_partial.c_str());
    g_partial.clear();
}
}  // namespace

void LinesFile::open(const std::string& p, bool keep_partial_file) {
    path = p;
    keep_partial = keep_partial_file;
    if (!keep_partial) set_exit_hook(drop_partial);
    f = std::fopen(p.c_str(), "wb");
    if (!f) fatal_error("cannot create %s", p.c_str());
    if (!keep_partial) g_partial = p;
    std::setvbuf(f, nullptr, _IOFBF, 1 << 20);
}
void LinesFile::close() {
    if (f && std::fclose(f) != 0) fatal_error("write failed (disk full?): %s", path.c_str());
    f = nullptr;
    if (!keep_partial) g_partial.clear();
}

void scan_reads(ReadRun& run, LinesFile& out, const std::function<void(ReadBatch&)>& query,
                const std::function<void(const ReadBatch&, size_t)>& line) {
    ReadFile& reads = *run.reads;
    ReadBatch b;
    // 0 none, 1 a malformed record, 2 a read that is empty: fatal, as in `run`
    int deferred = 0;
    std::string deferred_msg;
    auto flush = [&](size_t take) {
        if (!take) return;
        b.take = take;
        b.offs.assign(1, 0);
        size_t chars = 0;
        for (size_t i = 0; i < take; ++i) b.offs.push_back(chars += b.recs[i].seq_len);
        b.seqs.resize(chars + 1);
        for (size_t i = 0; i < take; ++i) reads.copy_seq_upper(b.recs[i], b.seqs.data() + b.offs[i]);
        b.values.resize(take + 1);
        query(b);
        for (size_t i = 0; i < take; ++i) {
            if (b.values[i] == 0) {  // compute_ms_pml.cpp:926-931
                deferred = 2;
                deferred_msg.assign(b.recs[i].id, b.recs[i].id_len);
                return;
            }
            line(b, i);
        }
    };
    reads.precompute_ranges(1000);
    ReadFile::Range range;
    size_t pending_chars = 0;
    while (!deferred && reads.next_range(1000, range)) {
        ReadFile::ParseError err;
        const size_t before = b.recs.size();
        reads.scan_range(range, b.recs, err);
        size_t take = b.recs.size();
        for (size_t i = before; i < b.recs.size(); ++i) {
            if (b.recs[i].seq_len == 0) {
                deferred = 2;
                deferred_msg.assign(b.recs[i].id, b.recs[i].id_len);
                take = i;
                break;
            }
            pending_chars += b.recs[i].seq_len;
        }
        if (!deferred && err.fatal) {
            deferred = 1;
            deferred_msg = err.message;
        }
        if (deferred && !out.keep_partial) break;
        if (deferred || pending_chars >= run.super_batch) {  // (what is in front of the failing read is written first)
            const int d = deferred;
            const std::string msg = deferred_msg;
            deferred = 0;
            flush(take);
            if (!deferred) {
                deferred = d;
                deferred_msg = msg;
            }
            b.recs.clear();
            pending_chars = 0;
        }
    }
    if (!deferred) flush(b.recs.size());
    if (!deferred || out.keep_partial) out.close();
    if (deferred == 1) fatal_error("%s", deferred_msg.c_str());
    if (deferred == 2) {
        std::cout << "\n\n";
        fatal_warning("%s was empty after digestion, commonly due to reads "
                      "consisting of mostly non-ACGT characters. Please remove "
                      "read or run SPUMONI without minimizer digestion.", deferred_msg.data());
    }
}

void for_each_piece(const ReadBatch& b, const std::function<void(size_t, size_t)>& call) {
    for (size_t q0 = 0, q1; q0 < b.take; q0 = q1) {
        for (q1 = q0 + 1; q1 < b.take && q1 - q0 < (4u << 20) && b.offs[q1 + 1] - b.offs[q0] <= (32u << 20);) ++q1;
        call(q0, q1);
    }
}

ReadCounts accumulate_reads(TableRun& run, const ReadOptions& o, const MapOptions& m, decltype(&spd_cover_add_batch) add) {
    const spc_params params = m.chain();
    const spa_params fill = m.fill();
    const spe_params ends = m.ends();
    LinesFile none;  // (nothing is written per read)
    none.keep_partial = false;
    ReadCounts counts;
    std::vector<spn_mapping> maps;
    scan_reads(
        run, none,
        [&](ReadBatch& b) {
            maps.resize(b.take + 1);
            for_each_piece(b, [&](size_t q0, size_t q1) {
                if (add(run.ix, 0, (uint32_t)o.k, (uint32_t)o.w, b.seqs.data(), b.offs.data() + q0, q1 - q0, run.min_length,
                        o.use_doc ? 1 : 0, &params, &fill, &ends, maps.data() + q0) != SPX_OK)
                    fatal_error("%s", spx_last_error());
                // (without digestion a read's values are its characters)
                for (size_t q = q0; q < q1; ++q) b.values[q] = b.offs[q + 1] - b.offs[q];
            });
        },
        [&](const ReadBatch&, size_t i) {
            counts.reads++;
            counts.mapped += maps[i].seq != SPN_UNMAPPED;
        });
    return counts;
}

}  // namespace spumoni_host
