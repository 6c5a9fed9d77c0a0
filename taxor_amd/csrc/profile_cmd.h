// profile_cmd.h -- `taxor profile`: the search TSV -> CAMI profile, sequence abundances and binning file
// (src/main/taxor_profile.cpp, src/taxonomy/profile_output.hpp).  Included by search_main.cpp inside its anonymous namespace.
//
//   options and their checks, the search file's readability   -- on the host, before any HIP call (:19-76,:860-878)
//   TSV -> CSR read -> matches                                 -- byte ranges of the file on parser threads, then one merge in file
//                                                                order; reads and accessions interned in byte-wise string order,
//                                                                the order of the reference's std::map keys (:93-163)
//   the three filtering rounds and the EM                      -- taxor_gpu_profile_* (profile.hip)
//   abundances, rank roll-up, the three files                  -- on the host from the device's integer sums (:568-636,:743-794)
// Errors print "[TAXOR PROFILE ERROR] ..." and return -1 like the reference (:874-878).

struct ProfileConfig {
    std::string search_file, report_file, binning_file, seq_abundance_file, sample_id;
    double threshold = 0.001;       // taxor_profile_configuration.hpp:14
    long em_steps = 100;
    int device = 0;
    bool have_search = false, have_report = false, have_binning = false, have_sample = false;
};

int profile_error(const std::string &msg)
{
    fflush(stdout);
    fprintf(stderr, "[TAXOR PROFILE ERROR] %s\n", msg.c_str());
    return -1;
}

void profile_help()
{
    printf("taxor-profile - Taxonomic profiling of a sample by giving read matching results of Taxor search\n"
           "=============================================================================================\n\n"
           "DESCRIPTION\n    Taxonomic profiling of the given read set\n\n"
           "OPTIONS\n"
           "    --search-file (std::string)\n          taxor search file containing results of read querying against the HIXF index\n"
           "    --cami-report-file (std::string)\n          output file reporting genomic abundances in CAMI profiling format\n"
           "    --seq-abundance-file (std::string)\n          output file reporting sequence abundance in CAMI profiling format (including unclassified reads)\n"
           "    --binning-file (std::string)\n          output file reporting read to taxa assignments in CAMI binning format\n"
           "    --sample-id (std::string)\n          Identifier of the analyzed sample\n"
           "    --min-abundance (double)\n          Minimum abundance to report (default: 0.001) Value must be in range [0,1].\n"
           "    --em-steps (unsigned 64 bit integer)\n          The number of steps for the expectation maximization (EM) algorithm (default: 100). Value must be in range [1,1000].\n"
           "    --gpu (signed 32 bit integer)\n          the device that runs the filtering rounds and the EM (default: 0)\n");
}

// one line of the TSV that the parse keeps (:126-141); views point into the file's bytes
struct ProfileLine {
    std::string_view read, acc, tax_id, tax_id_str, tax_str;
    uint64_t ref_len = 0, query_len = 0, hash_count = 0, hash_match = 0, line = 0;
    bool miss = false;
};

struct ProfileRange {
    std::vector<ProfileLine> lines;
    std::string error;
};

// std::stoull as the reference uses it: leading white space, then digits; anything else is an error there too
bool profile_number(std::string_view f, uint64_t *out)
{
    size_t i = 0;
    while (i < f.size() && isspace((unsigned char)f[i])) ++i;
    if (i < f.size() && f[i] == '+') ++i;
    if (i >= f.size() || !isdigit((unsigned char)f[i])) return false;
    uint64_t v = 0;
    for (; i < f.size() && isdigit((unsigned char)f[i]); ++i) v = v * 10 + (uint64_t)(f[i] - '0');
    *out = v;
    return true;
}

// lines of text[lo, hi) (lo at a line start); first_line = index of the first of them in the file
void profile_parse_range(const char *text, size_t lo, size_t hi, uint64_t first_line, ProfileRange &out)
{
    uint64_t ln = first_line;
    std::string_view f[10];
    for (size_t p = lo; p < hi; ++ln) {
        const char *nl = (const char *)memchr(text + p, '\n', hi - p);
        const size_t e = nl ? (size_t)(nl - text) : hi;
        const size_t line_lo = p;
        p = e + 1;
        if (ln == 0 || e == line_lo) continue;                             // the header (:120-121); an empty line holds nothing
        int nf = 0;
        for (size_t a = line_lo; nf < 10;) {
            const char *tab = (const char *)memchr(text + a, '\t', e - a);
            const size_t b = tab ? (size_t)(tab - text) : e;
            f[nf++] = std::string_view(text + a, b - a);
            if (!tab) break;
            a = b + 1;
        }
        auto bad = [&](const char *what) { out.error = "line " + std::to_string(ln + 1) + " of the search file: " + what; };
        if (nf < 2) return bad("fewer than two columns");
        ProfileLine L;
        L.line = ln;
        const size_t sp = f[0].find(' ');
        L.read = sp == std::string_view::npos ? f[0] : f[0].substr(0, sp);      // :124-125
        if (f[1] == "-") {
            L.miss = true;
            L.acc = f[1];
            if (nf < 6 || !profile_number(f[5], &L.query_len)) return bad("a read without a match needs its length in column 6");
        } else {
            if (nf < 10 || f[9].empty()) return bad("a match needs ten columns");
            L.acc = f[1];
            L.tax_id = f[3];
            L.tax_str = f[8];
            L.tax_id_str = f[9];
            if (!profile_number(f[4], &L.ref_len) || !profile_number(f[5], &L.query_len) || !profile_number(f[6], &L.hash_count) ||
                !profile_number(f[7], &L.hash_match))
                return bad("REF_LEN, QUERY_LEN, QHASH_COUNT and QHASH_MATCH must be numbers");
        }
        out.lines.push_back(L);
    }
}

std::vector<std::string> profile_split(const std::string &s, char d)       // str_split (:78-91): no trailing empty field
{
    std::vector<std::string> out;
    std::string cur;
    std::stringstream ss(s);
    while (std::getline(ss, cur, d)) out.push_back(cur);
    return out;
}

struct ProfileRank {             // taxonomy::Profile_Output
    std::string rank, taxid, taxid_string, taxname_string;
    double percentage = 0.0;
};

std::string profile_format(double percentage_times_100)                    // format(float f, 6): narrowed, then ostream's %g
{
    char buf[64];
    snprintf(buf, sizeof buf, "%.6g", (double)(float)percentage_times_100);
    return buf;
}

// calculate_higher_rank_abundances (:568-636).  species: (accession, abundance) in byte-wise key order, "unclassified" among them
bool profile_rank_rollup(const std::vector<std::pair<std::string, double>> &species, const std::map<std::string, std::pair<std::string, std::string>> &taxpath,
                         std::map<std::string, ProfileRank> &out, std::string &err)
{
    for (const auto &sp : species) {
        if (sp.second == 0) continue;
        if (sp.first == "unclassified") {
            ProfileRank pr;
            pr.taxid = sp.first;
            pr.percentage = sp.second;
            out.emplace(sp.first, std::move(pr));
            continue;
        }
        const auto &tp = taxpath.at(sp.first);
        const std::vector<std::string> ids = profile_split(tp.first, ';'), names = profile_split(tp.second, ';');
        if (ids.empty() || names.size() < ids.size() || names[0].size() < 3) {
            err = "the taxonomy strings of " + sp.first + " do not pair up (" + tp.first + " / " + tp.second + ")";
            return false;
        }
        for (size_t i = 0; i < ids.size(); ++i) {
            if (ids[i].empty()) continue;
            if (!out.count(ids[i])) {
                ProfileRank pr;
                pr.taxid = ids[i];
                pr.taxid_string = ids[0];
                pr.taxname_string = names[0].substr(3);
                for (size_t j = 1; j <= i; ++j) {
                    pr.taxid_string += "|";
                    pr.taxid_string += ids[j];
                    pr.taxname_string += "|";
                    if (names[j].size() > 1) {
                        if (names[j].size() < 3) {
                            err = "the taxonomy names of " + sp.first + " hold a rank shorter than its prefix (" + tp.second + ")";
                            return false;
                        }
                        pr.taxname_string += names[j].substr(3);
                    }
                }
                static const std::pair<char, const char *> ranks[] = {{'s', "species"}, {'g', "genus"}, {'f', "family"}, {'o', "order"},
                                                                      {'c', "class"},   {'p', "phylum"}, {'k', "superkingdom"}};
                for (const auto &rk : ranks)
                    if (!names[i].empty() && names[i][0] == rk.first) {
                        pr.rank = rk.second;
                        break;
                    }
                out.emplace(ids[i], std::move(pr));
            }
            out.at(ids[i]).percentage += sp.second;
        }
    }
    return true;
}

// write_biobox_profiling_file / write_sequence_abundance_file (profile_output.hpp:25-77)
bool profile_write_abundances(const std::string &path, const std::map<std::string, ProfileRank> &ranks, const std::string &sample_id, double threshold,
                              bool with_unclassified)
{
    std::string o = "@SampleID:" + sample_id + "\n@Version:0.10.0\n@Ranks:superkingdom|phylum|class|order|family|genus|species\n"
                    "@@TAXID\tRANK\tTAXPATH\tTAXPATHSN\tPERCENTAGE\n";
    if (with_unclassified) {
        const auto it = ranks.find("unclassified");
        if (it != ranks.end()) o += "unclassified\tno rank\t-\t-\t" + profile_format(it->second.percentage * 100) + "\n";
    }
    for (const char *tr : {"superkingdom", "phylum", "class", "order", "family", "genus", "species"})
        for (const auto &kv : ranks)
            if (kv.second.rank == tr && kv.second.percentage > threshold)
                o += kv.second.taxid + "\t" + kv.second.rank + "\t" + kv.second.taxid_string + "\t" + kv.second.taxname_string + "\t" +
                     profile_format(kv.second.percentage * 100) + "\n";
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(o.data(), 1, o.size(), f) == o.size();
    return fclose(f) == 0 && ok;
}

// the value of one of the profile's options into c, with the reference parser's messages (:19-76); false and *err on a value that
// does not parse or lies outside its range.  `taxor search` takes the same options for its one-run mode (search_cmd.h).
bool profile_set_option(const std::string &o, const std::string &v, ProfileConfig &c, std::string &err)
{
    char *end = nullptr;
    errno = 0;
    if (o == "--search-file") { c.search_file = v; c.have_search = true; }
    else if (o == "--cami-report-file") { c.report_file = v; c.have_report = true; }
    else if (o == "--seq-abundance-file") c.seq_abundance_file = v;
    else if (o == "--binning-file") { c.binning_file = v; c.have_binning = true; }
    else if (o == "--sample-id") { c.sample_id = v; c.have_sample = true; }
    else if (o == "--min-abundance") {
        const double x = strtod(v.c_str(), &end);
        if (v.empty() || *end || errno) { err = "Value parse failed for " + o + ": Argument " + v + " could not be parsed as type double."; return false; }
        if (!(x >= 0.0 && x <= 1.0)) {
            err = "Validation failed for option " + o + ": Value " + std::to_string(x) + " is not in range [" + std::to_string(0.0) + "," + std::to_string(1.0) + "].";
            return false;
        }
        c.threshold = x;
    } else {
        const long x = strtol(v.c_str(), &end, 10);
        if (v.empty() || *end || errno) { err = "Value parse failed for " + o + ": Argument " + v + " could not be parsed as an integer."; return false; }
        const long lo = o == "--em-steps" ? 1 : 0, hi = o == "--em-steps" ? 1000 : 1023;
        if (x < lo || x > hi) {
            err = "Validation failed for option " + o + ": Value " + std::to_string(x) + " is not in range [" + std::to_string(lo) + "," + std::to_string(hi) + "].";
            return false;
        }
        if (o == "--em-steps") c.em_steps = x;
        else c.device = (int)x;
    }
    return true;
}

// What the part after the device pipeline needs to know about the names behind the CSR's numbers: reads and references are
// numbered in byte-wise order of their names.  `taxor profile` answers from the lines of its search file, `taxor search` from the
// read ids it kept and the species table of the index.
struct ProfileNames {
    uint64_t n_reads = 0, n_refs = 0;
    const uint64_t *read_off = nullptr;                                   // [n_reads + 1]
    std::function<std::string_view(uint64_t)> read_id;                    // read -> its id, cut at the first space
    std::function<std::string_view(uint64_t)> accession;                  // reference -> accession
    std::function<std::string_view(uint64_t)> tax_id_str, tax_str;        // reference -> TAX_ID_STR / TAX_STR of its first line (:142-146)
    std::function<std::string_view(uint64_t)> match_tax_id;               // match -> TAXID of its original line
};

// abundances (:734-738,:743-794), rank roll-up, the two CAMI files and the binning file, from the device's results.  Returns "" or
// the error's text.
std::string profile_write_outputs(const ProfileConfig &c, const taxor_profile_results &res, const ProfileNames &nm)
{
    const uint64_t R = nm.n_reads, F = nm.n_refs;
    std::map<std::string, std::pair<std::string, std::string>> taxpath;      // accession -> (TAX_ID_STR, TAX_STR) (:142-146)
    for (uint64_t x = 0; x < F; ++x)
        if (res.has_prior[x]) taxpath.emplace(std::string(nm.accession(x)), std::make_pair(std::string(nm.tax_id_str(x)), std::string(nm.tax_str(x))));
    std::map<std::string, double> seq_ab, gen_ab;
    for (uint64_t x = 0; x < F; ++x)
        if (res.has_prior[x]) seq_ab.emplace(std::string(nm.accession(x)), exp(res.log_prior[x]));
    seq_ab.emplace("unclassified", exp(res.log_unclassified));               // insert: an accession of that name keeps its own value (:734)
    {
        double sum_avg_cov = 0.0;
        std::vector<double> cov(F, 0.0);
        for (uint64_t x = 0; x < F; ++x)
            if (res.has_prior[x]) {
                cov[x] = (double)res.ref_nts[x] / (double)res.taxa_len[x];
                sum_avg_cov += cov[x];
            }
        const double log_sum = log(sum_avg_cov);
        for (uint64_t x = 0; x < F; ++x)
            if (res.has_prior[x]) gen_ab.emplace(std::string(nm.accession(x)), exp(log(cov[x] + 0.000000000001) - log_sum));
    }
    std::string err;
    if (!c.seq_abundance_file.empty()) {
        std::map<std::string, ProfileRank> ranks;
        if (!profile_rank_rollup(std::vector<std::pair<std::string, double>>(seq_ab.begin(), seq_ab.end()), taxpath, ranks, err)) return err;
        if (!profile_write_abundances(c.seq_abundance_file, ranks, c.sample_id, c.threshold, true)) return "cannot write " + c.seq_abundance_file;
    }
    {
        std::map<std::string, ProfileRank> ranks;
        if (!profile_rank_rollup(std::vector<std::pair<std::string, double>>(gen_ab.begin(), gen_ab.end()), taxpath, ranks, err)) return err;
        if (!profile_write_abundances(c.report_file, ranks, c.sample_id, c.threshold, false)) return "cannot write " + c.report_file;
    }
    // ---- binning (profile_output.hpp:79-98): the first best match's tax_id as its ORIGINAL line has it; a read whose matches were
    //      all erased is not listed
    {
        std::string o = "@SampleID:" + c.sample_id + "\n@Version:0.10.0\n@@SEQUENCEID\tTAXID\n";
        for (uint64_t r = 0; r < R; ++r) {
            bool present = false;
            uint64_t first_best = ~0ull;
            for (uint64_t i = nm.read_off[r]; i < nm.read_off[r + 1]; ++i) {
                present |= res.alive[i] != 0 || res.best[i] != 0;
                if (first_best == ~0ull && res.best[i]) first_best = i;
            }
            if (!present) continue;
            o.append(nm.read_id(r));
            o += "\t";
            if (first_best != ~0ull) o.append(nm.match_tax_id(first_best));
            else o += "-";
            o += "\n";
        }
        FILE *f = fopen(c.binning_file.c_str(), "wb");
        if (!f || fwrite(o.data(), 1, o.size(), f) != o.size() || fclose(f) != 0) return "cannot write " + c.binning_file;
    }
    return "";
}

int profile_command(int argc, char **argv)
{
    const double t_start = now();
    ProfileConfig c;
    std::vector<std::string> args;
    for (int i = 2; i < argc; ++i) {
        const std::string tok = argv[i];
        const size_t eq = tok.find('=');
        if (tok.size() > 2 && tok[0] == '-' && tok[1] == '-' && eq != std::string::npos && eq > 2) {
            args.push_back(tok.substr(0, eq));
            args.push_back(tok.substr(eq + 1));
        } else
            args.push_back(tok);
    }
    for (const std::string &o : args)
        if (o == "--help" || o == "-h") {
            profile_help();
            return 0;
        }
    for (size_t i = 0; i < args.size(); ++i) {
        const std::string &o = args[i];
        if (o == "--output-verbose-statistics" || o == "--debug") continue;                 // hidden, accepted (:65-75)
        if (o == "--search-file" || o == "--cami-report-file" || o == "--seq-abundance-file" || o == "--binning-file" || o == "--sample-id" ||
            o == "--min-abundance" || o == "--em-steps" || o == "--gpu") {
            if (i + 1 >= args.size()) return profile_error("Missing value for option " + o);
            const std::string v = args[++i];
            std::string err;
            if (!profile_set_option(o, v, c, err)) return profile_error(err);
        } else
            return profile_error("Unknown option " + o + ". In case this is meant to be a non-option/argument/parameter, please specify the start of "
                                 "non-options with '--'. See -h/--help for program information.");
    }
    if (!c.have_search) return profile_error("Option --search-file is required but not set.");
    if (!c.have_report) return profile_error("Option --cami-report-file is required but not set.");
    if (!c.have_binning) return profile_error("Option --binning-file is required but not set.");
    if (!c.have_sample) return profile_error("Option --sample-id is required but not set.");
    // ---- the search file, whole (:103-107)
    std::string text;
    {
        std::ifstream in(c.search_file, std::ios::binary);
        if (!in) return profile_error("Could not open search results file: " + c.search_file);
        std::error_code ec;
        if (std::filesystem::is_directory(c.search_file, ec)) return profile_error("Could not open search results file: " + c.search_file);
        in.seekg(0, std::ios::end);
        const std::streamoff sz = in.tellg();
        if (sz < 0) return profile_error("Could not open search results file: " + c.search_file);
        text.resize((size_t)sz);
        in.seekg(0);
        if (sz && !in.read(text.data(), sz)) return profile_error("Could not read search results file: " + c.search_file);
    }
    // ---- parse: byte ranges cut at line starts, one per thread (the pattern of fastx.h's range readers); line numbers from a count
    //      of the newlines before each range
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const size_t n_ranges = std::max<size_t>(1, std::min<size_t>({(size_t)hw, (size_t)16, text.size() / (1u << 20) + 1}));
    std::vector<size_t> cut(n_ranges + 1, text.size());
    cut[0] = 0;
    for (size_t t = 1; t < n_ranges; ++t) {
        size_t p = std::max(cut[t - 1], text.size() / n_ranges * t);
        const char *nl = p < text.size() ? (const char *)memchr(text.data() + p, '\n', text.size() - p) : nullptr;
        cut[t] = nl ? (size_t)(nl - text.data()) + 1 : text.size();
    }
    std::vector<ProfileRange> ranges(n_ranges);
    {
        std::vector<uint64_t> newlines(n_ranges, 0);
        std::vector<std::thread> th;
        for (size_t t = 0; t < n_ranges; ++t)
            th.emplace_back([&, t] { newlines[t] = (uint64_t)std::count(text.begin() + (std::ptrdiff_t)cut[t], text.begin() + (std::ptrdiff_t)cut[t + 1], '\n'); });
        for (auto &x : th) x.join();
        th.clear();
        uint64_t first = 0;
        for (size_t t = 0; t < n_ranges; ++t) {
            th.emplace_back([&, t, first] { profile_parse_range(text.data(), cut[t], cut[t + 1], first, ranges[t]); });
            first += newlines[t];
        }
        for (auto &x : th) x.join();
    }
    for (const ProfileRange &r : ranges)
        if (!r.error.empty()) return profile_error(r.error);
    // ---- merge in file order (:142-159): a "-" line is dropped when the read holds anything; the first line of an accession fixes
    //      its taxonomy strings
    struct TmpRead {
        std::string_view id;
        uint64_t n = 0, query_len = 0, hash_count = 0;
        bool miss = false;
    };
    std::unordered_map<std::string_view, uint32_t> read_of, acc_of;
    std::vector<TmpRead> reads;
    std::vector<std::string_view> accs;
    std::vector<const ProfileLine *> acc_first;
    struct Kept {
        uint32_t read, acc;
        const ProfileLine *line;
    };
    std::vector<Kept> kept;
    for (const ProfileRange &rg : ranges)
        for (const ProfileLine &L : rg.lines) {
            auto ir = read_of.emplace(L.read, (uint32_t)reads.size());
            if (ir.second) {
                reads.emplace_back();
                reads.back().id = L.read;
            }
            TmpRead &rd = reads[ir.first->second];
            uint32_t a = ~0u;
            if (!L.miss) {
                auto ia = acc_of.emplace(L.acc, (uint32_t)accs.size());
                if (ia.second) {
                    accs.push_back(L.acc);
                    acc_first.push_back(&L);
                }
                a = ia.first->second;
            }
            if (rd.n > 0 && L.miss) continue;
            if (rd.n > 0 && rd.miss)
                return profile_error("line " + std::to_string(L.line + 1) + " of the search file: read " + std::string(L.read) +
                                     " has a match after its '-' line; the reference implementation does not define what a '-' among several matches means");
            if (rd.n == 0) {
                rd.miss = L.miss;
                rd.query_len = L.query_len;
                rd.hash_count = L.hash_count;
            } else if (rd.query_len != L.query_len || rd.hash_count != L.hash_count)
                return profile_error("line " + std::to_string(L.line + 1) + " of the search file: read " + std::string(L.read) +
                                     " changes its QUERY_LEN or QHASH_COUNT between lines");
            ++rd.n;
            kept.push_back({ir.first->second, a, &L});
        }
    if (accs.size() >= (1ull << 31) || reads.size() >= (1ull << 32)) return profile_error("the search file names too many reads or references");
    // ---- dense ids in byte-wise string order; CSR with reads in that order and matches in file order
    const uint64_t R = reads.size(), F = accs.size(), M = kept.size();
    std::vector<uint32_t> read_order(R), acc_order(F), read_rank(R), acc_rank(F);
    for (uint64_t i = 0; i < R; ++i) read_order[i] = (uint32_t)i;
    for (uint64_t i = 0; i < F; ++i) acc_order[i] = (uint32_t)i;
    std::sort(read_order.begin(), read_order.end(), [&](uint32_t a, uint32_t b) { return reads[a].id < reads[b].id; });
    std::sort(acc_order.begin(), acc_order.end(), [&](uint32_t a, uint32_t b) { return accs[a] < accs[b]; });
    for (uint64_t i = 0; i < R; ++i) read_rank[read_order[i]] = (uint32_t)i;
    for (uint64_t i = 0; i < F; ++i) acc_rank[acc_order[i]] = (uint32_t)i;
    std::vector<uint64_t> off(R + 1, 0), ref_len(M), hash_match(M), query_len(R), hash_count(R), cursor(R);
    std::vector<int32_t> ref(M);
    std::vector<const ProfileLine *> match_line(M);
    for (uint64_t i = 0; i < R; ++i) {
        off[i + 1] = off[i] + reads[read_order[i]].n;
        query_len[i] = reads[read_order[i]].query_len;
        hash_count[i] = reads[read_order[i]].hash_count;
        cursor[i] = off[i];
    }
    for (const Kept &k : kept) {
        const uint64_t at = cursor[read_rank[k.read]]++;
        ref[at] = k.line->miss ? -1 : (int32_t)acc_rank[k.acc];
        ref_len[at] = k.line->ref_len;
        hash_match[at] = k.line->hash_match;
        match_line[at] = k.line;
    }
    const double t_parsed = now();
    // ---- device pipeline
    taxor_profile_csr csr{};
    csr.n_reads = R;
    csr.n_refs = F;
    csr.n_matches = M;
    csr.read_off = off.data();
    csr.ref = ref.data();
    csr.ref_len = ref_len.data();
    csr.hash_match = hash_match.data();
    csr.query_len = query_len.data();
    csr.hash_count = hash_count.data();
    taxor_gpu_profile *gp = nullptr;
    if (taxor_gpu_profile_create(c.device, &csr, &gp) != TAXOR_OK) return profile_error(taxor_gpu_last_error());
    std::unique_ptr<taxor_gpu_profile, void (*)(taxor_gpu_profile *)> gp_guard(gp, taxor_gpu_profile_destroy);
    if (taxor_gpu_profile_run(gp, (uint32_t)c.em_steps, 0) != TAXOR_OK) return profile_error(taxor_gpu_last_error());
    taxor_profile_results res{};
    if (taxor_gpu_profile_results(gp, &res) != TAXOR_OK) return profile_error(taxor_gpu_last_error());
    printf("Number of EM steps needed: %u\n", res.em_steps_needed);
    fflush(stdout);
    const double t_device = now();
    // ---- abundances, rank roll-up and the three files
    {
        ProfileNames nm;
        nm.n_reads = R;
        nm.n_refs = F;
        nm.read_off = off.data();
        nm.read_id = [&](uint64_t r) { return reads[read_order[r]].id; };
        nm.accession = [&](uint64_t x) { return accs[acc_order[x]]; };
        nm.tax_id_str = [&](uint64_t x) { return acc_first[acc_order[x]]->tax_id_str; };
        nm.tax_str = [&](uint64_t x) { return acc_first[acc_order[x]]->tax_str; };
        nm.match_tax_id = [&](uint64_t i) { return match_line[i]->tax_id; };
        const std::string err = profile_write_outputs(c, res, nm);
        if (!err.empty()) return profile_error(err);
    }
    const double t_end = now();
    fprintf(stderr, "taxor profile: %llu reads, %llu references, %llu matches, %llu reference pairs, %u EM iterations; seconds: parse %.3f, "
                    "device %.3f (rounds %.3f, EM %.3f), write %.3f, total %.3f\n",
            (unsigned long long)R, (unsigned long long)F, (unsigned long long)M, (unsigned long long)res.n_pairs, res.em_iterations, t_parsed - t_start,
            t_device - t_parsed, res.seconds_filter, res.seconds_em, t_end - t_device, t_end - t_start);
    return 0;
}
