// build_cmd.h -- `taxor build`: reference genomes + a taxonomy TSV -> a searchable .hixf (src/main/taxor_build.cpp:545-597).
// Included by search_main.cpp inside its anonymous namespace, like pin_cmd.h.
//
//   options, sanity checks, TSV parsing and genome lookup  -- on the host, before any HIP call (taxor_build.cpp:51-166,238-293)
//   genome files -> per user bin distinct keys             -- fastx.h readers on --threads threads, the device keyer
//                                                            (genome_keys.hip) on the batches they fill, two batches in flight
//   layout                                                 -- taxor_build_layout over the exact counts (DESIGN.md "taxor build")
//   geometry, construction, store                          -- exact merged-bin unions, taxor_gpu_index_build_hixf_ex with the keys
//                                                            on the device, taxor_hixf_store
//   keys beyond device memory                              -- the genomes are keyed in waves into a host store (key_store.h) and the index is
//                                                            constructed with a bounded part of the keys on the device
//                                                            (taxor_gpu_index_build_hixf_stream_ranges)
// Errors print "[TAXOR BUILD ERROR] ..." and return -1 like the reference (:560-564,585-589).

struct BuildConfig {
    std::string input_file_name, input_sequence_folder, output_file_name;
    std::vector<std::string> input_files, input_folders;
    long threads = 1, kmer_size = 20, window_size = 20, syncmer_size = 10, scaling = 1;   // taxor_build_configuration.hpp:15-22
    bool use_syncmer = false, verbose = false, debug = false;
    int device = 0;
    uint64_t tmax = 0;            // hidden: force one t_max (0 = choose, taxor_build.cpp:168-233)
    uint64_t key_budget_mib = 0;  // hidden: MiB of distinct keys on the device at a time (0 = an eighth of the free device memory)
    uint64_t host_memory_mib = 0; // hidden: the host memory the key store is held against (0 = MemAvailable)
    bool group_similar = false;   // order the user bins of a merged level by sketch similarity ("Similarity-aware layout")
    long sketch_size = 1024, similarity_window = 4096;   // hidden
    double similarity_threshold = 0.1;                    // hidden
};

const char *const BUILD_ADVANCED_HELP =
    "taxor build - advanced options\n"
    "    --tmax <n>                  force one t_max, the largest number of bins of an IXF, in [2,1048576] (default: chosen from the\n"
    "                                candidates 64 .. 4096 and the square root of the number of genomes)\n"
    "    --device-key-budget <MiB>   at most this many MiB of distinct keys (8 bytes each) on the device at a time, in [1,16777216].\n"
    "                                Genomes whose keys may exceed it are keyed in waves into host memory and the index is built\n"
    "                                from there, byte-identical to a build with every key resident (default: such a build is chosen\n"
    "                                when the keys may not fit the free device memory, with an eighth of it as the budget)\n"
    "    --host-memory-mib <MiB>     host memory the key store of such a build may take, in [1,1073741824] (default: MemAvailable)\n"
    "    --group-similar             group similar genomes under one merged bin: the genomes' key sets are sketched and compared on\n"
    "                                the device, and the user bins of a merged level are ordered by similarity cluster instead of by\n"
    "                                key count before they are cut into groups (default: off; works with every route above)\n"
    "    --sketch-size <m>           values per sketch, in [16,1024] (default: 1024)\n"
    "    --similarity-window <W>     genomes compared with one another: consecutive runs of W in descending key count, in [2,8192]\n"
    "                                (default: 4096)\n"
    "    --similarity-threshold <J>  two genomes are linked when the estimated Jaccard index of their key sets reaches J, in (0,1]\n"
    "                                (default: 0.1, about 92.5 % identity at k = 22)\n"
    "ranges of the syncmer scheme (--use-syncmer)\n"
    "    --syncmer-size <s>          in [1,26] and below --kmer-size (at most 30 with syncmers); every such pair is built, and `taxor\n"
    "                                search` takes syncmer indexes of any s-mer size from 1 to 31 with k-mer sizes up to 32\n";

struct BuildSpecies {
    std::string accession, taxid, organism, taxnames, taxids, file_stem, path;
    uint64_t seq_len = 0;
};

int build_error(const std::string &msg)
{
    fflush(stdout);
    fprintf(stderr, "[TAXOR BUILD ERROR] %s\n", msg.c_str());
    return -1;
}

std::vector<std::string> build_split(const std::string &s, char d)   // taxor_build.cpp:105-118 (std::getline: no trailing empty field)
{
    std::vector<std::string> out;
    std::string cur;
    std::stringstream ss(s);
    while (std::getline(ss, cur, d)) out.push_back(cur);
    return out;
}

// parse_refseq_taxonomy_file (parse_ncbi_taxonomy.cpp:7-41): accession, taxid, file path[, organism, taxnames, taxids]
bool build_parse_tsv(const std::string &path, std::vector<BuildSpecies> &out, std::string &err)
{
    std::ifstream in(path);
    if (!in) { err = "Error parsing the taxonomy file: " + path; return false; }
    std::string line;
    while (std::getline(in, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        const std::vector<std::string> f = build_split(line, '\t');
        if (f.size() < 3) { err = "Error parsing the taxonomy file: " + path; return false; }
        BuildSpecies sp;
        sp.accession = f[0];
        sp.taxid = f[1];
        if (f.size() > 3) sp.organism = f[3];
        if (f.size() > 4) sp.taxnames = f[4];
        if (f.size() > 5) sp.taxids = f[5];
        const size_t sl = f[2].find_last_of("/\\");
        sp.file_stem = sl == std::string::npos ? f[2] : f[2].substr(sl + 1);
        if (sp.file_stem.empty() || sp.file_stem == " ") { err = "No file name found for" + sp.accession + " !!!"; return false; }
        out.push_back(std::move(sp));
    }
    return true;
}

// file_list<false> (taxor_build.cpp:238-266): regular files directly in each directory; accession = parts[0] + "_" + parts[1] of the
// stem split on '_'; the first file found wins.  Directory listings are sorted so that the result does not depend on their order.
std::map<std::string, std::string> build_file_list(const std::vector<std::string> &folders)
{
    std::map<std::string, std::string> res;
    for (const std::string &d : folders) {
        std::vector<std::filesystem::path> files;
        std::error_code ec;
        for (const auto &e : std::filesystem::directory_iterator(d, ec))
            if (e.is_regular_file(ec)) files.push_back(e.path());
        std::sort(files.begin(), files.end());
        for (const auto &f : files) {
            const std::vector<std::string> parts = build_split(f.stem().string(), '_');
            if (parts.size() > 1) res.emplace(parts[0] + "_" + parts[1], f.string());
        }
    }
    return res;
}

// one genome file, read whole: its records' ASCII bases back to back and their offsets
struct GenomeChunk {
    uint32_t bin = 0;
    std::string bases;
    std::vector<uint64_t> off{0};
    std::string error;
};

int build_command(int argc, char **argv)
{
    const double t_start = now();
    BuildConfig c;
    // seqan3::argument_parser takes "--opt value" and "--opt=value"
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
    bool have_input = false;
    auto number = [&](const std::string &opt, const std::string &v, long lo, long hi, long *out, std::string &err) {
        char *end = nullptr;
        errno = 0;
        const long x = strtol(v.c_str(), &end, 10);
        if (v.empty() || *end || errno) { err = "Value parse failed for " + opt + ": Argument " + v + " could not be parsed as type int32."; return false; }
        if (x < lo || x > hi) {
            err = "Validation failed for option " + opt + ": Value " + std::to_string(x) + " is not in range [" + std::to_string(lo) + "," + std::to_string(hi) + "].";
            return false;
        }
        *out = x;
        return true;
    };
    for (size_t i = 0; i < args.size(); ++i) {
        const std::string &o = args[i];
        std::string err;
        const bool has_v = i + 1 < args.size();
        if (o == "--advanced-help" || o == "-hh") { fputs(BUILD_ADVANCED_HELP, stdout); return 0; }
        else if (o == "--use-syncmer") c.use_syncmer = true;
        else if (o == "--group-similar") c.group_similar = true;
        else if (o == "--output-verbose-statistics") c.verbose = true;
        else if (o == "--debug") c.debug = true;
        else if (o == "--input-file" || o == "--input-sequence-dir" || o == "--output-filename" || o == "--kmer-size" || o == "--syncmer-size" ||
                 o == "--window-size" || o == "--scaling" || o == "--threads" || o == "--gpu" || o == "--tmax" || o == "--device-key-budget" ||
                 o == "--host-memory-mib" || o == "--sketch-size" || o == "--similarity-window" || o == "--similarity-threshold") {
            if (!has_v) return build_error("Missing value for option " + o);
            const std::string v = args[++i];
            long tmp = 0;
            if (o == "--input-file") { c.input_file_name = v; have_input = true; }
            else if (o == "--input-sequence-dir") c.input_sequence_folder = v;
            else if (o == "--output-filename") c.output_file_name = v;
            else if (o == "--kmer-size" && !number(o, v, 1, 64, &c.kmer_size, err)) return build_error(err);
            else if (o == "--syncmer-size" && !number(o, v, 1, 26, &c.syncmer_size, err)) return build_error(err);
            else if (o == "--window-size" && !number(o, v, 1, 96, &c.window_size, err)) return build_error(err);
            else if (o == "--scaling" && !number(o, v, 10, 1000, &c.scaling, err)) return build_error(err);
            else if (o == "--threads" && !number(o, v, 1, 32, &c.threads, err)) return build_error(err);
            else if (o == "--gpu") { if (!number(o, v, 0, 1023, &tmp, err)) return build_error(err); c.device = (int)tmp; }
            else if (o == "--tmax") { if (!number(o, v, 2, 1 << 20, &tmp, err)) return build_error(err); c.tmax = (uint64_t)tmp; }
            else if (o == "--device-key-budget") { if (!number(o, v, 1, 1 << 24, &tmp, err)) return build_error(err); c.key_budget_mib = (uint64_t)tmp; }
            else if (o == "--host-memory-mib") { if (!number(o, v, 1, 1 << 30, &tmp, err)) return build_error(err); c.host_memory_mib = (uint64_t)tmp; }
            else if (o == "--sketch-size" && !number(o, v, 16, 1024, &c.sketch_size, err)) return build_error(err);
            else if (o == "--similarity-window" && !number(o, v, 2, 8192, &c.similarity_window, err)) return build_error(err);
            else if (o == "--similarity-threshold") {
                char *end = nullptr;
                errno = 0;
                const double x = strtod(v.c_str(), &end);
                if (v.empty() || *end || errno) return build_error("Value parse failed for " + o + ": Argument " + v + " could not be parsed as type double.");
                if (!(x > 0.0 && x <= 1.0)) return build_error("Validation failed for option " + o + ": Value " + v + " is not in range (0,1].");
                c.similarity_threshold = x;
            }
        } else
            return build_error("Unknown option " + o + ". In case this is meant to be a non-option/argument/parameter, please specify the start of "
                               "non-options with '--'. See -h/--help for program information.");
    }
    if (!have_input) return build_error("Option --input-file is required but not set.");
    // ---- sanity_checks (taxor_build.cpp:120-166)
    printf("checking input ... ");
    fflush(stdout);
    if (c.use_syncmer && c.kmer_size > 30)
        return build_error("The chosen k-mer size is too large for the syncmer scheme. Please choose a k-mer size <= 30 or use the minimizer scheme");
    c.input_files = build_split(c.input_file_name, ',');
    for (const std::string &f : c.input_files)
        if (!std::filesystem::exists(f)) return build_error("Please check the given input file(s). \nThe following input file does not exist: " + f);
    std::vector<BuildSpecies> orgs;
    for (const std::string &f : c.input_files) {
        std::string err;
        if (!build_parse_tsv(f, orgs, err)) return build_error(err);
    }
    c.input_folders = build_split(c.input_sequence_folder, ',');
    for (const std::string &f : c.input_folders)
        if (!std::filesystem::exists(f)) return build_error("Please check the given input folder(s). \nThe following input folder does not exist: " + f);
    // what this build cannot do, said before any work
    if (c.output_file_name.empty()) return build_error("Please give the index's file name with --output-filename");
    const int k = (int)c.kmer_size, s = (int)c.syncmer_size, t = (k - s + 1) / 2;    // taxor_build.cpp:509-510 (integer division)
    if (c.use_syncmer && (s >= k || t < 1))
        return build_error("syncmer size " + std::to_string(s) + " with k-mer size " + std::to_string(k) +
                           ": the syncmer size must be smaller than the k-mer size, with k - s >= 1");
    if (!c.use_syncmer && (k > 32 || c.window_size < k))
        return build_error("the minimizer scheme needs k-mer size <= 32 and window size >= k-mer size (k " + std::to_string(k) + ", window " +
                           std::to_string(c.window_size) + ")");
    printf("done!\n");
    printf("parsing taxonomy input files ... ");
    if (orgs.empty()) return build_error("the taxonomy file(s) list no species");
    printf("done!\n");
    printf("creating HIXF layout ... ");
    fflush(stdout);
    // ---- genome lookup (create_filename_clusters, :268-293): one user bin per species, in taxonomy-file order
    {
        const std::map<std::string, std::string> files = build_file_list(c.input_folders);
        for (BuildSpecies &sp : orgs) {
            auto it = files.find(sp.accession);
            if (it == files.end()) return build_error("Could not find a genome file for " + sp.accession);
            sp.path = it->second;
        }
    }
    const uint64_t n = orgs.size();
    uint64_t file_bytes = 0;
    for (const BuildSpecies &sp : orgs) {
        std::error_code ec;
        file_bytes += std::filesystem::file_size(sp.path, ec);
    }
    // ---- scope.  Up front: the selection's density bound on the genome files' bytes.  Every distinct key (8 B), its sorted copy and
    //      the builder's index beside them in device memory: the resident build.  Else, or when the keys may exceed --device-key-budget:
    //      waves into a host store and a construction that keeps a bounded part of the keys on the device.  The refusals that numbers
    //      alone decide come before any HIP call.
    std::vector<uint64_t> key_bound(n);
    uint64_t bound_total = 0;
    for (uint64_t i = 0; i < n; ++i) {
        std::error_code ec;
        const uint64_t b = std::filesystem::file_size(orgs[i].path, ec);
        const std::string ext = std::filesystem::path(orgs[i].path).extension().string();
        key_bound[i] = taxor::key_bound_of_file(b, ext == ".gz" || ext == ".bz2", c.use_syncmer, k, s, t);
        bound_total += key_bound[i];
    }
    uint64_t budget_bytes = c.key_budget_mib << 20;
    bool stream = c.key_budget_mib && bound_total * 8 > budget_bytes;
    if (!stream) {
        uint64_t fr = 0, tot = 0;
        if (taxor_gpu_device_memory(c.device, &fr, &tot) != TAXOR_OK) return build_error(taxor_gpu_last_error());
        if ((double)bound_total * 8.0 * 3.0 > (double)fr) {      // keys, their sorted copy and the builder's index beside them
            stream = true;
            if (!budget_bytes) budget_bytes = fr / 8;
        }
    }
    std::vector<uint64_t> wave_first{0, n};
    if (stream) {
        const int64_t big = taxor::cut_waves(key_bound, budget_bytes / 8, wave_first);
        if (big >= 0)
            return build_error("the distinct keys of " + orgs[big].path + " alone (up to " + std::to_string(key_bound[big] * 8 >> 20) +
                               " MiB) may exceed the device key budget of " + std::to_string(budget_bytes >> 20) + " MiB");
        const std::string no = taxor::host_store_refusal(bound_total, c.host_memory_mib ? c.host_memory_mib << 20 : taxor::host_memory_available());
        if (!no.empty()) return build_error(no);
    }
    // ---- keys: parser threads read whole genome files, the device keys batches of them.  One wave = the genomes [g0, g1) through a keyer
    //      of their own, whose bins are numbered from g0
    const double t_key0 = now();
    taxor_keyer_params kp{};
    kp.kmer_size = (uint32_t)k;
    kp.syncmer_size = (uint32_t)s;
    kp.t_syncmer = (uint32_t)std::max(t, 0);
    kp.use_syncmer = c.use_syncmer ? 1 : 0;
    kp.window_size = (uint64_t)c.window_size;
    kp.scaling = (uint32_t)c.scaling;
    uint64_t n_bases = 0;
    auto key_wave = [&](uint64_t g0, uint64_t g1, taxor_gpu_keyer *kr) -> std::string {
        std::atomic<uint64_t> next_file{g0};
        BoundedQueue<std::unique_ptr<GenomeChunk>> ready((size_t)std::max<long>(2, 2 * c.threads));
        std::vector<std::thread> parsers;
        std::atomic<int> alive{(int)c.threads};
        for (long th = 0; th < c.threads; ++th)
            parsers.emplace_back([&] {
                for (;;) {
                    const uint64_t i = next_file.fetch_add(1);
                    if (i >= g1) break;
                    auto g = std::make_unique<GenomeChunk>();
                    g->bin = (uint32_t)(i - g0);
                    try {
                        fastx::FastxReader rd;
                        if (!rd.open(orgs[i].path)) g->error = "cannot open " + orgs[i].path;
                        std::string id;
                        while (g->error.empty() && rd.next(id, g->bases)) g->off.push_back(g->bases.size());
                    } catch (const std::exception &e) { g->error = orgs[i].path + ": " + e.what(); }
                    ready.push(std::move(g));
                }
                if (--alive == 0) ready.close();
            });
        const uint64_t batch_bases = (uint64_t)256 << 20;
        std::string err;
        {
            std::string bases;
            std::vector<uint64_t> off{0};
            std::vector<uint32_t> bin;
            auto flush = [&]() {
                if (bin.empty() || !err.empty()) return;
                if (taxor_gpu_keyer_add(kr, bases.data(), off.data(), bin.data(), bin.size()) != TAXOR_OK) err = taxor_gpu_last_error();
                bases.clear();
                off.assign(1, 0);
                bin.clear();
            };
            std::unique_ptr<GenomeChunk> g;
            while (ready.pop(g)) {
                if (!g->error.empty()) { if (err.empty()) err = g->error; continue; }
                uint64_t len = 0;
                for (size_t r = 0; r + 1 < g->off.size(); ++r) {
                    bases.append(g->bases, g->off[r], g->off[r + 1] - g->off[r]);
                    off.push_back(bases.size());
                    bin.push_back(g->bin);
                    len += g->off[r + 1] - g->off[r];
                }
                orgs[g0 + g->bin].seq_len = len;                          // sum of the file's record lengths (:522-526)
                n_bases += len;
                g.reset();
                if (bases.size() >= batch_bases) flush();
            }
            flush();
        }
        for (auto &th : parsers) th.join();
        return err;
    };
    taxor_gpu_keyer *kr = nullptr;
    std::unique_ptr<taxor_gpu_keyer, void (*)(taxor_gpu_keyer *)> kr_guard(nullptr, taxor_gpu_keyer_destroy);
    taxor::KeyStore store;
    taxor_keyer_stats ks{};
    const uint64_t *bin_off = nullptr, *d_keys = nullptr;
    const uint64_t n_waves = wave_first.size() - 1;
    // --group-similar: every keyer's bins are sketched while it holds their keys on the device
    const uint32_t sk_m = (uint32_t)c.sketch_size;
    std::vector<uint64_t> sketch;
    std::vector<uint32_t> sketch_len;
    double sketch_seconds = 0;
    if (c.group_similar) {
        sketch.resize(n * sk_m);
        sketch_len.resize(n);
    }
    auto sketch_wave = [&](uint64_t g0, uint64_t g1, const uint64_t *off, const uint64_t *keys_on_device) {
        const double t0 = now();
        const int rc = taxor_gpu_keys_sketch(c.device, keys_on_device, 1, off, g1 - g0, sk_m, sketch.data() + g0 * sk_m, sketch_len.data() + g0);
        sketch_seconds += now() - t0;
        return rc == TAXOR_OK;
    };
    if (stream && !store.reserve(bound_total)) return build_error("no address space for a key store of " + std::to_string(bound_total * 8 >> 20) + " MiB");
    for (uint64_t w = 0; w < n_waves; ++w) {
        const uint64_t g0 = wave_first[w], g1 = wave_first[w + 1];
        kp.n_bins = g1 - g0;
        if (taxor_gpu_keyer_create(c.device, &kp, &kr) != TAXOR_OK) return build_error(taxor_gpu_last_error());
        kr_guard.reset(kr);
        const std::string err = key_wave(g0, g1, kr);
        if (!err.empty()) return build_error(err);
        if (!stream) {
            if (taxor_gpu_keyer_finish(kr, &bin_off, nullptr, &d_keys) != TAXOR_OK) return build_error(taxor_gpu_last_error());
            if (c.group_similar && !sketch_wave(0, n, bin_off, d_keys)) return build_error(taxor_gpu_last_error());
            break;                                                        // (the resident keyer lives until the index is built)
        }
        // the wave's sorted, distinct keys per bin: into the store, and the keyer goes before the next one comes
        const uint64_t *w_off = nullptr, *w_keys = nullptr, *w_dkeys = nullptr;
        if (taxor_gpu_keyer_finish(kr, &w_off, &w_keys, &w_dkeys) != TAXOR_OK) return build_error(taxor_gpu_last_error());
        if (c.group_similar && !sketch_wave(g0, g1, w_off, w_dkeys)) return build_error(taxor_gpu_last_error());
        if (!store.append(w_keys, w_off, g1 - g0)) return build_error("the key store is full: the genomes hold more distinct keys than their density bound");
        taxor_keyer_stats wks{};
        (void)taxor_gpu_keyer_stats(kr, &wks);
        ks.seconds_device += wks.seconds_device;
        kr_guard.reset();
        kr = nullptr;
    }
    if (stream) bin_off = store.bin_off();
    const double t_key1 = now();
    // ---- layout over the exact counts
    std::vector<uint64_t> counts(n);
    for (uint64_t b = 0; b < n; ++b) counts[b] = bin_off[b + 1] - bin_off[b];
    taxor_layout *lay = nullptr;
    uint64_t sim_clusters = 0;
    double pairs_seconds = 0;
    if (c.group_similar) {
        // windows of genomes of similar size: all pairs on the device, single-linkage clusters, and the layout cuts along that order
        std::vector<uint64_t> rank(n);
        const double t0 = now();
        if (taxor_similarity_rank(c.device, sketch.data(), sketch_len.data(), counts.data(), n, sk_m, (uint64_t)c.similarity_window, c.similarity_threshold,
                                  rank.data(), &sim_clusters, nullptr) != TAXOR_OK)
            return build_error(taxor_gpu_last_error());
        pairs_seconds = now() - t0;
        std::vector<uint64_t>().swap(sketch);
        if (taxor_build_layout_ranked(counts.data(), n, c.tmax, rank.data(), &lay) != TAXOR_OK) return build_error("layout failed");
    } else if (taxor_build_layout(counts.data(), n, c.tmax, &lay) != TAXOR_OK)
        return build_error("layout failed");
    std::unique_ptr<taxor_layout, void (*)(taxor_layout *)> lay_guard(lay, taxor_layout_free);
    const uint64_t n_ixf = lay->n_ixf;
    // user bins below each IXF (merged bins need the exact union of their subtree)
    std::vector<std::vector<uint32_t>> below(n_ixf);
    for (uint64_t i = n_ixf; i-- > 0;)
        for (uint64_t b = lay->bin_first[i]; b < lay->bin_first[i + 1]; ++b) {
            if (lay->fname_idx[b] >= 0) {
                if (lay->part[b] == 0) below[i].push_back((uint32_t)lay->fname_idx[b]);
            } else {
                const auto &ch = below[lay->next_ixf[b]];                // children are numbered after their parents
                below[i].insert(below[i].end(), ch.begin(), ch.end());
            }
        }
    std::vector<taxor_ixf_view> views(n_ixf);
    std::vector<std::vector<int64_t>> nx(n_ixf), fn(n_ixf);
    std::vector<uint64_t> key_off{0}, first, count;
    std::vector<uint64_t> bin_first_key, bin_key_count;      // per technical bin, where its keys lie in the store (merged bins: none)
    taxor_ixf_schema schema;
    taxor_ixf_schema_default(&schema);
    uint32_t depth = lay->depth;
    for (uint64_t i = 0; i < n_ixf; ++i) {
        const uint64_t b0 = lay->bin_first[i], nb = lay->ixf_bins[i];
        uint64_t mx = 1;
        for (uint64_t b = b0; b < b0 + nb; ++b) {
            uint64_t sz = 0, f0 = 0;
            if (lay->fname_idx[b] >= 0) {
                const uint64_t ub = (uint64_t)lay->fname_idx[b], m = counts[ub], p = lay->parts[b], j = lay->part[b];
                taxor::key_part_range(bin_off[ub], m, p, j, &f0, &sz);   // contiguous parts of the sorted keys
                first.push_back(f0);
                count.push_back(sz);
            } else {
                const auto &ub = below[lay->next_ixf[b]];
                if (!stream) {
                    if (taxor_gpu_keyer_union_size(kr, ub.data(), ub.size(), &sz) != TAXOR_OK) return build_error(taxor_gpu_last_error());
                } else {
                    // no keyer holds these bins any more: their lists go up from the store.  (What a child brings to the device again
                    // when it is built; a subtree that does not fit the budget is refused here, by the name the builder would use.)
                    std::vector<const uint64_t *> lists;
                    std::vector<uint64_t> lens;
                    uint64_t sum = 0;
                    for (uint32_t u : ub) {
                        lists.push_back(store.keys() + bin_off[u]);
                        lens.push_back(counts[u]);
                        sum += counts[u];
                    }
                    if (sum * 8 > budget_bytes / 2)
                        return build_error("the subtree of IXF " + std::to_string(lay->next_ixf[b]) + " brings " + std::to_string(sum) + " keys (" +
                                           std::to_string(sum * 8 >> 20) + " MiB), more than half the device key budget of " +
                                           std::to_string(budget_bytes >> 20) + " MiB; a smaller --tmax keeps subtrees smaller");
                    if (taxor_gpu_keys_union(c.device, lists.data(), lens.data(), lists.size(), 0, nullptr, 0, 0, &sz) != TAXOR_OK)
                        return build_error(taxor_gpu_last_error());
                }
            }
            key_off.push_back(key_off.back() + (lay->fname_idx[b] >= 0 ? sz : 0));
            bin_first_key.push_back(lay->fname_idx[b] >= 0 ? f0 : 0);
            bin_key_count.push_back(lay->fname_idx[b] >= 0 ? sz : 0);
            mx = std::max(mx, sz);
            nx[i].push_back(lay->next_ixf[b]);
            fn[i].push_back(lay->fname_idx[b]);
        }
        taxor_ixf_view &v = views[i];
        v.bins = nb;
        v.stride = (nb + 63) / 64 * 64;
        v.seg_len = taxor_ixf_seg_len(mx);
        v.seed = schema.default_seed;
        v.data = nullptr;
        v.next_ixf = nx[i].data();
        v.fname_idx = fn[i].data();
        v.src_stride = 0;
    }
    const double t_lay = now();
    const uint64_t *d_arranged = nullptr;
    if (!stream && taxor_gpu_keyer_arrange(kr, first.data(), count.data(), first.size(), &d_arranged) != TAXOR_OK) return build_error(taxor_gpu_last_error());
    // ---- construction on the device
    taxor_hixf_view hv{};
    hv.n_ixf = n_ixf;
    hv.ixf = views.data();
    hv.n_user_bins = n;
    hv.kmer_size = (uint8_t)k;
    hv.syncmer_size = (uint8_t)s;
    hv.t_syncmer = (uint8_t)(c.use_syncmer ? t : 6);                           // build_arguments' default t_syncmer{6u} unless set (:509-510)
    hv.use_syncmer = c.use_syncmer ? 1 : 0;
    hv.scaling = (uint16_t)c.scaling;
    hv.window_size = (uint64_t)c.window_size;
    taxor_gpu_index *idx = nullptr;
    if (taxor_gpu_index_create(&hv, c.device, &idx) != TAXOR_OK) return build_error(taxor_gpu_last_error());
    std::unique_ptr<taxor_gpu_index, void (*)(taxor_gpu_index *)> idx_guard(idx, taxor_gpu_index_destroy);
    // bins without keys (genomes shorter than k) keep what their rows hold: a seeded fill makes that repeatable
    for (uint64_t i = 0; i < n_ixf; ++i)
        if (taxor_gpu_index_fill_random(idx, i, schema.default_seed + i) != TAXOR_OK) return build_error(taxor_gpu_last_error());
    taxor_build_stats bst{};
    if (!stream) {
        if (taxor_gpu_index_build_hixf_ex(idx, d_arranged, 1, key_off.data(), schema.default_seed, &bst) != TAXOR_OK) return build_error(taxor_gpu_last_error());
    } else {
        // a part is a range of the store: nothing is arranged, every technical bin says where its keys lie.  Half the budget: an IXF
        // larger than it is built from two buffers of that size, one peeling while the other fills
        if (taxor_gpu_index_build_hixf_stream_ranges(idx, store.keys(), bin_first_key.data(), bin_key_count.data(), schema.default_seed, budget_bytes / 2, &bst) != TAXOR_OK)
            return build_error(taxor_gpu_last_error());
    }
    printf("done!\n");
    printf("building HIXF index ... ");
    fflush(stdout);
    const double t_build = now();
    std::vector<std::vector<uint8_t>> data(n_ixf);
    uint64_t index_bytes = 0;
    for (uint64_t i = 0; i < n_ixf; ++i) {
        data[i].resize(3 * views[i].seg_len * views[i].stride);
        if (taxor_gpu_index_download_ixf(idx, i, data[i].data(), data[i].size()) != TAXOR_OK) return build_error(taxor_gpu_last_error());
        views[i].data = data[i].data();
        views[i].seed = taxor_gpu_index_ixf_seed(idx, i);
        index_bytes += data[i].size();
    }
    if (!stream) (void)taxor_gpu_keyer_stats(kr, &ks);
    kr_guard.reset();
    idx_guard.reset();
    std::vector<taxor_species> sp(n);
    std::vector<const char *> names(n);
    for (uint64_t i = 0; i < n; ++i) {
        sp[i].organism_name = orgs[i].organism.c_str();
        sp[i].accession_id = orgs[i].accession.c_str();
        sp[i].taxid = orgs[i].taxid.c_str();
        sp[i].taxnames_string = orgs[i].taxnames.c_str();
        sp[i].taxid_string = orgs[i].taxids.c_str();
        sp[i].user_bin = i;
        sp[i].seq_len = orgs[i].seq_len;
        names[i] = orgs[i].path.c_str();
    }
    taxor_hixf_meta meta{};
    meta.window_size = (uint64_t)c.window_size;
    meta.parts = 1;
    meta.compressed = 0;
    meta.n_species = n;
    meta.species = sp.data();
    meta.n_user_bin_filenames = n;
    meta.user_bin_filenames = names.data();
    if (taxor_hixf_store(c.output_file_name.c_str(), &hv, &meta) != TAXOR_OK) return build_error(taxor_gpu_last_error());
    printf("done!\n");
    const double t_end = now();
    uint64_t n_keys = 0;
    for (uint64_t b = 0; b < n; ++b) n_keys += counts[b];
    std::string similar;
    if (c.group_similar) {
        char buf[256];
        snprintf(buf, sizeof buf, "; similar genomes grouped: %llu clusters of more than one genome, sketches %.3f s, pairs and clustering %.3f s",
                 (unsigned long long)sim_clusters, sketch_seconds, pairs_seconds);
        similar = buf;
    }
    fprintf(stderr,
            "taxor build: %llu genomes, %llu bases (%llu file bytes), %llu distinct keys, %llu IXFs, depth %u, %llu index bytes, t_max %llu; "
            "seconds: read+key %.3f (keyer on the device %.3f), layout %.3f, construction %.3f, store %.3f, total %.3f; "
            "path %s: %llu waves, %u groups, %u bin ranges, %u restarts, key uploads %.3f s of which %.3f s were waited for%s\n",
            (unsigned long long)n, (unsigned long long)n_bases, (unsigned long long)file_bytes, (unsigned long long)n_keys,
            (unsigned long long)n_ixf, depth, (unsigned long long)index_bytes, (unsigned long long)lay->t_max, t_key1 - t_key0 - sketch_seconds, ks.seconds_device,
            t_lay - t_key1 - pairs_seconds,
            t_build - t_lay, t_end - t_build, t_end - t_start, stream ? "stream" : "resident", (unsigned long long)n_waves, bst.stream_groups, bst.stream_ranges,
            bst.stream_restarts, bst.seconds_upload + bst.seconds_stream_upload, bst.seconds_upload + bst.seconds_stream_upload_wait, similar.c_str());
    return 0;
}
