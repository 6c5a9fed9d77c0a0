// tools_cmd.h -- the small subcommands: `taxor probe` (a file's IXF record layout), `taxor verify` (positive control for an index of
// foreign provenance), `taxor inflate` (the parallel gzip reader alone) and `taxor reads` (the query reader alone), and the IXF
// variant helpers that `verify` shares with `taxor pin` (pin_cmd.h) and `taxor search --ixf-arithmetic`.  Included by search_main.cpp
// inside its anonymous namespace, after cli_util.h and query_reader.h.

// "kh=0,sm=1,rot=21,red=1,fp=1" -> arithmetic code (taxor_ixf_arith_code); fields left out keep this library's reading
bool parse_arith_spec(const std::string &spec, uint32_t *code)
{
    taxor_ixf_variant v;
    taxor_ixf_variant_default(&v, 0, 1, 64);
    for (const auto &tok : str_split(spec, ',')) {
        const size_t eq = tok.find('=');
        if (eq == std::string::npos) return false;
        const std::string key = tok.substr(0, eq);
        char *end = nullptr;
        const long x = strtol(tok.c_str() + eq + 1, &end, 10);
        if (!end || *end != '\0' || x < 0) return false;
        if (key == "kh" && x <= 3) v.key_hash = (uint8_t)x;
        else if (key == "sm" && x <= 3) v.seed_mode = (uint8_t)x;
        else if (key == "rot" && x >= 1 && x <= 63) v.rot = (uint8_t)x;
        else if (key == "red" && x <= 2) v.reduce = (uint8_t)x;
        else if (key == "fp" && x <= 3) v.fp_mode = (uint8_t)x;
        else return false;
    }
    *code = taxor_ixf_arith_code(&v);
    return true;
}

std::string arith_spec(const taxor_ixf_variant &v)
{
    return "kh=" + std::to_string(v.key_hash) + ",sm=" + std::to_string(v.seed_mode) + ",rot=" + std::to_string(v.rot) + ",red=" +
           std::to_string(v.reduce) + ",fp=" + std::to_string(v.fp_mode);
}

// the readings of the un-vendored IXF that `taxor verify --variants` and `taxor pin` probe a root IXF's RAW bytes under: seed (the
// file's, the prototype's fixed start seed, none) x shape (layout kind x pitch x row order, each with the segment length the
// array length implies and the one the loader took from the file) x key hash x seed entry x rotation step x range reduction x
// fingerprint fold.  `loaded_layout` = the code the loader settled on (its pitch rule says whether root.src_stride is a stored
// scalar).
std::vector<taxor_ixf_variant> variant_family(const taxor_ixf_view &root, uint64_t raw_len, uint32_t loaded_layout)
{
    std::vector<uint64_t> seeds{root.seed};
    for (uint64_t sd : {13572355802537770549ull, 0ull})
        if (std::find(seeds.begin(), seeds.end(), sd) == seeds.end()) seeds.push_back(sd);
    const uint64_t S = (root.bins + 63) / 64 * 64;
    struct Shape { uint32_t layout; uint64_t pitch, seg; };
    std::vector<Shape> shapes;
    auto add_shape = [&](uint32_t layout, uint64_t pitch) {
        if (!pitch || pitch < root.bins || raw_len % pitch != 0) return;
        for (uint64_t sg : {raw_len / pitch / 3, root.seg_len}) {
            if (!sg || 3 * sg * pitch > raw_len) continue;
            bool dup = false;
            for (const Shape &sh : shapes) dup = dup || ((sh.layout & ~taxor::IXF_PITCH_MASK) == (layout & ~taxor::IXF_PITCH_MASK) && sh.pitch == pitch && sh.seg == sg);
            if (!dup) shapes.push_back({layout, pitch, sg});
        }
    };
    // the pitch rule the loader settled on goes first: it fits EVERY IXF's array length (the loader checked), and where two rules
    // give the root the same pitch (a root of 64 k bins: padded == unpadded) the first one added is the one the shape keeps
    const uint32_t loaded_rule = loaded_layout & taxor::IXF_PITCH_MASK;
    auto pitch_of = [&](uint32_t rule) { return rule == taxor::IXF_PITCH_BINS ? root.bins : rule == taxor::IXF_PITCH_STORED ? (root.src_stride ? root.src_stride : root.stride) : S; };
    for (uint32_t pm : {0u, (uint32_t)taxor::IXF_ROWS_POSITION_MAJOR}) {
        for (uint32_t kind : {(uint32_t)taxor::IXF_KIND_ROWS, (uint32_t)taxor::IXF_KIND_BIN_MAJOR}) {
            add_shape(kind | pm | loaded_rule, pitch_of(loaded_rule));
            for (uint32_t rule : {(uint32_t)taxor::IXF_PITCH_PADDED, (uint32_t)taxor::IXF_PITCH_BINS})
                if (rule != loaded_rule) add_shape(kind | pm | rule, pitch_of(rule));
        }
        add_shape(taxor::IXF_KIND_BIT_SLICED | pm, S);
    }
    std::vector<taxor_ixf_variant> vs;
    for (uint64_t sd : seeds)
        for (const Shape &sh : shapes)
            for (int kh = 0; kh < 4; ++kh)
                for (int sm = 0; sm < 3; ++sm)
                    for (int rot : {21, 16, 32})
                        for (int red = 0; red < 3; ++red)
                            for (int fp = 0; fp < 4; ++fp) {
                                if (sd == 0 && sm != 0) continue;        // without a seed the three seed modes coincide
                                taxor_ixf_variant v;
                                taxor_ixf_variant_default(&v, sd, sh.seg, sh.pitch);
                                v.key_hash = (uint8_t)kh; v.seed_mode = (uint8_t)sm; v.rot = (uint8_t)rot;
                                v.reduce = (uint8_t)red; v.fp_mode = (uint8_t)fp; v.layout = (uint16_t)sh.layout;
                                vs.push_back(v);
                            }
    return vs;
}

// hash lists for a variant scan: at most `cap` hashes per list (the score is a ratio; the scan's cost is lists x variants x bins x hashes)
void cap_hash_lists(const uint64_t *hoff, const uint64_t *hs, uint64_t n_lists, uint64_t cap, std::vector<uint64_t> &off_out, std::vector<uint64_t> &hs_out)
{
    off_out.assign(1, 0);
    hs_out.clear();
    for (uint64_t l = 0; l < n_lists; ++l) {
        const uint64_t n = std::min<uint64_t>(cap, hoff[l + 1] - hoff[l]);
        hs_out.insert(hs_out.end(), hs + hoff[l], hs + hoff[l] + n);
        off_out.push_back(hs_out.size());
    }
}

// this library's own reading of the root as the loader took it: arithmetic code 0 in the search layout
bool variant_is_native(const taxor_ixf_variant &v, const taxor_ixf_view &root)
{
    return taxor_ixf_arith_code(&v) == 0 && taxor::ixf_layout_kind(v.layout) == taxor::IXF_KIND_ROWS && !(v.layout & taxor::IXF_ROWS_POSITION_MAJOR) &&
           v.stride == root.stride && v.seg_len == root.seg_len && v.seed == root.seed;
}

// (median best-bin match ratio over the hash lists, variant index), best first
std::vector<std::pair<float, size_t>> rank_variants(const std::vector<taxor_ixf_variant> &vs, const std::vector<float> &ratio, size_t n_lists)
{
    std::vector<std::pair<float, size_t>> rank;
    for (size_t i = 0; i < vs.size(); ++i) {
        std::vector<float> r(ratio.begin() + i * n_lists, ratio.begin() + (i + 1) * n_lists);
        std::sort(r.begin(), r.end());
        rank.push_back({r[r.size() / 2], i});
    }
    std::sort(rank.begin(), rank.end(), [](const auto &a, const auto &b) { return a.first != b.first ? a.first > b.first : a.second < b.second; });
    return rank;
}

int probe_command(int argc, char **argv)                       // hixf-probe: report a file's IXF record layout
{
    const char *path = nullptr;
    for (int i = 2; i < argc; ++i) {
        if (strcmp(argv[i], "--index-file") == 0 && i + 1 < argc) path = argv[++i];
        else if (argv[i][0] != '-') path = argv[i];
    }
    if (!path) die("usage: taxor probe --index-file <file.hixf>");
    taxor_ixf_schema sc;
    std::vector<char> rep(16384);
    const int rc = taxor_hixf_probe(path, &sc, rep.data(), rep.size());
    fputs(rep.data(), stdout);
    if (rc != TAXOR_OK) die(taxor_gpu_last_error());
    printf("schema: n_before=%u n_after=%u idx_bins=%d idx_stride=%d idx_seg_len=%d%s idx_seed=%d\n", sc.n_before, sc.n_after,
           sc.idx_bins, sc.idx_stride, sc.idx_seg_len, sc.seg_len_is_rows ? "(rows)" : "", sc.idx_seed);
    return 0;
}

// `taxor verify`, second part.  Which reading of the un-vendored IXF arithmetic does this file follow?  Probe the raw bytes of the
// root IXF (every indexed genome is in one of its bins, as a leaf or inside a merged bin) under a family of variants.  The scan
// copies the root's RAW bytes to the device in one piece (tens of GB under a 4096-bin root): the resident index has answered
// everything it was needed for, so it goes first (*sr and *gi are destroyed and set to null) instead of sitting beside that copy.
void verify_scan_variants(taxor_hixf *h, const taxor_hixf_view *view, int device, taxor_gpu_searcher **sr, taxor_gpu_index **gi,
                          const std::string &bases, const std::vector<uint64_t> &offsets)
{
    const uint64_t n_lists = std::min<uint64_t>(24, offsets.size() - 1);
    const uint64_t *hoff = nullptr, *hs = nullptr;
    if (taxor_gpu_syncmers(*sr, bases.data(), offsets.data(), n_lists, &hoff, &hs) != TAXOR_OK) die(taxor_gpu_last_error());
    const taxor_ixf_view &root = view->ixf[0];
    const uint64_t raw_len = taxor_hixf_ixf_raw_bytes(h, 0);
    std::vector<taxor_ixf_variant> vs = variant_family(root, raw_len, view->ixf_layout);
    std::vector<uint64_t> s_off, s_hs;
    cap_hash_lists(hoff, hs, n_lists, 160, s_off, s_hs);
    taxor_gpu_searcher_destroy(*sr);
    taxor_gpu_index_destroy(*gi);
    *sr = nullptr;
    *gi = nullptr;
    std::vector<float> ratio(vs.size() * n_lists);
    if (taxor_gpu_ixf_variant_scan(device, root.data, raw_len, root.bins, vs.data(), (uint32_t)vs.size(), s_hs.data(), s_off.data(), n_lists, ratio.data()) != TAXOR_OK)
        die(taxor_gpu_last_error());
    const std::vector<std::pair<float, size_t>> rank = rank_variants(vs, ratio, (size_t)n_lists);
    printf("variant scan of the root IXF (%zu readings of its %llu raw fingerprint bytes, %llu hash lists): median best-bin match ratio\n", vs.size(),
           (unsigned long long)raw_len, (unsigned long long)n_lists);
    char desc[512];
    for (size_t i = 0; i < std::min<size_t>(5, rank.size()); ++i) {
        const taxor_ixf_variant &v = vs[rank[i].second];
        taxor_ixf_variant_describe(&v, desc, sizeof desc);
        printf("  %.4f  %s%s\n", rank[i].first, desc, variant_is_native(v, root) ? "   [this library's reading, ixf_arith.h, in the search layout]" : "");
    }
    if (rank.empty() || rank[0].first < 0.9f) {
        printf("no variant answers: the key hash (wyhash / minimiser value) or the genome is not what the index holds\n");
        return;
    }
    const taxor_ixf_variant &bv = vs[rank[0].second];
    const bool is_mine = variant_is_native(bv, root);
    printf("%s\n", is_mine ? "the file follows this library's reading of the IXF arithmetic, in the search layout"
                           : "the file follows ANOTHER reading of the IXF (first line)");
    if (is_mine) return;
    char ld[128];
    taxor_ixf_layout_describe(bv.layout, ld, sizeof ld);
    if (bv.seed != root.seed)
        printf("that reading also uses another seed than the loader took from the file: `taxor probe` shows the record layout\n");
    else {
        const bool as_it_lies = taxor::ixf_layout_kind(bv.layout) == taxor::IXF_KIND_ROWS && !(bv.layout & taxor::IXF_ROWS_POSITION_MAJOR) && bv.stride == root.stride &&
                                bv.seg_len == root.seg_len;
        printf("search it with: taxor search%s%s%s%s ...\n", taxor_ixf_arith_code(&bv) ? " --ixf-arithmetic " : "",
               taxor_ixf_arith_code(&bv) ? arith_spec(bv).c_str() : "", as_it_lies ? "" : " --ixf-layout ", as_it_lies ? "" : ld);
    }
}

// Positive control for an index whose provenance is not this library: error-free windows cut
// from a genome that IS in the index must find (nearly) all of their hashes in one user bin.  A match ratio near
// the false-positive floor instead means that the hash (wyhash / minimiser) or the IXF arithmetic (seed, row
// stride, segment length) read from the file does not describe this index -- the two un-vendored boundaries.
int verify_command(int argc, char **argv)
{
    std::string index_file, genome_file;
    uint64_t n_reads = 2000, read_len = 5000;
    int device = 0;
    bool scan_variants = false;
    uint32_t verify_arith = 0, verify_layout = 0;
    bool layout_given = false;
    for (int i = 2; i < argc; ++i) {
        if (strcmp(argv[i], "--variants") == 0) { scan_variants = true; continue; }
        if (strcmp(argv[i], "--index-file") == 0 && i + 1 < argc) index_file = argv[++i];
        else if (strcmp(argv[i], "--genome-file") == 0 && i + 1 < argc) genome_file = argv[++i];
        else if (strcmp(argv[i], "--reads") == 0 && i + 1 < argc) n_reads = strtoull(argv[++i], nullptr, 10);
        else if (strcmp(argv[i], "--read-len") == 0 && i + 1 < argc) read_len = strtoull(argv[++i], nullptr, 10);
        else if (strcmp(argv[i], "--gpu") == 0 && i + 1 < argc) device = atoi(argv[++i]);
        else if (strcmp(argv[i], "--ixf-arithmetic") == 0 && i + 1 < argc) {
            if (!parse_arith_spec(argv[++i], &verify_arith)) die("--ixf-arithmetic: expected kh=..,sm=..,rot=..,red=..,fp=..");
        }
        else if (strcmp(argv[i], "--ixf-layout") == 0 && i + 1 < argc) {
            if (taxor_ixf_layout_parse(argv[++i], &verify_layout) != TAXOR_OK) die(taxor_gpu_last_error());
            layout_given = true;
        }
    }
    if (index_file.empty() || genome_file.empty() || !file_exists(index_file) || !file_exists(genome_file) || !n_reads || !read_len)
        die("usage: taxor verify --index-file <x.hixf> --genome-file <fasta of a genome contained in the index> [--reads n] [--read-len l]");
    taxor_hixf *h = nullptr;
    if (taxor_hixf_load(index_file.c_str(), &h) != TAXOR_OK) die(taxor_gpu_last_error());
    taxor_hixf_set_arith(h, verify_arith);
    if (layout_given && taxor_hixf_set_layout(h, verify_layout) != TAXOR_OK) die(taxor_gpu_last_error());
    const taxor_hixf_view *view = taxor_hixf_get_view(h);
    taxor_gpu_index *gi = nullptr;
    if (taxor_gpu_index_create(view, device, &gi) != TAXOR_OK) die(taxor_gpu_last_error());
    taxor_gpu_search_params prm{};
    prm.ratio = 0.05;                                  // report every bin holding >= 5 % of a window's hashes
    prm.model = TAXOR_THR_PERCENTAGE;
    taxor_gpu_searcher *sr = nullptr;
    if (taxor_gpu_searcher_create(gi, &prm, &sr) != TAXOR_OK) die(taxor_gpu_last_error());
    // windows: evenly spaced over the concatenated records, never across a record boundary
    std::string genome, id, bases;
    std::vector<uint64_t> rec_off{0};
    try {
        fastx::FastxReader rd;
        if (!rd.open(genome_file)) die("cannot open " + genome_file);
        while (rd.next(id, genome)) rec_off.push_back(genome.size());
    } catch (const std::exception &e) { die(e.what()); }
    std::vector<uint64_t> offsets{0};
    for (size_t r = 0; r + 1 < rec_off.size(); ++r) {
        const uint64_t len = rec_off[r + 1] - rec_off[r];
        if (len < read_len) continue;
        const uint64_t want = std::max<uint64_t>(1, n_reads * len / std::max<uint64_t>(1, genome.size()));
        const uint64_t step = std::max<uint64_t>(1, (len - read_len) / want);
        for (uint64_t p = 0; p + read_len <= len && offsets.size() <= n_reads; p += step) {
            bases.append(genome, rec_off[r] + p, read_len);
            offsets.push_back(bases.size());
        }
    }
    if (offsets.size() < 2) die("no record of the genome file is as long as --read-len");
    taxor_gpu_results res{};
    if (taxor_gpu_search_batch(sr, bases.data(), offsets.data(), offsets.size() - 1, &res) != TAXOR_OK) die(taxor_gpu_last_error());
    std::vector<double> best;
    std::map<int64_t, uint64_t> votes;
    uint64_t hashes = 0;
    for (uint64_t r = 0; r < res.n_reads; ++r) {
        uint32_t top = 0;
        int64_t top_bin = -1;
        for (uint64_t i = res.read_off[r]; i < res.read_off[r + 1]; ++i)
            if (res.count[i] > top) { top = res.count[i]; top_bin = res.user_bin[i]; }
        if (res.n_hashes[r]) best.push_back((double)top / (double)res.n_hashes[r]);
        if (top_bin >= 0) ++votes[top_bin];
        hashes += res.n_hashes[r];
    }
    std::sort(best.begin(), best.end());
    const double median = best.empty() ? 0.0 : best[best.size() / 2], low = best.empty() ? 0.0 : best[best.size() / 20];
    int64_t winner = -1;
    uint64_t winner_votes = 0;
    for (const auto &kv : votes)
        if (kv.second > winner_votes) { winner = kv.first; winner_votes = kv.second; }
    printf("windows %llu x %llu bp, %.1f hashes per window (%s, k=%u)\n", (unsigned long long)res.n_reads, (unsigned long long)read_len,
           res.n_reads ? (double)hashes / (double)res.n_reads : 0.0, view->use_syncmer ? "open syncmers" : "minimisers", (unsigned)view->kmer_size);
    printf("best-bin match ratio: median %.4f, 5th percentile %.4f (false-positive floor %.4f)\n", median, low, 1.0 / 256.0);
    if (winner >= 0) printf("most frequent best user bin: %lld (%llu of %llu windows)\n", (long long)winner, (unsigned long long)winner_votes, (unsigned long long)res.n_reads);
    const bool pass = median >= 0.9 && low >= 0.5;
    printf("%s\n", pass ? "PASS: the index answers for this genome -- hashing and IXF arithmetic match the file"
                        : "FAIL: an indexed genome must match itself; check `taxor probe` (seed / stride / segment length) and the hash");
    if (scan_variants || !pass) verify_scan_variants(h, view, device, &sr, &gi, bases, offsets);
    if (sr) taxor_gpu_searcher_destroy(sr);
    if (gi) taxor_gpu_index_destroy(gi);
    taxor_hixf_free(h);
    return pass ? 0 : 2;
}

// the parallel gzip reader alone: `taxor inflate --query-file x.fastq.gz [--threads n] [--chunk-mb m] [--output-file out]`
// decompresses (to a file, or nowhere) and reports the rate, the output's CRC-32 and how many chunks had to be decoded twice
int inflate_command(int argc, char **argv)
{
    std::string in, out_path;
    unsigned threads = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
    size_t chunk = 0;
    for (int i = 2; i < argc; ++i) {
        if (strcmp(argv[i], "--query-file") == 0 && i + 1 < argc) in = argv[++i];
        else if (strcmp(argv[i], "--threads") == 0 && i + 1 < argc) threads = (unsigned)atoi(argv[++i]);
        else if (strcmp(argv[i], "--chunk-mb") == 0 && i + 1 < argc) chunk = (size_t)(atof(argv[++i]) * 1048576.0);
        else if (strcmp(argv[i], "--output-file") == 0 && i + 1 < argc) out_path = argv[++i];
    }
    if (in.empty() || !file_exists(in)) die("usage: taxor inflate --query-file <x.gz> [--threads n] [--chunk-mb m] [--output-file out]");
    fastx::ParallelGz g;
    const double t0 = now();
    if (!g.open(in, threads, chunk, 0)) die(in + " is not a gzip file");
    FILE *of = out_path.empty() ? nullptr : fopen(out_path.c_str(), "wb");
    if (!out_path.empty() && !of) die("cannot write " + out_path);
    std::vector<char> buf;
    uint64_t total = 0;
    try {
        // chunk by chunk, the buffers changing hands like in `search` (ParallelGz::take): a copy out of them on this one thread
        // would be the limit (~5 GB/s) before the inflating threads are
        while (g.take(buf)) {
            total += buf.size();
            if (of && fwrite(buf.data(), 1, buf.size(), of) != buf.size()) die("write error on " + out_path);
            g.recycle(std::move(buf));
            buf = std::vector<char>();
        }
    } catch (const std::exception &e) { die(e.what()); }
    if (of) fclose(of);
    const double dt = now() - t0;
    printf("%llu bytes in %.3f s = %.2f GB/s on %u threads; %llu member(s), %llu chunks, %llu decoded again from a corrected start; CRC-32 and length of every member verified\n",
           (unsigned long long)total, dt, total / 1e9 / dt, threads, (unsigned long long)g.members, (unsigned long long)g.chunks_total, (unsigned long long)g.chunks_redecoded);
    printf("worker seconds: block search %.3f, decode %.3f, marker resolution + CRC %.3f\n", g.ns_find / 1e9, g.ns_decode / 1e9, g.ns_resolve / 1e9);
    printf("memory held by the reader at most: %.1f MB (largest chunk %.1f MB)\n", fastx::ParallelGz::memory_high_water() / 1048576.0, g.largest_chunk_bytes() / 1048576.0);
    return 0;
}

int reads_command(int argc, char **argv)                       // reader check: id, length, FNV-1a of every record
{
    ReaderOptions cfg;
    std::string query_file;
    bool allow_ranges = true, summary_only = false;
    for (int i = 2; i < argc; ++i) {
        if (strcmp(argv[i], "--query-file") == 0 && i + 1 < argc) query_file = argv[++i];
        else if (strcmp(argv[i], "--threads") == 0 && i + 1 < argc) cfg.threads = (unsigned)atoi(argv[++i]);
        else if (strcmp(argv[i], "--batch-reads") == 0 && i + 1 < argc) cfg.batch_reads = strtoull(argv[++i], nullptr, 10);
        else if (strcmp(argv[i], "--batch-bases") == 0 && i + 1 < argc) cfg.batch_bases = strtoull(argv[++i], nullptr, 10);      // (tests: small parser jobs)
        else if (strcmp(argv[i], "--sequential") == 0) allow_ranges = false;
        else if (strcmp(argv[i], "--summary-only") == 0) summary_only = true;      // the reader's rate: no record is printed or hashed
    }
    if (cfg.threads == 0) cfg.threads = 1;
    if (query_file.empty() || !file_exists(query_file)) die("usage: taxor reads --query-file <fasta|fastq[.gz]|bam> [--threads n] [--batch-reads n] [--batch-bases n] [--sequential] [--summary-only]");
    std::mutex mu;
    std::map<uint64_t, std::unique_ptr<Batch>> got;
    BatchPool pool;
    pool.cap = ~size_t(0);                                        // this check keeps every batch
    const double dt = produce_batches(query_file, cfg, allow_ranges, pool, [&](std::unique_ptr<Batch> b) {
        if (b->end_of_file) return;
        std::lock_guard<std::mutex> lk(mu);
        got.emplace(b->seq, std::move(b));
    });
    uint64_t n = 0, nb = 0, expect = 0;
    for (const auto &kv : got) {
        if (kv.first != expect++) die("batch numbering has a gap");
        const Batch &b = *kv.second;
        std::string restored;
        if (summary_only) { n += b.ids.size(); nb += b.offsets.back(); continue; }
        for (size_t r = 0; r < b.ids.size(); ++r) {
            const uint64_t lo = b.offsets[r], len = b.offsets[r + 1] - lo;
            if (b.raw_kind == 'B') {        // BAM: the read the record stands for (reverse-complemented back where flag 0x10 is set)
                restored.clear();
                bam::restore_read((const uint8_t *)b.raw.data() + b.nib_off[r], b.nib_len[r], b.nib_rev[r] != 0, restored);
                printf("%s\t%llu\t%016llx\n", b.ids.str(r).c_str(), (unsigned long long)len, (unsigned long long)fnv1a(restored.data(), restored.size()));
            } else
                printf("%s\t%llu\t%016llx\n", b.ids.str(r).c_str(), (unsigned long long)len, (unsigned long long)fnv1a(b.bases.data() + lo, len));
            ++n;
            nb += len;
        }
    }
    fprintf(stderr, "%llu reads, %llu bases, %zu batches, %.3f s\n", (unsigned long long)n, (unsigned long long)nb, got.size(), dt);
    return 0;
}
