// census_cmd.h -- `taxor census`: how many hashes every reference has in an index, and how full every IXF is, counted on the device from
// the resident fingerprints (census.hip; the sums and the text are census_format.h's).  `taxor search
// --coverage-breadth` takes the same census through census_of.  Included by search_main.cpp inside its anonymous namespace, after
// tools_cmd.h and before search_cmd.h.

struct CensusRun {
    taxor::census_tables tables;
    double seconds_wall = 0, seconds_kernel = 0;
    uint64_t bytes_read = 0, n_tiles = 0;
    uint32_t launches = 0;
};

// one census of a resident index, summed per user bin and per IXF through the view it was created from
CensusRun census_of(taxor_gpu_index *gi, const taxor_hixf_view *view)
{
    CensusRun out;
    const double t0 = now();
    taxor_gpu_census *c = nullptr;
    if (taxor_gpu_census_create(gi, &c) != TAXOR_OK) die(taxor_gpu_last_error());
    taxor_census_results r{};
    if (taxor_gpu_census_run(c, 0, 0, &r) != TAXOR_OK) die(taxor_gpu_last_error());
    if (r.n_ixf != view->n_ixf) die("census: the index holds " + std::to_string(r.n_ixf) + " IXFs, its file " + std::to_string(view->n_ixf));
    std::vector<taxor::census_ixf> fs(view->n_ixf);
    for (uint64_t x = 0; x < view->n_ixf; ++x) {
        const taxor_ixf_view &f = view->ixf[x];
        if (r.bin_first[x + 1] - r.bin_first[x] != f.bins) die("census: IXF " + std::to_string(x) + " has another bin count on the device than in its file");
        fs[x] = taxor::census_ixf{f.bins, f.seg_len, f.stride, f.fname_idx};
    }
    taxor::census_sum(fs.data(), view->n_ixf, r.nonzero, view->n_user_bins, out.tables);
    out.seconds_kernel = r.seconds_kernel;
    out.bytes_read = r.bytes_read;
    out.n_tiles = r.n_tiles;
    out.launches = r.launches;
    taxor_gpu_census_destroy(c);
    out.seconds_wall = now() - t0;
    return out;
}

int census_command(int argc, char **argv)
{
    std::string index_file, refs_file, ixfs_file;
    int device = 0;
    uint32_t layout = 0;
    bool layout_given = false;
    for (int i = 2; i < argc; ++i) {
        if (strcmp(argv[i], "--index-file") == 0 && i + 1 < argc) index_file = argv[++i];
        else if (strcmp(argv[i], "--output-file") == 0 && i + 1 < argc) refs_file = argv[++i];
        else if (strcmp(argv[i], "--ixf-file") == 0 && i + 1 < argc) ixfs_file = argv[++i];
        else if (strcmp(argv[i], "--gpu") == 0 && i + 1 < argc) device = atoi(argv[++i]);
        else if (strcmp(argv[i], "--ixf-layout") == 0 && i + 1 < argc) {
            if (taxor_ixf_layout_parse(argv[++i], &layout) != TAXOR_OK) die(taxor_gpu_last_error());
            layout_given = true;
        }
        else die(std::string("taxor census: unknown or incomplete option ") + argv[i]);
    }
    if (index_file.empty() || refs_file.empty())
        die("usage: taxor census --index-file <x.hixf> --output-file <refs.tsv> [--ixf-file <ixfs.tsv>] [--gpu n] [--ixf-layout spec]  (--index-file and --output-file are required)");
    if (!file_exists(index_file)) die("Validation failed for option --index-file: The file " + index_file + " does not exist.");
    taxor_hixf *h = nullptr;
    if (taxor_hixf_load(index_file.c_str(), &h) != TAXOR_OK) die(taxor_gpu_last_error());
    if (layout_given && taxor_hixf_set_layout(h, layout) != TAXOR_OK) die(taxor_gpu_last_error());
    const taxor_hixf_view *view = taxor_hixf_get_view(h);
    const taxor_hixf_meta *meta = taxor_hixf_get_meta(h);
    FILE *rf = fopen(refs_file.c_str(), "wb");
    if (!rf) die("cannot open output file " + refs_file);
    FILE *xf = ixfs_file.empty() ? nullptr : fopen(ixfs_file.c_str(), "wb");
    if (!ixfs_file.empty() && !xf) die("cannot open IXF file " + ixfs_file);
    const double t0 = now();
    taxor_gpu_index *gi = nullptr;
    const int rc = taxor_gpu_index_create(view, device, &gi);
    if (rc != TAXOR_OK) die(std::string(taxor_gpu_last_error()) + (rc == TAXOR_E_NOMEM ? "\n(taxor census counts a resident index: a paged one is not counted)" : ""));
    const double t1 = now();
    const CensusRun cr = census_of(gi, view);
    // the species of a user bin as the search names it (the first that carries it, species[0] if none)
    std::vector<uint32_t> bin_species(view->n_user_bins, 0u);
    for (uint64_t i = meta->n_species; i-- > 0;)
        if (meta->species[i].user_bin < view->n_user_bins) bin_species[meta->species[i].user_bin] = (uint32_t)i;
    std::string text = taxor::census_ref_header();
    uint64_t flagged = 0;
    for (uint64_t b = 0; b < view->n_user_bins; ++b) {
        static const taxor_species none{"-", "-", "-", "-", "-", 0, 0};
        const taxor_species &sp = meta->n_species ? meta->species[bin_species[b]] : none;
        taxor::census_ref_line(text, sp.accession_id, sp.organism_name, sp.taxid, sp.seq_len, cr.tables.leaf_bins[b], cr.tables.index_hashes[b]);
        flagged += cr.tables.index_hashes[b].flagged;
    }
    if (fwrite(text.data(), 1, text.size(), rf) != text.size() || fclose(rf) != 0) die("cannot write to " + refs_file + ": " + strerror(errno));
    if (xf) {
        text = taxor::census_ixf_header();
        for (uint64_t x = 0; x < view->n_ixf; ++x)
            taxor::census_ixf_line(text, x, view->ixf[x].bins, cr.tables.ixf[x].leaf_bins, view->ixf[x].seg_len, view->ixf[x].stride, cr.tables.ixf[x].max_bin_keys);
        if (fwrite(text.data(), 1, text.size(), xf) != text.size() || fclose(xf) != 0) die("cannot write to " + ixfs_file + ": " + strerror(errno));
    }
    printf("census: %llu user bins (%llu with a leaf bin that is no peeled filter: NA), %llu IXFs, %.3f GB of fingerprints\n", (unsigned long long)view->n_user_bins,
           (unsigned long long)flagged, (unsigned long long)view->n_ixf, cr.bytes_read / 1e9);
    printf("index resident in %.3f s; census %.3f s wall, %.3f ms in its kernel = %.1f GB/s (%llu tiles, %u launch%s)\n", t1 - t0, cr.seconds_wall, cr.seconds_kernel * 1e3,
           cr.seconds_kernel > 0 ? cr.bytes_read / 1e9 / cr.seconds_kernel : 0.0, (unsigned long long)cr.n_tiles, cr.launches, cr.launches == 1 ? "" : "es");
    taxor_gpu_index_destroy(gi);
    taxor_hixf_free(h);
    return 0;
}
