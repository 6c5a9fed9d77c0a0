// search_cmd.h -- `taxor search`: options, one index file against its query files (search_files), by one of two routes: the index
// resident on the devices and the host stages overlapped (search_resident), or an index larger than device memory searched in
// resident passes (search_paged).  DESIGN.md, "CLI host", names the stages and who owns which shared state.  Included by
// search_main.cpp inside its anonymous namespace, after query_reader.h, tools_cmd.h and profile_cmd.h.

struct Config : ReaderOptions {              // taxor_search_configuration.hpp:8-20
    std::string index_file, query_file, report_file;
    double threshold = -1.0, error_rate = 0.04;
    std::vector<int> gpus{0};   // devices that classify batches in parallel, each with its own index replica
    std::string expect_file;    // --expect: a TSV the reference wrote for the same reads and index, compared per read
    bool sequential = false;    // --sequential: one reader thread per file, no byte-range cutting (any legal FASTA/FASTQ)
    uint32_t ixf_arith = 0;     // --ixf-arithmetic: the reading of the un-vendored IXF arithmetic the index follows (0 = this library's)
    bool layout_given = false;  // --ixf-layout: how the file stores each IXF's fingerprints (ixf_layout.h); transposed on the device at load
    uint32_t ixf_layout = 0;
    uint64_t group_reads = 0;   // reads per GPU batch, made of queued chunks (0: 131072, or --batch-reads when that is given)
    uint64_t index_budget_mib = 0;   // hidden --device-index-budget: fingerprint bytes on the device at a time; the index is searched in resident passes
    bool paged_replay = false;       // hidden --paged-replay: the query file is read in the first resident pass only, the later ones replay the reads' saved hash lists
    bool paged_reread = false;       // hidden --paged-reread: every resident pass reads the query file again (the default, said aloud; wins over --paged-replay)
    std::string coverage_file;  // --coverage-file: per user bin the reads, the hash matches and the DISTINCT matched hashes of the whole run (coverage.hip)
    bool coverage_breadth = false;     // --coverage-breadth: the coverage file gains INDEX_HASHES, BREADTH, EXPECTED_BREADTH, BREADTH_RATIO (census.hip)
    uint32_t coverage_precision = 0;   // hidden --coverage-precision: registers per sketch = 2^this, in [4,16] (0: the library's 12)
    std::string lca_file;       // --lca-file: one line per read, its lowest common ancestor (lca.hip)
    std::string kraken_file;    // --report-file: Kraken-style clade report of the whole run
    std::string report_unit;    // --report-unit reads | bases (empty: reads): which tally fills the report's first three columns
    bool lca_mode() const { return !lca_file.empty() || !kraken_file.empty(); }
    double lca_confidence = -1.0;      // --lca-confidence: share of a read's hashes a call must have behind it, in [0,1] (below 0: not given; confidence.hip)
    bool confidence_mode() const { return lca_confidence >= 0.0; }
    std::string hitmap_file;    // --hitmap-file: one line per (read, reference) line of the TSV, the hits along the read's hash list (hitmap.hip)
    uint32_t hitmap_segments = 0;      // hidden --hitmap-segments: parts the ordered hash list is cut into, in [1,64] (0: 16)
    std::string breakpoint_file;       // --breakpoint-file: one line per read whose hash list splits between two of its references (breakpoint.hip)
    uint32_t breakpoint_min_gain = 0;  // --breakpoint-min-gain: hits the split must explain beyond the best single reference, >= 1 (0: not given, 1)
    std::string segments_file;         // --segments-file: one line per segment of a read whose best path among its references switches (segments.hip)
    uint32_t segments_switch_cost = 0; // --segments-switch-cost: hits a switch of reference costs, in [1,2^20] (0: not given, 16)
    bool base_positions = false;       // --base-positions: every hash's position in its read is captured (positions.hip); the two files above gain base columns
    std::string exclusive_file;        // --exclusive-file: per user bin the hashes that no other reference on a read's list holds, over the whole run (exclusive.hip)
    std::string exclusive_reads_file;  // --exclusive-reads-file: the same per line of the TSV, for reads with two candidates or more
    uint32_t exclusive_precision = 0;  // hidden --exclusive-precision: registers per sketch = 2^this, in [4,16] (0: the library's 12)
    bool exclusive_mode() const { return !exclusive_file.empty() || !exclusive_reads_file.empty(); }
    std::string gather;         // several devices: "rccl" | "host" (taxor_gpu_comm transports) | "none" (independent workers, each
                                // fetching its own results); empty = rccl when the devices are distinct, host when one repeats
};

void usage()
{
    fprintf(stderr,
            "taxor search - Queries files of DNA sequences against a list of HIXF index files (MI355X)\n"
            "  --index-file <f[,f..]>   taxor index file(s) containing HIXF index and reference information (required); syncmer\n"
            "                           indexes of k-mer size 2..32 and syncmer size 1..31 (below the k-mer size), minimiser indexes\n"
            "                           of k-mer size 1..32\n"
            "  --query-file <f[,f..]>   file(s) containing sequences to query against the index: FASTA or FASTQ, plain, .gz or .bz2, or BAM\n"
            "                           (unaligned or aligned; recognised by content; secondary and supplementary records are left out and\n"
            "                           reads stored reverse-complemented are restored, as `samtools fastq` does); kinds may be mixed\n"
            "  --output-file <f>        file name for the resulting output\n"
            "  --threads <1..32>        host threads parsing the query file (plain FASTA/FASTQ; gzip is one stream) and rendering\n"
            "                           the report; default 4-16 by the size of the machine (the reference's default of 1 is its\n"
            "                           classifying thread; here one host thread cannot feed the GPU)\n"
            "  --percentage <0..1>      if set, this threshold is used instead of the syncmer model\n"
            "  --error-rate <0..1>      expected error rate of the reads (default 0.04)\n"
            "  --gpu <id>               device ordinal (default 0)\n"
            "  --gpus <n>               use devices 0..n-1: the index is replicated, batches of reads are sharded\n"
            "  --gpu-list <a,b,..>      explicit device list (a device may be listed twice)\n"
            "  --gather <rccl|host|none> several devices: index broadcast + per-round gather of the results on the first device over\n"
            "                           RCCL/xGMI (default), the same staged through host memory, or independent workers\n"
            "  --batch-reads <n>        reads per parsed chunk (default: about 128 MB of query file, 65536 reads for gzip)\n"
            "  --sequential             read every query file front to back on one thread (FASTQ whose records wrap their lines)\n"
            "  --device-parse           plain FASTA / four-line FASTQ: the byte ranges go to the device as they are read and the records are\n"
            "                           found there (the host parses a range only where the device reports it irregular); compressed\n"
            "                           and --sequential input is parsed on the host as without the switch; a BAM file ignores it (its\n"
            "                           records are walked on the host and its 4-bit sequences unpacked on the device in any case)\n"
            "  --group-reads <n>        reads per GPU batch, made of whole chunks (default 131072; --batch-reads if that is given)\n"
            "  --ixf-arithmetic <spec>  search an index whose fingerprints follow another reading of the IXF arithmetic than this\n"
            "                           build's (the spec `taxor verify --variants` prints: kh=..,sm=..,rot=..,red=..,fp=..)\n"
            "  --ixf-layout <spec>      search an index whose fingerprint vectors are laid out otherwise than data[row*stride + bin]\n"
            "                           (the spec `taxor verify --variants` / `taxor pin` print, e.g. bin-major,unpadded,segment-major);\n"
            "                           they are transposed on the device while the index is uploaded\n"
            "  --coverage-file <f>      per reference that any read reported: the reads, their QHASH_MATCH summed, the number of DISTINCT\n"
            "                           index hashes they matched (a sketch's estimate) and the ratio of the two; ONE index file, ONE device\n"
            "  --coverage-breadth       with --coverage-file: per reference also its hashes in the index and the share of them the sample hit\n"
            "  --lca-file <f>           one line per read: C or U, the read, the taxid of the lowest common ancestor of the references it\n"
            "                           matched, its length, hash count, best match and the number of references  } ONE index file, ONE\n"
            "  --report-file <f>        Kraken-style report: per taxon the reads of its clade and its own            } device; --output-file\n"
            "  --report-unit <reads|bases> what --report-file counts (default reads)                                } is then optional\n"
            "  --lca-confidence <0..1>  with --lca-file / --report-file: a read is called at the deepest taxon of its call's lineage that this share\n"
            "                           of its hashes supports, or not at all; the call file gains SUPPORT, LCA_TAXID, LCA_SUPPORT\n"
            "  --hitmap-file <f>        per line of --output-file that a read with hashes produced: in which sixteenth of the read's ordered hash\n"
            "                           list the reference's hits lie (a chimeric read, an inserted element, one conserved operon); ONE index\n"
            "                           file, ONE device; --output-file is then optional\n"
            "  --breakpoint-file <f>    per read whose ordered hash list splits between two of the references it reported: where the split lies,\n"
            "                           the two references and the hits the split explains beyond the best single reference (a chimeric read,\n"
            "                           an inserted element, a host/microbe junction); ONE index file, ONE device; --output-file is then optional\n"
            "  --breakpoint-min-gain <n> with --breakpoint-file: report a read from this many hits gained on (default 1)\n"
            "  --segments-file <f>      per read whose ordered hash list is best explained by SEVERAL of the references it reported, one after the\n"
            "                           other: one line per segment (where it lies, its reference, its hits) and the read's shape, split, insert or\n"
            "                           mosaic (a chimeric read, a prophage or IS element inside a chromosome read, a concatemer); ONE index file,\n"
            "                           ONE device; --output-file is then optional\n"
            "  --segments-switch-cost <n> with --segments-file: the hits a switch of reference must pay for, in [1,1048576] (default 16)\n"
            "  --base-positions         with --breakpoint-file and/or --segments-file, syncmer indexes only: every hash's position in its read is\n"
            "                           recorded on the device (the first base at which the read shows the hashed k-mer, on either strand), and\n"
            "                           the files gain real base columns at the end of each line: LEFT_END_BASE, BREAK_BASE / BASE_START, BASE_END\n"
            "                           (where the reference's tie rule skips a k-mer's first occurrence the position is that earlier occurrence;\n"
            "                           a read of more than 2048 hashes is swept once per 2048)\n"
            "  --exclusive-file <f>    per reference that was a candidate of any read: its hits, and how many of them are hashes that NO other\n"
            "                           reference the same read reported holds (which of several near-identical strains a read supports); ONE\n"
            "                           index file, ONE device; --output-file is then optional\n"
            "  --exclusive-reads-file <f> the same per line of --output-file, for reads with two candidates or more; alone or beside --exclusive-file\n"
            "  --expect <tsv>           compare the output per read with a TSV the reference wrote for the same input (exit 3 if it differs)\n"
            "search to profile in one run (the options of `taxor profile`; results go from the device's search buffers into the profile's\n"
            "device pipeline, no TSV is written or parsed in between):\n"
            "  --cami-report-file <f>   CAMI profile of genomic abundances      } all three are required as soon as one of the options\n"
            "  --binning-file <f>       CAMI binning file (read -> taxid)       } of this group is given; --output-file is then optional\n"
            "  --sample-id <id>         identifier of the sample                } (given, the TSV is written as well)\n"
            "  --seq-abundance-file <f> sequence abundances in CAMI format (including unclassified reads)\n"
            "  --min-abundance <0..1>   minimum abundance to report (default 0.001)\n"
            "  --em-steps <1..1000>     steps of the expectation maximisation (default 100)\n"
            "                           Limits of this mode: ONE index file and ONE device (--gpus above 1, a --gpu-list of several\n"
            "                           devices and a comma list of index files are refused), and every read id -- the header up to its\n"
            "                           first space -- must occur once: `taxor profile` merges the lines of reads that share an id into\n"
            "                           one read, this mode refuses such input and names the id.\n");
}

void advanced_help()
{
    usage();
    fprintf(stderr, "advanced:\n"
                    "  --device-index-budget <MiB> at most this many MiB of the index's fingerprints on the device at a time, in [1,16777216]: the root\n"
                    "                           IXF stays resident, the subtrees under its merged bins are searched group by group (one pass\n"
                    "                           over the query file per group, the file is parsed -- a .gz inflated -- once per pass) and every\n"
                    "                           read's results are merged on the device.  Taken by itself when the index exceeds the device's\n"
                    "                           free memory.  ONE device, a query file that can be read again (no pipe); the output is\n"
                    "                           byte-identical to the resident search.  A BAM query file is read once per pass like any other.\n"
                    "  --paged-replay           with --device-index-budget: read, inflate, pack and hash the query in the first pass only; every\n"
                    "                           read's hash list is kept in host memory (8 bytes per hash) and the later passes replay the lists\n"
                    "                           without opening the file.  Same output.  When the lists' bound does not fit the host's available\n"
                    "                           memory the run reads the file again in every pass instead, and says so.  Not the default: it has\n"
                    "                           not been measured against re-reading from a file yet (docs/EXPERIMENTS.md).\n"
                    "  --coverage-file <f>      columns ACCESSION, REFERENCE_NAME, TAXID, REF_LEN, READS, HASH_MATCHES, DISTINCT_HASHES, DUPLICITY; one line per\n"
                    "                           user bin with READS > 0, in the index's user-bin order.  READS and HASH_MATCHES are by construction what one\n"
                    "                           gets by counting the lines of --output-file per accession and user bin and summing their QHASH_MATCH (the\n"
                    "                           lines that survive the 0.8 * max filter).  DISTINCT_HASHES: for every such line the read's hashes are looked\n"
                    "                           up in the reference's own leaf bins, and those found go into a HyperLogLog sketch per user bin (4096 byte\n"
                    "                           registers, standard error 1.6 %%); the column is its rounded estimate, at least 1 where HASH_MATCHES > 0.\n"
                    "                           DUPLICITY = HASH_MATCHES / DISTINCT_HASHES (0.00 where both are 0): near the depth for a genome that is\n"
                    "                           there, in the thousands for a handful of shared hashes hit again and again.  The searchers keep every\n"
                    "                           batch's hash lists in host memory until the batch is accumulated.  Refused: a comma list of index files,\n"
                    "                           several devices, a --gather transport, and an index that has to be paged (--device-index-budget below\n"
                    "                           the index's size, or an index larger than the device's free memory).\n"
                    "  --coverage-breadth       with --coverage-file: every line gains INDEX_HASHES, BREADTH, EXPECTED_BREADTH, BREADTH_RATIO.  INDEX_HASHES: the\n"
                    "                           keys of the reference's leaf bins, estimated once, when the index is resident, from the nonzero bytes of\n"
                    "                           their columns (nonzero * 256 / 255 per bin, standard deviation sqrt(n / 255): a key owns one slot, a free\n"
                    "                           slot stays 0; `taxor census` writes the same numbers for every reference).  BREADTH = min(1,\n"
                    "                           DISTINCT_HASHES / INDEX_HASHES); EXPECTED_BREADTH = 1 - exp(-HASH_MATCHES / INDEX_HASHES), what uniform\n"
                    "                           sampling at this depth would cover; BREADTH_RATIO their quotient: near 1 for a genome that is there, far\n"
                    "                           below for hits piled on a few shared hashes.  Reported, not thresholded.  NA where a leaf bin is no peeled\n"
                    "                           filter (more nonzero bytes than its IXF has room for keys) or INDEX_HASHES is 0; the ratio also where the\n"
                    "                           expectation prints as 0.0000.  Limits: 8-bit fingerprints, free slots assumed zero.\n"
                    "  --lca-file <f>           columns STATUS, QUERY_NAME, TAXID, QUERY_LEN, QHASH_COUNT, BEST_QHASH_MATCH, REFERENCES; one line per read in the\n"
                    "                           order --output-file lists the reads in.  The references of a read are the lines --output-file prints for\n"
                    "                           it (the tuples that survive the 0.8 * max filter); each reference's path is the non-empty ids of its\n"
                    "                           TAX_ID_STR, and TAXID is the last id of the paths' longest common prefix: 1 (root) where they share none.\n"
                    "                           A read whose best match is 0 is unclassified (U, TAXID 0, and 0 in the last three columns): a read\n"
                    "                           without a hash reports every reference with QHASH_MATCH 0, and --output-file prints those lines, but\n"
                    "                           nothing matched.  The index's taxonomy must be a tree: an id with two parents, an id twice in one path,\n"
                    "                           more than 64 ids or fewer names than ids in one path are refused with the ids and accessions involved.\n"
                    "  --report-file <f>        six tab-separated columns per taxon: percentage of the clade (%%6.2f of all reads), reads (or bases) of the clade,\n"
                    "                           reads called exactly there, rank code (U, R, D, P, C, O, F, G, S from the k p c o f g s prefixes of TAX_STR,\n"
                    "                           - otherwise), taxid, name indented by two spaces per depth.  unclassified first, then the tree from the\n"
                    "                           root, depth-first, children by clade count descending and taxid ascending; empty clades are left out.\n"
                    "                           Both options: a comma list of index files, several devices, a --gather transport and an index that has\n"
                    "                           to be paged are refused; without --output-file the per-read tuples never leave the device.\n"
                    "  --lca-confidence <C>     with --lca-file / --report-file.  A read's call above comes from the references within 0.8 of its best match\n"
                    "                           alone, however few of the read's hashes they hold.  With the option every hash of the read is looked up in\n"
                    "                           the leaf bins of EVERY reference the search reported for it (the survivors and the others); a hash stands\n"
                    "                           behind depth d of the call's lineage when a reference that found it shares the lineage's first d taxa, and\n"
                    "                           it counts once, however many references or parts of a split reference hold it.  The read is called at the\n"
                    "                           deepest taxon, from the call upwards, with at least C * QHASH_COUNT hashes behind it; U (TAXID 0) if not\n"
                    "                           even the root has them.  0 gives the calls above.  Both files come from these calls.  The call file gains\n"
                    "                           three columns: SUPPORT (hashes behind the taxon printed; behind the root for a read the threshold made U,\n"
                    "                           which keeps its real QHASH_COUNT, BEST_QHASH_MATCH and REFERENCES), LCA_TAXID (the call without a\n"
                    "                           threshold) and LCA_SUPPORT (hashes behind that); a read that was U anyway prints zeros.  The searchers keep\n"
                    "                           every batch's hash lists in host memory until the batch is called.  Refused like --lca-file.\n"
                    "  --hitmap-file <f>        columns QUERY_NAME, ACCESSION, TAXID, QUERY_LEN, QHASH_COUNT, QHASH_MATCH, LOCATED, SEGMENT_SIZES, SEGMENT_HITS; one\n"
                    "                           line per line of --output-file (the tuples that survive the 0.8 * max filter), in its order, except the\n"
                    "                           lines of a read without a hash (QHASH_COUNT 0: nothing to locate).  The read's hashes are kept in the order\n"
                    "                           of their first occurrence along the read; hash i of n lies in segment floor(i * S / n), and segment j\n"
                    "                           holds ceil((j+1) * n / S) - ceil(j * n / S) of them (SEGMENT_SIZES; zeros where n < S).  The segments cut\n"
                    "                           the ORDERED HASH LIST, not the bases: a hash list carries no positions, so a segment is a stretch of the\n"
                    "                           read only as far as its hashes are spread evenly.  SEGMENT_HITS: per segment the hashes found in at least\n"
                    "                           one of the reference's own leaf bins; LOCATED is their sum (QHASH_MATCH for a reference stored in one bin;\n"
                    "                           a reference split over several bins counts a hash once here and once per part there).  Both last columns\n"
                    "                           are comma lists of S numbers.  The searchers keep every batch's hash lists in host memory until the batch\n"
                    "                           is located.  Refused: a comma list of index files, several devices, a --gather transport, and an index\n"
                    "                           that has to be paged.\n"
                    "  --hitmap-segments <S>    with --hitmap-file: the number of segments, in [1,64] (default 16).\n"
                    "  --breakpoint-file <f>    columns QUERY_NAME, QUERY_LEN, QHASH_COUNT, CANDIDATES, BEST_ACCESSION, BEST_TAXID, BEST_LOCATED, BREAK_HASH,\n"
                    "                           BREAK_BASE_APPROX, LEFT_ACCESSION, LEFT_TAXID, LEFT_HITS, LEFT_HITS_OF_RIGHT, RIGHT_ACCESSION, RIGHT_TAXID, RIGHT_HITS,\n"
                    "                           RIGHT_HITS_OF_LEFT, GAIN; one line per reported read, in input order.  The CANDIDATES of a read are ALL the\n"
                    "                           references the search reported for it with QHASH_MATCH > 0, not only the lines of --output-file (the minor\n"
                    "                           partner of a chimera lies below the 0.8 * max filter); a read with a hash and two candidates or more is\n"
                    "                           examined.  Every hash of the read is looked up in every candidate's own leaf bins (--hitmap-file's lookup).\n"
                    "                           For a break in front of hash p of the ordered list, split(p) = the most hits any candidate has among the\n"
                    "                           hashes before p + the most any has from p on; BREAK_HASH is the smallest p with the greatest split, LEFT\n"
                    "                           and RIGHT the candidates that attain the two maxima there (the first in the search's order on a tie), and\n"
                    "                           GAIN = that split - BEST_LOCATED, the hits of the best single candidate.  A read is written when GAIN >=\n"
                    "                           --breakpoint-min-gain, so never for GAIN 0; LEFT and RIGHT then differ.  LEFT_HITS_OF_RIGHT and\n"
                    "                           RIGHT_HITS_OF_LEFT are the other reference's hits on that side.  BREAK_BASE_APPROX = floor(BREAK_HASH *\n"
                    "                           QUERY_LEN / QHASH_COUNT): the list carries no positions, so this is the base only as far as the read's\n"
                    "                           hashes are spread evenly (--hitmap-file's caveat).  A partner that did not pass the search threshold was\n"
                    "                           never reported and cannot be a candidate: lower --percentage to look for short inserts.  The searchers keep\n"
                    "                           every batch's hash lists in host memory until the batch is examined.  Refused: a comma list of index\n"
                    "                           files, several devices, a --gather transport, and an index that has to be paged.\n"
                    "  --segments-file <f>      columns QUERY_NAME, QUERY_LEN, QHASH_COUNT, CANDIDATES, SEGMENTS, SHAPE, PATH_HITS, SINGLE_HITS, SEGMENT, HASH_START,\n"
                    "                           HASH_END, BASE_START_APPROX, BASE_END_APPROX, ACCESSION, TAXID, HITS, BEST_ACCESSION, BEST_TAXID, HITS_OF_BEST; one\n"
                    "                           line per segment of a reported read, reads in input order, SEGMENT counting from 0.  Candidates, examined\n"
                    "                           reads and the lookup are --breakpoint-file's.  A path gives every hash of the ordered list to one candidate;\n"
                    "                           it scores the hashes that match the candidate they were given to, minus --segments-switch-cost for every\n"
                    "                           change of candidate.  The best path is found exactly (a Viterbi pass on the device); among equally good\n"
                    "                           paths the one with the fewest switches is taken, so a switch that gains nothing is never reported, and\n"
                    "                           equal candidates go to the first in the search's order.  A read is written when its path has two segments\n"
                    "                           or more.  SHAPE, from the references of the segments alone: split (two segments), insert (three, the outer\n"
                    "                           two the same reference: a prophage, an IS element), mosaic (anything else).  PATH_HITS is the sum of HITS,\n"
                    "                           SINGLE_HITS the hits of the best single candidate (BEST_*), HITS_OF_BEST that candidate's hits inside the\n"
                    "                           segment; PATH_HITS - cost * (SEGMENTS - 1) >= SINGLE_HITS.  BASE_*_APPROX = floor(HASH_* * QUERY_LEN /\n"
                    "                           QHASH_COUNT): the list carries no positions (--hitmap-file's caveat).  A partner that did not pass the\n"
                    "                           search threshold was never reported and cannot be a candidate: lower --percentage to look for short\n"
                    "                           inserts.  Beside --breakpoint-file every hash is looked up twice, once per option.  Refused: a comma list of\n"
                    "                           index files, several devices, a --gather transport, and an index that has to be paged.\n"
                    "  --segments-switch-cost <n> with --segments-file: an integer in [1,1048576], default 16.  The default is a choice, not a measurement: at\n"
                    "                           k = 22, s = 12 about one base in 11 starts a syncmer, so 16 hits are roughly 180 bases of exact match, and\n"
                    "                           an inner segment, which pays twice, has to beat its flank by some 350 bases' worth of hits -- less than the\n"
                    "                           mobile elements people look for.\n"
                    "  --base-positions         with --breakpoint-file and/or --segments-file; refused without either, and for a minimiser or k-mer index\n"
                    "                           (their lists are not deduplicated and their values are not wyhash(k-mer)).  For a read of L bases, k-mer\n"
                    "                           size k and its ordered hash list, pos[i] = min { p in [0, L-k] : wyhash(min(f_p, revcomp(f_p))) == hash i },\n"
                    "                           f_p the k-mer at base p after the dna4 mapping: the first base at which the read shows this k-mer, on either\n"
                    "                           strand.  It is computed on the device while the batch's packed reads are resident, one more kernel per\n"
                    "                           sub-batch, and kept beside the saved hash lists, 4 bytes per hash.  Existing columns stay as they are; appended\n"
                    "                           at the end of the header and of every line: --breakpoint-file LEFT_END_BASE = pos[BREAK_HASH - 1] + k and\n"
                    "                           BREAK_BASE = pos[BREAK_HASH]; --segments-file BASE_START = pos[HASH_START] and BASE_END = pos[HASH_END - 1] + k\n"
                    "                           (exclusive, at most QUERY_LEN).  The position is defined by CONTENT.  It is the start of the window that first\n"
                    "                           emitted the hash except where the reference's stateful tie rule leaves a k-mer's first occurrence unselected\n"
                    "                           and selects a later one (homopolymers, short tandem repeats): pos is then the earlier occurrence, and positions\n"
                    "                           need not increase along the list.  Cost: the read's list is taken in pieces of 2048 hashes, and every k-mer of\n"
                    "                           the read is hashed once per piece: a read with P pieces is swept P times (a 1-Mbp read: some 90,000 hashes, 45\n"
                    "                           sweeps).\n"
                    "  --exclusive-file <f>     columns ACCESSION, TAXID, CANDIDATE_READS, HITS, EXCLUSIVE_HITS, EXCLUSIVE_READS, DISTINCT_EXCLUSIVE,\n"
                    "                           EXCLUSIVE_FRACTION; one line per reference that was a candidate of an examined read, in the coverage file's\n"
                    "                           order.  Candidates and the lookup are --breakpoint-file's (every tuple of the read with a match, not only the\n"
                    "                           TSV's lines); a read is examined when it has a hash and at least ONE candidate.  A hash of the read is\n"
                    "                           exclusive to a candidate when that candidate matches it and no other candidate of the same read does, shared\n"
                    "                           when two or more do.  HITS sums the candidate's matches over its reads, EXCLUSIVE_HITS the exclusive ones,\n"
                    "                           EXCLUSIVE_READS counts the reads that gave it at least one, DISTINCT_EXCLUSIVE is a sketch's estimate of the\n"
                    "                           distinct exclusive hashes (the coverage file's sketch, at least 1 where EXCLUSIVE_HITS is above 0), and\n"
                    "                           EXCLUSIVE_FRACTION = EXCLUSIVE_HITS / HITS with four decimals, 0.0000 without hits -- reported, not\n"
                    "                           thresholded: 0.5 is no verdict.  Two limits.  Exclusivity is relative to the references the read REPORTED: a\n"
                    "                           reference below the search threshold is not a tuple and takes no hash away.  And fingerprints have 8 bits: a\n"
                    "                           foreign leaf bin answers yes at about 1/256, so a truly exclusive hash is lost at about (leaf bins of the other\n"
                    "                           candidates)/256, and a candidate that shares nothing still shows about QHASH_COUNT * leaves/256 hits, most of\n"
                    "                           them exclusive.  Refused: a comma list of index files, several devices, a --gather transport, and an index\n"
                    "                           that has to be paged.  Beside --breakpoint-file or --segments-file every hash is looked up once per option.\n"
                    "  --exclusive-reads-file <f> columns QUERY_NAME, ACCESSION, TAXID, QUERY_LEN, QHASH_COUNT, QHASH_MATCH, HITS, EXCLUSIVE_HITS, CANDIDATES, MATCHED,\n"
                    "                           SHARED; for every examined read with two candidates or more one line per line of --output-file, reads in\n"
                    "                           input order.  MATCHED counts the read's hashes that any candidate matches, SHARED those that two or more do:\n"
                    "                           the candidates' EXCLUSIVE_HITS (lines below the 0.8 * max filter included) and SHARED add up to MATCHED.\n"
                    "  --exclusive-precision <p> with --exclusive-file: registers per sketch = 2^p, in [4,16] (default 12).\n"
                    "  --paged-reread          the default said aloud: read the query file again in every pass; wins over --paged-replay.\n"
                    "BAM input: the BGZF blocks are inflated on --threads threads, one thread walks the records (block_size, flag, l_seq, read_name)\n"
                    "                           and copies the 4-bit SEQ fields into a page-locked buffer; CIGAR, QUAL and tags are never read.  A\n"
                    "                           missing BGZF end-of-file block is a warning; CRAM and SAM text are refused.  With TAXOR_CLI_TRACE the\n"
                    "                           run reports how many records were skipped as secondary or supplementary.\n");
}

// seqan3's FASTA/FASTQ readers drop white space and digits inside sequences (numbered or column-formatted files).  The
// parsers here append sequence lines raw -- a scan per byte would halve their rate for files that never need it -- and
// the device reports any character outside dna15 (TAXOR_E_ALPHABET); only then is the batch cleaned, in place, and run
// again.  Returns false if there was nothing to remove (the batch really holds a foreign character).
bool strip_space_and_digits(Batch &b)
{
    char *d = &b.bases[0];
    size_t w = 0;
    bool any = false;
    for (size_t r = 0; r + 1 < b.offsets.size(); ++r) {
        const size_t lo = b.offsets[r], hi = b.offsets[r + 1];
        b.offsets[r] = w;
        for (size_t i = lo; i < hi; ++i) {
            const unsigned char c = (unsigned char)d[i];
            if (c == ' ' || (c >= '\t' && c <= '\r') || (c >= '0' && c <= '9')) { any = true; continue; }
            d[w++] = (char)c;
        }
    }
    b.offsets.back() = w;
    b.bases.resize(w);          // shrinks: never reallocates, a page-locked buffer stays where it is
    return any;
}

// run() classifies `chunks` (anything whose elements point to a Batch); where the device met a character outside dna15, the chunks
// are cleaned and, if that removed anything, run once more
template <class Run, class Chunks> int run_with_alphabet_retry(Run &&run, Chunks &chunks)
{
    int rc = run();
    if (rc == TAXOR_E_ALPHABET) {
        bool any = false;
        for (auto &bt : chunks) any = strip_space_and_digits(*bt) || any;
        if (any) rc = run();
    }
    return rc;
}

// `--expect ref.tsv`: compare this run's output with a TSV the reference produced for the same reads and index
// (the day a published .hixf and its reference output are at hand).  The reference writes the lines
// of one read together but, with --threads > 1, the reads in no particular order (sync_out.hpp:24-29): reads are
// matched by id, the lines of a read are compared in order (the HIXF's DFS order).  Returns the number of differing reads.
uint64_t compare_tsv(const std::string &ours, const std::string &expect)
{
    auto load = [](const std::string &path, std::map<std::string, std::vector<std::string>> &by_read, std::vector<std::string> &order) {
        FILE *f = fopen(path.c_str(), "rb");
        if (!f) die("cannot open " + path);
        std::string line;
        std::vector<char> buf(1 << 20);
        std::string carry;
        size_t n;
        auto take = [&](const std::string &l) {
            if (l.empty() || l[0] == '#') return;
            const size_t tab = l.find('\t');
            const std::string id = l.substr(0, tab);
            auto it = by_read.find(id);
            if (it == by_read.end()) { it = by_read.emplace(id, std::vector<std::string>()).first; order.push_back(id); }
            it->second.push_back(l);
        };
        while ((n = fread(buf.data(), 1, buf.size(), f)) > 0) {
            size_t a = 0;
            for (size_t i = 0; i < n; ++i)
                if (buf[i] == '\n') {
                    carry.append(buf.data() + a, i - a);
                    if (!carry.empty() && carry.back() == '\r') carry.pop_back();
                    take(carry);
                    carry.clear();
                    a = i + 1;
                }
            carry.append(buf.data() + a, n - a);
        }
        if (!carry.empty()) take(carry);
        fclose(f);
    };
    std::map<std::string, std::vector<std::string>> a, b;
    std::vector<std::string> oa, ob;
    load(ours, a, oa);
    load(expect, b, ob);
    uint64_t same = 0, differ = 0, only_ours = 0, only_expect = 0, shown = 0;
    for (const auto &id : oa) {
        const auto it = b.find(id);
        if (it == b.end()) { ++only_ours; continue; }
        if (it->second == a[id]) { ++same; continue; }
        ++differ;
        if (shown++ < 10) {
            printf("read %s differs:\n", id.c_str());
            for (const auto &l : a[id]) printf("  ours    %s\n", l.c_str());
            for (const auto &l : it->second) printf("  expect  %s\n", l.c_str());
        }
    }
    for (const auto &id : ob)
        if (!a.count(id)) ++only_expect;
    printf("compared with %s: %llu reads identical, %llu differ, %llu only in this run, %llu only in the expected file\n", expect.c_str(),
           (unsigned long long)same, (unsigned long long)differ, (unsigned long long)only_ours, (unsigned long long)only_expect);
    const uint64_t bad = differ + only_ours + only_expect;
    printf("%s\n", bad == 0 ? "PASS: per-read output identical to the expected TSV"
                            : "FAIL: output differs from the expected TSV (run `taxor verify` to test the index arithmetic)");
    return bad;
}

// ---- search to profile in one run (`taxor search --cami-report-file ... --binning-file ... --sample-id ...`).
// The GPU workers hand every batch's device-resident results to a profile feed (profile_feed.hip); the host keeps the read ids, cut
// at the first space (taxor_profile.cpp:124-125), in input order.  At the end: rank the ids byte-wise, finish the feed, run the
// profile, write the three files through the part `taxor profile` writes them with (profile_write_outputs).
struct FusedProfile {
    taxor_gpu_profile_feed *feed = nullptr;
    const taxor_hixf_meta *meta = nullptr;
    std::atomic<uint64_t> next_read{0};        // the next batch's first index in the feed
    double t_feed = 0;                         // seconds inside taxor_gpu_profile_feed_add_batch, summed over workers
    std::vector<uint32_t> bin_species;         // user bin -> species (the first that names it, species[0] if none: taxor_search.cpp:172-178,289)
    std::vector<int32_t> ref_of_bin;
    std::vector<std::string_view> accs;        // distinct accessions of the index in byte-wise order: reference id -> accession
    std::string id_data;                       // read ids in input order
    std::vector<uint64_t> id_off{0}, feed_index;   // feed_index[i] = the index input read i has in the feed

    void begin(const taxor_hixf_view *view, const taxor_hixf_meta *m, int device)
    {
        meta = m;
        if (m->n_species == 0) die("the index names no species: nothing to profile against");
        const uint64_t nb = view->n_user_bins;
        bin_species.assign(nb, 0u);
        for (uint64_t i = m->n_species; i-- > 0;)
            if (m->species[i].user_bin < nb) bin_species[m->species[i].user_bin] = (uint32_t)i;
        for (uint64_t u = 0; u < nb; ++u) accs.emplace_back(m->species[bin_species[u]].accession_id);
        std::sort(accs.begin(), accs.end());
        accs.erase(std::unique(accs.begin(), accs.end()), accs.end());
        ref_of_bin.resize(nb);
        std::vector<uint64_t> ref_len_of_bin(nb);
        for (uint64_t u = 0; u < nb; ++u) {
            const taxor_species &sp = m->species[bin_species[u]];
            ref_of_bin[u] = (int32_t)(std::lower_bound(accs.begin(), accs.end(), std::string_view(sp.accession_id)) - accs.begin());
            ref_len_of_bin[u] = sp.seq_len;
        }
        if (taxor_gpu_profile_feed_create(device, nb, ref_of_bin.data(), ref_len_of_bin.data(), accs.size(), &feed) != TAXOR_OK) die(taxor_gpu_last_error());
    }

    // one chunk, in input order (the sequencer)
    void take_ids(const Batch &bt)
    {
        for (size_t r = 0; r < bt.ids.size(); ++r) {
            const char *p = bt.ids.ptr(r);
            size_t n = bt.ids.len(r);
            if (const void *sp = memchr(p, ' ', n)) n = (size_t)((const char *)sp - p);
            id_data.append(p, n);
            id_off.push_back(id_data.size());
            feed_index.push_back(bt.feed_first + r);
        }
    }

    std::string_view id(uint64_t i) const { return std::string_view(id_data.data() + id_off[i], id_off[i + 1] - id_off[i]); }

    // input reads in byte-wise order of their ids (bytes compared as unsigned, like std::string::operator<): ranges sorted on
    // `threads` threads, then merged pairwise
    std::vector<uint32_t> sorted_reads(unsigned threads) const
    {
        const uint64_t n = feed_index.size();
        std::vector<uint32_t> order(n);
        for (uint64_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
        auto less = [&](uint32_t a, uint32_t b) { const int c = id(a).compare(id(b)); return c != 0 ? c < 0 : a < b; };
        const uint64_t parts = std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)threads, 16, n / 65536 + 1}));
        std::vector<uint64_t> cut(parts + 1);
        for (uint64_t t = 0; t <= parts; ++t) cut[t] = n * t / parts;
        {
            std::vector<std::thread> th;
            for (uint64_t t = 0; t < parts; ++t) th.emplace_back([&, t] { std::sort(order.begin() + (std::ptrdiff_t)cut[t], order.begin() + (std::ptrdiff_t)cut[t + 1], less); });
            for (auto &x : th) x.join();
        }
        for (uint64_t w = 1; w < parts; w *= 2) {
            std::vector<std::thread> th;
            for (uint64_t t = 0; t + w < parts; t += 2 * w)
                th.emplace_back([&, t, w] {
                    std::inplace_merge(order.begin() + (std::ptrdiff_t)cut[t], order.begin() + (std::ptrdiff_t)cut[t + w],
                                       order.begin() + (std::ptrdiff_t)cut[std::min(parts, t + 2 * w)], less);
                });
            for (auto &x : th) x.join();
        }
        return order;
    }

    void finish(const ProfileConfig &c, unsigned threads, double seconds_search)
    {
        const double t0 = now();
        const uint64_t n = feed_index.size();
        if (n != next_read.load()) die("internal: the profile feed was given " + std::to_string(next_read.load()) + " reads, the sequencer saw " + std::to_string(n));
        if (n >= (1ull << 32)) die("more than 2^32 - 1 reads: search to profile in one run numbers reads in 32 bits");
        const std::vector<uint32_t> order = sorted_reads(threads);
        for (uint64_t k = 1; k < n; ++k)
            if (id(order[k - 1]) == id(order[k]))
                die("read id " + std::string(id(order[k])) + " occurs twice in the query (reads " + std::to_string(order[k - 1] + 1) + " and " + std::to_string(order[k] + 1) +
                    "); search to profile in one run needs unique read ids -- write a TSV with --output-file alone and run `taxor profile`, which merges such reads");
        std::vector<uint64_t> rank(n);                      // by feed index
        for (uint64_t k = 0; k < n; ++k) rank[feed_index[order[k]]] = k;
        const double t_ranked = now();
        taxor_gpu_profile *gp = nullptr;
        if (taxor_gpu_profile_feed_finish(feed, rank.data(), n, &gp) != TAXOR_OK) die(taxor_gpu_last_error());
        std::vector<uint64_t>().swap(rank);
        if (taxor_gpu_profile_run(gp, (uint32_t)c.em_steps, 0) != TAXOR_OK) die(taxor_gpu_last_error());
        taxor_profile_results res{};
        taxor_profile_csr csr{};
        const int64_t *match_bin = nullptr;
        if (taxor_gpu_profile_results(gp, &res) != TAXOR_OK || taxor_gpu_profile_feed_matches(feed, &csr, &match_bin) != TAXOR_OK) die(taxor_gpu_last_error());
        printf("Number of EM steps needed: %u\n", res.em_steps_needed);
        fflush(stdout);
        const double t_device = now();
        // the taxonomy strings of an accession are those of its first line in the TSV (taxor_profile.cpp:142-146): of the user bin
        // whose match comes first in input order.  That needs a look at the matches only where user bins of different species
        // share an accession
        std::vector<uint32_t> ref_species(accs.size(), ~0u);
        uint64_t open_refs = 0;
        {
            std::vector<uint8_t> shared(accs.size(), 0);
            for (uint64_t u = 0; u < ref_of_bin.size(); ++u) {
                uint32_t &sp = ref_species[(uint64_t)ref_of_bin[u]];
                if (sp == ~0u) sp = bin_species[u];
                else if (sp != bin_species[u]) shared[(uint64_t)ref_of_bin[u]] = 1;
            }
            for (uint8_t x : shared) open_refs += x;
            if (open_refs) {
                std::vector<uint32_t> rank_of_input(n);
                for (uint64_t k = 0; k < n; ++k) rank_of_input[order[k]] = (uint32_t)k;
                for (uint64_t i = 0; i < n && open_refs; ++i)
                    for (uint64_t j = csr.read_off[rank_of_input[i]]; j < csr.read_off[rank_of_input[i] + 1] && open_refs; ++j) {
                        if (match_bin[j] < 0) continue;
                        const uint64_t x = (uint64_t)ref_of_bin[(uint64_t)match_bin[j]];
                        if (!shared[x]) continue;
                        ref_species[x] = bin_species[(uint64_t)match_bin[j]];
                        shared[x] = 0;
                        --open_refs;
                    }
            }
        }
        ProfileNames nm;
        nm.n_reads = n;
        nm.n_refs = accs.size();
        nm.read_off = csr.read_off;
        nm.read_id = [&](uint64_t r) { return id(order[r]); };
        nm.accession = [&](uint64_t x) { return accs[x]; };
        nm.tax_id_str = [&](uint64_t x) { return std::string_view(meta->species[ref_species[x]].taxid_string); };
        nm.tax_str = [&](uint64_t x) { return std::string_view(meta->species[ref_species[x]].taxnames_string); };
        nm.match_tax_id = [&](uint64_t i) { return match_bin[i] < 0 ? std::string_view() : std::string_view(meta->species[bin_species[(uint64_t)match_bin[i]]].taxid); };
        const std::string err = profile_write_outputs(c, res, nm);
        if (!err.empty()) die(err);
        const double t_end = now();
        fprintf(stderr, "taxor search (profile): %llu reads, %llu references, %llu matches, %llu reference pairs, %u EM iterations; seconds: search %.3f "
                        "(feed %.3f inside), rank %.3f, device %.3f (rounds %.3f, EM %.3f), write %.3f, profile total %.3f\n",
                (unsigned long long)n, (unsigned long long)accs.size(), (unsigned long long)csr.n_matches, (unsigned long long)res.n_pairs, res.em_iterations,
                seconds_search, t_feed, t_ranked - t0, t_device - t_ranked, res.seconds_filter, res.seconds_em, t_end - t_device, t_end - t0);
        taxor_gpu_profile_destroy(gp);
        taxor_gpu_profile_feed_destroy(feed);
        feed = nullptr;
    }
};

// What outlives one index file: the options, the report, the profile feed, and the totals the run closes with.
struct SearchRun {
    Config cfg;
    ProfileConfig prof;             // search to profile in one run: the options of `taxor profile` (profile_cmd.h)
    bool profile_mode = false, write_tsv = true;
    std::string gpus_option;        // --gpus / --gpu-list as given (named when the profile options refuse several devices)
    FILE *out = nullptr;
    FusedProfile fused;             // search to profile in one run (profile_mode)
    taxor_gpu_coverage *coverage = nullptr;   // --coverage-file: the accumulator beside the resident index, for the whole run
    taxor_lineage_view lineage_view{};
    taxor_lineage *lineage = nullptr;         // --lca-file / --report-file: the index's taxonomy as a tree (lineage.h) ...
    taxor_gpu_lca *lca = nullptr;             // ... and the accumulator beside the resident index, for the whole run (lca.hip)
    FILE *lca_out = nullptr;                  // --lca-file; written by the sequencer, which sees the chunks in input order
    taxor_gpu_confidence *confidence = nullptr;   // --lca-confidence: stands in for `lca` (confidence.hip); fed from the saved hash lists
    double t_confidence = 0, t_confidence_kernels = 0;   // seconds inside taxor_gpu_confidence_add_batch and in its kernels, summed over workers
    uint64_t confidence_probes = 0, confidence_steps = 0, confidence_steps_full = 0;
    taxor_gpu_hitmap *hitmap = nullptr;       // --hitmap-file: the hit map beside the resident index, for the whole run (hitmap.hip)
    FILE *hitmap_out = nullptr;               // --hitmap-file; written by the sequencer as well
    std::vector<uint32_t> hitmap_species;     // user bin -> the species the TSV names for it
    double t_hitmap = 0, t_hitmap_kernels = 0;   // seconds inside taxor_gpu_hitmap_add_batch and in its kernels, summed over workers
    uint64_t hitmap_probes = 0, hitmap_lines = 0;
    taxor_gpu_breakpoint *breakpoint = nullptr;   // --breakpoint-file: the object beside the resident index, for the whole run (breakpoint.hip)
    FILE *breakpoint_out = nullptr;           // --breakpoint-file; written by the sequencer as well
    std::vector<uint32_t> breakpoint_species; // user bin -> the species the TSV names for it
    double t_breakpoint = 0, t_breakpoint_kernels = 0;   // seconds inside taxor_gpu_breakpoint_add_batch and in its kernels, summed over workers
    uint64_t breakpoint_lookups = 0, breakpoint_lines = 0, breakpoint_examined = 0, breakpoint_reads = 0;
    taxor_gpu_segments *segments = nullptr;   // --segments-file: the object beside the resident index, for the whole run (segments.hip)
    FILE *segments_out = nullptr;             // --segments-file; written by the sequencer as well
    std::vector<uint32_t> segments_species;   // user bin -> the species the TSV names for it
    double t_segments = 0, t_segments_kernels = 0;       // seconds inside taxor_gpu_segments_add_batch and in its kernels, summed over workers
    double t_positions_kernels = 0;           // --base-positions: seconds between the event pairs around k_hash_positions, summed over batches and workers
    uint64_t positions_hashes = 0;            // ... and the hashes that got a position
    uint64_t segments_lookups = 0, segments_lines = 0, segments_reported = 0, segments_examined = 0, segments_reads = 0, segments_groups = 0;
    taxor_gpu_exclusive *exclusive = nullptr; // --exclusive-file / --exclusive-reads-file: the object beside the resident index, for the whole run (exclusive.hip)
    FILE *exclusive_reads_out = nullptr;      // --exclusive-reads-file; written by the sequencer as well
    std::vector<uint32_t> exclusive_species;  // user bin -> the species the TSV names for it
    double t_exclusive = 0, t_exclusive_kernels = 0;     // seconds inside taxor_gpu_exclusive_add_batch and in its kernels, summed over workers
    uint64_t exclusive_probes = 0, exclusive_lines = 0, exclusive_examined = 0, exclusive_reads = 0;
    std::atomic<uint64_t> lca_next_read{0};   // the next batch's first read as the accumulator numbers it
    double t_lca = 0;               // seconds inside taxor_gpu_lca_add_batch, summed over workers
    std::vector<taxor::census_count> index_hashes;   // --coverage-breadth: per user bin, from the census taken when the index became resident
    double t_coverage = 0;          // seconds inside taxor_gpu_coverage_add_batch (taking and freeing the saved lists included), summed over workers
    double t_index = 0, t_reads = 0, t_compute = 0, t_pin = 0, t_search = 0, t_gather = 0, t_search_wall = 0;
    uint64_t n_batches = 0, n_gpu_batches = 0;
    uint64_t total_reads = 0, total_bases = 0;
    std::mutex stat_mu;             // the GPU workers' sums above
    void count_chunk(const Batch &bt) { std::lock_guard<std::mutex> lk(stat_mu); ++n_batches; total_reads += bt.ids.size(); total_bases += bt.offsets.back(); }
};

// The option loop and the checks that need nothing but the options.  False: help or the version was printed, there is nothing to run.
bool parse_search_args(const std::vector<std::string> &args, SearchRun &run)
{
    Config &cfg = run.cfg;
    ProfileConfig &prof = run.prof;
    for (size_t ai = 0; ai < args.size(); ++ai) {
        const std::string k = args[ai];
        auto val = [&]() -> std::string {
            if (ai + 1 >= args.size()) die("Missing value for option " + k);
            return args[++ai];
        };
        auto num = [&](const std::string &v, bool integer) -> double {   // seqan3 rejects "4x" / "abc" instead of reading a prefix
            char *end = nullptr;
            const double d = integer ? (double)strtoll(v.c_str(), &end, 10) : strtod(v.c_str(), &end);
            if (v.empty() || !end || *end != '\0') die("Value parse failed for " + k + ": Argument " + v + " could not be parsed as type " + (integer ? "unsigned 64 bit integer." : "double."));
            return d;
        };
        if (k == "--index-file") cfg.index_file = val();
        else if (k == "--query-file") cfg.query_file = val();
        else if (k == "--output-file") cfg.report_file = val();
        else if (k == "--threads") {
            const long t = (long)num(val(), true);
            if (t < 1 || t > 32) die("Validation failed for option --threads: Value not in range [1,32].");   // :51-55
            cfg.threads = (unsigned)t;
        } else if (k == "--percentage") {
            cfg.threshold = num(val(), false);
            if (cfg.threshold < 0.0 || cfg.threshold > 1.0) die("Validation failed for option --percentage: Value not in range [0,1]."); // :57-61
        } else if (k == "--error-rate") {
            cfg.error_rate = num(val(), false);
            if (cfg.error_rate < 0.0 || cfg.error_rate > 1.0) die("Validation failed for option --error-rate: Value not in range [0,1]."); // :63-67
        }
        // hidden flags of the reference's parser (taxor_search.cpp:68-79): accepted, without effect there as here
        else if (k == "--output-verbose-statistics" || k == "--debug") continue;
        else if (k == "--version") { printf("taxor-search version: 0.2.0 (MI355X build)\n"); return false; }               // :34
        else if (k == "--") break;
        else if (k == "--gpu") cfg.gpus.assign(1, atoi(val().c_str()));
        else if (k == "--gpus") {
            const int n = atoi(val().c_str());
            if (n < 1 || n > 64) die("Validation failed for option --gpus: Value not in range [1,64].");
            run.gpus_option = k;
            cfg.gpus.clear();
            for (int i = 0; i < n; ++i) cfg.gpus.push_back(i);
        } else if (k == "--gpu-list") {
            cfg.gpus.clear();
            for (const auto &t : str_split(val(), ',')) cfg.gpus.push_back(atoi(t.c_str()));
            if (cfg.gpus.empty()) die("--gpu-list is empty");
            run.gpus_option = k;
        }
        else if (k == "--cami-report-file" || k == "--binning-file" || k == "--sample-id" || k == "--seq-abundance-file" || k == "--min-abundance" ||
                 k == "--em-steps") {
            std::string err;
            if (!profile_set_option(k, val(), prof, err)) die(err);
            run.profile_mode = true;
        }
        else if (k == "--batch-reads") cfg.batch_reads = strtoull(val().c_str(), nullptr, 10);
        else if (k == "--device-index-budget") {
            const long long n = atoll(val().c_str());
            if (n < 1 || n > (1ll << 24)) die("Validation failed for option --device-index-budget: Value not in range [1,16777216].");
            cfg.index_budget_mib = (uint64_t)n;
        }
        else if (k == "--paged-replay") cfg.paged_replay = true;
        else if (k == "--paged-reread") cfg.paged_reread = true;
        else if (k == "--expect") cfg.expect_file = val();
        else if (k == "--coverage-file") {
            cfg.coverage_file = val();
            if (cfg.coverage_file.empty()) die("Validation failed for option --coverage-file: the file name is empty.");
        }
        else if (k == "--coverage-breadth") cfg.coverage_breadth = true;
        else if (k == "--coverage-precision") {
            const long n = (long)num(val(), true);
            if (n < 4 || n > 16) die("Validation failed for option --coverage-precision: Value not in range [4,16].");
            cfg.coverage_precision = (uint32_t)n;
        }
        else if (k == "--lca-file") {
            cfg.lca_file = val();
            if (cfg.lca_file.empty()) die("Validation failed for option --lca-file: the file name is empty.");
        }
        else if (k == "--lca-confidence") {
            cfg.lca_confidence = num(val(), false);
            if (!taxor::confidence_valid(cfg.lca_confidence)) die("Validation failed for option --lca-confidence: Value not in range [0,1].");
        }
        else if (k == "--hitmap-file") {
            cfg.hitmap_file = val();
            if (cfg.hitmap_file.empty()) die("Validation failed for option --hitmap-file: the file name is empty.");
        }
        else if (k == "--hitmap-segments") {
            const long n = (long)num(val(), true);
            if (n < 1 || n > 64) die("Validation failed for option --hitmap-segments: Value not in range [1,64].");
            cfg.hitmap_segments = (uint32_t)n;
        }
        else if (k == "--breakpoint-file") {
            cfg.breakpoint_file = val();
            if (cfg.breakpoint_file.empty()) die("Validation failed for option --breakpoint-file: the file name is empty.");
        }
        else if (k == "--breakpoint-min-gain") {
            const double n = num(val(), true);
            if (n < 1 || n > 4294967295.0) die("Validation failed for option --breakpoint-min-gain: Value not in range [1,4294967295].");
            cfg.breakpoint_min_gain = (uint32_t)n;
        }
        else if (k == "--segments-file") {
            cfg.segments_file = val();
            if (cfg.segments_file.empty()) die("Validation failed for option --segments-file: the file name is empty.");
        }
        else if (k == "--segments-switch-cost") {
            const double n = num(val(), true);
            if (n < 1 || n > (double)taxor::SEGMENTS_MAX_SWITCH_COST) die("Validation failed for option --segments-switch-cost: Value not in range [1,1048576].");
            cfg.segments_switch_cost = (uint32_t)n;
        }
        else if (k == "--base-positions") cfg.base_positions = true;
        else if (k == "--exclusive-file") {
            cfg.exclusive_file = val();
            if (cfg.exclusive_file.empty()) die("Validation failed for option --exclusive-file: the file name is empty.");
        }
        else if (k == "--exclusive-reads-file") {
            cfg.exclusive_reads_file = val();
            if (cfg.exclusive_reads_file.empty()) die("Validation failed for option --exclusive-reads-file: the file name is empty.");
        }
        else if (k == "--exclusive-precision") {
            const double n = num(val(), true);
            if (n < 4 || n > 16) die("Validation failed for option --exclusive-precision: Value not in range [4,16].");
            cfg.exclusive_precision = (uint32_t)n;
        }
        else if (k == "--report-file") {
            cfg.kraken_file = val();
            if (cfg.kraken_file.empty()) die("Validation failed for option --report-file: the file name is empty.");
        }
        else if (k == "--report-unit") {
            cfg.report_unit = val();
            if (cfg.report_unit != "reads" && cfg.report_unit != "bases") die("Validation failed for option --report-unit: Value not in {reads, bases}.");
        }
        else if (k == "--sequential") cfg.sequential = true;
        else if (k == "--device-parse") cfg.device_parse = true;
        else if (k == "--group-reads") cfg.group_reads = strtoull(val().c_str(), nullptr, 10);
        else if (k == "--ixf-arithmetic") {
            const std::string spec = val();
            if (!parse_arith_spec(spec, &cfg.ixf_arith)) die("Validation failed for option --ixf-arithmetic: expected kh=<0-3>,sm=<0-3>,rot=<1-63>,red=<0-2>,fp=<0-3> (as printed by `taxor verify --variants`), got " + spec);
        }
        else if (k == "--ixf-layout") {
            const std::string spec = val();
            if (taxor_ixf_layout_parse(spec.c_str(), &cfg.ixf_layout) != TAXOR_OK) die(std::string("Validation failed for option --ixf-layout: ") + taxor_gpu_last_error());
            cfg.layout_given = true;
        }
        else if (k == "--gather") {
            cfg.gather = val();
            if (cfg.gather != "rccl" && cfg.gather != "host" && cfg.gather != "none") die("Validation failed for option --gather: Value not in {rccl, host, none}.");
        }
        else if (k == "-hh" || k == "--advanced-help") { advanced_help(); return false; }
        else if (k == "-h" || k == "--help") { usage(); return false; }
        else die("Unknown option " + k + ". In case this is meant to be a non-option/argument/parameter, please specify the start of non-options with '--'.");
    }
    if (run.profile_mode) {            // like `taxor profile` (profile_cmd.h), and before any HIP call
        if (!prof.have_report) die("Option --cami-report-file is required but not set.");
        if (!prof.have_binning) die("Option --binning-file is required but not set.");
        if (!prof.have_sample) die("Option --sample-id is required but not set.");
    }
    if (cfg.index_file.empty()) die("Option --index-file is required but not set.");
    if (run.profile_mode) {
        if (cfg.index_file.find(',') != std::string::npos)
            die("Validation failed for option --index-file: the profile options (--cami-report-file, --binning-file, --sample-id) take ONE index file; "
                "search the indexes one by one, or write a TSV per index and run `taxor profile`.");
        if (cfg.gpus.size() > 1)
            die("Validation failed for option " + run.gpus_option + ": the profile options (--cami-report-file, --binning-file, --sample-id) run on ONE device; "
                "give --gpu <id>.");
        if (!cfg.gather.empty() && cfg.gather != "none")
            die("Validation failed for option --gather: the profile options run on ONE device, where nothing is gathered; leave --gather out.");
        if (!cfg.expect_file.empty() && cfg.report_file.empty()) die("Option --expect compares the TSV: it needs --output-file.");
        prof.device = cfg.gpus[0];
    }
    if (cfg.coverage_precision && cfg.coverage_file.empty()) die("Option --coverage-precision sizes the sketches of --coverage-file: it needs that option.");
    if (cfg.coverage_breadth && cfg.coverage_file.empty()) die("Option --coverage-breadth adds columns to --coverage-file: it needs that option.");
    if (!cfg.coverage_file.empty()) {   // before any HIP call
        if (cfg.index_file.find(',') != std::string::npos)
            die("Validation failed for option --index-file: --coverage-file takes ONE index file (a user bin's leaf bins are looked up in the index it belongs to); "
                "search the indexes one by one.");
        if (cfg.gpus.size() > 1)
            die("Validation failed for option " + run.gpus_option + ": --coverage-file accumulates on ONE device (the sketches of several would have to be merged); give --gpu <id>.");
        if (!cfg.gather.empty() && cfg.gather != "none")
            die("Validation failed for option --gather: --coverage-file runs on ONE device, where nothing is gathered; leave --gather out.");
    }
    if (!cfg.report_unit.empty() && cfg.kraken_file.empty()) die("Option --report-unit says what --report-file counts: it needs that option.");
    if (cfg.confidence_mode() && !cfg.lca_mode()) die("Option --lca-confidence weighs the calls of --lca-file / --report-file: it needs one of them.");
    if (cfg.confidence_mode()) {   // before any HIP call
        if (cfg.index_file.find(',') != std::string::npos)
            die("Validation failed for option --index-file: --lca-confidence takes ONE index file (a read's hashes are looked up in the leaf bins of the index its references belong to); "
                "search the indexes one by one.");
        if (cfg.gpus.size() > 1)
            die("Validation failed for option " + run.gpus_option + ": --lca-confidence weighs on ONE device (a batch's hash lists and its results must lie on the same one); give --gpu <id>.");
        if (!cfg.gather.empty() && cfg.gather != "none")
            die("Validation failed for option --gather: --lca-confidence runs on ONE device, where nothing is gathered; leave --gather out.");
    }
    if (cfg.lca_mode()) {   // before any HIP call
        const std::string opt = !cfg.lca_file.empty() ? "--lca-file" : "--report-file";
        if (cfg.index_file.find(',') != std::string::npos)
            die("Validation failed for option --index-file: " + opt + " takes ONE index file (a read's references are reduced within the taxonomy of the index they come from); "
                "search the indexes one by one.");
        if (cfg.gpus.size() > 1)
            die("Validation failed for option " + run.gpus_option + ": " + opt + " tallies on ONE device (the tallies of several would have to be merged); give --gpu <id>.");
        if (!cfg.gather.empty() && cfg.gather != "none")
            die("Validation failed for option --gather: " + opt + " runs on ONE device, where nothing is gathered; leave --gather out.");
        if (!cfg.expect_file.empty() && cfg.report_file.empty()) die("Option --expect compares the TSV: it needs --output-file.");
    }
    if (cfg.hitmap_segments && cfg.hitmap_file.empty()) die("Option --hitmap-segments cuts the hash lists of --hitmap-file: it needs that option.");
    if (!cfg.hitmap_file.empty()) {   // before any HIP call
        if (cfg.index_file.find(',') != std::string::npos)
            die("Validation failed for option --index-file: --hitmap-file takes ONE index file (a reference's hits are looked up in the leaf bins of the index it belongs to); "
                "search the indexes one by one.");
        if (cfg.gpus.size() > 1)
            die("Validation failed for option " + run.gpus_option + ": --hitmap-file locates on ONE device (a batch's hash lists and its results must lie on the same one); give --gpu <id>.");
        if (!cfg.gather.empty() && cfg.gather != "none")
            die("Validation failed for option --gather: --hitmap-file runs on ONE device, where nothing is gathered; leave --gather out.");
        if (!cfg.expect_file.empty() && cfg.report_file.empty()) die("Option --expect compares the TSV: it needs --output-file.");
    }
    if (cfg.breakpoint_min_gain && cfg.breakpoint_file.empty()) die("Option --breakpoint-min-gain says which reads --breakpoint-file reports: it needs that option.");
    if (!cfg.breakpoint_file.empty()) {   // before any HIP call
        if (cfg.index_file.find(',') != std::string::npos)
            die("Validation failed for option --index-file: --breakpoint-file takes ONE index file (a read's hashes are looked up in the leaf bins of the index its references belong to); "
                "search the indexes one by one.");
        if (cfg.gpus.size() > 1)
            die("Validation failed for option " + run.gpus_option + ": --breakpoint-file examines on ONE device (a batch's hash lists and its results must lie on the same one); give --gpu <id>.");
        if (!cfg.gather.empty() && cfg.gather != "none")
            die("Validation failed for option --gather: --breakpoint-file runs on ONE device, where nothing is gathered; leave --gather out.");
        if (!cfg.expect_file.empty() && cfg.report_file.empty()) die("Option --expect compares the TSV: it needs --output-file.");
    }
    if (cfg.segments_switch_cost && cfg.segments_file.empty()) die("Option --segments-switch-cost says what a switch costs in --segments-file: it needs that option.");
    if (!cfg.segments_file.empty()) {   // before any HIP call
        if (cfg.index_file.find(',') != std::string::npos)
            die("Validation failed for option --index-file: --segments-file takes ONE index file (a read's hashes are looked up in the leaf bins of the index its references belong to); "
                "search the indexes one by one.");
        if (cfg.gpus.size() > 1)
            die("Validation failed for option " + run.gpus_option + ": --segments-file examines on ONE device (a batch's hash lists and its results must lie on the same one); give --gpu <id>.");
        if (!cfg.gather.empty() && cfg.gather != "none")
            die("Validation failed for option --gather: --segments-file runs on ONE device, where nothing is gathered; leave --gather out.");
        if (!cfg.expect_file.empty() && cfg.report_file.empty()) die("Option --expect compares the TSV: it needs --output-file.");
    }
    if (cfg.base_positions && cfg.breakpoint_file.empty() && cfg.segments_file.empty())   // before any HIP call
        die("Option --base-positions adds base columns to --breakpoint-file and --segments-file: it needs one of them.");
    if (cfg.exclusive_precision && cfg.exclusive_file.empty()) die("Option --exclusive-precision sizes the sketches of --exclusive-file: it needs that option.");
    if (cfg.exclusive_mode()) {   // before any HIP call
        const std::string opt = !cfg.exclusive_file.empty() ? "--exclusive-file" : "--exclusive-reads-file";
        if (cfg.index_file.find(',') != std::string::npos)
            die("Validation failed for option --index-file: " + opt + " takes ONE index file (a read's hashes are looked up in the leaf bins of the index its references belong to); "
                "search the indexes one by one.");
        if (cfg.gpus.size() > 1)
            die("Validation failed for option " + run.gpus_option + ": " + opt + " examines on ONE device (a batch's hash lists and its results must lie on the same one); give --gpu <id>.");
        if (!cfg.gather.empty() && cfg.gather != "none")
            die("Validation failed for option --gather: " + opt + " runs on ONE device, where nothing is gathered; leave --gather out.");
        if (!cfg.expect_file.empty() && cfg.report_file.empty()) die("Option --expect compares the TSV: it needs --output-file.");
    }
    run.write_tsv = !(run.profile_mode || cfg.lca_mode() || !cfg.hitmap_file.empty() || !cfg.breakpoint_file.empty() || !cfg.segments_file.empty() || cfg.exclusive_mode()) ||
                    !cfg.report_file.empty();
    if (cfg.threads == 0) {
        // --threads not given.  The reference's default is one worker thread (taxor_search_configuration.hpp:17) -- there the
        // thread that classifies; here host threads only parse the query file and render text for the GPU, and one of them
        // delivers 1-3 Gbp/s to a device that classifies 25.  Default: a sixteenth of the machine, between 4 and 16 -- or what the
        // container's CPU quota allows, if it has one (threads beyond it only make the cgroup stop all of them for the rest of each
        // scheduler period).  A --threads the user gives is obeyed as it is.
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        const double quota = cpu_quota();
        cfg.threads = quota >= 1.0 ? std::min(16u, std::max(2u, (unsigned)quota)) : std::min(16u, std::max(4u, hw / 16u));
    }
    return true;
}

// ---- sanity checks (taxor_search.cpp:97-151): every file is there, the indexes agree, no query is CRAM or SAM -- before any HIP call
void check_search_inputs(const Config &cfg, const std::vector<std::string> &index_files, const std::vector<std::string> &query_files)
{
    printf("checking input ... ");
    fflush(stdout);
    for (const auto &f : index_files)
        if (!file_exists(f)) die("Please check the given index file(s). \nThe following index file does not exist: " + f);
    if (index_files.size() > 1) {
        uint8_t k0 = 1, s0 = 0, t0 = 0, syn0 = 0;
        uint64_t w0 = 0;
        uint16_t sc0 = 0;
        for (const auto &f : index_files) {
            taxor_hixf *h = nullptr;
            if (taxor_hixf_load(f.c_str(), &h) != TAXOR_OK) die(taxor_gpu_last_error());
            const taxor_hixf_view *v = taxor_hixf_get_view(h);
            const taxor_hixf_meta *m = taxor_hixf_get_meta(h);
            if (k0 == 1) { k0 = v->kmer_size; s0 = v->syncmer_size; t0 = v->t_syncmer; syn0 = v->use_syncmer; w0 = m->window_size; sc0 = v->scaling; }
            else if (k0 != v->kmer_size || s0 != v->syncmer_size || t0 != v->t_syncmer || syn0 != v->use_syncmer || w0 != m->window_size || sc0 != v->scaling)
                die("At least two index files have been created with different kmer selection schemes.\n Please provide only index files using the same kmer-/syncmer-/window-size!");
            taxor_hixf_free(h);
        }
    }
    for (const auto &f : query_files)
        if (!file_exists(f)) die("Please check the given input query files. \nThe following query file does not exist: " + f);
    for (const auto &f : query_files) {           // CRAM and SAM text are refused by name, before any HIP call
        try { (void)bam::sniff(f); } catch (const std::exception &e) { die(e.what()); }
    }
    if (!cfg.expect_file.empty() && !file_exists(cfg.expect_file)) die("The expected-output file does not exist: " + cfg.expect_file);
    printf("done!\n");
    trace("input checked");
}

// ---- what both routes do with a chunk ----------------------------------------------------------------------------------------

// a BAM chunk as the device takes it: ids and lengths are the reader's, the device unpacks the 4-bit sequences
taxor_nibble_segment nibble_segment(const Batch &bt)
{
    return taxor_nibble_segment{(const uint8_t *)bt.raw.data(), bt.nib_off.data(), bt.nib_len.data(), bt.nib_rev.data(), bt.ids.size()};
}

// TSV text of `n` reads into `text`, grown where it is too small; returns the text's length
uint64_t format_reads(const taxor_hixf *h, uint64_t n, const char *const *idp, const uint64_t *idl, const uint64_t *rl, const uint32_t *n_hashes,
                      const uint64_t *read_off, const int64_t *user_bin, const uint32_t *count, std::vector<char> &text)
{
    uint64_t need = taxor_format_reads(h, n, idp, idl, rl, n_hashes, read_off, user_bin, count, text.data(), text.size());
    if (need > text.size()) {
        text.resize(need + need / 8 + 4096);
        need = taxor_format_reads(h, n, idp, idl, rl, n_hashes, read_off, user_bin, count, text.data(), text.size());
    }
    return need;
}

// a file's size as the text it can hold: a compressed byte at four.  `bam_too`: the bound on bases counts .bam (4-bit sequences,
// deflated) as packed and wants a name longer than the suffix; the bound on reads does not, and wants one longer than 3
uint64_t unpacked_bound(const std::string &q, uint64_t size, bool bam_too)
{
    auto ends = [&](const char *e) { const size_t m = strlen(e); return q.size() > (bam_too ? m : 3) && q.size() >= m && q.compare(q.size() - m, m, e) == 0; };
    return size * (ends(".gz") || ends(".bz2") || (bam_too && ends(".bam")) ? 4 : 1);
}

// ---- an index that does not fit the device (or --device-index-budget): searched in resident passes (DESIGN.md section 9,
// "Search beyond device memory").  The outer loop runs over the passes, the inner one over the query file, cut into the SAME
// batches in every pass (the sequential reader cuts at exactly --batch-reads records); a pass's CSR is kept per batch in host
// memory with its DFS keys, the last pass merges them on the device and writes / feeds the profile as the resident route does.
//
// The query is read, inflated, packed and hashed in pass 0 only: with capture on, every batch leaves its reads' hash lists
// in host memory (taxor_gpu_search_take_saved), kept here with the batch's ids and read offsets, and passes 1 .. n-1 replay
// the kept batches (taxor_gpu_search_saved_begin) without opening the file.  The lists' store is metered like the results':
// a bound from the file sizes up front (8 B per hash at the densest selection the index's k, s, t admit), MemAvailable
// while it grows.  This is the route of --paged-replay; without it, and where the store does not fit, the run re-reads the file in
// every pass.  Either way one line on stderr says what was done with the query.
struct PagedPass {
    SearchRun &run;
    taxor_hixf *h;
    taxor_gpu_searcher *s;
    uint32_t passes;
    struct Saved { std::vector<uint64_t> ro; std::vector<int64_t> ub; std::vector<uint32_t> cnt, key; };
    std::vector<std::vector<Saved>> store;          // [batch][pass]
    uint64_t stored = 0;
    struct Kept { taxor_gpu_saved *lists = nullptr; fastx::IdList ids; std::vector<uint64_t> offsets; };
    std::vector<Kept> kept;
    uint64_t kept_bytes = 0, lists_bytes = 0;      // everything kept per batch / of it: the saved hash lists
    bool replay = false;
    bool last_pass = false, capturing = false;     // of the pass that is running
    size_t bi = 0;                                  // the batch's number in its pass
    std::vector<const char *> idp;
    std::vector<uint64_t> idl, rl;
    std::vector<char> text;
    std::vector<taxor_gpu_prior> pri;
    PagedPass(SearchRun &run_, taxor_hixf *h_, taxor_gpu_searcher *s_, uint32_t passes_) : run(run_), h(h_), s(s_), passes(passes_) {}

    void drop_kept()
    {
        for (Kept &k : kept) taxor_gpu_saved_free(k.lists);
        std::vector<Kept>().swap(kept);
        kept_bytes = 0;
    }
    // pass 0 only: the store is given up -- what it held goes, pass 0's results stay, the file is read again from pass 1 on
    void give_up_replay(const std::string &why_not)
    {
        fprintf(stderr, "taxor search: the query is read again in every pass (%s)\n", why_not.c_str());
        drop_kept();
        replay = false;
        if (taxor_gpu_search_capture(s, 0) != TAXOR_OK) die(taxor_gpu_last_error());
    }
    // pass 0 with capture on: the batch's hash lists, ids and offsets are kept for the later passes
    void keep_lists(const Batch &bt)
    {
        taxor_gpu_saved *sv = nullptr;
        if (taxor_gpu_search_take_saved(s, &sv) != TAXOR_OK) die(taxor_gpu_last_error());
        const uint64_t need = taxor_gpu_saved_bytes(sv) + bt.ids.data.size() + (bt.ids.off.size() + bt.offsets.size()) * 8;
        const uint64_t avail = taxor::host_memory_available();
        if (avail && avail < (1ull << 29)) {
            // the lists are in memory already, so what is left is the figure: below half a gibibyte -- twice what the
            // results' store below asks for, so that the lists go before the results' check can end the run
            taxor_gpu_saved_free(sv);
            give_up_replay("the reads' saved hash lists no longer fit host memory: " + std::to_string(kept_bytes + need) + " bytes kept so far, MemAvailable is " +
                           std::to_string(avail) + " bytes");
            return;
        }
        kept.emplace_back();
        kept.back().lists = sv;
        kept.back().ids = bt.ids;
        kept.back().offsets = bt.offsets;
        kept_bytes += need;
        lists_bytes += taxor_gpu_saved_bytes(sv);
    }
    // every pass but the last: the batch's CSR and DFS keys go to host memory
    void save_results(uint64_t n, const taxor_gpu_results &res)
    {
        const uint32_t *key = nullptr;
        if (taxor_gpu_results_keys(s, &key) != TAXOR_OK) die(taxor_gpu_last_error());
        const uint64_t need = (n + 1) * 8 + res.n_tuples * 16;
        uint64_t avail = taxor::host_memory_available();
        if (avail && need + (1ull << 28) > avail && capturing && replay) {      // the saved lists go first: the run does not end on their account
            give_up_replay("the passes' results need the memory the reads' saved hash lists hold: " + std::to_string(kept_bytes) + " bytes of lists dropped, MemAvailable was " +
                           std::to_string(avail) + " bytes");
            avail = taxor::host_memory_available();
        }
        if (avail && need + (1ull << 28) > avail)
            die("the passes' results no longer fit host memory: " + std::to_string(stored + need) + " bytes kept so far, MemAvailable is " + std::to_string(avail) + " bytes.");
        stored += need;
        Saved sv;
        sv.ro.assign(res.read_off, res.read_off + n + 1);
        sv.ub.assign(res.user_bin, res.user_bin + res.n_tuples);
        sv.cnt.assign(res.count, res.count + res.n_tuples);
        sv.key.assign(key, key + res.n_tuples);
        store[bi].push_back(std::move(sv));
    }
    // the last pass: the earlier passes' results are merged in on the device; then the profile feed and the TSV, like the resident route
    void merge_and_report(Batch &bt, taxor_gpu_results &res)
    {
        const uint64_t n = bt.ids.size();
        if (store[bi].size() != passes - 1) die("internal: the query file was cut into other batches than in the pass before");
        pri.clear();
        for (const Saved &sv : store[bi]) {
            if (sv.ro.size() != n + 1) die("internal: the query file was cut into other batches than in the pass before");
            pri.push_back(taxor_gpu_prior{n, (uint64_t)sv.ub.size(), sv.ro.data(), sv.ub.data(), sv.cnt.data(), sv.key.data()});
        }
        if (taxor_gpu_search_merge_prior(s, pri.data(), (uint32_t)pri.size()) != TAXOR_OK) die(taxor_gpu_last_error());
        std::vector<Saved>().swap(store[bi]);
        if (run.profile_mode) {
            bt.feed_first = run.fused.next_read.fetch_add(n);
            run.fused.take_ids(bt);
            const double f0 = now();
            if (taxor_gpu_profile_feed_add_batch(run.fused.feed, s, bt.feed_first, 0) != TAXOR_OK) die(taxor_gpu_last_error());
            run.fused.t_feed += now() - f0;
        }
        if (run.write_tsv) {
            if (taxor_gpu_batch_fetch(s, &res) != TAXOR_OK) die(taxor_gpu_last_error());
            idp.resize(n); idl.resize(n); rl.resize(n);
            for (uint64_t r = 0; r < n; ++r) { idp[r] = bt.ids.ptr(r); idl[r] = bt.ids.len(r); rl[r] = bt.offsets[r + 1] - bt.offsets[r]; }
            const uint64_t need = format_reads(h, n, idp.data(), idl.data(), rl.data(), res.n_hashes, res.read_off, res.user_bin, res.count, text);
            if (need && fwrite(text.data(), 1, need, run.out) != need) die("cannot write to " + run.cfg.report_file + ": " + strerror(errno));
        }
        run.count_chunk(bt);
        ++run.n_gpu_batches;
    }
    // one batch of one pass: from its bases (lists == nullptr) or from its saved hash lists
    void process(Batch &bt, const taxor_gpu_saved *lists)
    {
        const uint64_t n = bt.ids.size();
        const double t1 = now();
        taxor_gpu_results res{};
        const bool nibbles = bt.raw_kind == 'B';      // a BAM chunk: its 4-bit sequences are unpacked on the device
        bt.raw_kind = 0;
        auto once = [&]() -> int {
            if (lists) {
                const int rb = taxor_gpu_search_saved_begin(s, lists);
                return rb != TAXOR_OK ? rb : taxor_gpu_search_batch_end(s, &res);
            }
            if (!nibbles) return taxor_gpu_search_batch(s, bt.bases.data(), bt.offsets.data(), n, &res);
            const taxor_nibble_segment seg = nibble_segment(bt);
            const int rb = taxor_gpu_search_nibbles_begin(s, &seg, 1);
            return rb != TAXOR_OK ? rb : taxor_gpu_search_batch_end(s, &res);
        };
        Batch *const text_chunk[] = {&bt};
        int rc = nibbles ? once() : run_with_alphabet_retry(once, text_chunk);
        if (rc == TAXOR_E_NOMEM && capturing && replay) {      // (a kernel that commits every mapping in full refuses the lists' reservation)
            give_up_replay("a batch's hash lists found no room: " + std::string(taxor_gpu_last_error()));
            rc = once();
        }
        if (rc != TAXOR_OK) die(taxor_gpu_last_error());
        if (capturing && replay) keep_lists(bt);          // (replay goes off when the store stops fitting: the rest of pass 0 keeps nothing)
        if (store.size() <= bi) store.resize(bi + 1);
        if (!last_pass) save_results(n, res);
        else merge_and_report(bt, res);
        ++bi;
        run.t_compute += now() - t1;
        run.t_search += now() - t1;
    }
};

void search_paged(SearchRun &run, taxor_hixf *h, const taxor_hixf_view *view, const taxor_gpu_search_params &prm, const std::vector<std::string> &queries,
                  uint64_t budget, const char *why, double t0)
{
    const Config &cfg = run.cfg;
    if (cfg.gpus.size() > 1) die("paging an index through device memory (" + std::string(why) + ") runs on ONE device; give --gpu <id> instead of " + run.gpus_option + ".");
    uint64_t query_bytes = 0;
    for (const auto &q : queries) {
        struct stat sb;
        if (stat(q.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode))
            die("paging an index through device memory (" + std::string(why) + ") reads the query once per pass: " + q + " is not a regular file and cannot be read again "
                "(a pipe, standard input); write it to a file first.");
        query_bytes += unpacked_bound(q, (uint64_t)sb.st_size, false);
    }
    taxor_gpu_index *idx = nullptr;
    if (taxor_gpu_index_create_paged(view, cfg.gpus[0], budget, &idx) != TAXOR_OK) die(taxor_gpu_last_error());
    const uint32_t passes = taxor_gpu_index_passes(idx);
    fprintf(stderr, "taxor search: the index is searched in %u resident pass%s over the query (%s)\n", passes, passes == 1 ? "" : "es", why);
    // host memory for the earlier passes' results: per pass 8 B per read (offsets) and 16 B per tuple (user bin, count, key).
    // Bound: reads at one per 200 bytes of (inflated: x 4) query file, tuples at the 12 per read the library sizes a batch for
    {
        const uint64_t bound = (uint64_t)(passes - 1) * (query_bytes / 200 + 1) * (8 + 16 * 12), avail = taxor::host_memory_available();
        if (passes > 1 && avail && bound > avail)
            die("the results of " + std::to_string(passes - 1) + " passes are kept in host memory until the last one merges them: up to " + std::to_string(bound) +
                " bytes (8 per read and 16 per tuple and pass), MemAvailable is " + std::to_string(avail) + " bytes.");
    }
    taxor_gpu_searcher *s = nullptr;
    if (taxor_gpu_searcher_create(idx, &prm, &s) != TAXOR_OK) die(taxor_gpu_last_error());
    if (run.profile_mode) run.fused.begin(view, taxor_hixf_get_meta(h), run.prof.device);
    run.t_index += now() - t0;
    Config seq_cfg = cfg;
    if (!seq_cfg.batch_reads) seq_cfg.batch_reads = 131072;
    BatchPool pool;
    PagedPass pp(run, h, s, passes);
    pp.replay = passes > 1 && cfg.paged_replay && !cfg.paged_reread;
    std::string reread_why = cfg.paged_reread ? "--paged-reread" : "the default; --paged-replay keeps the reads' hash lists in host memory instead";
    if (pp.replay) {
        uint64_t bases = 0;         // what the files can hold: a compressed byte at four bases (BAM: 4-bit sequences, deflated)
        for (const auto &q : queries) {
            struct stat sb;
            if (stat(q.c_str(), &sb) == 0) bases += unpacked_bound(q, (uint64_t)sb.st_size, true);
        }
        const uint64_t bound = taxor_saved_bytes_bound(bases, view->use_syncmer, view->kmer_size, view->syncmer_size, view->t_syncmer);
        const uint64_t avail = taxor::host_memory_available();
        if (!taxor_saved_store_fits(bound, avail)) {
            pp.replay = false;
            reread_why = "the reads' saved hash lists may need " + std::to_string(bound) + " bytes of host memory, MemAvailable is " + std::to_string(avail) + " bytes";
        }
    }
    if (passes > 1 && !pp.replay) fprintf(stderr, "taxor search: the query is read again in every pass (%s)\n", reread_why.c_str());
    const double t_search0 = now();
    for (uint32_t p = 0; p < passes; ++p) {
        const double tl = now();
        if (taxor_gpu_index_load_pass(idx, view, p) != TAXOR_OK) die(taxor_gpu_last_error());
        run.t_index += now() - tl;
        pp.last_pass = p + 1 == passes;
        pp.capturing = pp.replay && p == 0;
        if (taxor_gpu_search_capture(s, pp.capturing ? 1 : 0) != TAXOR_OK) die(taxor_gpu_last_error());
        pp.bi = 0;
        if (p == 0 || !pp.replay) {
            for (size_t f = 0; f < queries.size(); ++f)
                run.t_reads += produce_batches(queries[f], seq_cfg, false, pool, [&](std::unique_ptr<Batch> b) {
                    if (b->end_of_file) return;
                    pp.process(*b, nullptr);
                    pool.put(std::move(b));
                }, (uint32_t)f, 1);
        } else {
            Batch bt;           // carries a kept batch's ids and offsets: what the last pass formats and feeds the profile with
            for (PagedPass::Kept &k : pp.kept) {
                bt.ids = std::move(k.ids);
                bt.offsets = std::move(k.offsets);
                pp.process(bt, k.lists);
                if (pp.last_pass) {
                    taxor_gpu_saved_free(k.lists);
                    k.lists = nullptr;
                } else {
                    k.ids = std::move(bt.ids);
                    k.offsets = std::move(bt.offsets);
                }
            }
        }
        if (p == 0 && pp.replay)
            fprintf(stderr, "taxor search: passes 1 to %u replay %llu batch%s from %llu bytes of saved hash lists (the query file is read once)\n", passes - 1,
                    (unsigned long long)pp.kept.size(), pp.kept.size() == 1 ? "" : "es", (unsigned long long)pp.lists_bytes);
    }
    pp.drop_kept();
    run.t_search_wall += now() - t_search0;
    if (tune_env("TAXOR_CLI_TRACE"))
        fprintf(stderr, "[trace] paged search: %u passes, %.3f s waiting for uploads, %.2f GB of earlier passes' results held at most\n", passes,
                taxor_gpu_index_upload_wait_seconds(idx), pp.stored / 1e9);
    taxor_gpu_searcher_destroy(s);
    taxor_gpu_index_destroy(idx);
    if (run.profile_mode) run.fused.finish(run.prof, cfg.threads, run.t_search_wall);
    taxor_hixf_free(h);
}

// ---- the resident route: readers -> pinners -> GPU workers -> sequencer -> piece threads, overlapped ("CLI host":
// the stages, the queues between them, and who owns which shared state)

// a file that is not being written yet may run at most two chunks ahead, so that the file whose turn it is can
// always get buffers
struct FileTurns {
    std::mutex fmu;
    std::condition_variable fcv;
    size_t current_file = 0;
    std::vector<int> ahead;
    void gate(size_t f)             // a reader of file f, before it takes a buffer
    {
        std::unique_lock<std::mutex> lk(fmu);
        fcv.wait(lk, [&] { return f == current_file || ahead[f] < 2; });
    }
    void chunk_parsed(size_t f) { std::lock_guard<std::mutex> lk(fmu); ++ahead[f]; }
    void chunk_written(size_t f) { std::lock_guard<std::mutex> lk(fmu); --ahead[f]; fcv.notify_all(); }
    void turn_of(size_t f) { std::lock_guard<std::mutex> lk(fmu); current_file = f; fcv.notify_all(); }   // every chunk of the files before f is on its way to the report
};

// what connects the stages: parsers -> q_parsed -> pinners -> q_in -> GPU workers -> q_fmt -> sequencer; the pool every chunk
// comes from and goes back to (it, not a queue's depth, bounds how far the parsers run ahead)
struct Pipes {
    BoundedQueue<std::unique_ptr<Batch>> q_parsed{4096}, q_in{4096}, q_fmt{8};
    BatchPool pool;
    FileTurns turns;
};

// Chunk buffers stay pageable ("CLI host", has the measurements); TAXOR_CLI_PIN_AFTER=n (under TAXOR_TUNING) registers
// a buffer at its n-th fill, on the pinner stage (and, for a chunk that got past it, in the worker).
void pin_bases(Batch &bt)       // recycled with the chunk: pinned once, DMA source from then on
{
    static const uint32_t pin_after = [] { const char *e = tune_env("TAXOR_CLI_PIN_AFTER"); const int v = e ? atoi(e) : 0; return v >= 1 ? (uint32_t)v : ~0u; }();
    if (bt.may_pin && !bt.pinned && bt.fills >= pin_after && bt.bases.capacity() >= (1u << 20) &&
        taxor_gpu_host_register(&bt.bases[0], bt.bases.capacity()) == TAXOR_OK)
        bt.pinned = &bt.bases[0];
}

// the reader threads (each takes the next query file), the pinners behind them, and the thread that closes the queues after them
struct QueryFeed {
    const Config &cfg;
    const std::vector<std::string> &queries;
    Pipes &p;
    unsigned readers, parse_threads;
    std::atomic<size_t> next_file{0};
    std::vector<double> reader_time;
    std::vector<std::thread> reader_threads, pinners;
    std::thread closer;
    QueryFeed(const Config &c, const std::vector<std::string> &q, Pipes &p_, unsigned r, unsigned pt) : cfg(c), queries(q), p(p_), readers(r), parse_threads(pt) {}

    void read_files(unsigned rt)
    {
        for (;;) {
            const size_t f = next_file.fetch_add(1);
            if (f >= queries.size()) break;
            reader_time[rt] += produce_batches(queries[f], cfg, !cfg.sequential, p.pool, [this, f](std::unique_ptr<Batch> b) {
                if (!b->end_of_file) p.turns.chunk_parsed(f);
                p.q_parsed.push(std::move(b));
            }, (uint32_t)f, parse_threads, [this, f] { p.turns.gate(f); });
        }
    }
    void pin_chunks()
    {
        std::unique_ptr<Batch> b;
        while (p.q_parsed.pop(b)) {
            if (!b->end_of_file) pin_bases(*b);
            // a BAM chunk's SEQ bytes go to the device as they are: page-locked here, beside the walker, once per buffer
            if (!b->end_of_file && b->raw_kind == 'B' && !b->raw_pinned && b->raw.capacity() >= (1u << 20) &&
                taxor_gpu_host_register(b->raw.data(), b->raw.capacity()) == TAXOR_OK)
                b->raw_pinned = b->raw.data();
            p.q_in.push(std::move(b));
        }
    }
    void start()
    {
        reader_time.assign(readers, 0.0);
        for (unsigned rt = 0; rt < readers; ++rt) reader_threads.emplace_back([this, rt] { read_files(rt); });
        static const int n_pinners = [] { const char *e = tune_env("TAXOR_CLI_PINNERS"); const int v = e ? atoi(e) : 2; return v >= 1 && v <= 32 ? v : 2; }();
        for (int pt = 0; pt < n_pinners; ++pt) pinners.emplace_back([this] { pin_chunks(); });
        closer = std::thread([this] {
            for (auto &t : reader_threads) t.join();
            p.q_parsed.close();
            for (auto &t : pinners) t.join();
            p.q_in.close();
            trace("readers done");
        });
    }
};

// ---- TSV text and the report file.  The report is ONE file and the kernel serialises a file's buffered writes, so there is one
// stream of write() calls whatever the threads.  The text is made in PIECES of about a megabyte, each written by the thread that
// formatted it while it is still in that core's cache ("CLI host": the measurements, and what else was tried):
//   sequencer       : chunks (GPU workers, any order) -> file and chunk order -> pieces (ranges of a chunk's reads), numbered
//   piece threads   : tuples -> 0.8*max filter -> TSV text of the piece (:266-306) -> wait for the piece's turn -> write()
struct ReportWriter {
    SearchRun &run;
    const taxor_hixf *h;
    Pipes &p;
    unsigned formatters;
    struct Hold { std::unique_ptr<Batch> b; std::atomic<uint32_t> left{0}; };
    struct Piece { Hold *h = nullptr; uint32_t r0 = 0, r1 = 0; uint64_t ticket = 0; };
    BoundedQueue<Piece> q_piece;
    int out_fd = -1;
    std::atomic<uint64_t> out_written{0};
    double t_write = 0;            // seconds inside write()
    std::mutex turn_mu;
    std::condition_variable turn_cv[64];            // a waiting piece thread sleeps on the one of its ticket: passing the turn wakes one thread
    uint64_t next_ticket = 0;
    std::atomic<uint64_t> turn_now{0};              // next_ticket, readable without the lock: the thread whose turn is next spins on it
    double t_first_write = 0, t_last_write = 0;
    std::atomic<uint64_t> line_bytes_guess{192};   // bytes of text per tuple, learnt from the pieces formatted so far
    std::thread sequencer;
    std::vector<std::thread> fmt_threads;

    ReportWriter(SearchRun &run_, const taxor_hixf *h_, Pipes &p_, unsigned formatters_) : run(run_), h(h_), p(p_), formatters(formatters_), q_piece(4 * formatters_ + 16) {}
    const uint64_t piece_bytes = [] { static const uint64_t v = [] { const char *e = tune_env("TAXOR_CLI_PIECE_KB"); const int v = e ? atoi(e) : 0; return (uint64_t)(v >= 16 ? v : 1024) << 10; }(); return v; }();
    void chunk_done(Hold *hd)
    {
        p.turns.chunk_written(hd->b->file);
        p.pool.put(std::move(hd->b));
        delete hd;
    }
    void sequence()
    {
        std::unique_ptr<Batch> b;
        std::map<std::pair<uint32_t, uint64_t>, std::unique_ptr<Batch>> pending; // chunks that arrived ahead of their turn
        uint32_t cur_file = 0;
        uint64_t next_seq = 0, ticket = 0;
        while (p.q_fmt.pop(b)) {
            const auto key = std::make_pair(b->file, b->seq);
            pending.emplace(key, std::move(b));
            while (!pending.empty() && pending.begin()->first == std::make_pair(cur_file, next_seq)) {
                std::unique_ptr<Batch> cur = std::move(pending.begin()->second);
                pending.erase(pending.begin());
                if (cur->end_of_file) {                 // every chunk of this file is on its way: the next file's turn
                    next_seq = 0;
                    p.turns.turn_of(++cur_file);
                    continue;
                }
                ++next_seq;
                Hold *hd = new Hold;
                hd->b = std::move(cur);
                const Batch &bt = *hd->b;
                const size_t n = bt.ids.size();
                if (run.profile_mode) run.fused.take_ids(bt);            // chunks pass here in input order
                if (run.lca_out) write_lca_lines(bt);
                if (run.hitmap_out) write_hitmap_lines(bt);
                if (run.breakpoint_out) write_breakpoint_lines(*hd->b);
                if (run.segments_out) write_segments_lines(*hd->b);
                if (run.exclusive_reads_out) write_exclusive_lines(*hd->b);
                if (n == 0 || !run.write_tsv) { chunk_done(hd); continue; }
                // cut where the estimated text passes piece_bytes
                const uint64_t per_tuple = line_bytes_guess.load();
                std::vector<uint32_t> cuts{0};
                uint64_t est = 0;
                for (size_t r = 0; r < n; ++r) {
                    est += (bt.read_off[r + 1] - bt.read_off[r]) * per_tuple + bt.ids.len(r) + 32;
                    if (est >= piece_bytes && r + 1 < n) { cuts.push_back((uint32_t)(r + 1)); est = 0; }
                }
                cuts.push_back((uint32_t)n);
                hd->left = (uint32_t)(cuts.size() - 1);
                for (size_t c = 0; c + 1 < cuts.size(); ++c) q_piece.push(Piece{hd, cuts[c], cuts[c + 1], ticket++});
            }
        }
        q_piece.close();
    }
    // --lca-file: the chunk's reads, one line each, by the sequencer (one line per read is little next to the TSV's six and more)
    std::string lca_text;
    void write_lca_lines(const Batch &bt)
    {
        const taxor_lineage_view &lv = run.lineage_view;
        const size_t n = bt.ids.size();
        if (bt.lca_node.size() != n || bt.n_hashes.size() != n) die("internal: a chunk reached the writer without its reads' calls");
        lca_text.clear();
        if (run.cfg.confidence_mode()) {                   // the confident calls and their three further columns (confidence_format.h)
            if (bt.cf_lca_node.size() != n) die("internal: a chunk reached the writer without its reads' supports");
            auto id_of = [&](int32_t node) -> const char * { return node == TAXOR_LCA_UNCLASSIFIED ? nullptr : node == TAXOR_LCA_ROOT ? "1" : lv.id[node]; };
            for (size_t r = 0; r < n; ++r)
                taxor::confidence_line(lca_text, bt.ids.ptr(r), bt.ids.len(r), id_of(bt.lca_node[r]), bt.offsets[r + 1] - bt.offsets[r], bt.n_hashes[r], bt.lca_best[r],
                                       bt.lca_refs[r], bt.cf_support[r], id_of(bt.cf_lca_node[r]), bt.cf_lca_support[r]);
            if (!lca_text.empty() && fwrite(lca_text.data(), 1, lca_text.size(), run.lca_out) != lca_text.size())
                die("cannot write to " + run.cfg.lca_file + ": " + strerror(errno));
            return;
        }
        char num[4][24];
        for (size_t r = 0; r < n; ++r) {
            const int32_t node = bt.lca_node[r];
            const bool u = node == TAXOR_LCA_UNCLASSIFIED;
            lca_text += u ? "U\t" : "C\t";
            lca_text.append(bt.ids.ptr(r), bt.ids.len(r));
            lca_text += '\t';
            lca_text += u ? "0" : node == TAXOR_LCA_ROOT ? "1" : lv.id[node];
            snprintf(num[0], sizeof num[0], "%llu", (unsigned long long)(bt.offsets[r + 1] - bt.offsets[r]));
            snprintf(num[1], sizeof num[1], "%u", u ? 0u : bt.n_hashes[r]);
            snprintf(num[2], sizeof num[2], "%u", bt.lca_best[r]);
            snprintf(num[3], sizeof num[3], "%u", bt.lca_refs[r]);
            for (const auto &x : num) { lca_text += '\t'; lca_text += x; }
            lca_text += '\n';
        }
        if (!lca_text.empty() && fwrite(lca_text.data(), 1, lca_text.size(), run.lca_out) != lca_text.size())
            die("cannot write to " + run.cfg.lca_file + ": " + strerror(errno));
    }
    // --hitmap-file: the chunk's mapped tuples, one line each, by the sequencer (hitmap_format.h)
    std::string hitmap_text;
    void write_hitmap_lines(const Batch &bt)
    {
        const size_t n = bt.ids.size();
        const uint32_t S = run.cfg.hitmap_segments ? run.cfg.hitmap_segments : taxor::HITMAP_DEFAULT_SEGMENTS;
        if (bt.hm_off.size() != n + 1 || bt.n_hashes.size() != n || bt.hm_hits.size() != bt.hm_count.size() * S)
            die("internal: a chunk reached the writer without its reads' hit maps");
        const taxor_hixf_meta *meta = taxor_hixf_get_meta(h);
        hitmap_text.clear();
        for (size_t r = 0; r < n; ++r)
            for (uint64_t t = bt.hm_off[r]; t < bt.hm_off[r + 1]; ++t) {
                const uint64_t b = (uint64_t)bt.hm_user_bin[t];
                const taxor_species *sp = meta->n_species ? &meta->species[b < run.hitmap_species.size() ? run.hitmap_species[b] : 0] : nullptr;
                taxor::hitmap_line(hitmap_text, bt.ids.ptr(r), bt.ids.len(r), sp ? sp->accession_id : nullptr, sp ? sp->taxid : nullptr, bt.offsets[r + 1] - bt.offsets[r],
                                   bt.n_hashes[r], bt.hm_count[t], bt.hm_hits.data() + t * S, S);
            }
        run.hitmap_lines += bt.hm_count.size();
        if (!hitmap_text.empty() && fwrite(hitmap_text.data(), 1, hitmap_text.size(), run.hitmap_out) != hitmap_text.size())
            die("cannot write to " + run.cfg.hitmap_file + ": " + strerror(errno));
    }
    // --breakpoint-file: the chunk's reported reads, one line each, by the sequencer (breakpoint_format.h)
    std::string breakpoint_text;
    void write_breakpoint_lines(Batch &bt)
    {
        const size_t n = bt.ids.size();
        if (!bt.bp_set || bt.n_hashes.size() != n) die("internal: a chunk reached the writer without its reads' breaks");
        bt.bp_set = false;
        const taxor_hixf_meta *meta = taxor_hixf_get_meta(h);
        auto ref = [&](int64_t bin) {     // the species `taxor_format_read` prints for the user bin
            const uint64_t b = (uint64_t)bin;
            const taxor_species *sp = meta->n_species ? &meta->species[b < run.breakpoint_species.size() ? run.breakpoint_species[b] : 0] : nullptr;
            return taxor::breakpoint_ref{sp ? sp->accession_id : nullptr, sp ? sp->taxid : nullptr};
        };
        breakpoint_text.clear();
        for (const Batch::BreakRow &x : bt.bp_rows) {
            if (x.read >= n) die("internal: a break names a read outside its chunk");
            if (run.cfg.base_positions)
                taxor::breakpoint_line_positions(breakpoint_text, bt.ids.ptr(x.read), bt.ids.len(x.read), bt.offsets[x.read + 1] - bt.offsets[x.read], bt.n_hashes[x.read],
                                                 x.n_cand, ref(x.bin_best), x.single, x.break_hash, ref(x.bin_a), x.pre_a, x.pre_b, ref(x.bin_b), x.suf_b, x.suf_a, x.gain,
                                                 x.left_end_base, x.break_base);
            else
                taxor::breakpoint_line(breakpoint_text, bt.ids.ptr(x.read), bt.ids.len(x.read), bt.offsets[x.read + 1] - bt.offsets[x.read], bt.n_hashes[x.read], x.n_cand,
                                       ref(x.bin_best), x.single, x.break_hash, ref(x.bin_a), x.pre_a, x.pre_b, ref(x.bin_b), x.suf_b, x.suf_a, x.gain);
        }
        run.breakpoint_lines += bt.bp_rows.size();
        if (!breakpoint_text.empty() && fwrite(breakpoint_text.data(), 1, breakpoint_text.size(), run.breakpoint_out) != breakpoint_text.size())
            die("cannot write to " + run.cfg.breakpoint_file + ": " + strerror(errno));
    }
    // --segments-file: the chunk's reported reads, one line per segment, by the sequencer (segments_format.h)
    std::string segments_text;
    std::vector<int64_t> segments_bins;
    void write_segments_lines(Batch &bt)
    {
        const size_t n = bt.ids.size();
        if (!bt.sg_set || bt.n_hashes.size() != n) die("internal: a chunk reached the writer without its reads' segments");
        bt.sg_set = false;
        const taxor_hixf_meta *meta = taxor_hixf_get_meta(h);
        auto ref = [&](int64_t bin) {     // the species `taxor_format_read` prints for the user bin
            const uint64_t b = (uint64_t)bin;
            const taxor_species *sp = meta->n_species ? &meta->species[b < run.segments_species.size() ? run.segments_species[b] : 0] : nullptr;
            return taxor::breakpoint_ref{sp ? sp->accession_id : nullptr, sp ? sp->taxid : nullptr};
        };
        segments_text.clear();
        for (const Batch::SegRow &x : bt.sg_rows) {
            if (x.read >= n || x.n_seg < 2 || x.first + x.n_seg > bt.sg_segs.size()) die("internal: a segmented read lies outside its chunk");
            segments_bins.clear();
            for (uint32_t j = 0; j < x.n_seg; ++j) segments_bins.push_back(bt.sg_segs[x.first + j].bin);
            const char *shape = taxor::segments_shape(x.n_seg, segments_bins.data());
            for (uint32_t j = 0; j < x.n_seg; ++j) {
                const Batch::Seg &sg = bt.sg_segs[x.first + j];
                if (run.cfg.base_positions)
                    taxor::segments_line_positions(segments_text, bt.ids.ptr(x.read), bt.ids.len(x.read), bt.offsets[x.read + 1] - bt.offsets[x.read], bt.n_hashes[x.read],
                                                   x.n_cand, x.n_seg, shape, x.path_hits, x.single, j, sg.start, sg.end, ref(sg.bin), sg.hits, ref(x.bin_best), sg.best_hits,
                                                   sg.base_start, sg.base_end);
                else
                    taxor::segments_line(segments_text, bt.ids.ptr(x.read), bt.ids.len(x.read), bt.offsets[x.read + 1] - bt.offsets[x.read], bt.n_hashes[x.read], x.n_cand,
                                         x.n_seg, shape, x.path_hits, x.single, j, sg.start, sg.end, ref(sg.bin), sg.hits, ref(x.bin_best), sg.best_hits);
            }
            run.segments_lines += x.n_seg;
        }
        run.segments_reported += bt.sg_rows.size();
        if (!segments_text.empty() && fwrite(segments_text.data(), 1, segments_text.size(), run.segments_out) != segments_text.size())
            die("cannot write to " + run.cfg.segments_file + ": " + strerror(errno));
    }
    // --exclusive-reads-file: the chunk's rows, one line each, by the sequencer (exclusive_format.h)
    std::string exclusive_text;
    void write_exclusive_lines(Batch &bt)
    {
        const size_t n = bt.ids.size();
        if (!bt.ex_set || bt.n_hashes.size() != n) die("internal: a chunk reached the writer without its reads' exclusive hashes");
        bt.ex_set = false;
        const taxor_hixf_meta *meta = taxor_hixf_get_meta(h);
        exclusive_text.clear();
        for (const Batch::ExRow &x : bt.ex_rows) {
            if (x.read >= n) die("internal: an exclusive row names a read outside its chunk");
            const uint64_t b = (uint64_t)x.bin;     // the species `taxor_format_read` prints for the user bin
            const taxor_species *sp = meta->n_species ? &meta->species[b < run.exclusive_species.size() ? run.exclusive_species[b] : 0] : nullptr;
            taxor::exclusive_read_line(exclusive_text, bt.ids.ptr(x.read), bt.ids.len(x.read), taxor::exclusive_ref{sp ? sp->accession_id : nullptr, sp ? sp->taxid : nullptr},
                                       bt.offsets[x.read + 1] - bt.offsets[x.read], bt.n_hashes[x.read], x.count, x.hits, x.excl, x.n_cand, x.matched, x.shared);
        }
        run.exclusive_lines += bt.ex_rows.size();
        if (!exclusive_text.empty() && fwrite(exclusive_text.data(), 1, exclusive_text.size(), run.exclusive_reads_out) != exclusive_text.size())
            die("cannot write to " + run.cfg.exclusive_reads_file + ": " + strerror(errno));
    }
    // a piece's text goes to the file when its ticket comes up
    void write_in_turn(const Piece &pc, const char *text, uint64_t need)
    {
        static const bool turn_spin = [] { const char *e = tune_env("TAXOR_CLI_TURN_SPIN"); return e ? atoi(e) != 0 : true; }();
        // (the thread that is next in line does not go to sleep for the ~0.1 ms its predecessor writes: a wake-up costs
        // 10-20 us of every 120)
        if (turn_spin && pc.ticket - turn_now.load(std::memory_order_acquire) == 1)
            for (int spin = 0; spin < 20000 && turn_now.load(std::memory_order_acquire) != pc.ticket; ++spin) _mm_pause();
        std::unique_lock<std::mutex> lk(turn_mu);
        turn_cv[pc.ticket % 64].wait(lk, [&] { return next_ticket == pc.ticket; });
        const double w0 = now();
        if (t_first_write == 0) t_first_write = w0;
        for (uint64_t done = 0; done < need;) {
            const ssize_t w = ::write(out_fd, text + done, need - done);
            if (w < 0 && errno == EINTR) continue;            // a signal (SIGSTOP / SIGCONT, a debugger) is not an I/O error
            if (w <= 0) die("cannot write to " + run.cfg.report_file + ": " + (w < 0 ? strerror(errno) : "write() returned 0"));
            done += (uint64_t)w;
        }
        t_last_write = now();
        t_write += t_last_write - w0;
        ++next_ticket;
        turn_now.store(next_ticket, std::memory_order_release);
        turn_cv[next_ticket % 64].notify_all();
    }
    void format_pieces()
    {
        Piece pc;
        std::vector<const char *> idp;
        std::vector<uint64_t> idl, rl;
        std::vector<char> text(piece_bytes + piece_bytes / 2);
        while (q_piece.pop(pc)) {
            const Batch &bt = *pc.h->b;
            const size_t n = pc.r1 - pc.r0;
            idp.resize(n); idl.resize(n); rl.resize(n);
            for (size_t r = 0; r < n; ++r) {
                idp[r] = bt.ids.ptr(pc.r0 + r);
                idl[r] = bt.ids.len(pc.r0 + r);
                rl[r] = bt.offsets[pc.r0 + r + 1] - bt.offsets[pc.r0 + r];
            }
            const uint64_t need = format_reads(h, n, idp.data(), idl.data(), rl.data(), bt.n_hashes.data() + pc.r0, bt.read_off.data() + pc.r0,
                                               bt.user_bin.data(), bt.count.data(), text);
            const uint64_t tuples = bt.read_off[pc.r1] - bt.read_off[pc.r0];
            if (tuples > 64) line_bytes_guess = std::max<uint64_t>(64, need / tuples + 16);
            write_in_turn(pc, text.data(), need);
            out_written += need;
            if (pc.h->left.fetch_sub(1) == 1) chunk_done(pc.h);
        }
    }
    void start()
    {
        // from here on the report goes to the file descriptor: the header line was the last thing written through the FILE*
        // (flushed now); nothing may use `out`'s stdio buffer again until the pieces are done, or it would land out of order
        if (run.out) fflush(run.out);
        out_fd = run.out ? fileno(run.out) : -1;
        sequencer = std::thread([this] { sequence(); });
        for (unsigned ft = 0; ft < formatters; ++ft) fmt_threads.emplace_back([this] { format_pieces(); });
    }
    void join()
    {
        sequencer.join();
        for (auto &t : fmt_threads) t.join();
    }
};

// How many queued chunks make one GPU batch: ~group_reads reads -- the kernels want >= 10^5 reads in flight, the parsers want
// chunks small enough to hand out to many threads; short reads (`grow_short`: neither --batch-reads nor --group-reads given): more
// of them, until the batch holds 2^29 bases -- the library's sub-batches then reach their full size
struct GroupLimits {
    uint64_t group_reads;
    bool grow_short;
    static constexpr size_t max_chunks = 32;
    bool wants_more(uint64_t reads, uint64_t bases, size_t chunks) const
    {
        return (reads < group_reads || (grow_short && bases < (1ull << 29) && reads < (1u << 20))) && bases < (3ull << 30) && chunks < max_chunks;
    }
};

// --device-parse, where the device reported a range irregular: the chunk's file bytes parsed by the reader a range thread would
// have used (the same records, the same messages for a malformed file).  Returns the message, empty if all went well.
std::string host_parse(Batch &bt)
{
    try {
        ChunkParser ps;
        std::deque<std::vector<char>> parts;
        parts.emplace_back(bt.raw.data(), bt.raw.data() + bt.raw.size());
        ps.rd.open_mem(std::move(parts), bt.raw_kind == '@');
        bt.ids.clear();
        bt.bases.clear();
        bt.bases.reserve(fastx::bases_bound(bt.raw.size(), bt.raw_kind));
        bt.offsets.assign(1, 0);
        ps.parse(bt);
    } catch (const std::exception &ex) { return ex.what(); }
    bt.raw_kind = 0;
    return std::string();
}

// ---- `--coverage-file`: the run's table, fetched once.  One line per user bin that any read reported, in user-bin order; the species
// of a user bin as the TSV names it (the first that carries it, species[0] if none: taxor_search.cpp:172-178,289).
void write_coverage_file(SearchRun &run, const taxor_hixf_meta *meta)
{
    taxor_coverage_results cr{};
    if (taxor_gpu_coverage_results(run.coverage, &cr) != TAXOR_OK) die(taxor_gpu_last_error());
    const std::string &path = run.cfg.coverage_file;
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) die("cannot open coverage file " + path);
    std::vector<uint32_t> bin_species(cr.n_user_bins, 0u);
    for (uint64_t i = meta->n_species; i-- > 0;)
        if (meta->species[i].user_bin < cr.n_user_bins) bin_species[meta->species[i].user_bin] = (uint32_t)i;
    const bool breadth = run.cfg.coverage_breadth;
    fprintf(f, "#ACCESSION\tREFERENCE_NAME\tTAXID\tREF_LEN\tREADS\tHASH_MATCHES\tDISTINCT_HASHES\tDUPLICITY%s\n", breadth ? taxor::census_breadth_header() : "");
    std::string more;
    uint64_t lines = 0;
    for (uint64_t b = 0; b < cr.n_user_bins; ++b) {
        if (cr.reads[b] == 0) continue;
        long long distinct = llround(taxor_hll_estimate(cr.registers + (b << cr.precision), cr.precision));
        if (cr.hash_matches[b] > 0 && distinct < 1) distinct = 1;
        static const taxor_species none{"-", "-", "-", "-", "-", 0, 0};
        const taxor_species &sp = meta->n_species ? meta->species[bin_species[b]] : none;
        more.clear();
        if (breadth) taxor::census_breadth_columns(more, (uint64_t)distinct, cr.hash_matches[b], b < run.index_hashes.size() ? run.index_hashes[b] : taxor::census_count{0, true});
        fprintf(f, "%s\t%s\t%s\t%llu\t%llu\t%llu\t%lld\t%.2f%s\n", sp.accession_id, sp.organism_name, sp.taxid, (unsigned long long)sp.seq_len,
                (unsigned long long)cr.reads[b], (unsigned long long)cr.hash_matches[b], distinct, distinct ? (double)cr.hash_matches[b] / (double)distinct : 0.0, more.c_str());
        ++lines;
    }
    if (ferror(f) || fclose(f) != 0) die("cannot write to " + path + ": " + strerror(errno));
    if (tune_env("TAXOR_CLI_TRACE"))
        fprintf(stderr, "[trace] coverage: %llu of %llu user bins reported, precision %u; %.3f s inside the accumulation (summed over workers), %.3f s in its kernel, "
                        "%llu lookups of a hash in a leaf bin = %.2f G gathers/s, %.1f GB/s of 128-B lines\n",
                (unsigned long long)lines, (unsigned long long)cr.n_user_bins, cr.precision, run.t_coverage, cr.seconds_kernels, (unsigned long long)cr.probes,
                cr.seconds_kernels > 0 ? 3.0 * cr.probes / cr.seconds_kernels / 1e9 : 0.0, cr.seconds_kernels > 0 ? 3.0 * 128.0 * cr.probes / cr.seconds_kernels / 1e9 : 0.0);
    taxor_gpu_coverage_destroy(run.coverage);
    run.coverage = nullptr;
}

// ---- `--hitmap-file`: the lines were written chunk by chunk; the file is closed here
void finish_hitmap(SearchRun &run)
{
    if (run.hitmap_out) {
        if (ferror(run.hitmap_out) || fclose(run.hitmap_out) != 0) die("cannot write to " + run.cfg.hitmap_file + ": " + strerror(errno));
        run.hitmap_out = nullptr;
    }
    if (tune_env("TAXOR_CLI_TRACE"))
        fprintf(stderr, "[trace] hitmap: %llu lines; %.3f s inside the locating (summed over workers), %.3f s in its kernels, "
                        "%llu lookups of a hash in a leaf bin = %.2f G gathers/s, %.1f GB/s of 128-B lines\n",
                (unsigned long long)run.hitmap_lines, run.t_hitmap, run.t_hitmap_kernels, (unsigned long long)run.hitmap_probes,
                run.t_hitmap_kernels > 0 ? 3.0 * run.hitmap_probes / run.t_hitmap_kernels / 1e9 : 0.0,
                run.t_hitmap_kernels > 0 ? 3.0 * 128.0 * run.hitmap_probes / run.t_hitmap_kernels / 1e9 : 0.0);
    taxor_gpu_hitmap_destroy(run.hitmap);
    run.hitmap = nullptr;
}

// ---- `--breakpoint-file`: the lines were written chunk by chunk; the file is closed here
void finish_breakpoint(SearchRun &run)
{
    if (run.breakpoint_out) {
        if (ferror(run.breakpoint_out) || fclose(run.breakpoint_out) != 0) die("cannot write to " + run.cfg.breakpoint_file + ": " + strerror(errno));
        run.breakpoint_out = nullptr;
    }
    if (tune_env("TAXOR_CLI_TRACE"))
        fprintf(stderr, "[trace] breakpoint: %llu lines from %llu examined reads of %llu; %.3f s inside the examining (summed over workers), %.6f s in its kernels, "
                        "%llu lookups of a hash in a leaf bin = %.2f G gathers/s\n",
                (unsigned long long)run.breakpoint_lines, (unsigned long long)run.breakpoint_examined, (unsigned long long)run.breakpoint_reads, run.t_breakpoint,
                run.t_breakpoint_kernels, (unsigned long long)run.breakpoint_lookups,
                run.t_breakpoint_kernels > 0 ? 3.0 * run.breakpoint_lookups / run.t_breakpoint_kernels / 1e9 : 0.0);
    taxor_gpu_breakpoint_destroy(run.breakpoint);
    run.breakpoint = nullptr;
}

// ---- `--segments-file`: the lines were written chunk by chunk; the file is closed here
void finish_segments(SearchRun &run)
{
    if (run.segments_out) {
        if (ferror(run.segments_out) || fclose(run.segments_out) != 0) die("cannot write to " + run.cfg.segments_file + ": " + strerror(errno));
        run.segments_out = nullptr;
    }
    if (tune_env("TAXOR_CLI_TRACE"))
        fprintf(stderr, "[trace] segments: %llu lines from %llu reported reads of %llu examined reads of %llu; %.3f s inside the segmenting (summed over workers), %.6f s in its "
                        "kernels, %llu lookups of a hash in a leaf bin, %llu groups of reads under the scratch budget\n",
                (unsigned long long)run.segments_lines, (unsigned long long)run.segments_reported, (unsigned long long)run.segments_examined,
                (unsigned long long)run.segments_reads, run.t_segments, run.t_segments_kernels, (unsigned long long)run.segments_lookups,
                (unsigned long long)run.segments_groups);
    taxor_gpu_segments_destroy(run.segments);
    run.segments = nullptr;
}

// ---- `--exclusive-file`: the run's table, fetched once and written here, one line per user bin that was a candidate of an examined read, in
// user-bin order (the coverage file's; the species of a user bin as the TSV names it).  `--exclusive-reads-file` was written chunk by chunk
// and is closed here
void finish_exclusive(SearchRun &run, const taxor_hixf_meta *meta)
{
    if (run.exclusive_reads_out) {
        if (ferror(run.exclusive_reads_out) || fclose(run.exclusive_reads_out) != 0) die("cannot write to " + run.cfg.exclusive_reads_file + ": " + strerror(errno));
        run.exclusive_reads_out = nullptr;
    }
    uint64_t lines = 0;
    if (!run.cfg.exclusive_file.empty()) {
        taxor_exclusive_results er{};
        if (taxor_gpu_exclusive_results(run.exclusive, &er) != TAXOR_OK) die(taxor_gpu_last_error());
        const std::string &path = run.cfg.exclusive_file;
        FILE *f = fopen(path.c_str(), "wb");
        if (!f) die("cannot open exclusive file " + path);
        std::string text = taxor::exclusive_header();
        for (uint64_t b = 0; b < er.n_user_bins; ++b) {
            if (er.cand_reads[b] == 0) continue;
            const taxor_species *sp = meta->n_species ? &meta->species[b < run.exclusive_species.size() ? run.exclusive_species[b] : 0] : nullptr;
            taxor::exclusive_bin_line(text, taxor::exclusive_ref{sp ? sp->accession_id : nullptr, sp ? sp->taxid : nullptr}, er.cand_reads[b], er.hits[b], er.exclusive_hits[b],
                                      er.exclusive_reads[b], taxor::exclusive_distinct(taxor_hll_estimate(er.registers + (b << er.precision), er.precision), er.exclusive_hits[b]));
            ++lines;
        }
        if (fwrite(text.data(), 1, text.size(), f) != text.size() || ferror(f) || fclose(f) != 0) die("cannot write to " + path + ": " + strerror(errno));
    }
    if (tune_env("TAXOR_CLI_TRACE"))
        fprintf(stderr, "[trace] exclusive: %llu user bins and %llu read lines from %llu examined reads of %llu; %.3f s inside the examining (summed over workers), %.6f s in its "
                        "kernels, %llu lookups of a hash in a leaf bin = %.2f G gathers/s\n",
                (unsigned long long)lines, (unsigned long long)run.exclusive_lines, (unsigned long long)run.exclusive_examined, (unsigned long long)run.exclusive_reads,
                run.t_exclusive, run.t_exclusive_kernels, (unsigned long long)run.exclusive_probes,
                run.t_exclusive_kernels > 0 ? 3.0 * run.exclusive_probes / run.t_exclusive_kernels / 1e9 : 0.0);
    taxor_gpu_exclusive_destroy(run.exclusive);
    run.exclusive = nullptr;
}

// ---- `--report-file`: the run's tallies, fetched once, rolled up the tree on the host (a few hundred thousand nodes at most, once per
// run) and written as a Kraken-style report; `--lca-file` is closed here as well.  The layout: percentage of
// the clade, clade count, direct count, rank code, taxid, name indented by two spaces per depth; unclassified first, then the tree from
// the root depth-first, children by clade count descending, ties by id string byte-wise ascending; empty clades are left out.
void finish_lca(SearchRun &run)
{
    const Config &cfg = run.cfg;
    if (run.lca_out) {
        if (ferror(run.lca_out) || fclose(run.lca_out) != 0) die("cannot write to " + cfg.lca_file + ": " + strerror(errno));
        run.lca_out = nullptr;
    }
    taxor_lca_results lr{};
    if ((run.confidence ? taxor_gpu_confidence_results(run.confidence, &lr) : taxor_gpu_lca_results(run.lca, &lr)) != TAXOR_OK) die(taxor_gpu_last_error());
    const taxor_lineage_view &lv = run.lineage_view;
    const uint64_t nn = lr.n_nodes;
    if (!cfg.kraken_file.empty()) {
        const uint64_t *direct = cfg.report_unit == "bases" ? lr.direct_bases : lr.direct_reads;
        FILE *f = fopen(cfg.kraken_file.c_str(), "wb");
        if (!f) die("cannot open report file " + cfg.kraken_file);
        // clade counts: a node's parent has the smaller depth, so deepest first
        std::vector<uint64_t> clade(direct, direct + nn + 1);           // [nn] = ROOT
        std::vector<uint32_t> by_depth(nn);
        for (uint64_t x = 0; x < nn; ++x) by_depth[x] = (uint32_t)x;
        std::stable_sort(by_depth.begin(), by_depth.end(), [&](uint32_t a, uint32_t b) { return lv.depth[a] > lv.depth[b]; });
        for (uint32_t x : by_depth) clade[lv.parent[x] < 0 ? nn : (uint64_t)lv.parent[x]] += clade[x];
        const uint64_t total = clade[nn] + direct[nn + 1];
        // children of every node (ROOT at nn), in the order they are printed; node numbers ascend with the id strings
        std::vector<uint64_t> child_off(nn + 2, 0);
        for (uint64_t x = 0; x < nn; ++x)
            if (clade[x]) ++child_off[(lv.parent[x] < 0 ? nn : (uint64_t)lv.parent[x]) + 1];
        for (uint64_t x = 0; x <= nn; ++x) child_off[x + 1] += child_off[x];
        std::vector<uint32_t> child(child_off[nn + 1]);
        {
            std::vector<uint64_t> at(child_off.begin(), child_off.end() - 1);
            for (uint64_t x = 0; x < nn; ++x)
                if (clade[x]) child[at[lv.parent[x] < 0 ? nn : (uint64_t)lv.parent[x]]++] = (uint32_t)x;
        }
        for (uint64_t x = 0; x <= nn; ++x)
            std::stable_sort(child.begin() + (std::ptrdiff_t)child_off[x], child.begin() + (std::ptrdiff_t)child_off[x + 1], [&](uint32_t a, uint32_t b) { return clade[a] > clade[b]; });
        auto rank_code = [](char r) { switch (r) { case 'k': return 'D'; case 'p': return 'P'; case 'c': return 'C'; case 'o': return 'O'; case 'f': return 'F'; case 'g': return 'G'; case 's': return 'S'; default: return '-'; } };
        if (total) {
            if (direct[nn + 1]) fprintf(f, "%6.2f\t%llu\t%llu\tU\t0\tunclassified\n", 100.0 * (double)direct[nn + 1] / (double)total, (unsigned long long)direct[nn + 1], (unsigned long long)direct[nn + 1]);
            if (clade[nn]) {
                fprintf(f, "%6.2f\t%llu\t%llu\tR\t1\troot\n", 100.0 * (double)clade[nn] / (double)total, (unsigned long long)clade[nn], (unsigned long long)direct[nn]);
                std::vector<std::pair<uint64_t, uint64_t>> stack;      // (node, next child) -- depth-first without recursion
                stack.emplace_back(nn, child_off[nn]);
                while (!stack.empty()) {
                    auto &top = stack.back();
                    if (top.second == child_off[top.first + 1]) { stack.pop_back(); continue; }
                    const uint32_t x = child[top.second++];
                    fprintf(f, "%6.2f\t%llu\t%llu\t%c\t%s\t%*s%s\n", 100.0 * (double)clade[x] / (double)total, (unsigned long long)clade[x], (unsigned long long)direct[x],
                            rank_code(lv.rank[x]), lv.id[x], (int)(2 * lv.depth[x]), "", lv.name[x]);
                    stack.emplace_back(x, child_off[x]);
                }
            }
        }
        if (ferror(f) || fclose(f) != 0) die("cannot write to " + cfg.kraken_file + ": " + strerror(errno));
    }
    if (tune_env("TAXOR_CLI_TRACE"))
        fprintf(stderr, "[trace] lca: %llu nodes, %llu reads called, %llu of them unclassified; %.3f s inside the accumulation (summed over workers), %.6f s in its kernel\n",
                (unsigned long long)nn, (unsigned long long)lr.n_reads, (unsigned long long)lr.direct_reads[nn + 1], run.confidence ? run.t_confidence : run.t_lca, lr.seconds_kernel);
    if (run.confidence && tune_env("TAXOR_CLI_TRACE"))
        fprintf(stderr, "[trace] confidence: threshold %g; %.3f s inside the weighing (summed over workers), %.6f s in its kernels, %llu (hash, leaf bin) lookups, "
                        "%llu of %llu (64 hashes, tuple) steps made\n",
                cfg.lca_confidence, run.t_confidence, run.t_confidence_kernels, (unsigned long long)run.confidence_probes, (unsigned long long)run.confidence_steps,
                (unsigned long long)run.confidence_steps_full);
    taxor_gpu_confidence_destroy(run.confidence);
    run.confidence = nullptr;
    taxor_gpu_lca_destroy(run.lca);
    run.lca = nullptr;
    taxor_lineage_free(run.lineage);
    run.lineage = nullptr;
}

// ---- the devices: one index replica per device (reads are independent, taxor_search.cpp:214: the index is replicated,
// batches are sharded), the searchers, and the workers that make GPU batches of the queued chunks.  Several devices (north star:
// "reads sharded across the GPUs, per-read results gathered over RCCL/xGMI"): one communicator; the index crosses PCIe once and is
// broadcast, rounds of ng batches are classified side by side and their results gathered on the first device (taxor_gpu.h,
// "Several GPUs of one node").  The transport is decided in upload_index, once, by rule -- never by a failure.
struct GpuStage {
    using Chunks = std::vector<std::unique_ptr<Batch>>;
    SearchRun &run;
    Pipes &p;
    size_t ng;
    unsigned wpg;       // workers per device; with a communicator: that many searcher SETS (one searcher per device each), rounds alternate between them
    GroupLimits limits;
    std::vector<taxor_gpu_index *> gidx;
    taxor_gpu_comm *comm = nullptr;
    std::string gather;
    std::vector<taxor_gpu_searcher *> sr;      // device-major: sr[g * wpg + w]
    std::mutex comm_mu;     // a communicator is single-caller, and its result arrays live until its next gather
    std::atomic<int> n_running{0};      // GPU batches in flight (single-device workers)
    std::atomic<uint64_t> n_bam{0};        // BAM chunks unpacked on the device
    std::atomic<uint64_t> n_scanned{0}, n_host_parsed{0}, n_pageable{0};   // n_pageable: chunks whose buffer could not be page-locked
    std::vector<std::thread> workers;
    GpuStage(SearchRun &run_, Pipes &p_, size_t ng_, unsigned wpg_, GroupLimits l) : run(run_), p(p_), ng(ng_), wpg(wpg_), limits(l) {}

    void upload_index(const taxor_hixf_view *view)
    {
        const Config &cfg = run.cfg;
        gidx.assign(ng, nullptr);
        gather = cfg.gather;
        if (gather.empty()) {
            bool distinct = true;
            for (size_t i = 0; i < ng; ++i)
                for (size_t j = i + 1; j < ng; ++j) distinct = distinct && cfg.gpus[i] != cfg.gpus[j];
            gather = ng == 1 ? "none" : (distinct ? "rccl" : "host");
        }
        if (gather != "none") {
            if (taxor_gpu_comm_create(cfg.gpus.data(), (uint32_t)ng, gather == "rccl" ? TAXOR_COMM_RCCL : TAXOR_COMM_HOST, &comm) != TAXOR_OK)
                die(std::string(taxor_gpu_last_error()) + "\n(--gather host stages the same transfers through host memory)");
            if (taxor_gpu_index_create_replicated(comm, view, gidx.data()) != TAXOR_OK) die(taxor_gpu_last_error());
            taxor_gpu_comm_stats cs{};
            taxor_gpu_comm_info(comm, &cs);
            if (tune_env("TAXOR_CLI_TRACE"))
                fprintf(stderr, "[trace] index on %zu devices (%s): %.2f GB per replica, %.2f GB over PCIe, %.2f GB by ncclBroadcast, %.3f s\n", ng,
                        gather.c_str(), cs.index_bytes / 1e9, cs.index_upload_bytes / 1e9, cs.index_broadcast_bytes / 1e9, cs.index_seconds);
            return;
        }
        std::vector<std::thread> up;
        std::vector<std::string> errs(ng);
        for (size_t g = 0; g < ng; ++g)
            up.emplace_back([this, view, g, &errs] {
                const int rc = taxor_gpu_index_create(view, run.cfg.gpus[g], &gidx[g]);
                if (rc != TAXOR_OK) errs[g] = std::string(taxor_gpu_last_error()) + (rc == TAXOR_E_NOMEM ? "\n(--device-index-budget <MiB> searches an index in resident passes: taxor search --advanced-help)" : "");
            });
        for (auto &t : up) t.join();
        for (const auto &e : errs)
            if (!e.empty()) die(e);
    }
    void create_searchers(const taxor_gpu_search_params &prm)
    {
        sr.assign(ng * wpg, nullptr);
        for (size_t g = 0; g < ng; ++g)
            for (unsigned w = 0; w < wpg; ++w)
                if (taxor_gpu_searcher_create(gidx[g], &prm, &sr[g * wpg + w]) != TAXOR_OK) die(taxor_gpu_last_error());
    }
    // --coverage-file / --hitmap-file / --lca-confidence / --breakpoint-file / --segments-file / --exclusive-file: the consumers beside the (one) index, and every searcher leaves its batches' hash lists for them
    void begin_saved_consumers(const taxor_hixf_view *view, const taxor_hixf_meta *meta)
    {
        const Config &cfg = run.cfg;
        if (!cfg.coverage_file.empty() && taxor_gpu_coverage_create(gidx[0], view, cfg.coverage_precision, &run.coverage) != TAXOR_OK) die(taxor_gpu_last_error());
        if (cfg.coverage_breadth) {      // the census runs once, now that the index is resident
            CensusRun cr = census_of(gidx[0], view);
            run.index_hashes = std::move(cr.tables.index_hashes);
            if (tune_env("TAXOR_CLI_TRACE"))
                fprintf(stderr, "[trace] census: %.2f GB of fingerprints in %.3f s wall, %.3f ms in its kernel = %.1f GB/s, %llu tiles in %u launch(es)\n", cr.bytes_read / 1e9,
                        cr.seconds_wall, cr.seconds_kernel * 1e3, cr.seconds_kernel > 0 ? cr.bytes_read / 1e9 / cr.seconds_kernel : 0.0, (unsigned long long)cr.n_tiles, cr.launches);
        }
        if (!cfg.hitmap_file.empty()) {
            if (taxor_gpu_hitmap_create(gidx[0], view, cfg.hitmap_segments ? cfg.hitmap_segments : taxor::HITMAP_DEFAULT_SEGMENTS, &run.hitmap) != TAXOR_OK) die(taxor_gpu_last_error());
            // the species of a user bin as the TSV names it (the first that carries it, species[0] if none: taxor_search.cpp:172-178,289)
            run.hitmap_species.assign(view->n_user_bins, 0u);
            for (uint64_t i = meta->n_species; i-- > 0;)
                if (meta->species[i].user_bin < view->n_user_bins) run.hitmap_species[meta->species[i].user_bin] = (uint32_t)i;
        }
        if (cfg.confidence_mode() && taxor_gpu_confidence_create(gidx[0], view, run.lineage, cfg.lca_confidence, &run.confidence) != TAXOR_OK) die(taxor_gpu_last_error());
        if (!cfg.breakpoint_file.empty()) {
            if (taxor_gpu_breakpoint_create(gidx[0], view, cfg.breakpoint_min_gain ? cfg.breakpoint_min_gain : taxor::BREAKPOINT_DEFAULT_MIN_GAIN, &run.breakpoint) != TAXOR_OK)
                die(taxor_gpu_last_error());
            run.breakpoint_species.assign(view->n_user_bins, 0u);     // as for the hit map
            for (uint64_t i = meta->n_species; i-- > 0;)
                if (meta->species[i].user_bin < view->n_user_bins) run.breakpoint_species[meta->species[i].user_bin] = (uint32_t)i;
        }
        if (!cfg.segments_file.empty()) {
            if (taxor_gpu_segments_create(gidx[0], view, cfg.segments_switch_cost ? cfg.segments_switch_cost : taxor::SEGMENTS_DEFAULT_SWITCH_COST, &run.segments) != TAXOR_OK)
                die(taxor_gpu_last_error());
            run.segments_species.assign(view->n_user_bins, 0u);       // as for the hit map
            for (uint64_t i = meta->n_species; i-- > 0;)
                if (meta->species[i].user_bin < view->n_user_bins) run.segments_species[meta->species[i].user_bin] = (uint32_t)i;
        }
        if (cfg.exclusive_mode()) {
            if (taxor_gpu_exclusive_create(gidx[0], view, cfg.exclusive_precision, &run.exclusive) != TAXOR_OK) die(taxor_gpu_last_error());
            run.exclusive_species.assign(view->n_user_bins, 0u);      // as for the hit map
            for (uint64_t i = meta->n_species; i-- > 0;)
                if (meta->species[i].user_bin < view->n_user_bins) run.exclusive_species[meta->species[i].user_bin] = (uint32_t)i;
        }
        for (auto *s : sr)
            if (taxor_gpu_search_capture(s, 1) != TAXOR_OK) die(taxor_gpu_last_error());
        if (cfg.base_positions)      // --base-positions: the saved batches carry every hash's position in its read (positions.hip)
            for (auto *s : sr)
                if (taxor_gpu_search_capture_positions(s, 1) != TAXOR_OK) die(taxor_gpu_last_error());
    }
    // after a batch's end: its saved lists are taken ONCE, used by the consumers that are on and freed -- none is kept across batches,
    // so host memory stays bounded by the batches in flight.  The hit map's share goes to each chunk of the batch
    void use_saved(taxor_gpu_searcher *s, Chunks &group)
    {
        const double c0 = now();
        taxor_gpu_saved *sv = nullptr;
        if (taxor_gpu_search_take_saved(s, &sv) != TAXOR_OK) die(taxor_gpu_last_error());
        const double c1 = now();
        int rc = run.coverage ? taxor_gpu_coverage_add_batch(run.coverage, s, sv) : TAXOR_OK;
        const double c2 = now();
        taxor_hitmap_batch hb{};
        if (rc == TAXOR_OK && run.hitmap) rc = taxor_gpu_hitmap_add_batch(run.hitmap, s, sv, &hb);
        if (rc == TAXOR_OK && run.hitmap) {
            uint64_t nr = 0;
            for (auto &bt : group) nr += bt->ids.size();
            if (hb.n_reads != nr) die("internal: a batch's hit maps do not cover its chunks");
            const uint64_t S = hb.segments;
            uint64_t r0 = 0;
            for (auto &bt : group) {
                const uint64_t n = bt->ids.size(), lo = hb.map_off[r0], hi = hb.map_off[r0 + n];
                bt->hm_off.resize(n + 1);
                for (uint64_t i = 0; i <= n; ++i) bt->hm_off[i] = hb.map_off[r0 + i] - lo;
                bt->hm_user_bin.assign(hb.user_bin + lo, hb.user_bin + hi);
                bt->hm_count.assign(hb.count + lo, hb.count + hi);
                bt->hm_hits.assign(hb.hits + lo * S, hb.hits + hi * S);
                if (!run.write_tsv) bt->n_hashes.assign(hb.n_hashes + r0, hb.n_hashes + r0 + n);
                r0 += n;
            }
        }
        const double c3 = now();
        // --lca-confidence: the batch's reads are called from its results on the device and these lists; the calls go to the chunks
        taxor_confidence_calls cc{};
        if (rc == TAXOR_OK && run.confidence) {
            uint64_t nr = 0;
            for (auto &bt : group) nr += bt->ids.size();
            rc = taxor_gpu_confidence_add_batch(run.confidence, s, sv, run.lca_next_read.fetch_add(nr), &cc);
            if (rc == TAXOR_OK && cc.n_reads != nr) die("internal: a batch's calls do not cover its chunks");
            uint64_t r0 = 0;
            for (auto &bt : group) {
                if (rc != TAXOR_OK) break;
                const uint64_t n = bt->ids.size();
                bt->lca_node.assign(cc.node + r0, cc.node + r0 + n);
                bt->lca_best.assign(cc.best + r0, cc.best + r0 + n);
                bt->lca_refs.assign(cc.n_refs + r0, cc.n_refs + r0 + n);
                bt->cf_lca_node.assign(cc.lca_node + r0, cc.lca_node + r0 + n);
                bt->cf_support.assign(cc.support + r0, cc.support + r0 + n);
                bt->cf_lca_support.assign(cc.lca_support + r0, cc.lca_support + r0 + n);
                if (!run.write_tsv) bt->n_hashes.assign(cc.n_hashes + r0, cc.n_hashes + r0 + n);
                r0 += n;
            }
        }
        const double c3b = now();
        // --base-positions: the batch's positions, parallel to its hashes; the base columns are host lookups at the indices the analyses return
        const uint32_t *hpos = nullptr;
        taxor_gpu_saved_view svv{};
        if (rc == TAXOR_OK && run.cfg.base_positions) {
            if (taxor_gpu_saved_positions(sv, &hpos) != TAXOR_OK || taxor_gpu_saved_view_get(sv, &svv) != TAXOR_OK) die(taxor_gpu_last_error());
            if (!hpos && svv.total_hashes) die("internal: a batch was saved without the positions --base-positions asked for");
        }
        // the position of hash i of read r of the batch
        auto pos_of = [&](uint64_t r, uint64_t i) -> uint64_t {
            if (r >= svv.n_reads || i >= svv.hash_off[r + 1] - svv.hash_off[r]) die("internal: a base position is asked for a hash outside its read's list");
            return hpos[svv.hash_off[r] + i];
        };
        // --breakpoint-file: the reported reads of the batch go to the chunks that hold them
        taxor_breakpoint_batch bb{};
        if (rc == TAXOR_OK && run.breakpoint) rc = taxor_gpu_breakpoint_add_batch(run.breakpoint, s, sv, &bb);
        if (rc == TAXOR_OK && run.breakpoint) {
            uint64_t nr = 0;
            for (auto &bt : group) nr += bt->ids.size();
            if (bb.n_reads != nr) die("internal: a batch's breaks do not cover its chunks");
            uint64_t r0 = 0;
            for (auto &bt : group) {
                const uint64_t n = bt->ids.size();
                bt->bp_rows.clear();
                for (uint64_t i = 0; i < n; ++i) {
                    const uint64_t r = r0 + i;
                    if (bb.examined[r] && bb.gain[r] >= bb.min_gain)
                        bt->bp_rows.push_back(Batch::BreakRow{(uint32_t)i, bb.gain[r], bb.break_hash[r], bb.pre_a[r], bb.suf_b[r], bb.pre_b[r], bb.suf_a[r], bb.single[r],
                                                              bb.n_candidates[r], bb.bin_a[r], bb.bin_b[r], bb.bin_best[r]});
                    if (hpos && !bt->bp_rows.empty() && bt->bp_rows.back().read == (uint32_t)i) {
                        Batch::BreakRow &x = bt->bp_rows.back();
                        if (x.break_hash == 0) die("internal: a reported break stands in front of the read's first hash");
                        x.left_end_base = pos_of(r, x.break_hash - 1) + svv.kmer_size;
                        x.break_base = pos_of(r, x.break_hash);
                    }
                }
                bt->bp_set = true;
                if (!run.write_tsv) bt->n_hashes.assign(bb.n_hashes + r0, bb.n_hashes + r0 + n);
                r0 += n;
            }
        }
        const double c3c = now();
        // --segments-file: the reported reads of the batch and their segments go to the chunks that hold them
        taxor_segments_batch gb{};
        if (rc == TAXOR_OK && run.segments) rc = taxor_gpu_segments_add_batch(run.segments, s, sv, &gb);
        if (rc == TAXOR_OK && run.segments) {
            uint64_t nr = 0;
            for (auto &bt : group) nr += bt->ids.size();
            if (gb.n_reads != nr) die("internal: a batch's segments do not cover its chunks");
            uint64_t r0 = 0;
            for (auto &bt : group) {
                const uint64_t n = bt->ids.size();
                bt->sg_rows.clear();
                bt->sg_segs.clear();
                for (uint64_t i = 0; i < n; ++i) {
                    const uint64_t r = r0 + i, k = gb.seg_off[r + 1] - gb.seg_off[r];
                    if (k == 0) continue;
                    bt->sg_rows.push_back(Batch::SegRow{(uint32_t)i, gb.n_candidates[r], (uint32_t)k, gb.path_hits[r], gb.single[r], gb.bin_best[r], bt->sg_segs.size()});
                    for (uint64_t j = gb.seg_off[r]; j < gb.seg_off[r + 1]; ++j) {
                        bt->sg_segs.push_back(Batch::Seg{gb.seg_start[j], gb.seg_end[j], gb.seg_hits[j], gb.seg_best_hits[j], gb.seg_bin[j]});
                        if (hpos) {
                            Batch::Seg &g = bt->sg_segs.back();
                            if (g.end <= g.start) die("internal: a reported segment holds no hash");
                            g.base_start = pos_of(r, g.start);
                            g.base_end = pos_of(r, g.end - 1) + svv.kmer_size;
                        }
                    }
                }
                bt->sg_set = true;
                if (!run.write_tsv) bt->n_hashes.assign(gb.n_hashes + r0, gb.n_hashes + r0 + n);
                r0 += n;
            }
        }
        const double c3d = now();
        // --exclusive-file / --exclusive-reads-file: the per-user-bin sums stay on the device; the surviving tuples (the TSV's lines: the
        // 0.8 * max filter in fp64 as written, the maximum over the candidates being the maximum over the read's tuples) of the examined
        // reads with two candidates or more go to the chunks that hold them
        taxor_exclusive_batch eb{};
        if (rc == TAXOR_OK && run.exclusive) rc = taxor_gpu_exclusive_add_batch(run.exclusive, s, sv, &eb);
        if (rc == TAXOR_OK && run.exclusive && run.exclusive_reads_out) {
            uint64_t nr = 0;
            for (auto &bt : group) nr += bt->ids.size();
            if (eb.n_reads != nr) die("internal: a batch's exclusive hashes do not cover its chunks");
            uint64_t r0 = 0;
            for (auto &bt : group) {
                const uint64_t n = bt->ids.size();
                bt->ex_rows.clear();
                for (uint64_t i = 0; i < n; ++i) {
                    const uint64_t r = r0 + i;
                    if (!eb.examined[r] || eb.n_candidates[r] < 2) continue;
                    uint32_t mx = 0;
                    for (uint64_t g = eb.cand_off[r]; g < eb.cand_off[r + 1]; ++g) mx = std::max(mx, eb.cand_count[g]);
                    for (uint64_t g = eb.cand_off[r]; g < eb.cand_off[r + 1]; ++g)
                        if (!((double)eb.cand_count[g] < (double)mx * 0.8))
                            bt->ex_rows.push_back(Batch::ExRow{(uint32_t)i, eb.cand_count[g], eb.cand_hits[g], eb.cand_excl[g], eb.n_candidates[r], eb.matched[r], eb.shared[r],
                                                               eb.cand_bin[g]});
                }
                bt->ex_set = true;
                if (!run.write_tsv) bt->n_hashes.assign(eb.n_hashes + r0, eb.n_hashes + r0 + n);
                r0 += n;
            }
        }
        const double c3e = now();
        const double pos_seconds = run.cfg.base_positions ? taxor_gpu_saved_positions_seconds(sv) : 0.0;
        taxor_gpu_saved_free(sv);
        if (rc != TAXOR_OK) die(taxor_gpu_last_error());
        const double c4 = now(), shared = (c1 - c0) + (c4 - c3e);       // taking and freeing the lists: the first consumer's
        std::lock_guard<std::mutex> lk(run.stat_mu);
        if (run.cfg.base_positions) {
            run.t_positions_kernels += pos_seconds;
            run.positions_hashes += svv.total_hashes;
        }
        if (run.exclusive) {
            run.t_exclusive += c3e - c3d + (run.coverage || run.hitmap || run.confidence || run.breakpoint || run.segments ? 0.0 : shared);
            run.t_exclusive_kernels += eb.seconds_kernels;
            run.exclusive_probes += eb.probes;
            run.exclusive_examined += eb.n_examined;
            run.exclusive_reads += eb.n_reads;
        }
        if (run.confidence) {
            run.t_confidence += c3b - c3 + (run.coverage || run.hitmap ? 0.0 : shared);
            run.t_confidence_kernels += cc.seconds_kernels;
            run.confidence_probes += cc.probes;
            run.confidence_steps += cc.tuple_steps;
            run.confidence_steps_full += cc.tuple_steps_full;
        }
        if (run.breakpoint) {
            run.t_breakpoint += c3c - c3b + (run.coverage || run.hitmap || run.confidence ? 0.0 : shared);
            run.t_breakpoint_kernels += bb.seconds_kernels;
            run.breakpoint_lookups += bb.lookups;
            run.breakpoint_examined += bb.n_examined;
            run.breakpoint_reads += bb.n_reads;
        }
        if (run.segments) {
            run.t_segments += c3d - c3c + (run.coverage || run.hitmap || run.confidence || run.breakpoint ? 0.0 : shared);
            run.t_segments_kernels += gb.seconds_kernels;
            run.segments_lookups += gb.lookups;
            run.segments_examined += gb.n_examined;
            run.segments_reads += gb.n_reads;
            run.segments_groups += gb.n_groups;
        }
        if (run.coverage) run.t_coverage += c2 - c1 + shared;
        if (run.hitmap) {
            run.t_hitmap += c3 - c2 + (run.coverage ? 0.0 : shared);
            run.t_hitmap_kernels += hb.seconds_kernels;
            run.hitmap_probes += hb.probes;
        }
    }
    // --lca-file / --report-file: the batch's reads are called where its results lie on the device; the calls (and, without a TSV,
    // QHASH_COUNT) go to the chunks
    void add_lca(taxor_gpu_searcher *s, Chunks &group)
    {
        const double c0 = now();
        uint64_t nr = 0;
        for (auto &bt : group) nr += bt->ids.size();
        taxor_lca_calls calls{};
        if (taxor_gpu_lca_add_batch(run.lca, s, run.lca_next_read.fetch_add(nr), &calls) != TAXOR_OK) die(taxor_gpu_last_error());
        if (calls.n_reads != nr) die("internal: a batch's calls do not cover its chunks");
        uint64_t r0 = 0;
        for (auto &bt : group) {
            const uint64_t n = bt->ids.size();
            bt->lca_node.assign(calls.node + r0, calls.node + r0 + n);
            bt->lca_best.assign(calls.best + r0, calls.best + r0 + n);
            bt->lca_refs.assign(calls.n_refs + r0, calls.n_refs + r0 + n);
            if (!run.write_tsv) bt->n_hashes.assign(calls.n_hashes + r0, calls.n_hashes + r0 + n);
            r0 += n;
        }
        std::lock_guard<std::mutex> lk(run.stat_mu);
        run.t_lca += now() - c0;
    }
    // the CSR of several chunks classified as one batch -> each chunk's own CSR
    void split_results(Chunks &chunks, const taxor_gpu_results &res)
    {
        uint64_t r0 = 0;
        for (auto &bt : chunks) {
            const uint64_t n = bt->ids.size(), lo = res.read_off[r0], hi = res.read_off[r0 + n];
            bt->read_off.resize(n + 1);
            for (uint64_t i = 0; i <= n; ++i) bt->read_off[i] = res.read_off[r0 + i] - lo;
            bt->user_bin.assign(res.user_bin + lo, res.user_bin + hi);
            bt->count.assign(res.count + lo, res.count + hi);
            bt->n_hashes.assign(res.n_hashes + r0, res.n_hashes + r0 + n);
            r0 += n;
            run.count_chunk(*bt);
        }
        if (r0 != res.n_reads) die("internal: a batch's results do not cover its chunks");
    }
    // A chunk of file bytes (--device-parse) or of BAM sequences is a GPU batch by itself.  scan_begin hands it to the device: 0 =
    // enqueued on s (file bytes: ids and offsets are filled from the scanner's table); 1 = the device reported the bytes irregular
    // (or met a byte outside dna15, which the parsed path may still repair) and the chunk was parsed here (host_parse) -- it goes on
    // like any parsed chunk; -1 = err says why
    int scan_begin(taxor_gpu_searcher *s, Batch &bt, std::string &err)
    {
        if (bt.raw_kind == 'B') {
            const taxor_nibble_segment seg = nibble_segment(bt);
            if (taxor_gpu_search_nibbles_begin(s, &seg, 1) != TAXOR_OK) { err = taxor_gpu_last_error(); return -1; }
            bt.raw_kind = 0;
            ++n_bam;
            return 0;
        }
        taxor_fastx_scan sc{};
        if (!bt.raw_pinned) ++n_pageable;
        const int rc = taxor_gpu_search_fastx_begin(s, bt.raw.data(), bt.raw.size(), bt.raw_kind, &sc);
        if (rc != TAXOR_OK && rc != TAXOR_E_ALPHABET) { err = taxor_gpu_last_error(); return -1; }
        if (rc != TAXOR_OK || sc.status != 0) {
            err = host_parse(bt);
            if (!err.empty()) return -1;
            ++n_host_parsed;
            return 1;
        }
        uint64_t id_bytes = 0;
        for (uint64_t r = 0; r < sc.n_reads; ++r) id_bytes += sc.id_len[r];
        bt.ids.clear();
        bt.ids.reserve(sc.n_reads, id_bytes);
        bt.offsets.assign(1, 0);
        bt.offsets.reserve(sc.n_reads + 1);
        for (uint64_t r = 0; r < sc.n_reads; ++r) {
            bt.ids.data.append(bt.raw.data() + sc.id_off[r], sc.id_len[r]);
            bt.ids.off.push_back(bt.ids.data.size());
            bt.offsets.push_back(bt.offsets.back() + sc.read_len[r]);
        }
        bt.raw_kind = 0;
        ++n_scanned;
        return 0;
    }
    // one GPU batch: its chunks handed over as segments (unless the scanner enqueued it already, `scanned`), then waited for; the
    // results come to *res, or (res == nullptr) stay on the device
    int classify(taxor_gpu_searcher *s, Chunks &chunks, bool scanned, taxor_gpu_results *res)
    {
        std::vector<taxor_read_segment> segs;
        auto once = [&]() -> int {
            if (!scanned) {
                segs.clear();
                for (auto &bt : chunks) segs.push_back({bt->bases.data(), bt->offsets.data(), bt->ids.size()});
                const int rc = taxor_gpu_search_segments_begin(s, segs.data(), segs.size());
                if (rc != TAXOR_OK) return rc;
            }
            return res ? taxor_gpu_search_batch_end(s, res) : taxor_gpu_batch_sync(s);
        };
        return run_with_alphabet_retry(once, chunks);
    }

    // device g's share of a communicator round; an error message in err
    void round_on_device(taxor_gpu_searcher *s, Chunks &chunks, std::string &err)
    {
        static const uint64_t zero_off[1] = {0};
        if (chunks.empty()) {       // a device without a batch runs an empty one, so that every searcher has a finished run to gather
            if (taxor_gpu_search_batch_begin(s, nullptr, zero_off, 0) != TAXOR_OK) err = taxor_gpu_last_error();
            return;
        }
        const bool scanned = chunks[0]->raw_kind && scan_begin(s, *chunks[0], err) == 0;
        if (!err.empty()) return;
        for (auto &bt : chunks) pin_bases(*bt);
        if (classify(s, chunks, scanned, nullptr) != TAXOR_OK) err = taxor_gpu_last_error();
    }
    // With a communicator, worker `set`.  One round = up to ng GPU batches, batch g on device g, classified side by side; then ONE
    // gather of the round's per-read results on the first device and one copy to the host.  A GPU batch is made of queued chunks
    // like in the single-device workers below (handed over as segments).
    void gather_worker(unsigned set)
    {
        std::vector<taxor_gpu_searcher *> mine(ng);     // searcher of device g in this worker's set
        for (size_t g = 0; g < ng; ++g) mine[g] = sr[g * wpg + set];
        std::vector<Chunks> round(ng);
        Chunks eofs, flat;
        std::unique_ptr<Batch> b, held;         // held: a chunk of file bytes met while a batch of parsed chunks was being collected
        bool open = true;
        while (open || held) {
            for (auto &g : round) g.clear();
            eofs.clear();
            size_t used = 0;
            // the first chunk of a round is waited for; after that only what is already queued is taken
            for (size_t g = 0; g < ng; ++g) {
                uint64_t gr = 0, gb = 0;
                while (limits.wants_more(gr, gb, round[g].size())) {
                    bool got;
                    if (held) { b = std::move(held); got = true; }
                    else if (used == 0 && round[g].empty() && eofs.empty()) { got = p.q_in.pop(b); if (!got) open = false; }
                    else got = p.q_in.try_pop(b);
                    if (!got) break;
                    if (b->end_of_file) { eofs.push_back(std::move(b)); continue; }
                    if (b->raw_kind && !round[g].empty()) { held = std::move(b); break; }     // file bytes are a batch by themselves
                    const bool alone = b->raw_kind != 0;
                    gr += b->ids.size();
                    gb += b->bases.size();
                    round[g].push_back(std::move(b));
                    ++used;
                    if (alone) break;
                }
                if (round[g].empty()) break;
            }
            if (used == 0) {
                for (auto &e : eofs) p.q_fmt.push(std::move(e));
                continue;
            }
            const double t1 = now();
            std::vector<std::thread> dev;
            std::vector<std::string> errs(ng);
            for (size_t g = 0; g < ng; ++g) dev.emplace_back([this, g, &mine, &round, &errs] { round_on_device(mine[g], round[g], errs[g]); });
            for (auto &t : dev) t.join();
            for (const auto &e : errs)
                if (!e.empty()) die(e);
            const double t2 = now();
            flat.clear();                           // the gathered CSR is in device order, and in chunk order within a device
            for (auto &g : round)
                for (auto &bt : g) flat.push_back(std::move(bt));
            double t3;
            {
                std::lock_guard<std::mutex> lk(comm_mu);      // the other set's round keeps the devices busy meanwhile
                taxor_gpu_results res{};
                if (taxor_gpu_gather_results(comm, mine.data(), &res) != TAXOR_OK) die(taxor_gpu_last_error());
                t3 = now();
                split_results(flat, res);
            }
            {
                std::lock_guard<std::mutex> lk(run.stat_mu);
                run.t_search += t2 - t1;
                run.t_gather += t3 - t2;
                run.t_compute += now() - t1;
                run.n_gpu_batches += std::min(used, ng);
            }
            for (auto &bt : flat) p.q_fmt.push(std::move(bt));
            for (auto &e : eofs) p.q_fmt.push(std::move(e));
        }
    }
    // search to profile: the batch's results go into the profile's CSR where they lie.  Chunks reach a worker in any order, so a
    // batch is numbered as it arrives; the sequencer, which sees the chunks in input order, notes which number each read got
    // (FusedProfile::take_ids)
    void feed_profile(taxor_gpu_searcher *s, Chunks &group)
    {
        uint64_t nr = 0;
        for (auto &bt : group) nr += bt->ids.size();
        const uint64_t first = run.fused.next_read.fetch_add(nr);
        uint64_t at = first;
        for (auto &bt : group) { bt->feed_first = at; at += bt->ids.size(); }
        const double f0 = now();
        if (taxor_gpu_profile_feed_add_batch(run.fused.feed, s, first, 0) != TAXOR_OK) die(taxor_gpu_last_error());
        std::lock_guard<std::mutex> lk(run.stat_mu);
        run.fused.t_feed += now() - f0;
    }
    // Without a communicator, worker wi on its own searcher.
    void device_worker(size_t wi)
    {
        static const double fill_seconds = [] { const char *e = tune_env("TAXOR_CLI_FILL_MS"); return e ? atof(e) * 1e-3 : 0.020; }();
        // (a third and fourth worker per device that copy their results out and collect the next batch while two "slots" stay taken:
        // 25-32 Gbp/s against 33-35 with two workers, profiles/r04/cli_variants.txt -- more searchers share the same hardware queues)
        static const int fill_running = [] { const char *e = tune_env("TAXOR_CLI_FILL_RUNNING"); return e ? atoi(e) : 1; }();
        Chunks group, eofs;
        std::unique_ptr<Batch> b, held;     // held: a chunk of file bytes met while a batch of parsed chunks was being collected
        for (;;) {
            if (held) b = std::move(held);
            else if (!p.q_in.pop(b)) break;
            if (b->end_of_file) { p.q_fmt.push(std::move(b)); continue; }
            group.clear();
            eofs.clear();
            const bool raw = b->raw_kind != 0;      // file bytes: a batch by themselves
            uint64_t gr = b->ids.size(), gb = b->bases.size();
            group.push_back(std::move(b));
            const double t_fill0 = now();
            while (!raw && limits.wants_more(gr, gb, group.size())) {
                if (!p.q_in.try_pop(b)) {
                    // nothing queued: the GPU is the faster side right now.  Launching what there is makes the batches
                    // small exactly then (a quarter of the size the kernels are fastest at); while enough OTHER batches
                    // are in flight to keep the device busy this worker goes on collecting instead -- for a bounded
                    // time, because the chunks it holds may be what the writer is waiting for
                    if (!(gr < limits.group_reads && gb < (1ull << 29) && now() - t_fill0 < fill_seconds && n_running.load() >= fill_running)) break;
                    if (!p.q_in.pop_for(b, 100e-6)) { if (p.q_in.done()) break; continue; }
                }
                if (b->end_of_file) { eofs.push_back(std::move(b)); continue; }
                if (b->raw_kind) { held = std::move(b); break; }
                gr += b->ids.size();
                gb += b->bases.size();
                group.push_back(std::move(b));
            }
            ++n_running;
            const double t1 = now();
            for (auto &bt : group) pin_bases(*bt);
            const double t2 = now();
            taxor_gpu_results res{};
            bool scanned = false;
            if (raw) {
                std::string err;
                scanned = scan_begin(sr[wi], *group[0], err) == 0;
                if (!err.empty()) die(err);
            }
            // without a TSV nothing on the host reads the tuples: they stay on the device for the profile feed
            if (classify(sr[wi], group, scanned, run.write_tsv ? &res : nullptr) != TAXOR_OK) die(taxor_gpu_last_error());
            if (run.profile_mode) feed_profile(sr[wi], group);
            if (run.coverage || run.hitmap || run.confidence || run.breakpoint || run.segments || run.exclusive) use_saved(sr[wi], group);
            if (run.lca) add_lca(sr[wi], group);
            --n_running;
            const double t3 = now();
            if (run.write_tsv) split_results(group, res);
            else
                for (auto &bt : group) run.count_chunk(*bt);
            {
                std::lock_guard<std::mutex> lk(run.stat_mu);
                run.t_pin += t2 - t1;
                run.t_search += t3 - t2;
                ++run.n_gpu_batches;
                run.t_compute += now() - t1;
            }
            for (auto &bt : group) p.q_fmt.push(std::move(bt));
            for (auto &e : eofs) p.q_fmt.push(std::move(e));
        }
    }
    void run_workers()
    {
        if (comm)
            for (unsigned set = 0; set < wpg; ++set) workers.emplace_back([this, set] { gather_worker(set); });
        else
            for (size_t wi = 0; wi < ng * wpg; ++wi) workers.emplace_back([this, wi] { device_worker(wi); });
        for (auto &t : workers) t.join();
        trace("GPU workers done");
        if (run.cfg.device_parse && tune_env("TAXOR_CLI_TRACE"))
            fprintf(stderr, "[trace] --device-parse: %llu ranges scanned on the device, %llu parsed on the host; %llu copied from pageable memory\n",
                    (unsigned long long)n_scanned.load(), (unsigned long long)n_host_parsed.load(), (unsigned long long)n_pageable.load());
        if (n_bam.load() && tune_env("TAXOR_CLI_TRACE"))
            fprintf(stderr, "[trace] BAM: %llu chunks of 4-bit sequences unpacked on the device\n", (unsigned long long)n_bam.load());
    }
    void release()
    {
        for (auto *x : sr) taxor_gpu_searcher_destroy(x);
        if (comm) {
            taxor_gpu_comm_stats cs{};
            taxor_gpu_comm_info(comm, &cs);
            if (tune_env("TAXOR_CLI_TRACE"))
                fprintf(stderr, "[trace] %llu gathers (%s): %.1f MB from peer devices, %.3f s inside taxor_gpu_gather_results\n",
                        (unsigned long long)cs.gathers, gather.c_str(), cs.gather_bytes / 1e6, cs.gather_seconds);
            taxor_gpu_comm_destroy(comm);
        }
        for (size_t g = 0; g < ng; ++g) taxor_gpu_index_destroy(gidx[g]);
        trace("GPU memory released");
    }
};

void search_resident(SearchRun &run, taxor_hixf *h, const taxor_hixf_view *view, const taxor_gpu_search_params &prm, const std::vector<std::string> &queries,
                     bool last, double t0)
{
    const Config &cfg = run.cfg;
    const size_t ng = cfg.gpus.size(), nf = queries.size();
    const unsigned readers = (unsigned)std::max<size_t>(1, std::min<size_t>({nf, cfg.threads, 8}));
    const unsigned parse_threads = std::max(1u, std::min(cfg.threads, 32u) / readers);
    static const unsigned fmt_div = [] { const char *e = tune_env("TAXOR_CLI_FORMATTER_DIV"); const int v = e ? atoi(e) : 0; return v >= 1 && v <= 32 ? (unsigned)v : 4u; }();
    const unsigned formatters = std::max(1u, std::min(cfg.threads, 32u) / fmt_div);
    static const unsigned workers_per_gpu = [] { const char *e = tune_env("TAXOR_CLI_WORKERS_PER_GPU"); const int v = e ? atoi(e) : 0; return v >= 1 && v <= 4 ? (unsigned)v : 2u; }();
    const GroupLimits limits{cfg.group_reads ? cfg.group_reads : (cfg.batch_reads ? cfg.batch_reads : 131072), !cfg.batch_reads && !cfg.group_reads};
    Pipes p;
    BatchPool &pool = p.pool;
    pool.cap = readers * parse_threads + 16 + 2 + 32 + ng * workers_per_gpu * GroupLimits::max_chunks + 8 + formatters + 8 + 8 + 2 * readers;
    // ... by count for small chunks; by bytes for the usual ~128 MB ones: 6 GiB for the host stages + 6 GiB per device (two GPU
    // batches of ~1.3 GB in flight per device, the chunks being parsed, formatted and written) instead of cap x 128 MB
    // = 19 GB at one device and 75 GB at eight.  The floor lets every stage hold one buffer whatever the budget.
    pool.floor = readers * parse_threads + 2 * readers + ng * workers_per_gpu + formatters + 8;
    {
        const char *e = tune_env("TAXOR_CLI_POOL_GB");
        const double gb = e ? atof(e) : 0.0;
        pool.byte_budget = gb > 0.0 ? (uint64_t)(gb * (double)(1ull << 30)) : (6ull + 6ull * ng) << 30;
    }
    p.turns.ahead.assign(nf, 0);
    QueryFeed feed(cfg, queries, p, readers, parse_threads);
    feed.start();
    ReportWriter writer(run, h, p, formatters);
    writer.start();
    GpuStage gpu(run, p, ng, workers_per_gpu, limits);
    gpu.upload_index(view);
    run.t_index += now() - t0;
    trace("index resident in HBM");
    const CpuMark cpu0 = cpu_mark();
    if (tune_env("TAXOR_CLI_TRACE"))
        fprintf(stderr, "[trace] index: %.2f GB per replica in %.3f s = %.1f GB/s (file open to resident)\n", taxor_gpu_index_data_bytes(gpu.gidx[0]) / 1e9,
                now() - t0, taxor_gpu_index_data_bytes(gpu.gidx[0]) / 1e9 / (now() - t0));
    // the host mapping of the index is not needed any more: its pages go back on a helper thread, beside the search
    std::thread releaser([h] { taxor_hixf_release_data(h); });
    const double t_search0 = now();
    if (run.profile_mode) run.fused.begin(view, taxor_hixf_get_meta(h), run.prof.device);
    gpu.create_searchers(prm);
    if (!cfg.coverage_file.empty() || !cfg.hitmap_file.empty() || cfg.confidence_mode() || !cfg.breakpoint_file.empty() || !cfg.segments_file.empty() || cfg.exclusive_mode())
        gpu.begin_saved_consumers(view, taxor_hixf_get_meta(h));
    // (with --lca-confidence the confident calls fill both files: the plain accumulator is not created)
    if (run.lineage && !run.confidence && taxor_gpu_lca_create(gpu.gidx[0], run.lineage, &run.lca) != TAXOR_OK) die(taxor_gpu_last_error());
    gpu.run_workers();
    run.t_search_wall += now() - t_search0;
    if (run.coverage) {
        write_coverage_file(run, taxor_hixf_get_meta(h));
        trace("coverage written");
    }
    if (tune_env("TAXOR_CLI_TRACE")) {
        const CpuMark c1 = cpu_mark();
        const double w = now() - t_search0;
        fprintf(stderr, "[trace] search phase: %.3f s wall, %.2f s user + %.2f s system CPU = %.1f CPUs busy (allowance %.0f); the cgroup throttled the process in %llu of %llu periods, %.2f thread-seconds\n",
                w, c1.user - cpu0.user, c1.sys - cpu0.sys, w > 0 ? (c1.user - cpu0.user + c1.sys - cpu0.sys) / w : 0.0, cpu_allowance(),
                (unsigned long long)(c1.throttled_periods - cpu0.throttled_periods), (unsigned long long)(c1.periods - cpu0.periods), c1.throttled - cpu0.throttled);
    }
    p.q_fmt.close();
    writer.join();
    feed.closer.join();
    trace("writer done");
    if (tune_env("TAXOR_CLI_TRACE"))
        fprintf(stderr, "[trace] report: %.2f GB in %llu pieces by %u threads, %.3f s from the first write to the last = %.1f GB/s (%.3f s inside write() = %.1f GB/s)\n",
                writer.out_written.load() / 1e9, (unsigned long long)writer.next_ticket, formatters, writer.t_last_write - writer.t_first_write,
                writer.t_last_write > writer.t_first_write ? writer.out_written.load() / 1e9 / (writer.t_last_write - writer.t_first_write) : 0.0, writer.t_write,
                writer.t_write > 0 ? writer.out_written.load() / 1e9 / writer.t_write : 0.0);
    run.t_reads += *std::max_element(feed.reader_time.begin(), feed.reader_time.end());
    if (run.lca || run.confidence) {
        finish_lca(run);
        trace("calls and report written");
    }
    if (run.hitmap) {
        finish_hitmap(run);
        trace("hit maps written");
    }
    if (run.cfg.base_positions && tune_env("TAXOR_CLI_TRACE"))
        fprintf(stderr, "[trace] positions: %llu hashes placed, %.6f s in k_hash_positions (event pairs, one per sub-batch, summed over workers)\n",
                (unsigned long long)run.positions_hashes, run.t_positions_kernels);
    if (run.breakpoint) {
        finish_breakpoint(run);
        trace("breaks written");
    }
    if (run.segments) {
        finish_segments(run);
        trace("segments written");
    }
    if (run.exclusive) {
        finish_exclusive(run, taxor_hixf_get_meta(h));
        trace("exclusive hashes written");
    }
    gpu.release();
    if (run.profile_mode) {
        run.fused.finish(run.prof, cfg.threads, run.t_search_wall);
        trace("profile written");
    }
    releaser.join();
    taxor_hixf_free(h);
    trace("host index released");
    if (last) {
        // the process is about to end: unpinning and unmapping gigabytes of staging buffers page by page
        // would only delay the exit (~0.1 s per GB)
        for (auto &b : pool.free_) (void)b.release();
    } else {
        for (auto &b : pool.free_) unpin_buffers(*b);
    }
    pool.free_.clear();
    if (tune_env("TAXOR_CLI_TRACE"))
        fprintf(stderr, "[trace] chunk buffers: %zu made (floor %zu, cap %zu), peak %.2f GB on the books against a budget of %.2f GB, %llu released early\n",
                pool.made, pool.floor, pool.cap, pool.peak_bytes / 1073741824.0, pool.byte_budget / 1073741824.0, (unsigned long long)pool.trimmed);
    trace("batch buffers released");
}

// One index, all of `queries`: the index is loaded and uploaded once; query files are read concurrently (a gzip
// stream inflates on one thread, so several files are the only way to read gzip input faster) and written in the
// order they were given.
void search_files(SearchRun &run, const std::string &hixf_file, const std::vector<std::string> &queries, bool last)
{
    const Config &cfg = run.cfg;
    const double t0 = now();
    taxor_hixf *h = nullptr;
    if (taxor_hixf_load(hixf_file.c_str(), &h) != TAXOR_OK) die(taxor_gpu_last_error());
    trace("index file loaded");
    if (cfg.ixf_arith) {
        taxor_hixf_set_arith(h, cfg.ixf_arith);
        taxor_ixf_variant av{};
        taxor_ixf_arith_decode(cfg.ixf_arith, &av);
        char desc[512];
        taxor_ixf_variant_describe(&av, desc, sizeof desc);
        fprintf(stderr, "[TAXOR SEARCH WARNING] %s is searched under --ixf-arithmetic %s, not under this build's own reading of the\n"
                        "  un-vendored IXF arithmetic: %s (seed, segment length and row stride per IXF from the file)\n", hixf_file.c_str(),
                arith_spec(av).c_str(), desc);
    }
    if (cfg.layout_given) {
        if (taxor_hixf_set_layout(h, cfg.ixf_layout) != TAXOR_OK) die(taxor_gpu_last_error());
        char ld[128];
        taxor_ixf_layout_describe(cfg.ixf_layout, ld, sizeof ld);
        fprintf(stderr, "[TAXOR SEARCH WARNING] %s is read under --ixf-layout %s: its fingerprint vectors are transposed into the search layout on the device\n",
                hixf_file.c_str(), ld);
    }
    const taxor_hixf_view *view = taxor_hixf_get_view(h);
    if (taxor_hixf_get_meta(h)->foreign_schema)
        fprintf(stderr, "[TAXOR SEARCH WARNING] %s was not written by this library (its IXF records follow another layout, read by probing).\n"
                        "  The arithmetic of seqan3's interleaved_xor_filter is not part of the reference sources; this build's reading of it has\n"
                        "  not been checked against this file.  Run `taxor verify --index-file %s --genome-file <a genome in the index>` first:\n"
                        "  a wrong reading still loads and classifies at the false-positive floor.\n", hixf_file.c_str(), hixf_file.c_str());
    // threshold model (threshold.hpp:22-47)
    taxor_gpu_search_params prm{};
    if (taxor_threshold_select(view, cfg.error_rate, cfg.threshold, &prm) != TAXOR_OK)
        die("no threshold model for k=" + std::to_string(view->kmer_size) + " and error rate " + std::to_string(cfg.error_rate));
    switch (prm.model) {                                            // the reference's messages, threshold.hpp:32-46
    case TAXOR_THR_PERCENTAGE: printf("use percentage-model\t%g\n", cfg.threshold); break;
    case TAXOR_THR_SYNCMER: printf("use syncmer model\n"); break;
    case TAXOR_THR_KMER: printf("use kmer-model\n"); break;
    default: printf("use frac minhash\n"); break;
    }
    // paged (--device-index-budget, or an index that does not fit the device) or resident
    taxor_pass_plan whole{};
    if (taxor_index_plan_passes(view, ~0ull >> 1, &whole, nullptr, nullptr) != TAXOR_OK) die(taxor_gpu_last_error());
    uint64_t budget = cfg.index_budget_mib << 20;
    char why[256] = "";
    if (budget) snprintf(why, sizeof why, "--device-index-budget %llu MiB", (unsigned long long)cfg.index_budget_mib);
    else if (whole.index_bytes >= (1ull << 30)) {
        // (asked only for an index of a gigabyte or more: the question starts the HIP runtime on this thread, before the reader
        // threads exist, and a reader that dies on a malformed file then ends the process while the runtime is up -- its exit
        // handlers ran into this thread's index upload.  A smaller index on a device that is full fails as before, and the
        // message names the option)
        uint64_t fr = 0, tot = 0;
        if (taxor_gpu_device_memory(cfg.gpus[0], &fr, &tot) != TAXOR_OK) die(taxor_gpu_last_error());
        if (whole.index_bytes > fr) {
            budget = fr - std::min<uint64_t>(4ull << 30, fr / 4);       // the searcher's own buffers live beside the index
            snprintf(why, sizeof why, "the index needs %llu MiB on the device, %llu MiB are free", (unsigned long long)(whole.index_bytes >> 20), (unsigned long long)(fr >> 20));
        }
    }
    if (!cfg.coverage_file.empty()) {
        // the accumulator looks a user bin's hashes up in ALL its leaf bins: they must be resident together.  A budget the index fits
        // within pages nothing: the resident route is taken
        if (budget && cfg.index_budget_mib && whole.index_bytes <= budget) budget = 0;
        if (budget)
            die("Validation failed for option --coverage-file: the index would be searched in resident passes (" + std::string(why) + "; it holds " +
                std::to_string(whole.index_bytes >> 20) + " MiB), and its leaf bins are then never resident together; accumulating pass by pass is not built.");
    }
    if (!cfg.hitmap_file.empty()) {
        // a reference's hits are looked up in ALL its leaf bins, and a read's final tuples exist only after the last pass's merge
        if (budget && cfg.index_budget_mib && whole.index_bytes <= budget) budget = 0;
        if (budget)
            die("Validation failed for option --hitmap-file: the index would be searched in resident passes (" + std::string(why) + "; it holds " +
                std::to_string(whole.index_bytes >> 20) + " MiB), and its leaf bins are then never resident together; locating hits pass by pass is not built.");
    }
    if (!cfg.breakpoint_file.empty()) {
        // a read's hashes are looked up in ALL the leaf bins of its candidates, and its final tuples exist only after the last pass's merge
        if (budget && cfg.index_budget_mib && whole.index_bytes <= budget) budget = 0;
        if (budget)
            die("Validation failed for option --breakpoint-file: the index would be searched in resident passes (" + std::string(why) + "; it holds " +
                std::to_string(whole.index_bytes >> 20) + " MiB), and its leaf bins are then never resident together; finding breaks pass by pass is not built.");
    }
    if (!cfg.segments_file.empty()) {
        // as for --breakpoint-file
        if (budget && cfg.index_budget_mib && whole.index_bytes <= budget) budget = 0;
        if (budget)
            die("Validation failed for option --segments-file: the index would be searched in resident passes (" + std::string(why) + "; it holds " +
                std::to_string(whole.index_bytes >> 20) + " MiB), and its leaf bins are then never resident together; segmenting pass by pass is not built.");
    }
    if (cfg.base_positions && !view->use_syncmer)
        die("Validation failed for option --base-positions: the index does not hash syncmers (a minimiser or k-mer index); its hash lists are not deduplicated and their "
            "values are not wyhash(k-mer), so a position by content is not defined.");
    if (cfg.exclusive_mode()) {
        // as for --breakpoint-file
        if (budget && cfg.index_budget_mib && whole.index_bytes <= budget) budget = 0;
        if (budget)
            die("Validation failed for option " + std::string(!cfg.exclusive_file.empty() ? "--exclusive-file" : "--exclusive-reads-file") +
                ": the index would be searched in resident passes (" + std::string(why) + "; it holds " + std::to_string(whole.index_bytes >> 20) +
                " MiB), and its leaf bins are then never resident together; counting exclusive hashes pass by pass is not built.");
    }
    if (cfg.confidence_mode()) {
        // a read's hashes are looked up in ALL the leaf bins of its references, and its final tuples exist only after the last pass's merge
        if (budget && cfg.index_budget_mib && whole.index_bytes <= budget) budget = 0;
        if (budget)
            die("Validation failed for option --lca-confidence: the index would be searched in resident passes (" + std::string(why) + "; it holds " +
                std::to_string(whole.index_bytes >> 20) + " MiB), and its leaf bins are then never resident together; weighing calls pass by pass is not built.");
    }
    if (cfg.lca_mode()) {
        // a read is called from its FINAL tuples, which a paged search has only after the last pass's merge
        const std::string opt = !cfg.lca_file.empty() ? "--lca-file" : "--report-file";
        if (budget && cfg.index_budget_mib && whole.index_bytes <= budget) budget = 0;
        if (budget)
            die("Validation failed for option " + opt + ": the index would be searched in resident passes (" + std::string(why) + "; it holds " +
                std::to_string(whole.index_bytes >> 20) + " MiB), and a read's final tuples then exist only after the last pass's merge; calling reads there is not built.");
        if (taxor_lineage_create(taxor_hixf_get_meta(h), view->n_user_bins, &run.lineage) != TAXOR_OK || taxor_lineage_get_view(run.lineage, &run.lineage_view) != TAXOR_OK)
            die(std::string("Validation failed for option ") + opt + ": the index's taxonomy is not a tree: " + taxor_gpu_last_error());
    }
    if (budget) search_paged(run, h, view, prm, queries, budget, why, t0);
    else search_resident(run, h, view, prm, queries, last, t0);
}
